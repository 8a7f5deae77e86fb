"""GPU: the adjoint of a field run (api.field_vjp, zeldovich_plt_amd.autograd.field_run; definition in
zeldovich_plt_amd/csrc/zd_kernels_field_adj.hip).

The yardsticks are tests/field_adj_ref.py — the definition restated with numpy.fft, held to field_ref.displace in
tests/test_field_adj.py —, the existing forward path generate_field (an independent route: generator, passes, epilogue) through the
dot-product identity, and a closed form.  The tolerance is the project's parity bound, 1e-10 of the reference's maximum, wherever no
other bound is stated; every test prints its figures before it asserts."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import field_adj_ref
import field_ref
from conftest import ROOT, WMAP

pytestmark = pytest.mark.gpu

BOX = 720.0
TOL = 1e-10
PLT = dict(qPLT=1, qPLTrescale=1, PLT_target_z=5.0, f_cluster=0.97)


@pytest.fixture(scope="module")
def zd():
    import zeldovich_plt_amd.api as api
    return api


@pytest.fixture(scope="module")
def ps(zd):
    return zd.PowerSpectrum.from_file(WMAP, BOX)


@pytest.fixture(scope="module")
def eig(oracle):
    return oracle.synthetic_eigenmodes(128)


_DRAWS = {}


def _draws(n):
    """default_rng(3).standard_normal: a field and the cotangents g_q, g_v, g_dens — Nyquist, corner and k = 0 content that the
    adjoint must remove (once per size; shared, read-only)"""
    if n not in _DRAWS:
        rng = np.random.default_rng(3)
        d = (rng.standard_normal((n, n, n)), rng.standard_normal((n, n, n, 3)), rng.standard_normal((n, n, n, 3)),
             rng.standard_normal((n, n, n)))
        for a in d:
            a.setflags(write=False)
        _DRAWS[n] = d
    return _DRAWS[n]


def _norm(*arrays):
    return np.sqrt(sum(float(np.sum(np.square(np.asarray(a, dtype=np.float64)))) for a in arrays))


def _rel(got, ref):
    return np.abs(got - ref).max() / np.abs(ref).max()


# ---- 1. against the numpy reference ------------------------------------------------------------------------------------------
OPTIONS = [dict(k_cutoff=2.0), dict(k_cutoff=2.0, corner_modes=1), dict(qonemode=1, one_mode=(3, 2, -4)), dict(qonemode=1, one_mode=(-5, 0, 7)),
           dict(f_cluster=0.9)]
CASES = [(32, {}), (64, {}), (128, {})] + [(64, kw) for kw in OPTIONS]


@pytest.mark.parametrize("n,kw", CASES, ids=["%d-%s" % (n, "-".join("%s%s" % kv for kv in kw.items()) or "plain") for n, kw in CASES])
def test_against_numpy(zd, ps, n, kw):
    _a, g_q, g_v, g_dens = _draws(n)
    p = zd.make_params(n, boxsize=BOX, **kw)
    ref = field_adj_ref.vjp(p, g_q, g_v, g_dens)
    got = zd.field_vjp(p, ps, g_q=g_q, g_v=g_v, g_dens=g_dens)
    assert got.dtype == np.float64 and got.shape == (n, n, n)
    err = _rel(got, ref)
    print("PPD", n, kw, "max|abar| =", np.abs(ref).max(), "error / max", err)
    assert np.abs(ref).max() > 0 and err <= TOL


def test_against_numpy_plt(zd, ps, oracle, eig):
    n = 64
    _a, g_q, g_v, g_dens = _draws(n)
    p = zd.make_params(n, boxsize=BOX, **PLT)
    ref = field_adj_ref.vjp(p, g_q, g_v, g_dens, eig=eig, oracle=oracle)
    got = zd.field_vjp(p, ps, g_q=g_q, g_v=g_v, g_dens=g_dens, eig=eig)
    err = _rel(got, ref)
    print("PPD 64 PLT + rescale: max|abar| =", np.abs(ref).max(), "error / max", err)
    assert err <= TOL
    for name, kw in (("g_q", dict(g_q=g_q)), ("g_v", dict(g_v=g_v))):  # each six-transform half alone
        e1 = _rel(zd.field_vjp(p, ps, eig=eig, **kw), field_adj_ref.vjp(p, eig=eig, oracle=oracle, **kw))
        print("PPD 64 PLT + rescale,", name, "alone: error / max", e1)
        assert e1 <= TOL


def test_against_numpy_white(zd, ps):
    n = 64
    _a, g_q, g_v, g_dens = _draws(n)
    p = zd.make_params(n, boxsize=BOX)
    ref = field_adj_ref.vjp(p, g_q, g_v, g_dens, kind="white", ps=ps)
    got = zd.field_vjp(p, ps, g_q=g_q, g_v=g_v, g_dens=g_dens, kind="white")
    err = _rel(got, ref)
    print("PPD 64 white: max|abar| =", np.abs(ref).max(), "error / max", err)
    assert err <= TOL


# ---- 2. against the forward path ------------------------------------------------------------------------------------------------
FORWARD = [(64, {}, "density"), (128, {}, "density"), (64, PLT, "density"), (64, {}, "white")]


@pytest.mark.parametrize("n,kw,kind", FORWARD, ids=["%d-%s-%s" % (n, "plt" if kw else "za", kind) for n, kw, kind in FORWARD])
def test_dot_product_with_the_forward_run(zd, ps, eig, n, kw, kind):
    a, g_q, g_v, _g_dens = _draws(n)
    p = zd.make_params(n, boxsize=BOX, **kw)
    e = eig if kw else None
    rec = zd.generate_field(p, ps, a, kind=kind, eig=e)["records"]
    abar = zd.field_vjp(p, ps, g_q=g_q, g_v=g_v, kind=kind, eig=e)
    lhs = float(np.sum(rec["d"] * g_q) + np.sum(rec["v"] * g_v))
    rhs = float(np.sum(a * abar))
    bound = TOL * _norm(rec["d"], rec["v"]) * _norm(g_q, g_v)
    print("PPD", n, kw, kind, "lhs", lhs, "rhs", rhs, "|lhs - rhs|", abs(lhs - rhs), "bound", bound)
    assert abs(lhs - rhs) <= bound


def test_dot_product_with_the_delivered_density(zd, ps):
    """ZD_qdensity = 1: the forward side of the density term is float32, so that term alone is held to 2^-23 ||dens|| ||g_dens||
    (one float32 rounding per site, as test_gpu_field.test_density_output argues); displacements and velocities as above"""
    n = 64
    a, g_q, g_v, g_dens = _draws(n)
    p = zd.make_params(n, boxsize=BOX, qdensity=1)
    got = zd.generate_field(p, ps, a)
    rec, dens = got["records"], got["density"].astype(np.float64)
    abar = zd.field_vjp(p, ps, g_q=g_q, g_v=g_v)
    abar_d = zd.field_vjp(p, ps, g_dens=g_dens)
    both = zd.field_vjp(p, ps, g_q=g_q, g_v=g_v, g_dens=g_dens)
    d1 = abs(float(np.sum(rec["d"] * g_q) + np.sum(rec["v"] * g_v)) - float(np.sum(a * abar)))
    b1 = TOL * _norm(rec["d"], rec["v"]) * _norm(g_q, g_v)
    d2 = abs(float(np.sum(dens * g_dens)) - float(np.sum(a * abar_d)))
    b2 = 2.0 ** -23 * _norm(dens) * _norm(g_dens)
    split = _rel(both, abar + abar_d)
    print("ZD_qdensity = 1: records", d1, "bound", b1, "density term", d2, "bound", b2, "all three against the sum of the parts", split)
    assert d1 <= b1 and d2 <= b2 and split <= TOL


# ---- 3. one Jacobian entry both ways ------------------------------------------------------------------------------------------
def test_one_jacobian_entry_both_ways(zd, ps):
    n = 64
    y0, x0 = (5, 9, 13), (20, 3, 41)
    p = zd.make_params(n, boxsize=BOX)
    a = np.zeros((n, n, n))
    a[y0] = 1.0
    d = zd.generate_field(p, ps, a)["records"]["d"]
    scale = np.abs(d).max()
    for c in range(3):
        g = np.zeros((n, n, n, 3))
        g[x0 + (c,)] = 1.0
        abar = zd.field_vjp(p, ps, g_q=g)
        print("component", c, "forward", d[x0 + (c,)], "adjoint", abar[y0], "difference / max|d|", abs(d[x0 + (c,)] - abar[y0]) / scale)
        assert d[x0 + (c,)] != 0.0 and abs(d[x0 + (c,)] - abar[y0]) <= TOL * scale


# ---- 4. the closed form at the larger tile shapes ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [256, 512, 1024])
def test_closed_form_on_the_device(zd, ps, n):
    """A plane-wave cotangent built ON THE DEVICE plane by plane; abar at 64 seeded sites and on the whole planes z = 0 and
    z = N/2 + 1.  1024: float32 cotangents holding float32-exact values — the wave (N/4, N/4, -N/4) with phase 0 takes the values
    0 and +-1 only (a generic wave rounded to float32 is no plane wave to 1e-10)."""
    import torch
    if n == 1024:
        m, phi, dtype = (n // 4, n // 4, -(n // 4)), 0.0, torch.float32
    else:
        m, phi, dtype = (-7, 11, 5), 0.3, torch.float64
    c, B, cv, Bv, fc = 2, 1.0, 0, 0.5, 0.9
    p = zd.make_params(n, boxsize=BOX, f_cluster=fc)
    g_q, g_v = field_adj_ref.plane_wave_cotangent(n, m, phi, c, B, cv=cv, Bv=Bv, xp=torch, device="cuda", dtype=dtype)
    abar = zd.field_vjp(p, ps, g_q=g_q, g_v=g_v)
    del g_q, g_v
    assert abar.is_cuda and abar.dtype == torch.float64 and tuple(abar.shape) == (n, n, n)
    sites = np.random.default_rng(n).integers(0, n, (64, 3))
    idx = torch.from_numpy(sites).cuda()
    got = abar[idx[:, 0], idx[:, 1], idx[:, 2]].cpu().numpy()
    want = field_adj_ref.plane_wave_adjoint(n, m, phi, c, B, BOX, sites, cv=cv, Bv=Bv, f_cluster=fc)
    scale = abs(B * m[0] + (np.sqrt(1 + 24 * fc) - 1) / 4 * Bv * m[2]) / (float(sum(k * k for k in m)) * 2 * np.pi / BOX)  # the amplitude
    worst = np.abs(got - want).max()
    y, x = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    for z in (0, n // 2 + 1):
        plane = np.stack([np.full(n * n, z), y.ravel(), x.ravel()], axis=-1)
        wantp = field_adj_ref.plane_wave_adjoint(n, m, phi, c, B, BOX, plane, cv=cv, Bv=Bv, f_cluster=fc).reshape(n, n)
        worst = max(worst, np.abs(abar[z].cpu().numpy() - wantp).max())
    del abar
    torch.cuda.empty_cache()
    print("PPD", n, "closed form: amplitude", scale, "worst error / amplitude", worst / scale)
    assert scale > 0 and worst <= TOL * scale


# ---- 5. forms ------------------------------------------------------------------------------------------------------------------
def test_forms_give_identical_bits(zd, ps):
    import torch
    n = 64
    _a, g_q, g_v, g_dens = _draws(n)
    q64, v64, d64 = (g.astype(np.float32).astype(np.float64) for g in (g_q, g_v, g_dens))  # float64 values that float32 holds exactly
    q32, v32, d32 = (g.astype(np.float32) for g in (q64, v64, d64))
    p = zd.make_params(n, boxsize=BOX)
    base = zd.field_vjp(p, ps, g_q=q64, g_v=v64, g_dens=d64)
    assert isinstance(base, np.ndarray)
    forms = {"host float32": (q32, v32, d32), "device float64": tuple(torch.from_numpy(g).cuda() for g in (q64, v64, d64)),
             "device float32": tuple(torch.from_numpy(g).cuda() for g in (q32, v32, d32))}
    for name, (q, v, d) in forms.items():
        got = zd.field_vjp(p, ps, g_q=q, g_v=v, g_dens=d)
        assert isinstance(got, np.ndarray) != name.startswith("device"), name
        got = got.cpu().numpy() if name.startswith("device") else got
        assert got.tobytes() == base.tobytes(), name
    assert zd.field_vjp(p, ps, g_q=q64, g_v=v64, g_dens=d64).tobytes() == base.tobytes()  # twice the same
    # an absent cotangent is an exact zero
    only_q = zd.field_vjp(p, ps, g_q=q64)
    assert zd.field_vjp(p, ps, g_q=q64, g_v=np.zeros_like(v64)).tobytes() == only_q.tobytes()
    assert np.abs(only_q).max() > 0 and only_q.tobytes() != base.tobytes()
    # out= is filled in place, host and device
    out = np.full((n, n, n), np.nan)
    assert zd.field_vjp(p, ps, g_q=q64, g_v=v64, g_dens=d64, out=out) is out and out.tobytes() == base.tobytes()
    tout = torch.full((n, n, n), float("nan"), dtype=torch.float64, device="cuda")
    q, v, d = forms["device float64"]
    assert zd.field_vjp(p, ps, g_q=q, g_v=v, g_dens=d, out=tout) is tout and tout.cpu().numpy().tobytes() == base.tobytes()


# ---- 6. autograd ---------------------------------------------------------------------------------------------------------------
def test_backward_reaches_the_field(zd, ps):
    import torch
    from zeldovich_plt_amd.autograd import field_run
    n = 64
    a, _g_q, g_v, _g_dens = _draws(n)
    p = zd.make_params(n, boxsize=BOX, icformat="RVZel")  # (the format of a delivered run does not enter)
    w = torch.from_numpy(g_v.copy()).cuda()
    field = torch.from_numpy(a.copy()).cuda().requires_grad_(True)
    q, v = field_run(field, p, ps)
    assert q.dtype == torch.float64 and tuple(q.shape) == (n, n, n, 3) and q.is_cuda and v.dtype == torch.float64 and tuple(v.shape) == (n, n, n, 3)
    loss = 0.5 * (q * q).sum() + (v * w).sum()
    loss.backward()
    direct = zd.field_vjp(p, ps, g_q=q.detach(), g_v=w)
    assert field.grad is not None and field.grad.dtype == torch.float64
    assert field.grad.cpu().numpy().tobytes() == direct.cpu().numpy().tobytes()
    ref = field_adj_ref.vjp(p, g_q=q.detach().cpu().numpy(), g_v=g_v)
    err = _rel(field.grad.cpu().numpy(), ref)
    print("autograd at PPD 64: max|grad| =", np.abs(ref).max(), "error / max", err)
    assert err <= TOL
    f32 = torch.from_numpy(a.astype(np.float32)).cuda().requires_grad_(True)
    q32, _v32 = field_run(f32, p, ps)
    (0.5 * (q32 * q32).sum()).backward()
    assert f32.grad.dtype == torch.float32 and tuple(f32.grad.shape) == (n, n, n) and float(f32.grad.abs().max()) > 0


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------
REFUSED = [(dict(f_NL=50.0), {}, "ZD_f_NL"), (dict(q2LPT=1), {}, "ZD_q2LPT"), (dict(q2LPT=1, q3LPT=1), {}, "ZD_q3LPT"), (dict(version=1), {}, "ZD_Version"),
           ({}, dict(fix_to_mean=1), "ZD_qPk_fix_to_mean"), (dict(ngpu=2), {}, "ZD_NumGPU"), (dict(ppd=48), {}, "PPD")]


def _one_field_line(err, word):
    lines = [ln for ln in err.splitlines() if ln.startswith("zeldovich_hip: ZD_Field")]
    assert len(lines) == 1 and word in lines[0], (word, err)


@pytest.mark.parametrize("kw,pkw,word", REFUSED, ids=[r[2] for r in REFUSED])
def test_refusals(zd, capfd, kw, pkw, word):
    import torch
    kw = dict(kw)
    n = kw.pop("ppd", 32)
    pw = zd.PowerSpectrum.from_file(WMAP, BOX, **pkw)
    p = zd.make_params(n, boxsize=BOX, **kw)
    for g in (np.zeros((n, n, n, 3), dtype=np.float32), torch.zeros((n, n, n, 3), dtype=torch.float64, device="cuda")):
        capfd.readouterr()
        with pytest.raises(RuntimeError):
            zd.field_vjp(p, pw, g_v=g)
        _one_field_line(capfd.readouterr().err, word)


def test_refusals_of_the_c_call(zd, ps, capfd):
    n = 32
    L = zd.load_library()
    p = zd.make_params(n, boxsize=BOX)
    g = np.zeros((n, n, n, 3))
    out = np.zeros((n, n, n))
    capfd.readouterr()
    for args, word in (((7, 1, g.ctypes.data, None, None, 0, out.ctypes.data, 0), "kind"), ((0, 5, g.ctypes.data, None, None, 0, out.ctypes.data, 0), "dtype"),
                       ((0, 1, None, None, None, 0, out.ctypes.data, 0), "cotangent")):
        assert L.zd_field_vjp(C.byref(p), C.byref(ps.pk), None, 0, *args, None) != 0
        _one_field_line(capfd.readouterr().err, word)


def test_arrays_python_refuses(zd, ps):
    import torch
    n = 32
    p = zd.make_params(n, boxsize=BOX)
    good = np.zeros((n, n, n, 3))
    bad = [good[..., :2], good[..., 0], good.astype(np.int32), good.astype(np.float16), good.transpose(2, 1, 0, 3), good.tolist(),
           torch.zeros((n, n, n, 3), dtype=torch.float64), torch.zeros((n, n, n, 3), dtype=torch.int32, device="cuda"),
           torch.zeros((n, n, n, 6), dtype=torch.float64, device="cuda")[..., ::2], torch.zeros((n, n, n), dtype=torch.float64, device="cuda")]
    for g in bad:
        with pytest.raises((TypeError, ValueError)):
            zd.field_vjp(p, ps, g_q=g)
    with pytest.raises(ValueError):
        zd.field_vjp(p, ps, g_q=good, g_v=torch.zeros((n, n, n, 3), dtype=torch.float64, device="cuda"))  # host and device mixed
    with pytest.raises(ValueError):
        zd.field_vjp(p, ps)


# ---- 8. launch sites (after the tests above) ----------------------------------------------------------------------------------
def test_every_launch_site_was_launched(zd):
    """the adjoint's stages at every length the suite runs (2048 belongs to scripts/field_vjp_times.py) have been launched by the
    tests of this file"""
    txt = open(os.path.join(ROOT, "zeldovich_plt_amd", "csrc", "zd_kernels_field_adj.hip")).read()
    assert txt.count("ZD_LAUNCH_CHECK();") == 5
    sizes = re.findall(r"X\((\d+), (\d+), (\d+), (\d+)\)", re.search(r"#define FADJ_SIZES\(X\)(.*)", txt).group(1))
    assert [int(s[0]) for s in sizes] == [32, 64, 128, 256, 512, 1024, 2048]
    names = [name for (name, _l), cnt in zd.dispatch_report().items() if cnt > 0]
    for N, E, W, ROWS in sizes[:-1]:
        rows, cols = "N = %s, E = %s, ROWS = %s" % (N, E, ROWS), "N = %s, E = %s, W = %s" % (N, E, W)
        for launcher, want in (("launch_fadj_x_t", rows), ("launch_fadj_z_t", cols + ", PLT = false"), ("launch_fadj_iz_t", cols),
                               ("launch_fadj_iy_t", cols), ("launch_fadj_ix_t", rows)):
            assert any(launcher in nm and want in nm for nm in names), "%s<%s> never launched" % (launcher, want)
    assert any("launch_fadj_z_t" in nm and "N = 64, E = 16, W = 32, PLT = true" in nm for nm in names)
