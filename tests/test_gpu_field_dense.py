"""GPU: field runs (zd_kernels_field.hip, make_field_phik) and their adjoint (zd_kernels_field_adj.hip, zd_field_vjp) on DENSE spectra at
the line lengths 256 ... 2048, where tests/test_gpu_field.py and tests/test_gpu_field_adj.py send a handful of plane waves.

The yardstick is tests/field_sum_ref.py: separable fields whose values float32 holds exactly and whose spectrum has no empty bin, and
the direct sum of the run (or of its adjoint) over every mode of the half space at chosen lattice sites, in float64 on the device,
with no N^3 transform; tests/test_field_sum.py holds it to field_ref / field_adj_ref / the oracle's eigenmode lookup at 32 and 64.
Records are read as test_gpu_field.py::test_every_length_against_plane_waves reads them: Plan.from_field, the staged calls, single
planes into a device buffer, 1400 sites of each of three planes of pass 0 (x = 0, x = N/2, y = 0 among them, the last plane beyond
N/2); nothing N^3-sized comes to the host but where a test is about host arrays.

Bound: the project's parity bound, 1e-10, against the rms of the quantity over the whole lattice (Parseval: the sum of |C(k)|^2 the
sweep returns), which is stricter than the maximum; the delivered float32 density 2^-23 of the largest reference value among the
sites (one float32 rounding, as test_gpu_field.py::test_density_output argues; the largest over the lattice is larger still); byte
comparisons are exact.  Every test prints its figures and its seconds before it asserts.

Measured on one MI355X with the whole suite, seconds per case as printed (worst error / rms over all cases 3.2e-14):
intake density 256 0.9 (the first case), 512 0.2, 1024 0.3, 2048 2.5; float32 field 0.1; white 0.1 - 0.3; PLT 256 0.2, 512 0.3 - 0.5
(6.0 in one run); adjoint ZA 256 0.2, 512 0.3, 1024 0.9, 2048 2.5; adjoint PLT 256 0.2, 512 0.4, 1024 1.7, 2048 9.0;
dot product 0.2; host fields 0.6; host cotangents 1.2 and 0.5.  test_gpu_field.py::test_every_length_against_plane_waves[2048-8] took
0.6 s beside them, so the 2048 cases are 4 and 15 times that, not the twice that was hoped for: the sweep of the reference over
4.3e9 modes is some forty torch operations on a 2048 x 2048 row, 1025 times, and the calls themselves allocate 69 GB arrays."""
import time

import numpy as np
import pytest

import field_sum_ref as fs
from conftest import WMAP

pytestmark = pytest.mark.gpu

BOX = 720.0
TOL = 1e-10
PLT = dict(qPLT=1, qPLTrescale=1, PLT_target_z=5.0, f_cluster=0.97)
REC = 56  # bytes of an RVdoubleZel record: ijk (3 x u2), pad, d (3 x f8), v (3 x f8)
NSITES = 1400


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


class _Clock:
    def __init__(self, label):
        self.label, self.t0 = label, time.perf_counter()

    def done(self):
        import torch
        torch.cuda.synchronize()
        print(self.label, "took %.1f s" % (time.perf_counter() - self.t0))


def _free():
    import gc
    import torch
    gc.collect()
    torch.cuda.empty_cache()


# ---- reading records ---------------------------------------------------------------------------------------------------------
def _probe(plan, n, with_density=False):
    """[(z, records of the plane as uint8 [N*N][56], density float32 [N*N] or None)] for the local planes 0, a third and the last of
    pass 0, all on the device"""
    import torch
    R = plan.R
    assert plan.record_size == REC
    store = torch.empty(plan.exchange_bytes, dtype=torch.uint8, device="cuda")
    rec = torch.empty(n * n * REC, dtype=torch.uint8, device="cuda")
    dens = torch.empty(n * n, dtype=torch.float32, device="cuda") if with_density else None
    plan.stage_z(0, store.data_ptr())
    plan.stage_y(store.data_ptr())
    out = []
    for lp in (0, (n // R) // 3, n // R - 1):
        z = plan.plane_z(0, lp)
        plan.stage_x(0, store.data_ptr(), lp, 1, rec.data_ptr(), dens.data_ptr() if with_density else None)
        torch.cuda.synchronize()
        out.append((z, rec.view(n * n, REC).clone(), dens.clone() if with_density else None))
    assert out[-1][0] > n // 2
    return out


def _planes_of(zd, ps, p, field, **kw):
    plan = zd.Plan.from_field(p, ps, field, **kw)
    try:
        assert plan.R == p.stream_factor
        return _probe(plan, int(p.ppd), with_density=bool(p.qdensity))
    finally:
        plan.close()


def _yx(n):
    """(y, x) of NSITES sites on each of the three planes: seeded, with x = 0, x = N/2, y = 0 and the far corner put in"""
    yx = np.random.default_rng(n).integers(0, n, (3, NSITES, 2))
    yx[:, 0], yx[:, 1], yx[:, 2], yx[:, 3], yx[:, 4] = (0, 0), (0, n // 2), (n // 2, 0), (n - 1, n - 1), (n // 2 + 1, n // 2)
    return yx


def _records_at(zd, planes, n):
    """(sites [3 NSITES][3], records there, density there or None) on the host"""
    import torch
    yx = _yx(n)
    sites, recs, dens = [], [], []
    for i, (z, rec, den) in enumerate(planes):
        rows = torch.from_numpy(yx[i, :, 0] * n + yx[i, :, 1]).cuda()
        recs.append(rec[rows].cpu().numpy().view(zd.RECORD_DTYPES["RVdoubleZel"]).reshape(-1))
        sites.append(np.column_stack([np.full(NSITES, z), yx[i]]))
        if den is not None:
            dens.append(den[rows].cpu().numpy())
    return np.concatenate(sites), np.concatenate(recs), (np.concatenate(dens) if dens else None)


def _forward_check(label, zd, planes, p, fac, **ref_kw):
    n = int(p.ppd)
    sites, got, dens = _records_at(zd, planes, n)
    assert np.array_equal(got["ijk"], sites.astype(got["ijk"].dtype))
    ref = fs.forward(fac, p, sites, device="cuda", **ref_kw)
    assert ref["rms_q"] > 0 and ref["rms_v"] > 0
    eq, ev = np.abs(got["d"] - ref["q"]).max() / ref["rms_q"], np.abs(got["v"] - ref["v"]).max() / ref["rms_v"]
    print(label, "rms q =", ref["rms_q"], "max|q| at the sites =", np.abs(ref["q"]).max(), "displacement error / rms", eq, "velocity error / rms", ev)
    assert eq <= TOL and ev <= TOL, (label, eq, ev)
    if dens is not None:
        want = ref["dens"].astype(np.float32).astype(np.float64)
        ed = np.abs(dens.astype(np.float64) - want).max() / np.abs(ref["dens"]).max()
        print(label, "delivered density: largest |delta| at the sites =", np.abs(ref["dens"]).max(), "error / that", ed, "bound", 2.0 ** -23)
        assert dens.dtype == np.float32 and ed <= 2.0 ** -23, (label, ed)


def _forward_case(label, zd, ps, n, R, kw=None, kind="density", eig=None, amp=None, pw=None):
    import torch
    clock = _Clock(label)
    p = zd.make_params(n, boxsize=BOX, stream_factor=R, **(kw or {}))
    fac = fs.factors(n, n + 1)
    field = fs.build_field(fac, torch.float64, "cuda")
    planes = _planes_of(zd, pw or ps, p, field, kind=kind, eig=eig)
    del field
    _free()
    _forward_check(label, zd, planes, p, fac, kind=kind, eig=eig, amp=amp)
    clock.done()
    return planes


# ---- 1. intake: density, ZA, a float64 device field at every length -----------------------------------------------------------------
_BYTES_512 = {}


def _device_planes_512(zd, ps):
    """the probed planes of the float64 device field at 512, stream factor 2 (once; what the float32 and the host forms must equal)"""
    import torch
    if not _BYTES_512:
        p = zd.make_params(512, boxsize=BOX, stream_factor=2)
        field = fs.build_field(fs.factors(512, 513), torch.float64, "cuda")
        _BYTES_512["planes"] = [(z, rec.cpu()) for z, rec, _d in _planes_of(zd, ps, p, field)]
        del field
        _free()
    return _BYTES_512["planes"]


def _same_planes(label, planes, base):
    for (z, rec, _d), (zb, recb) in zip(planes, base):
        assert z == zb and bool((rec.cpu() == recb).all()), "%s: plane z = %d differs from the float64 device field's" % (label, z)


@pytest.mark.parametrize("n,R", [(256, 1), (512, 2), (1024, 4), (2048, 8)])
def test_intake_density(zd, ps, n, R):
    planes = _forward_case("intake, density, ZA, PPD %d, stream factor %d" % (n, R), zd, ps, n, R)
    if n == 512:
        _same_planes("float64 device field, twice", planes, _device_planes_512(zd, ps))


def test_intake_float32_field_gives_the_same_bytes(zd, ps):
    import torch
    clock = _Clock("intake, float32 device field, PPD 512")
    base = _device_planes_512(zd, ps)
    p = zd.make_params(512, boxsize=BOX, stream_factor=2)
    field = fs.build_field(fs.factors(512, 513), torch.float32, "cuda")
    planes = _planes_of(zd, ps, p, field)
    del field
    _free()
    _same_planes("float32 device field", planes, base)
    clock.done()


# ---- 2. intake: white noise --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,R,spectrum", [(256, 1, "powerlaw"), (512, 2, "powerlaw"), (1024, 4, "powerlaw"), (512, 2, "tabulated")])
def test_intake_white(zd, ps, n, R, spectrum):
    p = zd.make_params(n, boxsize=BOX)
    count = (n // 2) ** 2  # every integer |k|^2 the zero rule leaves alive lies below the cut-off (N/2)^2
    if spectrum == "powerlaw":
        pw = zd.PowerSpectrum.from_powerlaw(-1.5, BOX)
        amp = fs.amp_powerlaw(pw, p, -1.5, count)
        probe = np.unique(np.concatenate([np.arange(1, 40), np.random.default_rng(0).integers(1, count, 200), [count - 1]]))
        each = np.array([np.sqrt(pw.power(np.sqrt(float(i) * p.fundamental ** 2)) / float(n) ** 3) for i in probe])
        worst = np.abs(amp[probe] / each - 1).max()
        print("power law amplitude, vectorised against one call per entry at", len(probe), "entries: worst relative difference", worst)
        assert worst <= 1e-13
    else:
        pw = ps
        amp = fs.amp_table(ps, p, count)
    _forward_case("intake, white (%s), ZA, PPD %d" % (spectrum, n), zd, ps, n, R, kind="white", amp=amp, pw=pw)


# ---- 3. intake: PLT + rescale ------------------------------------------------------------------------------------------------------
PLT_CASES = [(256, 1, {}), (512, 2, {}), (256, 1, dict(qdensity=1)), (256, 1, dict(k_cutoff=2.0, corner_modes=1))]


@pytest.mark.parametrize("n,R,kw", PLT_CASES, ids=["%d-%s" % (n, "-".join("%s%s" % kv for kv in kw.items()) or "plain") for n, R, kw in PLT_CASES])
def test_intake_plt(zd, ps, eig, n, R, kw):
    _forward_case("intake, density, PLT + rescale, PPD %d %r" % (n, kw), zd, ps, n, R, kw=dict(PLT, **kw), eig=eig)


# ---- 4. the adjoint ----------------------------------------------------------------------------------------------------------------
def _adjoint_sites(n, whole_planes):
    s = np.random.default_rng(n).integers(0, n, (64 if whole_planes else 4, 3))
    s[0], s[1], s[2], s[3] = (0, 0, 0), (n // 2 + 1, 0, n // 2), (n - 1, n // 2, 0), (n // 2, n - 1, n - 1)
    if not whole_planes:
        return s
    y, x = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    return np.concatenate([s] + [np.stack([np.full(n * n, z), y.ravel(), x.ravel()], axis=-1) for z in (0, n // 2 + 1)])


def _adjoint_case(label, zd, ps, n, dtype, parts, kw=None, eig=None, whole_planes=True, out_given=False):
    """field_vjp of dense separable cotangents built on the device (`parts`: which of q, v, dens) against the direct sum at 64 seeded
    sites and on the whole planes z = 0 and z = N/2 + 1 (whole_planes = False: four sites), error against the rms of abar"""
    import torch
    clock = _Clock(label)
    p = zd.make_params(n, boxsize=BOX, **(kw or {}))
    fq = fs.cotangent_factors(n, 2) if "q" in parts else None
    fv = fs.cotangent_factors(n, 3) if "v" in parts else None
    fd = fs.factors(n, 4) if "dens" in parts else None
    g = dict(g_q=fs.build_cotangent(fq, dtype, "cuda") if fq is not None else None, g_v=fs.build_cotangent(fv, dtype, "cuda") if fv is not None else None,
             g_dens=fs.build_field(fd, dtype, "cuda") if fd is not None else None)
    out = torch.empty((n, n, n), dtype=torch.float64, device="cuda") if out_given else None  # (lends T its storage)
    abar = zd.field_vjp(p, ps, eig=eig, out=out, **g)
    assert abar.is_cuda and abar.dtype == torch.float64 and tuple(abar.shape) == (n, n, n) and (out is None or abar is out)
    del g
    sites = _adjoint_sites(n, whole_planes)
    idx = torch.from_numpy(sites).cuda()
    got = abar[idx[:, 0], idx[:, 1], idx[:, 2]].cpu().numpy()
    del abar, out, idx
    _free()
    ref, rms = fs.adjoint(p, sites, fac_q=fq, fac_v=fv, fac_dens=fd, eig=eig, device="cuda")
    err = np.abs(got - ref).max() / rms
    print(label, "rms abar =", rms, "max|abar| at the", len(sites), "sites =", np.abs(ref).max(), "error / rms", err)
    assert rms > 0 and err <= TOL, (label, err)
    clock.done()


ADJ_ZA = [(256, "float64", "q-v-dens"), (512, "float64", "q-v-dens"), (1024, "float32", "q-v-dens"), (2048, "float32", "q")]
ADJ_PLT = [(256, "float64", "q-v"), (512, "float64", "q-v"), (1024, "float64", "q-v"), (2048, "float32", "q")]


@pytest.mark.parametrize("n,dtype,parts", ADJ_ZA, ids=["%d-%s-%s" % c for c in ADJ_ZA])
def test_adjoint_za(zd, ps, n, dtype, parts):
    import torch
    _adjoint_case("adjoint, ZA, PPD %d, %s g_%s" % (n, dtype, parts), zd, ps, n, getattr(torch, dtype), parts.split("-"), kw=dict(f_cluster=0.9),
                  whole_planes=n < 2048, out_given=n == 2048)


@pytest.mark.parametrize("n,dtype,parts", ADJ_PLT, ids=["%d-%s-%s" % c for c in ADJ_PLT])
def test_adjoint_plt(zd, ps, eig, n, dtype, parts):
    import torch
    _adjoint_case("adjoint, PLT + rescale, PPD %d, %s g_%s" % (n, dtype, parts), zd, ps, n, getattr(torch, dtype), parts.split("-"), kw=PLT, eig=eig,
                  whole_planes=n < 2048, out_given=n == 2048)


# ---- 5. the dot product at 512, on the device ---------------------------------------------------------------------------------------
def test_dot_product_at_512(zd, ps):
    """<q, g_q> + <v, g_v> over ALL records of the run on a dense field (both passes through the staged calls into a device buffer,
    7.5 GB of records in two halves) against <a, abar>; the bound of test_gpu_field_adj.py::test_dot_product_with_the_forward_run"""
    import torch
    n, R = 512, 2
    clock = _Clock("dot product, PPD 512")
    p = zd.make_params(n, boxsize=BOX, stream_factor=R)
    fac, fq, fv = fs.factors(n, 513), fs.cotangent_factors(n, 2), fs.cotangent_factors(n, 3)
    a = fs.build_field(fac, torch.float64, "cuda")
    g_q, g_v = fs.build_cotangent(fq, torch.float64, "cuda"), fs.build_cotangent(fv, torch.float64, "cuda")
    abar = zd.field_vjp(p, ps, g_q=g_q, g_v=g_v)
    rhs = float((a * abar).sum())
    del abar
    plan = zd.Plan.from_field(p, ps, a)
    lhs, rec2 = 0.0, 0.0
    try:
        assert plan.R == R and plan.record_size == REC and plan.local_planes == n // R
        store = torch.empty(plan.exchange_bytes, dtype=torch.uint8, device="cuda")
        rec = torch.empty((n // R) * n * n * REC, dtype=torch.uint8, device="cuda")
        for r in range(R):
            plan.stage_z(r, store.data_ptr())
            plan.stage_y(store.data_ptr())
            plan.stage_x(r, store.data_ptr(), 0, n // R, rec.data_ptr())
            torch.cuda.synchronize()
            w = rec.view(torch.float64).view(n // R, n, n, 7)  # (ijk and pad, d, v)
            assert plan.plane_z(r, 1) == r + R
            lhs += float((w[..., 1:4] * g_q[r::R]).sum() + (w[..., 4:7] * g_v[r::R]).sum())
            rec2 += float((w[..., 1:7] ** 2).sum())
    finally:
        plan.close()
    bound = TOL * np.sqrt(rec2) * np.sqrt(float((g_q ** 2).sum() + (g_v ** 2).sum()))
    print("PPD 512 dense: lhs", lhs, "rhs", rhs, "|lhs - rhs|", abs(lhs - rhs), "bound", bound)
    assert rec2 > 0 and abs(lhs - rhs) <= bound
    del a, g_q, g_v, rec, store, w
    _free()
    clock.done()


# ---- 6. host-staged chunks at 512: 8 chunks of 64 planes ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_host_field_in_chunks(zd, ps, dtype):
    clock = _Clock("intake, host %s field, PPD 512" % dtype)
    base = _device_planes_512(zd, ps)
    p = zd.make_params(512, boxsize=BOX, stream_factor=2)
    field = fs.field_numpy(fs.factors(512, 513)).astype(dtype)
    planes = _planes_of(zd, ps, p, field)
    del field
    _same_planes("host %s field" % dtype, planes, base)
    clock.done()


@pytest.mark.parametrize("dtype,parts", [("float32", "q-v"), ("float64", "dens")])
def test_host_cotangents_in_chunks(zd, ps, dtype, parts):
    """host cotangents and a host result at 512 (float32 g_q + g_v: both staging buffers) against the call with device cotangents and
    a device result, byte for byte"""
    import torch
    n = 512
    clock = _Clock("adjoint, host %s g_%s, PPD 512" % (dtype, parts))
    p = zd.make_params(n, boxsize=BOX, f_cluster=0.9)
    dt = getattr(torch, dtype)
    if parts == "q-v":
        dev = dict(g_q=fs.build_cotangent(fs.cotangent_factors(n, 2), dt, "cuda"), g_v=fs.build_cotangent(fs.cotangent_factors(n, 3), dt, "cuda"))
    else:
        dev = dict(g_dens=fs.build_field(fs.factors(n, 4), dt, "cuda"))
    want = zd.field_vjp(p, ps, **dev)
    host = {k: g.cpu().numpy() for k, g in dev.items()}
    del dev
    _free()
    got = zd.field_vjp(p, ps, **host)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (n, n, n)
    del host
    same = bool((torch.from_numpy(got).cuda() == want).all())
    scale = float(want.abs().max())
    del got, want
    _free()
    print("PPD 512 host", dtype, parts, "max|abar| =", scale, "bytes equal:", same)
    assert scale > 0 and same
    clock.done()


# ---- 7. launch sites (after the tests above) -----------------------------------------------------------------------------------------
def test_the_2048_adjoint_instances_were_launched(zd):
    names = [name for (name, _l), cnt in zd.dispatch_report().items() if cnt > 0]
    for plt in ("false", "true"):
        assert any("launch_fadj_z_t" in nm and "N = 2048" in nm and "PLT = %s" % plt in nm for nm in names), "k_fadj_z<2048, PLT = %s> never launched" % plt
