"""CPU: tests/field_adj_ref.py — the numpy restatement the GPU tests of field_vjp compare against — held to field_ref.displace by
the dot-product identity <q, g_q> + <v, g_v> + <dens, g_dens> = <a, abar>, and to the closed form of a plane-wave cotangent.  The
refusals of zd_field_vjp come before the GPU is touched, so they are asked here as well.

Bound of the identity: 1e-12 ||(q, v, dens)||_2 ||(g_q, g_v, g_dens)||_2 — float64 transform round-off (1e-18 of that product when
the definition was written down) with three orders of margin."""
import ctypes as C

import numpy as np
import pytest

import field_adj_ref
import field_ref
from conftest import WMAP

BOX = 720.0
PLT = dict(qPLT=1, qPLTrescale=1, PLT_target_z=5.0, f_cluster=0.97)
OPTIONS = [{}, dict(k_cutoff=2.0), dict(k_cutoff=2.0, corner_modes=1), dict(qonemode=1, one_mode=(3, 2, -4)),
           dict(qonemode=1, one_mode=(-5, 0, 7)), dict(f_cluster=0.9)]


@pytest.fixture(scope="module")
def zd():
    import zeldovich_plt_amd.api as api
    return api


_DRAWS = {}


def _draws(n):
    """default_rng(2).standard_normal: a field and the three cotangents, once per size (shared, read-only)"""
    if n not in _DRAWS:
        rng = np.random.default_rng(2)
        d = (rng.standard_normal((n, n, n)), rng.standard_normal((n, n, n, 3)), rng.standard_normal((n, n, n, 3)),
             rng.standard_normal((n, n, n)))
        for a in d:
            a.setflags(write=False)
        _DRAWS[n] = d
    return _DRAWS[n]


def _norm(*arrays):
    return np.sqrt(sum(float(np.sum(np.square(a))) for a in arrays))


def _identity(label, a, fwd, g_q, g_v, g_dens, abar, residue):
    q, v, dens = fwd
    lhs = float(np.sum(q * g_q) + np.sum(v * g_v) + np.sum(dens * g_dens))
    rhs = float(np.sum(a * abar))
    bound = 1e-12 * _norm(q, v, dens) * _norm(g_q, g_v, g_dens)
    print(label, "lhs", lhs, "rhs", rhs, "|lhs - rhs|", abs(lhs - rhs), "bound", bound, "max|Im| / max|abar|", residue / max(np.abs(abar).max(), 1e-300))
    assert abs(lhs - rhs) <= bound, (label, lhs, rhs, bound)
    assert residue <= 1e-12 * max(np.abs(abar).max(), 1e-300), (label, residue)  # H is Hermitian: the ky = 0 plane included


@pytest.mark.parametrize("n", [16, 32])
@pytest.mark.parametrize("kw", OPTIONS, ids=["-".join("%s%s" % kv for kv in kw.items()) or "plain" for kw in OPTIONS])
def test_dot_product_identity_za(zd, n, kw):
    a, g_q, g_v, g_dens = _draws(n)
    p = zd.make_params(n, boxsize=BOX, **kw)
    fwd = field_ref.displace(a, p)
    assert n == 16 or np.abs(fwd[0]).max() > 0  # (at 16 the mode (-5, 0, 7) lies beyond the cut-off: everything is zero there)
    abar, res = field_adj_ref.vjp(p, g_q, g_v, g_dens, with_residue=True)
    _identity("ZA PPD %d %r" % (n, kw), a, fwd, g_q, g_v, g_dens, abar, res)
    # each cotangent alone is its own term: an absent one is an exact zero
    parts = field_adj_ref.vjp(p, g_q=g_q) + field_adj_ref.vjp(p, g_v=g_v) + field_adj_ref.vjp(p, g_dens=g_dens)
    assert np.abs(parts - abar).max() <= 1e-12 * np.abs(abar).max()


def test_dot_product_identity_plt(zd, oracle):
    n = 32
    a, g_q, g_v, g_dens = _draws(n)
    eig = oracle.synthetic_eigenmodes(128)
    p = zd.make_params(n, boxsize=BOX, **PLT)
    fwd = field_ref.displace(a, p, eig=eig, oracle=oracle)
    abar, res = field_adj_ref.vjp(p, g_q, g_v, g_dens, eig=eig, oracle=oracle, with_residue=True)
    _identity("PLT + rescale PPD 32", a, fwd, g_q, g_v, g_dens, abar, res)


def test_dot_product_identity_white(zd):
    n = 32
    w, g_q, g_v, g_dens = _draws(n)
    ps = zd.PowerSpectrum.from_file(WMAP, BOX)
    p = zd.make_params(n, boxsize=BOX)
    fwd = field_ref.displace(field_ref.white_to_density(w, ps, p), p)
    abar, res = field_adj_ref.vjp(p, g_q, g_v, g_dens, kind="white", ps=ps, with_residue=True)
    _identity("white PPD 32", w, fwd, g_q, g_v, g_dens, abar, res)


@pytest.mark.parametrize("n", [16, 32])
def test_closed_form(zd, n):
    """g_q = B cos(theta) in one component + g_v = B' cos(theta) in another: abar = (B m_c + f B' m_c') sin(theta) / (|m|^2 fundamental)"""
    p = zd.make_params(n, boxsize=BOX, f_cluster=0.9)
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    sites = np.stack([z, y, x], axis=-1).reshape(-1, 3)
    for m, phi, c, B, cv, Bv in [((3, -2, 1), 0.3, 2, 1.0, 0, 0.7), ((-5, 0, 2), 1.1, 0, 0.4, 1, -1.3), ((0, 4, 0), -0.6, 1, 2.0, 2, 0.5)]:
        g_q, g_v = field_adj_ref.plane_wave_cotangent(n, m, phi, c, B, cv=cv, Bv=Bv)
        want = field_adj_ref.plane_wave_adjoint(n, m, phi, c, B, BOX, sites, cv=cv, Bv=Bv, f_cluster=0.9).reshape(n, n, n)
        got = field_adj_ref.vjp(p, g_q, g_v)
        err = np.abs(got - want).max() / np.abs(want).max()
        print("PPD", n, "m =", m, "closed form: error / max", err)
        assert err <= 1e-12, (m, err)


# ---- refusals: before the GPU is touched, one line each --------------------------------------------------------------------------
REFUSED = [(dict(f_NL=50.0), {}, "ZD_f_NL"), (dict(q2LPT=1), {}, "ZD_q2LPT"), (dict(q2LPT=1, q3LPT=1), {}, "ZD_q3LPT"), (dict(version=1), {}, "ZD_Version"),
           ({}, dict(fix_to_mean=1), "ZD_qPk_fix_to_mean"), (dict(ngpu=2), {}, "ZD_NumGPU"), (dict(ppd=48), {}, "PPD"), (dict(ppd=16), {}, "PPD"),
           (dict(qPLT=1), {}, "ZD_qPLT")]


def _one_field_line(err, word):
    lines = [ln for ln in err.splitlines() if ln.startswith("zeldovich_hip: ZD_Field")]
    assert len(lines) == 1 and word in lines[0], (word, err)


@pytest.mark.parametrize("kw,pkw,word", REFUSED, ids=["%s-%d" % (r[2], i) for i, r in enumerate(REFUSED)])
def test_refusals(zd, capfd, kw, pkw, word):
    kw = dict(kw)
    n = kw.pop("ppd", 32)
    g = np.zeros((n, n, n, 3), dtype=np.float32)
    pw = zd.PowerSpectrum.from_file(WMAP, BOX, **pkw)
    p = zd.make_params(n, boxsize=BOX, **kw)
    capfd.readouterr()
    with pytest.raises(RuntimeError):
        zd.field_vjp(p, pw, g_q=g)
    _one_field_line(capfd.readouterr().err, word)


def test_refusals_of_the_c_call(zd, capfd):
    """what the Python layer never lets through: an unknown kind or dtype, no cotangent at all, no place for the result"""
    n = 32
    L = zd.load_library()
    pw = zd.PowerSpectrum.from_file(WMAP, BOX)
    p = zd.make_params(n, boxsize=BOX)
    g = np.zeros((n, n, n, 3))
    out = np.zeros((n, n, n))
    capfd.readouterr()
    for args, word in (((7, 1, g.ctypes.data, None, None, 0, out.ctypes.data, 0), "kind"), ((0, 5, g.ctypes.data, None, None, 0, out.ctypes.data, 0), "dtype"),
                       ((0, 1, None, None, None, 0, out.ctypes.data, 0), "cotangent"), ((0, 1, g.ctypes.data, None, None, 0, None, 0), "zd_field_vjp needs")):
        assert L.zd_field_vjp(C.byref(p), C.byref(pw.pk), None, 0, *args, None) != 0
        _one_field_line(capfd.readouterr().err, word)


def test_arrays_python_refuses(zd):
    n = 32
    pw = zd.PowerSpectrum.from_file(WMAP, BOX)
    p = zd.make_params(n, boxsize=BOX)
    good = np.zeros((n, n, n, 3))
    for bad in (good[..., :2], good[..., 0], good.astype(np.int32), good.astype(np.float16), good.transpose(2, 1, 0, 3), good.tolist()):
        with pytest.raises((TypeError, ValueError)):
            zd.field_vjp(p, pw, g_q=bad)
        with pytest.raises((TypeError, ValueError)):
            zd.field_vjp(p, pw, g_v=bad)
    with pytest.raises((TypeError, ValueError)):
        zd.field_vjp(p, pw, g_dens=good)  # (a vector where the scalar cotangent goes)
    with pytest.raises(TypeError):
        zd.field_vjp(p, pw, g_q=good, g_v=good.astype(np.float32))  # one dtype
    with pytest.raises(ValueError):
        zd.field_vjp(p, pw)  # no cotangent
    with pytest.raises(ValueError):
        zd.field_vjp(p, pw, g_q=good, kind="pink")
    with pytest.raises((TypeError, ValueError)):
        zd.field_vjp(p, pw, g_q=good, out=np.zeros((n, n, n), dtype=np.float32))
