"""CPU: tests/field_sum_ref.py — separable dense fields, the direct sums of a field run and of its adjoint, and the vectorised eigenmode
lookup, the yardstick of tests/test_gpu_field_dense.py — held to field_ref.displace, field_adj_ref.vjp and the oracle's
zdo_get_eigenmode at N = 32 and 64.

Bound: 1e-12 of the largest value of the reference (float64 sums of N^3 / 2 terms against numpy's transforms: a few 1e-16 when this
was written); every test prints its figure before it asserts."""
import ctypes as C

import numpy as np
import pytest

import field_adj_ref
import field_ref
import field_sum_ref as fs
from conftest import WMAP

BOX = 720.0
TOL = 1e-12
PLT = dict(qPLT=1, qPLTrescale=1, PLT_target_z=5.0, f_cluster=0.97)
OPTIONS = [{}, dict(k_cutoff=2.0), dict(k_cutoff=2.0, corner_modes=1), dict(qonemode=1, one_mode=(3, 2, -4)), dict(qonemode=1, one_mode=(-5, 0, 7)),
           dict(f_cluster=0.9)]
IDS = ["-".join("%s%s" % kv for kv in kw.items()) or "plain" for kw in OPTIONS]


@pytest.fixture(scope="module")
def zd():
    import zeldovich_plt_amd.api as api
    return api


def _sites(n):
    """16 sites: the edges x = 0, x = N/2, y = 0, z > N/2 and seeded ones"""
    s = np.random.default_rng(n).integers(0, n, (16, 3))
    s[0] = (0, 0, 0)
    s[1] = (n // 2 + 1, 0, n // 2)
    s[2] = (n - 1, n - 1, 0)
    s[3] = (n // 2, n // 2, n // 2)
    return s


def _at(a, s):
    return a[s[:, 0], s[:, 1], s[:, 2]]


def _rel(got, ref, full):
    return np.abs(got - ref).max() / np.abs(full).max()


def _forward_case(label, p, fac, s, ref, **kw):
    q, v, dens = ref
    got = fs.forward(fac, p, s, **kw)
    assert np.abs(q).max() > 0
    eq, ev, ed = _rel(got["q"], _at(q, s), q), _rel(got["v"], _at(v, s), v), _rel(got["dens"], _at(dens, s), dens)
    rq, rv, rd = (abs(got[k] / np.sqrt(np.mean(a * a)) - 1) for k, a in (("rms_q", q), ("rms_v", v), ("rms_dens", dens)))
    print(label, "max|q| =", np.abs(q).max(), "errors / max: q", eq, "v", ev, "dens", ed, "| Parseval rms / rms - 1: q", rq, "v", rv, "dens", rd)
    assert max(eq, ev, ed) <= TOL and max(rq, rv, rd) <= TOL, (label, eq, ev, ed, rq, rv, rd)


def _adjoint_case(label, p, s, ref, **kw):
    got, rms = fs.adjoint(p, s, **kw)
    assert np.abs(ref).max() > 0
    e, r = _rel(got, _at(ref, s), ref), abs(rms / np.sqrt(np.mean(ref * ref)) - 1)
    print(label, "max|abar| =", np.abs(ref).max(), "error / max", e, "| Parseval rms / rms - 1", r)
    assert e <= TOL and r <= TOL, (label, e, r)


def _cot(fac3):
    return np.stack([fs.field_numpy(fac3[c]) for c in range(3)], axis=-1)


# ---- the fields themselves ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [32, 64])
def test_separable_fields(n):
    """exact in float32; the spectrum is the outer product of three 1-D transforms and is dense; the device builder (on the CPU
    here) gives the same numbers in both dtypes"""
    import torch
    fac = fs.factors(n, 5)
    a = fs.field_numpy(fac)
    assert np.array_equal(a.astype(np.float32).astype(np.float64), a) and np.abs(a).max() <= 2.0
    F = fs.spectrum_numpy(fac)
    err = np.abs(F - np.fft.fftn(a)).max() / np.abs(F).max()
    dense = np.mean(np.abs(F) > 1e-3 * np.abs(F).max())
    print("N", n, "separable spectrum against fftn: error / max", err, "bins above 1e-3 of the largest:", dense)
    assert err <= TOL and dense > 0.99
    for dt in (torch.float32, torch.float64):
        assert np.array_equal(fs.build_field(fac, dt, "cpu").numpy().astype(np.float64), a)
    s = _sites(n)
    assert np.array_equal(fs.field_values(fac, s), _at(a, s))
    fac3 = fs.cotangent_factors(n, 2)
    g = _cot(fac3)
    assert np.array_equal(fs.build_cotangent(fac3, torch.float32, "cpu").numpy().astype(np.float64), g)
    assert np.abs(g[..., 0] - g[..., 1]).max() > 0 and np.abs(g[..., 1] - g[..., 2]).max() > 0


# ---- the direct sums -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [32, 64])
@pytest.mark.parametrize("kw", OPTIONS, ids=IDS)
def test_sums_za(zd, n, kw):
    p = zd.make_params(n, boxsize=BOX, **kw)
    fac, fq, fv, fd = fs.factors(n, 1), fs.cotangent_factors(n, 2), fs.cotangent_factors(n, 3), fs.factors(n, 4)
    s = _sites(n)
    _forward_case("ZA N %d %r" % (n, kw), p, fac, s, field_ref.displace(fs.field_numpy(fac), p))
    g_q, g_v, g_d = _cot(fq), _cot(fv), fs.field_numpy(fd)
    _adjoint_case("ZA adjoint N %d %r" % (n, kw), p, s, field_adj_ref.vjp(p, g_q, g_v, g_d), fac_q=fq, fac_v=fv, fac_dens=fd)
    _adjoint_case("ZA adjoint, g_v alone, N %d %r" % (n, kw), p, s, field_adj_ref.vjp(p, g_v=g_v), fac_v=fv)


@pytest.mark.parametrize("n", [32, 64])
@pytest.mark.parametrize("spectrum", ["tabulated", "powerlaw"])
def test_sums_white(zd, n, spectrum):
    p = zd.make_params(n, boxsize=BOX)
    count = 3 * (n // 2) ** 2 + 1
    if spectrum == "tabulated":
        ps = zd.PowerSpectrum.from_file(WMAP, BOX)
        amp = fs.amp_table(ps, p, count)
    else:
        ps = zd.PowerSpectrum.from_powerlaw(-1.5, BOX)
        amp = fs.amp_powerlaw(ps, p, -1.5, count)
        err = np.abs(amp[1:] / fs.amp_table(ps, p, count)[1:] - 1).max()
        print("power law: vectorised amplitude against one ps.power call per entry, worst relative difference", err)
        assert err <= TOL
    fac, fq, fv, fd = fs.factors(n, 1), fs.cotangent_factors(n, 2), fs.cotangent_factors(n, 3), fs.factors(n, 4)
    s = _sites(n)
    ref = field_ref.displace(field_ref.white_to_density(fs.field_numpy(fac), ps, p), p)
    _forward_case("white (%s) N %d" % (spectrum, n), p, fac, s, ref, kind="white", amp=amp)
    want = field_adj_ref.vjp(p, _cot(fq), _cot(fv), fs.field_numpy(fd), kind="white", ps=ps)
    _adjoint_case("white (%s) adjoint N %d" % (spectrum, n), p, s, want, fac_q=fq, fac_v=fv, fac_dens=fd, kind="white", amp=amp)


@pytest.mark.parametrize("n", [32, 64])
def test_sums_plt(zd, oracle, n):
    eig = oracle.synthetic_eigenmodes(128 if n == 32 else 48)  # the exact stride; interpolated, seam and wrap
    p = zd.make_params(n, boxsize=BOX, **PLT)
    fac, fq, fv, fd = fs.factors(n, 1), fs.cotangent_factors(n, 2), fs.cotangent_factors(n, 3), fs.factors(n, 4)
    s = _sites(n)
    _forward_case("PLT + rescale N %d" % n, p, fac, s, field_ref.displace(fs.field_numpy(fac), p, eig=eig, oracle=oracle), eig=eig)
    want = field_adj_ref.vjp(p, _cot(fq), _cot(fv), fs.field_numpy(fd), eig=eig, oracle=oracle)
    _adjoint_case("PLT + rescale adjoint N %d" % n, p, s, want, fac_q=fq, fac_v=fv, fac_dens=fd, eig=eig)


# ---- the eigenmode lookup --------------------------------------------------------------------------------------------------------
LOOKUPS = [(32, 24, "plain"), (32, 48, "plain"), (32, 128, "plain"), (32, 64, "plain"), (32, 24, "singular"), (64, 48, "plain"), (32, 64, "perpendicular")]


@pytest.mark.parametrize("n,eig_ppd,table", LOOKUPS, ids=["%d-table%d-%s" % c for c in LOOKUPS])
def test_lookup_against_the_oracle(oracle, n, eig_ppd, table):
    """every mode of the rows ky = 0 ... N/2 (the half space and more) but k = 0, whose direction 0/0 the zero rule never asks for.
    "perpendicular": the entries of the modes (1, 2, 0) and (-3, 0, 0) replaced by unit vectors at right angles to k, so that
    k^2 / (k.e) is a division by an exact zero and has to come out as 0"""
    import torch
    singular = table == "singular"
    eig = np.ascontiguousarray(oracle.synthetic_eigenmodes(eig_ppd, singular=singular), dtype=np.float64)
    if table == "perpendicular":
        st = eig_ppd // n
        eig[1 * st, 2 * st, 0, :3] = np.array([2.0, -1.0, 0.0]) / np.sqrt(5.0)
        eig[(n - 3) * st, 0, 0, :3] = np.array([0.0, 1.0, 0.0])
    L = oracle.lib()
    k = field_ref.wavenumbers(n)
    out = (C.c_double * 4)()
    want = np.zeros((n // 2 + 1, n, n, 4))
    for ky in range(n // 2 + 1):
        for iz, kz in enumerate(k):
            for ix, kx in enumerate(k):
                L.zdo_get_eigenmode(eig.ctypes.data, eig_ppd, int(kx), ky, int(kz), n, 1, out)
                want[ky, iz, ix] = out[:]
    kt = torch.from_numpy(k)
    got = fs.eigenmode_lookup(torch.from_numpy(eig), n, kt[None, None, :], torch.arange(n // 2 + 1)[:, None, None], kt[None, :, None]).numpy()
    got[0, 0, 0], want[0, 0, 0] = 0.0, 0.0
    assert np.isfinite(want).all() and np.isfinite(got).all()
    err = np.abs(got - want).max() / np.abs(want).max()
    zeros = int(np.sum((want[..., :3] == 0).all(axis=-1))) - 1
    print("N", n, "table", eig_ppd, "exact stride" if eig_ppd % n == 0 else "interpolated", table, "max|e| =",
          np.abs(want).max(), "error / max", err, "modes with k^2 / (k.e) set to 0:", zeros)
    assert err <= TOL
    assert np.array_equal((got[..., :3] == 0).all(axis=-1), (want[..., :3] == 0).all(axis=-1))
    assert zeros == (2 if table == "perpendicular" else 0)
    # the row form the sweep uses (two matrix products per row)
    modes = fs.Modes(oracle.make_params(n, qPLT=1), "cpu", eig=eig)
    rows = np.stack([modes.eig_row(ky).numpy() for ky in range(n // 2 + 1)]).transpose(0, 2, 3, 1)
    rows[0, 0, 0] = 0.0
    err_rows = np.abs(rows - want).max() / np.abs(want).max()
    print("the same by rows: error / max", err_rows)
    assert np.isfinite(rows).all() and err_rows <= TOL
    assert np.array_equal((rows[..., :3] == 0).all(axis=-1), (want[..., :3] == 0).all(axis=-1))
