"""GPU: second-order displacements (ZD_q2LPT; definition in zeldovich_plt_amd/csrc/zd_kernels_lpt2.hip).

The reference has no second order, so the yardstick is the definition restated in numpy (tests/lpt2_ref.py, pinned by a closed form
in tests/test_lpt2.py) applied to ORACLE Zel'dovich records.  The second-order part of a run is compared on its own —
(2LPT displacement - ZA displacement) against psi2_ref, (2LPT velocity - alpha ZA displacement) against f2 psi2_ref — to
1e-10 of max|psi2_ref|, the project's parity bound applied to the small term; ZD_Pk_sigma is raised so that the term is at least
5 % of the first order at every size used (asserted on the reference).  Sizes numpy cannot reach hang on the 128-point run through
exact oversampling links (nothing aliases at ZD_k_cutoff >= 2)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lpt2_ref
from conftest import ROOT, WMAP

pytestmark = pytest.mark.gpu

BOX = 720.0
SIGMA = 0.42  # 20 x the example's: max|psi2| / max|psi1| = 0.06 (PPD 32) ... 0.17 (PPD 128) on the CPU reference
EXE = os.path.join(ROOT, "zeldovich_plt_amd", "csrc", "build", "zeldovich")


@pytest.fixture(scope="module")
def zd():
    import zeldovich_plt_amd.api as api
    return api


_REF = {}


def _reference(oracle, n, k_cutoff=1.0, fix=0, f_cluster=1.0):
    """oracle ZA records and psi2 / gamma-free pieces of the numpy restatement, computed once per configuration"""
    key = (n, k_cutoff, fix, f_cluster)
    if key not in _REF:
        pk = oracle.pk_from_file(WMAP, BOX, Pk_sigma=SIGMA, fix_to_mean=fix)
        rec = oracle.run(oracle.make_params(n, k_cutoff=k_cutoff, f_cluster=f_cluster), pk)["records"]
        q = np.ascontiguousarray(rec["d"], dtype=np.float64)
        psi2 = lpt2_ref.second_order(q, BOX, lpt2_ref.alive_mask(n, BOX, k_cutoff), lpt2_ratio=-1.0)  # gamma = 1: scaled by the caller
        psi2.setflags(write=False)
        _REF[key] = (rec, psi2)
    return _REF[key]


def _ps(zd, fix=0):
    return zd.PowerSpectrum.from_file(WMAP, BOX, Pk_sigma=SIGMA, fix_to_mean=fix)


def _check_second_order(got2, gotza, psi2_ref, alpha, f2, label):
    """the second-order part on its own, displacement and velocity; prints the figures before it asserts"""
    scale = np.abs(psi2_ref).max()
    ed = np.abs((got2["d"] - gotza["d"]) - psi2_ref).max() / scale
    ev = np.abs((got2["v"] - alpha * gotza["d"]) - f2 * psi2_ref).max() / scale
    print(label, "max|psi2_ref| =", scale, "displacement error", ed, "velocity error", ev)
    assert np.array_equal(got2["ijk"], gotza["ijk"]) and np.array_equal(got2["pad"], gotza["pad"])
    assert ed <= 1e-10 and ev <= 1e-10, (label, ed, ev)


# ---- 1. every record against numpy ------------------------------------------------------------------------------------------
CASES = [(32, 1.0, 0, 0), (64, 1.0, 0, 0), (128, 1.0, 0, 0), (64, 2.0, 0, 0), (64, 1.0, 1, 0), (128, 2.0, 0, 0), (64, 1.0, 0, 2), (64, 1.0, 0, 4),
         (128, 1.0, 0, 4), (32, 1.0, 0, 2)]


@pytest.mark.parametrize("n,k_cutoff,fix,R", CASES, ids=["%d-kc%g-fix%d-R%d" % c for c in CASES])
def test_records_against_numpy(zd, oracle, n, k_cutoff, fix, R):
    """(64 at stream factor 4: z lines of 16 points, which only the second-order final pass runs)"""
    rec, psi2_unit = _reference(oracle, n, k_cutoff, fix)
    psi2_ref = (3.0 / 7.0) * psi2_unit  # gamma = -lpt2_ratio = 3/7 at f_cluster = 1
    ratio = np.abs(psi2_ref).max() / np.abs(rec["d"]).max()
    print("PPD", n, "reference max|psi2| / max|psi1| =", ratio)
    assert ratio >= 0.05
    ps = _ps(zd, fix)
    za = zd.generate(zd.make_params(n, k_cutoff=k_cutoff), ps)["records"]
    assert np.abs(za["d"] - rec["d"]).max() <= 1e-10 * np.abs(rec["d"]).max()  # (the first order itself, as everywhere)
    got = zd.generate(zd.make_params(n, k_cutoff=k_cutoff, q2LPT=1, stream_factor=R), ps)
    assert got["stream_factor"] == max(R, 1) and sorted(got["planes_seen"]) == list(range(n))
    _check_second_order(got["records"], za, psi2_ref, 1.0, 2.0, "PPD %d k_cutoff %g fix %d R %d" % (n, k_cutoff, fix, R))
    if R > 1:  # the same field whatever the stream factor
        one = zd.generate(zd.make_params(n, k_cutoff=k_cutoff, q2LPT=1, stream_factor=1), ps)["records"]
        for f in ("d", "v"):
            assert np.abs(got["records"][f] - one[f]).max() <= 1e-12 * np.abs(one[f]).max()
        assert np.array_equal(got["records"]["ijk"], one["ijk"])


@pytest.mark.parametrize("fmt", ["RVZel", "Zeldovich", "ZelSimple"])
def test_other_record_formats(zd, fmt):
    """the same fields in the other three ICFormats (float32 fields to 1e-6 as everywhere)"""
    n, ps = 32, _ps(zd)
    want = zd.generate(zd.make_params(n, q2LPT=1), ps)["records"]
    got = zd.generate(zd.make_params(n, q2LPT=1, icformat=fmt), ps)["records"]
    dt = zd.RECORD_DTYPES[fmt]
    if "ijk" in dt.names:
        assert np.array_equal(got["ijk"], want["ijk"])
    tol = 1e-6 if dt["d"].base == np.float32 else 0.0
    assert np.abs(got["d"] - want["d"]).max() <= tol * np.abs(want["d"]).max()
    if "v" in dt.names:
        assert np.abs(got["v"] - want["v"]).max() <= tol * np.abs(want["v"]).max()


# ---- 2. non-default coefficients --------------------------------------------------------------------------------------------
def test_given_coefficients_scale_the_two_parts(zd, oracle):
    n, fcl = 64, 0.9
    rec, psi2_unit = _reference(oracle, n, 1.0, 0, fcl)
    alpha = (np.sqrt(1 + 24 * fcl) - 1) / 4
    ps = _ps(zd)
    za = zd.generate(zd.make_params(n, f_cluster=fcl), ps)["records"]
    assert np.abs(za["v"] - alpha * za["d"]).max() <= 1e-15 * np.abs(za["d"]).max()
    got = zd.generate(zd.make_params(n, f_cluster=fcl, q2LPT=1, lpt2_ratio=-0.5, lpt2_f2=1.7), ps)["records"]
    _check_second_order(got, za, 0.5 * psi2_unit, alpha, 1.7, "given coefficients")
    # and the defaults of that background
    _, ratio, f2 = lpt2_ref.default_coefficients(fcl)
    got = zd.generate(zd.make_params(n, f_cluster=fcl, q2LPT=1), ps)["records"]
    _check_second_order(got, za, -ratio * psi2_unit, alpha, f2, "defaults at f_cluster 0.9")


# ---- 3. one mode: S = 0 -----------------------------------------------------------------------------------------------------
def _one_plane(zd, ps, n, z, **kw):
    """the records of plane z of a run that delivers only that plane (ZD_qoneslab)"""
    got = {}

    def take(zz, plane):
        got[zz] = plane.copy()

    info = zd.generate_planes(zd.make_params(n, qoneslab=z, **kw), ps, take)
    assert list(got) == [z] and info["planes"] == 1
    return got[z]


@pytest.mark.parametrize("n", [64, 1024])
def test_one_mode_has_no_second_order(zd, n):
    ps = _ps(zd)
    kw = dict(qonemode=1, one_mode=(3, 5, -2))
    za = _one_plane(zd, ps, n, 7, **kw)
    got = _one_plane(zd, ps, n, 7, q2LPT=1, **kw)
    scale = np.abs(za["d"]).max()
    assert scale > 0 and np.array_equal(got["ijk"], za["ijk"])
    print("PPD", n, "one mode:", np.abs(got["d"] - za["d"]).max() / scale, np.abs(got["v"] - za["v"]).max() / scale)
    assert np.abs(got["d"] - za["d"]).max() <= 1e-12 * scale
    assert np.abs(got["v"] - za["v"]).max() <= 1e-12 * scale


# ---- 4. oversampling chain --------------------------------------------------------------------------------------------------
_PLANES = {}


def _chain_plane(zd, n, q2):
    """plane z = 5 n / 128 of the PPD = n run with ZD_k_cutoff = n / 64 (the modes of PPD = 128 at ZD_k_cutoff = 2)"""
    if (n, q2) not in _PLANES:
        _PLANES[(n, q2)] = _one_plane(zd, _ps(zd), n, 5 * n // 128, k_cutoff=n / 64.0, q2LPT=q2)
    return _PLANES[(n, q2)]


def test_chain_anchor_against_numpy(zd, oracle):
    """PPD = 128 at ZD_k_cutoff = 2, the lower end of the chain, plane 5 through ZD_qoneslab, against numpy"""
    rec, psi2_unit = _reference(oracle, 128, 2.0, 0)
    psi2_ref = (3.0 / 7.0) * psi2_unit[5]
    _check_second_order(_chain_plane(zd, 128, 1), _chain_plane(zd, 128, 0), psi2_ref, 1.0, 2.0, "chain anchor, plane 5")


@pytest.mark.parametrize("n", [128, 256, 512, 1024])
def test_oversampling_chain(zd, n):
    """PPD = 2n at twice the ZD_k_cutoff equals PPD = n at the shared lattice sites: k_max <= N/3, so the source aliases in neither"""
    lo, lo_za, hi = _chain_plane(zd, n, 1), _chain_plane(zd, n, 0), _chain_plane(zd, 2 * n, 1)[::2, ::2]
    scale = np.abs(lo["d"] - lo_za["d"]).max()  # max|psi2| of the coarser run's plane
    assert scale > 0
    assert np.array_equal(2 * lo["ijk"].astype(np.int64), hi["ijk"].astype(np.int64))
    ed, ev = np.abs(hi["d"] - lo["d"]).max() / scale, np.abs(hi["v"] - lo["v"]).max() / scale
    print("PPD", n, "<->", 2 * n, "max|psi2| =", scale, "displacement", ed, "velocity", ev)
    assert ed <= 1e-10 and ev <= 1e-10
    _PLANES.pop((n, 1), None)
    _PLANES.pop((n, 0), None)


# ---- 5. command line, refusals ----------------------------------------------------------------------------------------------
PAR = """BoxSize = 720
CPD = 5
ICFormat = "RVdoubleZel"
InitialConditionsDirectory = "%(out)s"
InitialRedshift = 49
NP = 32768
ZD_NumBlock = 2
ZD_Pk_filename = "%(pk)s"
ZD_Pk_norm = 8.0
ZD_Pk_scale = 1.0
ZD_Pk_sigma = %(sigma).17g
ZD_Pk_smooth = 0.0
ZD_Seed = 12346
ZD_Version = 2
ZD_q2LPT = 1
"""


def test_cli(zd, oracle, tmp_path):
    n, cpd = 32, 5
    out = tmp_path / "ic"
    out.mkdir()
    par = tmp_path / "t.par"
    par.write_text(PAR % dict(out=out, pk=WMAP, sigma=SIGMA))
    r = subprocess.run([EXE, str(par)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    want = zd.generate(zd.make_params(n, q2LPT=1, cpd=cpd), _ps(zd))["records"]
    dt = zd.RECORD_DTYPES["RVdoubleZel"]
    for f in sorted(set(z * cpd // n for z in range(n))):
        zs = [z for z in range(n) if z * cpd // n == f]
        got = np.fromfile(out / ("ic_%d" % f), dtype=dt).reshape(len(zs), n, n)
        assert np.array_equal(got, want[zs])
    # the same file with the coefficients given: the values of the defaults, the same records to rounding
    par.write_text(PAR % dict(out=out, pk=WMAP, sigma=SIGMA) + "ZD_2LPT_D2 = -0.42857142857142855\nZD_2LPT_f2 = 2.0\n")
    r = subprocess.run([EXE, str(par)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(out / "ic_0", dtype=dt).reshape(-1, n, n)
    assert np.abs(got["d"] - want[:got.shape[0]]["d"]).max() <= 1e-14 * np.abs(want["d"]).max()
    # ... and with PLT: refused with one line, exit status 1
    eig = oracle.synthetic_eigenmodes(32)
    eigfile = tmp_path / "eigmodes32"
    with open(eigfile, "wb") as f:
        np.array([32], dtype=np.int32).tofile(f)
        eig.tofile(f)
    par.write_text(PAR % dict(out=out, pk=WMAP, sigma=SIGMA) + 'ZD_qPLT = 1\nZD_PLT_filename = "%s"\n' % eigfile)
    r = subprocess.run([EXE, str(par)], capture_output=True, text=True)
    assert r.returncode == 1
    lines = [ln for ln in r.stderr.splitlines() if "ZD_q2LPT" in ln]
    assert lines == ["zeldovich_hip: ZD_q2LPT = 1 is not supported together with ZD_qPLT"], r.stderr


def test_refusals_through_the_api(zd, capfd):
    ps = _ps(zd)
    with pytest.raises(RuntimeError):
        zd.measure_power(zd.make_params(32, q2LPT=1), ps)
    assert "ZD_q2LPT" in capfd.readouterr().err
    plan = zd.Plan(zd.make_params(32, q2LPT=1), ps)
    try:
        assert plan.narray == 4 and plan.store_mode == "reference" and plan.passes == 1
        with pytest.raises(RuntimeError):
            plan.measure_power()
    finally:
        plan.close()
    for kw in (dict(f_NL=50.0), dict(qdensity=1), dict(version=1), dict(ngpu=2), dict(corner_modes=1, k_cutoff=2.0)):
        with pytest.raises(RuntimeError):
            zd.generate(zd.make_params(32, q2LPT=1, **kw), ps)
        assert "ZD_q2LPT = 1" in capfd.readouterr().err, kw
    with pytest.raises(RuntimeError):
        zd.Plan(zd.make_params(64, q2LPT=1), ps, rank=0, nranks=2)
    with pytest.raises(RuntimeError):
        zd.generate(zd.make_params(96, q2LPT=1), ps)


def test_power_law_spectrum(zd, oracle):
    """the power-law form of the generator (its own instantiation) against numpy"""
    n = 32
    kw = dict(Pk_sigma=1.0)
    pk = oracle.pk_from_powerlaw(-1.5, BOX, **kw)
    rec = oracle.run(oracle.make_params(n), pk)["records"]
    psi2_ref = lpt2_ref.second_order(np.ascontiguousarray(rec["d"], dtype=np.float64), BOX, lpt2_ref.alive_mask(n, BOX))
    assert np.abs(psi2_ref).max() >= 0.05 * np.abs(rec["d"]).max()
    ps = zd.PowerSpectrum.from_powerlaw(-1.5, BOX, **kw)
    za = zd.generate(zd.make_params(n), ps)["records"]
    got = zd.generate(zd.make_params(n, q2LPT=1), ps)["records"]
    _check_second_order(got, za, psi2_ref, 1.0, 2.0, "power law")


# ---- 6. launch sites (after the tests above) --------------------------------------------------------------------------------
def test_every_launch_site_was_launched(zd):
    """every instantiation of the new launchers' tables — the x lines of the second-order round at every length, the generator's
    gradient and final forms with a tabulated and a power-law spectrum — has been launched by the tests of this file"""
    rep = zd.dispatch_report()
    names = [name for (name, _l), cnt in rep.items() if cnt > 0]
    txt = open(os.path.join(ROOT, "zeldovich_plt_amd", "csrc", "zd_kernels_lpt2.hip")).read()
    table = re.search(r"int launch_lpt2_xsrc\(.*?#undef LCASE", txt, re.S).group(0)
    sizes = re.findall(r"LCASE\((\d+), (\d+), (\d+)\)", table)
    assert len(sizes) == 7
    for N, E, ROWS in sizes:
        want = "N = %s, E = %s, ROWS = %s" % (N, E, ROWS)
        assert any("launch_lpt2_xsrc_t" in nm and want in nm for nm in names), "k_xlpt2<%s> never launched" % want
    for nj in (2, 7):
        for plaw in ("false", "true"):
            want = "NJ = %d, PLAW = %s" % (nj, plaw)
            assert any("launch_gen_lpt2_t" in nm and want in nm for nm in names), "k_gen_lpt2<%s> never launched" % want
