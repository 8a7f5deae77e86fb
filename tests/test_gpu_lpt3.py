"""GPU: third-order displacements (ZD_q3LPT; definition in zeldovich_plt_amd/csrc/zd_kernels_lpt3.hip).

The reference has no third order, so the yardstick is the definition restated in numpy (tests/lpt3_ref.py, held to the equation of
motion in tests/test_lpt3.py) applied to ORACLE Zel'dovich records.  The third-order part of a run is compared on its own —
(3LPT displacement - 2LPT displacement) against psi3_ref, (3LPT velocity - 2LPT velocity) against f3 psi3_ref — to 1e-10 of
max|psi3_ref|, the project's parity bound applied to the small term; ZD_Pk_sigma is raised so that the term is at least 3 % of the
first order, and its transverse part 0.3 %, at every size of the table below (asserted on the reference).  Sizes numpy cannot reach
hang on the 64-point run through exact oversampling links (k_max = N/8: neither the cubic products nor S alias)."""
import os
import re
import subprocess

import numpy as np
import pytest

import lpt2_ref
import lpt3_ref
from conftest import ROOT, WMAP

pytestmark = pytest.mark.gpu

BOX = 720.0
SIGMA = 0.84  # 40 x the example's.  Measured at 0.42 on oracle records, max|psi3| / max|psi1| (transverse part alone): PPD 32 0.0115
              # (0.0012), 64 0.0488 (0.0033), 64 at k_cutoff 2 0.0137 (0.0011); both scale with sigma^2
FLOORS = {(32, 1.0), (64, 1.0), (64, 2.0)}  # the configurations whose ratios are asserted: >= 0.03, transverse >= 0.003
EXE = os.path.join(ROOT, "zeldovich_plt_amd", "csrc", "build", "zeldovich")
G = lpt3_ref.DEFAULTS


@pytest.fixture(scope="module")
def zd():
    import zeldovich_plt_amd.api as api
    return api


_REF = {}


def _reference(oracle, n, k_cutoff=1.0, fix=0):
    """oracle ZA records and the three unit-coefficient parts of psi3 of the numpy restatement, computed once per configuration"""
    key = (n, k_cutoff, fix)
    if key not in _REF:
        pk = oracle.pk_from_file(WMAP, BOX, Pk_sigma=SIGMA, fix_to_mean=fix)
        rec = oracle.run(oracle.make_params(n, k_cutoff=k_cutoff), pk)["records"]
        q = np.ascontiguousarray(rec["d"], dtype=np.float64)
        parts = lpt3_ref.third_order(q, BOX, lpt2_ref.alive_mask(n, BOX, k_cutoff))
        for part in parts:
            part.setflags(write=False)
        full, trans = lpt3_ref.combine(parts), G["g3c"] * parts[2]
        r = np.abs(full).max() / np.abs(q).max(), np.abs(trans).max() / np.abs(q).max()
        print("PPD", n, "k_cutoff", k_cutoff, "fix", fix, "reference max|psi3| / max|psi1| =", r[0], "transverse part", r[1])
        if fix == 0 and (n, k_cutoff) in FLOORS:
            assert r[0] >= 0.03 and r[1] >= 0.003, r
        _REF[key] = (rec, parts)
    return _REF[key]


def _ps(zd, fix=0):
    return zd.PowerSpectrum.from_file(WMAP, BOX, Pk_sigma=SIGMA, fix_to_mean=fix)


def _check_third_order(got3, got2, psi3_ref, f3, label):
    """the third-order part on its own, displacement and velocity; prints the figures before it asserts"""
    scale = np.abs(psi3_ref).max()
    assert scale > 0
    ed = np.abs((got3["d"] - got2["d"]) - psi3_ref).max() / scale
    ev = np.abs((got3["v"] - got2["v"]) - f3 * psi3_ref).max() / scale
    print(label, "max|psi3_ref| =", scale, "displacement error", ed, "velocity error", ev)
    assert np.array_equal(got3["ijk"], got2["ijk"]) and np.array_equal(got3["pad"], got2["pad"])
    assert ed <= 1e-10 and ev <= 1e-10, (label, ed, ev)


# ---- 1. every record against numpy ------------------------------------------------------------------------------------------
CASES = [(32, 1.0, 0, 0), (64, 1.0, 0, 0), (64, 2.0, 0, 0), (64, 1.0, 1, 0), (32, 1.0, 0, 2), (64, 1.0, 0, 2), (64, 1.0, 0, 4)]


@pytest.mark.parametrize("n,k_cutoff,fix,R", CASES, ids=["%d-kc%g-fix%d-R%d" % c for c in CASES])
def test_records_against_numpy(zd, oracle, n, k_cutoff, fix, R):
    """(64 at stream factor 4: z lines of 16 points, which only the final passes of the second and third order run)"""
    rec, parts = _reference(oracle, n, k_cutoff, fix)
    ps = _ps(zd, fix)
    kw = dict(k_cutoff=k_cutoff, q2LPT=1, stream_factor=R)
    two = zd.generate(zd.make_params(n, **kw), ps)["records"]
    got = zd.generate(zd.make_params(n, q3LPT=1, **kw), ps)
    assert got["stream_factor"] == max(R, 1) and sorted(got["planes_seen"]) == list(range(n))
    _check_third_order(got["records"], two, lpt3_ref.combine(parts), G["f3"], "PPD %d k_cutoff %g fix %d R %d" % (n, k_cutoff, fix, R))
    if R > 1:  # the same field whatever the stream factor
        one = zd.generate(zd.make_params(n, k_cutoff=k_cutoff, q2LPT=1, q3LPT=1, stream_factor=1), ps)["records"]
        for f in ("d", "v"):
            assert np.abs(got["records"][f] - one[f]).max() <= 1e-12 * np.abs(one[f]).max()
        assert np.array_equal(got["records"]["ijk"], one["ijk"])


def test_power_law_spectrum(zd, oracle):
    """the power-law forms of the generator (their own instantiations) against numpy"""
    n = 32
    kw = dict(Pk_sigma=2.0)
    pk = oracle.pk_from_powerlaw(-1.5, BOX, **kw)
    rec = oracle.run(oracle.make_params(n), pk)["records"]
    q = np.ascontiguousarray(rec["d"], dtype=np.float64)
    psi3_ref = lpt3_ref.combine(lpt3_ref.third_order(q, BOX, lpt2_ref.alive_mask(n, BOX)))
    print("power law: reference max|psi3| / max|psi1| =", np.abs(psi3_ref).max() / np.abs(q).max())
    ps = zd.PowerSpectrum.from_powerlaw(-1.5, BOX, **kw)
    two = zd.generate(zd.make_params(n, q2LPT=1), ps)["records"]
    got = zd.generate(zd.make_params(n, q2LPT=1, q3LPT=1), ps)["records"]
    _check_third_order(got, two, psi3_ref, G["f3"], "power law")


# ---- 2. the terms one by one, given coefficients ----------------------------------------------------------------------------
@pytest.mark.parametrize("terms", [4, 1, 2, 3])
def test_terms_against_their_parts(zd, oracle, terms):
    """ZD_3LPT_terms = 4 is the transverse term alone, to 1e-10 of ITS maximum: a sign or index error in either cross product shows here"""
    n = 64
    rec, parts = _reference(oracle, n)
    ps = _ps(zd)
    two = zd.generate(zd.make_params(n, q2LPT=1), ps)["records"]
    got = zd.generate(zd.make_params(n, q2LPT=1, q3LPT=1, lpt3_terms=terms), ps)["records"]
    _check_third_order(got, two, lpt3_ref.combine(parts, terms=terms), G["f3"], "terms %d" % terms)


def test_given_coefficients(zd, oracle):
    n = 64
    rec, parts = _reference(oracle, n)
    ps = _ps(zd)
    g = dict(lpt3_g3a=-0.29, lpt3_g3b=0.51, lpt3_g3c=-0.17, lpt3_f3=2.6)
    want = lpt3_ref.combine(parts, g3a=g["lpt3_g3a"], g3b=g["lpt3_g3b"], g3c=g["lpt3_g3c"])
    two = zd.generate(zd.make_params(n, q2LPT=1), ps)["records"]
    got = zd.generate(zd.make_params(n, q2LPT=1, q3LPT=1, **g), ps)["records"]
    _check_third_order(got, two, want, g["lpt3_f3"], "given coefficients")
    # another background: the first-order field is the same one, the second order has that background's coefficients in both runs
    two = zd.generate(zd.make_params(n, f_cluster=0.9, q2LPT=1), ps)["records"]
    got = zd.generate(zd.make_params(n, f_cluster=0.9, q2LPT=1, q3LPT=1, **g), ps)["records"]
    _check_third_order(got, two, want, g["lpt3_f3"], "given coefficients at f_cluster 0.9")
    # a term that is out needs no coefficient there
    g2 = dict(lpt3_g3c=0.2, lpt3_f3=2.7, lpt3_terms=4)
    got = zd.generate(zd.make_params(n, f_cluster=0.9, q2LPT=1, q3LPT=1, **g2), ps)["records"]
    _check_third_order(got, two, 0.2 * parts[2], 2.7, "transverse term at f_cluster 0.9")


@pytest.mark.parametrize("fmt", ["RVZel", "Zeldovich", "ZelSimple"])
def test_other_record_formats(zd, fmt):
    """the same fields in the other three ICFormats (float32 fields to 1e-6 as everywhere)"""
    n, ps = 32, _ps(zd)
    want = zd.generate(zd.make_params(n, q2LPT=1, q3LPT=1), ps)["records"]
    got = zd.generate(zd.make_params(n, q2LPT=1, q3LPT=1, icformat=fmt), ps)["records"]
    dt = zd.RECORD_DTYPES[fmt]
    if "ijk" in dt.names:
        assert np.array_equal(got["ijk"], want["ijk"])
    tol = 1e-6 if dt["d"].base == np.float32 else 0.0
    assert np.abs(got["d"] - want["d"]).max() <= tol * np.abs(want["d"]).max()
    if "v" in dt.names:
        assert np.abs(got["v"] - want["v"]).max() <= tol * np.abs(want["v"]).max()


# ---- 3. one mode: no third order --------------------------------------------------------------------------------------------
def _one_plane(zd, ps, n, z, **kw):
    """the records of plane z of a run that delivers only that plane (ZD_qoneslab)"""
    got = {}

    def take(zz, plane):
        got[zz] = plane.copy()

    info = zd.generate_planes(zd.make_params(n, qoneslab=z, **kw), ps, take)
    assert list(got) == [z] and info["planes"] == 1
    return got[z]


@pytest.mark.parametrize("n", [64, 1024])
def test_one_mode_has_no_third_order(zd, n):
    ps = _ps(zd)
    kw = dict(qonemode=1, one_mode=(3, 5, -2))
    za = _one_plane(zd, ps, n, 7, **kw)
    got = _one_plane(zd, ps, n, 7, q2LPT=1, q3LPT=1, **kw)
    scale = np.abs(za["d"]).max()
    assert scale > 0 and np.array_equal(got["ijk"], za["ijk"])
    print("PPD", n, "one mode:", np.abs(got["d"] - za["d"]).max() / scale, np.abs(got["v"] - za["v"]).max() / scale)
    assert np.abs(got["d"] - za["d"]).max() <= 1e-12 * scale
    assert np.abs(got["v"] - za["v"]).max() <= 1e-12 * scale


# ---- 4. oversampling chain --------------------------------------------------------------------------------------------------
_PLANES = {}


def _chain_plane(zd, n, order):
    """plane z = 5 n / 64 of the PPD = n run with ZD_k_cutoff = n / 16 (the modes of PPD = 64 at ZD_k_cutoff = 4); order 1, 2 or 3"""
    if (n, order) not in _PLANES:
        kw = dict(q2LPT=int(order >= 2), q3LPT=int(order >= 3))
        _PLANES[(n, order)] = _one_plane(zd, _ps(zd), n, 5 * n // 64, k_cutoff=n / 16.0, **kw)
    return _PLANES[(n, order)]


def test_chain_anchor_against_numpy(zd, oracle):
    """PPD = 64 at ZD_k_cutoff = 4, the lower end of the chain, plane 5 through ZD_qoneslab, against numpy"""
    rec, parts = _reference(oracle, 64, 4.0, 0)
    _check_third_order(_chain_plane(zd, 64, 3), _chain_plane(zd, 64, 2), lpt3_ref.combine(parts)[5], G["f3"], "chain anchor, plane 5")


@pytest.mark.parametrize("n", [64, 128, 256, 512])
def test_oversampling_chain(zd, n):
    """PPD = 2n at twice the ZD_k_cutoff equals PPD = n at the shared lattice sites: k_max = N/8 < N/4, so neither the cubic products
    nor S alias in either.  (The only test at the 512 and 1024 line lengths.)"""
    lo, lo2, lo1, hi = _chain_plane(zd, n, 3), _chain_plane(zd, n, 2), _chain_plane(zd, n, 1), _chain_plane(zd, 2 * n, 3)[::2, ::2]
    scale = np.abs(lo["d"] - lo2["d"]).max()  # max|psi3| of the coarser run's plane
    assert scale > 0
    assert np.array_equal(2 * lo["ijk"].astype(np.int64), hi["ijk"].astype(np.int64))
    ed, ev = np.abs(hi["d"] - lo["d"]).max() / scale, np.abs(hi["v"] - lo["v"]).max() / scale
    print("PPD", n, "<->", 2 * n, "plane max|psi3| / max|psi1| =", scale / np.abs(lo1["d"]).max(), "displacement", ed, "velocity", ev)
    assert ed <= 1e-10 and ev <= 1e-10
    for order in (1, 2, 3):
        _PLANES.pop((n, order), None)


# ---- 5. command line, refusals ----------------------------------------------------------------------------------------------
PAR = """BoxSize = 720
CPD = 5
ICFormat = "RVdoubleZel"
InitialConditionsDirectory = "%(out)s"
InitialRedshift = 49
NP = %(np)d
ZD_NumBlock = 2
ZD_Pk_filename = "%(pk)s"
ZD_Pk_norm = 8.0
ZD_Pk_scale = 1.0
ZD_Pk_sigma = %(sigma).17g
ZD_Pk_smooth = 0.0
ZD_Seed = 12346
ZD_Version = 2
"""
ON = "ZD_q2LPT = 1\nZD_q3LPT = 1\n"
CLI_REFUSALS = [
    ("ZD_q3LPT = 1\n", 32, "ZD_q3LPT = 1 needs ZD_q2LPT = 1"),
    (ON + "ZD_2LPT_dealias = 1\n", 32, "ZD_2LPT_dealias = 1"),
    (ON, 2048, "PPD <= 1024"),
    (ON + "ZD_f_cluster = 0.9\n", 32, "ZD_f_cluster != 1"),
    (ON + "ZD_f_cluster = 0.9\nZD_3LPT_D3a = -0.3\nZD_3LPT_D3b = 0.4\nZD_3LPT_D3c = 0.1\n", 32, "ZD_f_cluster != 1"),
    (ON + "ZD_3LPT_terms = 8\n", 32, "ZD_3LPT_terms"),
    ("ZD_q2LPT = 1\nZD_q3LPT = 2\n", 32, "must be 0 or 1"),
]


def test_cli(zd, tmp_path):
    n, cpd = 32, 5
    out = tmp_path / "ic"
    out.mkdir()
    par = tmp_path / "t.par"
    base = dict(out=out, pk=WMAP, sigma=SIGMA, np=n ** 3)
    par.write_text(PAR % base + ON)
    r = subprocess.run([EXE, str(par)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    want = zd.generate(zd.make_params(n, q2LPT=1, q3LPT=1, cpd=cpd), _ps(zd))["records"]
    dt = zd.RECORD_DTYPES["RVdoubleZel"]
    for f in sorted(set(z * cpd // n for z in range(n))):
        zs = [z for z in range(n) if z * cpd // n == f]
        got = np.fromfile(out / ("ic_%d" % f), dtype=dt).reshape(len(zs), n, n)
        assert np.array_equal(got, want[zs])
    # the same file with the coefficients given: the values of the defaults, the same records to rounding
    par.write_text(PAR % base + ON + "ZD_3LPT_D3a = -0.33333333333333331\nZD_3LPT_D3b = 0.47619047619047616\n"
                   "ZD_3LPT_D3c = 0.14285714285714285\nZD_3LPT_f3 = 3.0\nZD_3LPT_terms = 7\n")
    r = subprocess.run([EXE, str(par)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(out / "ic_0", dtype=dt).reshape(-1, n, n)
    for f in ("d", "v"):
        assert np.abs(got[f] - want[:got.shape[0]][f]).max() <= 1e-14 * np.abs(want[f]).max()
    # every refusal: one line that names ZD_q3LPT, exit status 1
    for extra, ppd, word in CLI_REFUSALS:
        par.write_text(PAR % dict(base, np=ppd ** 3) + extra)
        r = subprocess.run([EXE, str(par)], capture_output=True, text=True)
        assert r.returncode == 1, (extra, r.stderr)
        lines = [ln for ln in r.stderr.splitlines() if "ZD_q3LPT" in ln]
        assert len(lines) == 1 and lines[0].startswith("zeldovich_hip: ZD_q3LPT") and word in lines[0], (extra, r.stderr)


def test_refusals_through_the_api(zd, capfd):
    ps = _ps(zd)
    with pytest.raises(RuntimeError):
        zd.measure_power(zd.make_params(32, q2LPT=1, q3LPT=1), ps)
    assert "ZD_q2LPT" in capfd.readouterr().err
    plan = zd.Plan(zd.make_params(32, q2LPT=1, q3LPT=1), ps)
    try:
        assert plan.narray == 4 and plan.store_mode == "reference" and plan.passes == 1
        with pytest.raises(RuntimeError):
            plan.measure_power()
        with pytest.raises(RuntimeError):
            plan.direct_sum([(0, 0, 0)])
    finally:
        plan.close()
    for kw in (dict(q2LPT=0), dict(q2LPT=1, lpt2_dealias=1), dict(q2LPT=1, f_cluster=0.9), dict(q2LPT=1, lpt3_terms=9)):
        with pytest.raises(RuntimeError):
            zd.generate(zd.make_params(32, q3LPT=1, **kw), ps)
        assert "ZD_q3LPT" in capfd.readouterr().err, kw
        with pytest.raises(RuntimeError):
            zd.Plan(zd.make_params(32, q3LPT=1, **kw), ps)
        assert "ZD_q3LPT" in capfd.readouterr().err, kw
    with pytest.raises(RuntimeError):
        zd.generate(zd.make_params(32, q2LPT=1, q3LPT=1, f_NL=50.0), ps)
    assert "ZD_q2LPT = 1" in capfd.readouterr().err


# ---- 6. launch sites (after the tests above) --------------------------------------------------------------------------------
def test_every_launch_site_was_launched(zd):
    """every instantiation of the new launchers' tables — the x lines of the third-order round in both directions at every length, the
    generator's pair and final forms with a tabulated and a power-law spectrum, the pointwise kernel — has been launched by the tests
    of this file"""
    rep = zd.dispatch_report()
    names = [name for (name, _l), cnt in rep.items() if cnt > 0]
    txt = open(os.path.join(ROOT, "zeldovich_plt_amd", "csrc", "zd_kernels_lpt3.hip")).read()
    for launcher, kernel in (("launch_lpt3_xpair", "k_xlpt3"), ("launch_lpt3_xfwd", "k_xfwd3")):
        table = re.search(r"int %s\(.*?#undef LCASE" % launcher, txt, re.S).group(0)
        sizes = re.findall(r"LCASE\((\d+), (\d+), (\d+)\)", table)
        assert len(sizes) == 6
        for N, E, ROWS in sizes:
            want = "N = %s, E = %s, ROWS = %s" % (N, E, ROWS)
            assert any(launcher + "_t" in nm and want in nm for nm in names), "%s<%s> never launched" % (kernel, want)
    table = re.search(r"int launch_gen_lpt3\(.*?#undef GCASE", txt, re.S).group(0)
    njs = re.findall(r"GCASE\((\d+)\)", table)
    assert sorted(njs) == ["2", "7"]
    for nj in njs:
        for plaw in ("false", "true"):
            want = "NJ = %s, PLAW = %s" % (nj, plaw)
            assert any("launch_gen_lpt3_t" in nm and want in nm for nm in names), "k_gen_lpt3<%s> never launched" % want
    assert any("launch_lpt3_point" in nm for nm in names), "k_lpt3_point never launched"
