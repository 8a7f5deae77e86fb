"""GPU: the de-aliased second-order source (ZD_2LPT_dealias; step 2' of the definition in zeldovich_plt_amd/csrc/zd_kernels_lpt2.hip).

The yardstick is that of tests/test_gpu_lpt2.py: the definition restated in numpy (tests/lpt2_dealias_ref.py, pinned by a closed form
in tests/test_lpt2_dealias.py) applied to ORACLE Zel'dovich records, the second-order part of a run compared on its own —
(2LPT displacement - ZA displacement) against psi2_ref, (2LPT velocity - alpha ZA displacement) against f2 psi2_ref — to 1e-10 of
max|psi2_ref|.  At ZD_k_cutoff = 1 the reference of the plain definition differs from it by 10-20 % of max|psi2| (asserted on the
references), so a build that runs the plain round cannot pass.  Sizes numpy cannot reach hang on an exact link to the existing code:
the de-aliased run at N, ZD_k_cutoff = 1 is the plain ZD_q2LPT run at 2 N, ZD_k_cutoff = 2 (where nothing aliases) at the shared sites.

Ragged tiles: the forward y transform of the round covers the columns -N/2 < kx < 0 in one launch of N/2 - 1 columns, which no tile
width divides — every case here has that ragged last tile (15 of 16 columns at PPD 32, 31 = 16 + 15 at 64, ...)."""
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import lpt2_dealias_ref
import lpt2_ref
from conftest import GOLDEN, ROOT, WMAP

pytestmark = pytest.mark.gpu

BOX = 720.0
SIGMA = 0.42
EXE = os.path.join(ROOT, "zeldovich_plt_amd", "csrc", "build", "zeldovich")


@pytest.fixture(scope="module")
def zd():
    import zeldovich_plt_amd.api as api
    return api


_REF = {}


def _reference(oracle, n, k_cutoff=1.0, fix=0, f_cluster=1.0):
    """oracle ZA records, psi2 of the de-aliased and of the plain restatement at gamma = 1; computed once per configuration"""
    key = (n, k_cutoff, fix, f_cluster)
    if key not in _REF:
        pk = oracle.pk_from_file(WMAP, BOX, Pk_sigma=SIGMA, fix_to_mean=fix)
        rec = oracle.run(oracle.make_params(n, k_cutoff=k_cutoff, f_cluster=f_cluster), pk)["records"]
        q = np.ascontiguousarray(rec["d"], dtype=np.float64)
        mask = lpt2_ref.alive_mask(n, BOX, k_cutoff)
        psi2 = lpt2_dealias_ref.second_order(q, BOX, mask, lpt2_ratio=-1.0)
        plain = lpt2_ref.second_order(q, BOX, mask, lpt2_ratio=-1.0)
        psi2.setflags(write=False)
        plain.setflags(write=False)
        _REF[key] = (rec, psi2, plain)
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
CASES = [(32, 0, 1), (64, 0, 1), (128, 0, 1), (64, 0, 2), (64, 0, 4), (128, 0, 4), (64, 1, 1)]


@pytest.mark.parametrize("n,fix,R", CASES, ids=["%d-fix%d-R%d" % c for c in CASES])
def test_records_against_numpy(zd, oracle, n, fix, R):
    """lattices of 48, 96 and 192 points (Q = 3 lines of 16, 32 and 64 x 3); stream factors 1, 2, 4 of the final pass"""
    rec, psi2_unit, plain_unit = _reference(oracle, n, 1.0, fix)
    psi2_ref = (3.0 / 7.0) * psi2_unit
    apart = np.abs(plain_unit - psi2_unit).max() / np.abs(psi2_unit).max()
    ratio = np.abs(psi2_ref).max() / np.abs(rec["d"]).max()
    print("PPD", n, "references: max|psi2_plain - psi2_dealiased| / max|psi2| =", apart, " max|psi2| / max|psi1| =", ratio)
    assert apart >= 0.05 and ratio >= 0.05
    ps = _ps(zd, fix)
    za = zd.generate(zd.make_params(n), ps)["records"]
    assert np.abs(za["d"] - rec["d"]).max() <= 1e-10 * np.abs(rec["d"]).max()
    got = zd.generate(zd.make_params(n, q2LPT=1, lpt2_dealias=1, stream_factor=R), ps)
    assert got["stream_factor"] == R and sorted(got["planes_seen"]) == list(range(n))
    _check_second_order(got["records"], za, psi2_ref, 1.0, 2.0, "PPD %d fix %d R %d" % (n, fix, R))


# ---- 2. no aliasing, no change ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k_cutoff", [2.0, 1.5])
def test_no_aliasing_no_change(zd, k_cutoff):
    n, ps = 64, _ps(zd)
    za = zd.generate(zd.make_params(n, k_cutoff=k_cutoff), ps)["records"]
    plain = zd.generate(zd.make_params(n, k_cutoff=k_cutoff, q2LPT=1), ps)["records"]
    got = zd.generate(zd.make_params(n, k_cutoff=k_cutoff, q2LPT=1, lpt2_dealias=1), ps)["records"]
    scale = np.abs(plain["d"] - za["d"]).max()
    ed, ev = np.abs(got["d"] - plain["d"]).max() / scale, np.abs(got["v"] - plain["v"]).max() / scale
    print("k_cutoff", k_cutoff, "max|psi2| =", scale, "de-aliased against plain: displacement", ed, "velocity", ev)
    assert scale > 0 and ed <= 1e-10 and ev <= 1e-10
    assert np.array_equal(got["ijk"], plain["ijk"])


# ---- 3. the link to the existing code ---------------------------------------------------------------------------------------
def _one_plane(zd, ps, n, z, **kw):
    """the records of plane z of a run that delivers only that plane (ZD_qoneslab)"""
    got = {}

    def take(zz, plane):
        got[zz] = plane.copy()

    info = zd.generate_planes(zd.make_params(n, qoneslab=z, **kw), ps, take)
    assert list(got) == [z] and info["planes"] == 1
    return got[z]


@pytest.mark.parametrize("n", [64, 256, 1024])
def test_link_to_the_plain_round_at_twice_the_size(zd, n):
    """de-aliased at N, ZD_k_cutoff = 1 == plain at 2 N, ZD_k_cutoff = 2, at the sites [::2, ::2] of plane 2 z (1024: the lattice of
    1536 points, the (512, 3) transforms — the largest round that fits)"""
    ps, z = _ps(zd), 5 * n // 64
    lo_za = _one_plane(zd, ps, n, z)
    lo = _one_plane(zd, ps, n, z, q2LPT=1, lpt2_dealias=1)
    hi = _one_plane(zd, ps, 2 * n, 2 * z, k_cutoff=2.0, q2LPT=1)[::2, ::2]
    scale = np.abs(lo["d"] - lo_za["d"]).max()
    assert scale > 0
    assert np.array_equal(2 * lo["ijk"].astype(np.int64), hi["ijk"].astype(np.int64))
    ed, ev = np.abs(hi["d"] - lo["d"]).max() / scale, np.abs(hi["v"] - lo["v"]).max() / scale
    print("PPD", n, "de-aliased <->", 2 * n, "plain: max|psi2| =", scale, "displacement", ed, "velocity", ev)
    assert ed <= 1e-10 and ev <= 1e-10


def test_lattice_of_768(zd):
    """PPD 512 (x, y, z lines of 768 = 256 x 3 points), one plane: against the plain run at 1024, ZD_k_cutoff = 2"""
    ps, n, z = _ps(zd), 512, 41
    lo_za = _one_plane(zd, ps, n, z)
    lo = _one_plane(zd, ps, n, z, q2LPT=1, lpt2_dealias=1)
    hi = _one_plane(zd, ps, 2 * n, 2 * z, k_cutoff=2.0, q2LPT=1)[::2, ::2]
    scale = np.abs(lo["d"] - lo_za["d"]).max()
    ed, ev = np.abs(hi["d"] - lo["d"]).max() / scale, np.abs(hi["v"] - lo["v"]).max() / scale
    print("PPD 512 de-aliased <-> 1024 plain: max|psi2| =", scale, "displacement", ed, "velocity", ev)
    assert scale > 0 and ed <= 1e-10 and ev <= 1e-10


# ---- 4. one mode: S = 0 -----------------------------------------------------------------------------------------------------
def test_one_mode_has_no_second_order(zd):
    ps, n = _ps(zd), 64
    kw = dict(qonemode=1, one_mode=(3, 5, -2))
    za = _one_plane(zd, ps, n, 7, **kw)
    got = _one_plane(zd, ps, n, 7, q2LPT=1, lpt2_dealias=1, **kw)
    scale = np.abs(za["d"]).max()
    assert scale > 0 and np.array_equal(got["ijk"], za["ijk"])
    print("one mode:", np.abs(got["d"] - za["d"]).max() / scale, np.abs(got["v"] - za["v"]).max() / scale)
    assert np.abs(got["d"] - za["d"]).max() <= 1e-12 * scale
    assert np.abs(got["v"] - za["v"]).max() <= 1e-12 * scale


# ---- 5. formats, coefficients, command line ---------------------------------------------------------------------------------
def test_rvzel(zd):
    n, ps = 32, _ps(zd)
    want = zd.generate(zd.make_params(n, q2LPT=1, lpt2_dealias=1), ps)["records"]
    got = zd.generate(zd.make_params(n, q2LPT=1, lpt2_dealias=1, icformat="RVZel"), ps)["records"]
    assert np.array_equal(got["ijk"], want["ijk"])
    for f in ("d", "v"):
        assert np.abs(got[f] - want[f]).max() <= 1e-6 * np.abs(want[f]).max()


def test_given_coefficients(zd, oracle):
    n, fcl = 64, 0.9
    rec, psi2_unit, _ = _reference(oracle, n, 1.0, 0, fcl)
    alpha = (np.sqrt(1 + 24 * fcl) - 1) / 4
    ps = _ps(zd)
    za = zd.generate(zd.make_params(n, f_cluster=fcl), ps)["records"]
    got = zd.generate(zd.make_params(n, f_cluster=fcl, q2LPT=1, lpt2_dealias=1, lpt2_ratio=-0.5, lpt2_f2=1.7), ps)["records"]
    _check_second_order(got, za, 0.5 * psi2_unit, alpha, 1.7, "given coefficients")


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
ZD_2LPT_dealias = 1
"""


def test_cli(zd, tmp_path):
    n, cpd = 32, 5
    out = tmp_path / "ic"
    out.mkdir()
    par = tmp_path / "t.par"
    par.write_text(PAR % dict(out=out, pk=WMAP, sigma=SIGMA) + "ZD_q2LPT = 1\n")
    r = subprocess.run([EXE, str(par)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    want = zd.generate(zd.make_params(n, q2LPT=1, lpt2_dealias=1, cpd=cpd), _ps(zd))["records"]
    plain = zd.generate(zd.make_params(n, q2LPT=1, cpd=cpd), _ps(zd))["records"]
    assert not np.array_equal(want["d"], plain["d"])
    dt = zd.RECORD_DTYPES["RVdoubleZel"]
    for f in sorted(set(z * cpd // n for z in range(n))):
        zs = [z for z in range(n) if z * cpd // n == f]
        got = np.fromfile(out / ("ic_%d" % f), dtype=dt).reshape(len(zs), n, n)
        assert np.array_equal(got, want[zs])
    # the key without ZD_q2LPT: refused with one line that names it, exit status 1
    par.write_text(PAR % dict(out=out, pk=WMAP, sigma=SIGMA))
    r = subprocess.run([EXE, str(par)], capture_output=True, text=True)
    assert r.returncode == 1
    lines = [ln for ln in r.stderr.splitlines() if "ZD_2LPT_dealias" in ln]
    assert lines == ["zeldovich_hip: ZD_2LPT_dealias = 1 needs ZD_q2LPT = 1"], r.stderr


# ---- 6. refusals through the API --------------------------------------------------------------------------------------------
def test_refusals_through_the_api(zd, capfd):
    ps = _ps(zd)
    for kw, word in ((dict(q2LPT=1, corner_modes=1), "ZD_CornerModes"), (dict(q2LPT=0), "ZD_q2LPT = 1")):
        with pytest.raises(RuntimeError):
            zd.generate(zd.make_params(32, lpt2_dealias=1, **kw), ps)
        err = capfd.readouterr().err
        assert "ZD_2LPT_dealias" in err and word in err, err
        with pytest.raises(RuntimeError):
            zd.Plan(zd.make_params(32, lpt2_dealias=1, **kw), ps)
        assert "ZD_2LPT_dealias" in capfd.readouterr().err
    for make in (lambda p: zd.generate(p, ps), lambda p: zd.Plan(p, ps)):
        with pytest.raises(RuntimeError):
            make(zd.make_params(2048, q2LPT=1, lpt2_dealias=1))
        err = capfd.readouterr().err
        # the round's lattice of 3072 points has no k_xlpt2q / k_lpt2q_zsrc (they end at 1536): the route refuses the job on the host,
        # before the round's 701 GB are asked for (the byte accounting: tests/test_lpt2_dealias.py, on the choosers' budgets)
        assert "PPD = 2048: no kernel for the second-order round: x stage of this job (launch_lpt2q_xsrc_t, n = 3072)" in err, err
        assert "launch failed" not in err


# ---- 7. a job without the key is the parent commit's, bit for bit -----------------------------------------------------------
def test_jobs_without_the_key_are_unchanged(zd, oracle):
    """sha-256 of the records of three PPD = 64 jobs, recorded with the library of the commit before ZD_2LPT_dealias
    (tests/golden/lpt2_dealias_parent_sha.json)"""
    want = json.load(open(os.path.join(GOLDEN, "lpt2_dealias_parent_sha.json")))
    ps = _ps(zd)
    jobs = {"za": (dict(), None), "plt": (dict(qPLT=1), oracle.synthetic_eigenmodes(32)), "q2lpt": (dict(q2LPT=1), None)}
    for name, (kw, eig) in jobs.items():
        rec = zd.generate(zd.make_params(64, **kw), ps, eig=eig)["records"]
        assert hashlib.sha256(np.ascontiguousarray(rec).tobytes()).hexdigest() == want[name], name


# ---- 8. launch sites (after the tests above) --------------------------------------------------------------------------------
def test_every_launch_site_was_launched(zd):
    """every instantiation of the two launchers' table — lattices of 48, 96, 192, 384 (the 256 link), 768 and 1536 points — has been
    launched by the tests of this file"""
    rep = zd.dispatch_report()
    names = [name for (name, _l), cnt in rep.items() if cnt > 0]
    txt = open(os.path.join(ROOT, "zeldovich_plt_amd", "csrc", "zd_kernels_lpt2q.hip")).read()
    sizes = re.findall(r"X\((\d+), (\d+), (\d+), (\d+)\)", re.search(r"#define LPT2Q_SIZES\(X\)(.*)", txt).group(1))
    assert len(sizes) == 6
    for P, Q, WX, WZ in sizes:
        want = "P = %s, E = 16, Q = %s, W = %s" % (P, Q, WX)
        assert any("launch_lpt2q_xsrc_t" in nm and want in nm for nm in names), "k_xlpt2q<%s> never launched" % want
        want = "P = %s, E = 16, Q = %s, W = %s" % (P, Q, WZ)
        assert any("launch_lpt2q_zsrc_t" in nm and want in nm for nm in names), "k_lpt2q_zsrc<%s> never launched" % want
