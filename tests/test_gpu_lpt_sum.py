"""GPU: direct sums and band power of ZD_q2LPT / ZD_q3LPT plans (zd_plan_lpt_direct_sum, zd_plan_lpt_power and their one-call forms;
definition in zeldovich_plt_amd/csrc/zd_kernels_lpt_ds.hip).

The yardstick and constants of tests/test_gpu_lpt3.py: oracle ZA records at ZD_Pk_sigma = 0.84 and the numpy restatements of the
second and third order applied to them; its floors are re-asserted on the reference, so the higher orders do not vanish.  Order n of
a direct sum is compared with the numpy field at the site to 1e-10 of max|psi^n_ref| (the project's parity bound applied to the small
term), the sum of the orders with delivered records to 1e-10 of max|q|."""
import os
import re
import subprocess

import numpy as np
import pytest

import lpt2_ref
import lpt3_ref
import lpt_sum_ref as ls
import power_ref as pr
from conftest import ROOT, WMAP

pytestmark = pytest.mark.gpu

BOX = 720.0
SIGMA = 0.84
FLOORS = {(32, 1.0), (64, 1.0), (64, 2.0)}  # as in test_gpu_lpt3.py: max|psi3| / max|psi1| >= 0.03, transverse part >= 0.003
EXE = os.path.join(ROOT, "zeldovich_plt_amd", "csrc", "build", "zeldovich")
G = lpt3_ref.DEFAULTS
XYZ = [2, 1, 0]  # (qx, qy, qz) of the library -> components along the array axes (z, y, x) of the records and the numpy fields


@pytest.fixture(scope="module")
def zd():
    import zeldovich_plt_amd.api as api
    return api


_REF = {}


def _spectra(zd, oracle, kind, fix=0):
    if kind == "plaw":
        kw = dict(Pk_sigma=2.0, fix_to_mean=fix)
        return zd.PowerSpectrum.from_powerlaw(-1.5, BOX, **kw), oracle.pk_from_powerlaw(-1.5, BOX, **kw)
    kw = dict(Pk_sigma=SIGMA, fix_to_mean=fix)
    return zd.PowerSpectrum.from_file(WMAP, BOX, **kw), oracle.pk_from_file(WMAP, BOX, **kw)


def _reference(zd, oracle, n, k_cutoff=1.0, fix=0, kind="file"):
    """oracle ZA records, the mask, psi2 at the default ratio and the unit-coefficient parts of psi3, once per configuration, read-only"""
    key = (n, k_cutoff, fix, kind)
    if key not in _REF:
        opk = _spectra(zd, oracle, kind, fix)[1]
        rec = oracle.run(oracle.make_params(n, k_cutoff=k_cutoff), opk)["records"]
        q = np.ascontiguousarray(rec["d"], dtype=np.float64)
        v = np.ascontiguousarray(rec["v"], dtype=np.float64)
        mask = lpt2_ref.alive_mask(n, BOX, k_cutoff)
        psi2 = lpt2_ref.second_order(q, BOX, mask)
        parts = lpt3_ref.third_order(q, BOX, mask)
        for a in (q, v, psi2) + parts:
            a.setflags(write=False)
        full, trans = lpt3_ref.combine(parts), G["g3c"] * parts[2]
        r = np.abs(full).max() / np.abs(q).max(), np.abs(trans).max() / np.abs(q).max()
        print("PPD", n, "k_cutoff", k_cutoff, "fix", fix, kind, "reference max|psi2| / max|psi1| =", np.abs(psi2).max() / np.abs(q).max(),
              "max|psi3| / max|psi1| =", r[0], "transverse part", r[1])
        if fix == 0 and kind == "file" and (n, k_cutoff) in FLOORS:
            assert r[0] >= 0.03 and r[1] >= 0.003, r
        _REF[key] = dict(q=q, v=v, mask=mask, psi2=psi2, parts=parts)
    return _REF[key]


def _sites(n):
    """nine sites (z, y, x): the corners of the index range, the centre, and six without symmetry"""
    rng = np.random.default_rng(n)
    return np.concatenate([np.array([(0, 0, 0), (n - 1, n - 1, n - 1), (n // 2, n // 2, n // 2)]), rng.integers(0, n, size=(6, 3))]).astype(np.int64)


def _at(field, sites):
    return field[sites[:, 0], sites[:, 1], sites[:, 2]]


def _check_order(label, got, want_d, want_v, scale):
    """order `label` of a direct sum [nsites, 6] against the fields at the sites [nsites, 3] (components z, y, x); prints, then asserts"""
    ed = np.abs(got[:, 0:3][:, XYZ] - want_d).max() / scale
    ev = np.abs(got[:, 3:6][:, XYZ] - want_v).max() / scale
    print(label, "scale", scale, "displacement error", ed, "velocity error", ev)
    assert ed <= 1e-10 and ev <= 1e-10, (label, ed, ev)


# ---- 1. the orders against numpy at sites ---------------------------------------------------------------------------------------
CASES = [(32, 1.0, 0, "file"), (64, 1.0, 0, "file"), (64, 2.0, 0, "file"), (64, 1.0, 1, "file"), (32, 1.0, 0, "plaw")]


@pytest.mark.parametrize("n,k_cutoff,fix,kind", CASES, ids=["%d-kc%g-fix%d-%s" % c for c in CASES])
def test_orders_against_numpy_at_sites(zd, oracle, n, k_cutoff, fix, kind):
    """PPD 32: N below the workgroup width and equal to the re-seed interval; 64: re-seeding; nine sites: a short second launch group"""
    ref = _reference(zd, oracle, n, k_cutoff, fix, kind)
    ps = _spectra(zd, oracle, kind, fix)[0]
    sites = _sites(n)
    psi3 = lpt3_ref.combine(ref["parts"])
    got = zd.lpt_direct_sum(zd.make_params(n, k_cutoff=k_cutoff, q2LPT=1, q3LPT=1), ps, sites)
    assert got.shape == (9, 3, 6)
    _check_order("order 1", got[:, 0], _at(ref["q"], sites), _at(ref["v"], sites), np.abs(ref["q"]).max())
    _check_order("order 2", got[:, 1], _at(ref["psi2"], sites), 2.0 * _at(ref["psi2"], sites), np.abs(ref["psi2"]).max())
    _check_order("order 3", got[:, 2], _at(psi3, sites), G["f3"] * _at(psi3, sites), np.abs(psi3).max())
    # a plan without the third order: the same first and second order, order 3 zero
    two = zd.lpt_direct_sum(zd.make_params(n, k_cutoff=k_cutoff, q2LPT=1), ps, sites)
    assert np.array_equal(two[:, 0], got[:, 0]) and np.all(two[:, 2] == 0.0)
    _check_order("order 2 of a 2LPT plan", two[:, 1], _at(ref["psi2"], sites), 2.0 * _at(ref["psi2"], sites), np.abs(ref["psi2"]).max())


def test_transverse_term_and_given_coefficients(zd, oracle):
    n = 64
    ref = _reference(zd, oracle, n)
    ps = _spectra(zd, oracle, "file")[0]
    sites = _sites(n)
    want = lpt3_ref.combine(ref["parts"], terms=4)
    got = zd.lpt_direct_sum(zd.make_params(n, q2LPT=1, q3LPT=1, lpt3_terms=4), ps, sites)
    _check_order("transverse term alone", got[:, 2], _at(want, sites), G["f3"] * _at(want, sites), np.abs(want).max())
    # given coefficients on another background: alpha, D2 / D1^2 and f2 are that background's, the third order's are given
    g = dict(lpt3_g3a=-0.29, lpt3_g3b=0.51, lpt3_g3c=-0.17, lpt3_f3=2.6)
    alpha, ratio, f2 = lpt2_ref.default_coefficients(0.9)
    psi2 = lpt2_ref.second_order(ref["q"], BOX, ref["mask"], ratio)
    psi3 = lpt3_ref.combine(ref["parts"], g3a=g["lpt3_g3a"], g3b=g["lpt3_g3b"], g3c=g["lpt3_g3c"])
    got = zd.lpt_direct_sum(zd.make_params(n, f_cluster=0.9, q2LPT=1, q3LPT=1, **g), ps, sites)
    _check_order("order 1 at f_cluster 0.9", got[:, 0], _at(ref["q"], sites), alpha * _at(ref["q"], sites), np.abs(ref["q"]).max())
    _check_order("order 2 at f_cluster 0.9", got[:, 1], _at(psi2, sites), f2 * _at(psi2, sites), np.abs(psi2).max())
    _check_order("order 3, given coefficients", got[:, 2], _at(psi3, sites), g["lpt3_f3"] * _at(psi3, sites), np.abs(psi3).max())


# ---- 2. delivered records, small sizes --------------------------------------------------------------------------------------------
def _check_records(label, got, rec, sites):
    scale = np.abs(rec["d"]).max()
    tot = got.sum(axis=1)
    ed = np.abs(tot[:, 0:3][:, XYZ] - _at(rec["d"], sites)).max() / scale
    ev = np.abs(tot[:, 3:6][:, XYZ] - _at(rec["v"], sites)).max() / scale
    print(label, "max|q| =", scale, "displacement error", ed, "velocity error", ev,
          "max|psi2| / max|q| =", np.abs(got[:, 1, 0:3]).max() / scale, "max|psi3| / max|q| =", np.abs(got[:, 2, 0:3]).max() / scale)
    assert ed <= 1e-10 and ev <= 1e-10, (label, ed, ev)


@pytest.mark.parametrize("kw", [dict(q3LPT=1, stream_factor=1), dict(q3LPT=1, stream_factor=2), dict(q3LPT=1, stream_factor=4),
                                dict(lpt2_dealias=1)], ids=["R1", "R2", "R4", "dealias"])
def test_sum_of_orders_against_delivered_records(zd, oracle, kw):
    n = 64
    ps = _spectra(zd, oracle, "file")[0]
    p = zd.make_params(n, q2LPT=1, **kw)
    rec = zd.generate(p, ps)["records"]
    sites = _sites(n)
    got = zd.lpt_direct_sum(p, ps, sites)
    assert np.abs(got[:, 1]).max() > 0 and (np.abs(got[:, 2]).max() > 0) == bool(kw.get("q3LPT"))
    _check_records("PPD 64 %r" % kw, got, rec, sites)


# ---- 3. delivered records, PPD 512 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q3", [0, 1], ids=["2LPT", "3LPT"])
def test_delivered_records_at_512(zd, oracle, q3):
    """two workgroups along x, eight launch groups in one call; then five sites: one short group"""
    n = 512
    ps = _spectra(zd, oracle, "file")[0]
    p = zd.make_params(n, q2LPT=1, q3LPT=q3, stream_factor=2)
    rng = np.random.default_rng(512 + q3)
    sites = rng.integers(0, n, size=(64, 3)).astype(np.int64)
    sites[0] = (17, 300, 0)      # x = 0
    sites[1] = (18, 5, 511)      # the next plane (the other z residue of stream factor 2), the last x
    sites[2] = (17, 255, 256)    # the first lane of the second workgroup
    sites[3] = (0, 0, 0)
    sites[4] = (511, 511, 400)
    assert (sites[:, 2] >= 256).sum() >= 8
    planes = {}

    def take(z, plane):
        if z in set(sites[:, 0].tolist()):
            planes[z] = plane.copy()

    info = zd.generate_planes(p, ps, take)
    assert info["planes"] == n and info["stream_factor"] == 2
    plan = zd.Plan(p, ps)
    try:
        got = plan.lpt_direct_sum(sites)
        few = plan.lpt_direct_sum(sites[:5])
    finally:
        plan.close()
    assert np.array_equal(few, got[:5])
    scale = max(np.abs(pl["d"]).max() for pl in planes.values())
    tot = got.sum(axis=1)
    ed = ev = 0.0
    for i, (z, y, x) in enumerate(sites):
        r = planes[int(z)][y, x]
        ed = max(ed, np.abs(tot[i, 0:3][XYZ] - r["d"]).max() / scale)
        ev = max(ev, np.abs(tot[i, 3:6][XYZ] - r["v"]).max() / scale)
    print("PPD 512 q3LPT", q3, "max|q| over the planes =", scale, "displacement error", ed, "velocity error", ev,
          "max|psi2| / max|q| =", np.abs(got[:, 1, 0:3]).max() / scale, "max|psi3| / max|q| =", np.abs(got[:, 2, 0:3]).max() / scale)
    assert np.abs(got[:, 1]).max() > 0 and (np.abs(got[:, 2]).max() > 0) == bool(q3)
    assert ed <= 1e-10 and ev <= 1e-10


# ---- 4. repeatability -----------------------------------------------------------------------------------------------------------
def test_two_calls_return_the_same_bits(zd, oracle):
    ps = _spectra(zd, oracle, "file")[0]
    plan = zd.Plan(zd.make_params(64, q2LPT=1, q3LPT=1), ps)
    try:
        a, b = plan.lpt_direct_sum(_sites(64)), plan.lpt_direct_sum(_sites(64))
    finally:
        plan.close()
    assert np.abs(a).min() > 0 and a.tobytes() == b.tobytes()


# ---- 5. band power against numpy ------------------------------------------------------------------------------------------------
POWER_CASES = [(32, 1, 1, "file"), (64, 1, 1, "file"), (64, 3, 1, "file"), (32, 1, 0, "file"), (32, 1, 1, "plaw"), (32, 1, 0, "plaw")]


@pytest.mark.parametrize("n,w,q3,kind", POWER_CASES, ids=["%d-w%d-q3LPT%d-%s" % c for c in POWER_CASES])
def test_band_power_against_numpy(zd, oracle, n, w, q3, kind):
    ref = _reference(zd, oracle, n, 1.0, 0, kind)
    ps, opk = _spectra(zd, oracle, kind)
    got = zd.lpt_power(zd.make_params(n, q2LPT=1, q3LPT=q3), ps, bin_width=w)
    D = oracle.mode_cube(oracle.make_params(n, qdensity=2), opk)[0]
    base = pr.reference_sums(oracle, opk, n, BOX, D, w)
    assert len(got["count"]) == pr.nbins(n, w) and np.array_equal(got["count"], base["count"]) and base["count"].sum() > 0
    for key, tol in (("sum_k", 1e-14), ("sum_dens", 1e-12), ("sum_input", 1e-12)):
        print(key, "worst relative difference over the bins", pr.worst(got[key], base[key]))
        assert pr.close(got[key], base[key], tol), key
    live = got["count"] > 0
    assert np.array_equal(got["k_mean"][live], got["sum_k"][live] / got["count"][live])
    psi3 = lpt3_ref.combine(ref["parts"]) if q3 else np.zeros_like(ref["q"])
    fields = dict(sum_disp1=ref["q"], sum_disp2=ref["psi2"], sum_disp3=psi3, sum_disp=ref["q"] + ref["psi2"] + psi3,
                  sum_vel=ref["v"] + 2.0 * ref["psi2"] + G["f3"] * psi3)
    for key, field in fields.items():
        want = ls.binned_field(field, ref["mask"], w)
        if not q3 and key == "sum_disp3":
            assert np.all(got[key] == 0.0)
            continue
        err = float(np.abs(np.asarray(got[key], dtype=np.longdouble) - want).max() / want.max())
        print(key, "largest bin", float(want.max()), "error / largest bin", err)
        assert want.max() > 0 and err <= 1e-10, key


def test_one_mode_plan_has_no_higher_order_power(zd, oracle):
    """A one-mode plan: sum_disp2 = sum_disp3 = 0 exactly, and so are orders 2 and 3 of the direct sum.  A single plane wave has no
    higher order (the definition in zd_kernels_lpt_ds.hip); the arrays of such a plan hold the rounds' rounding residue — P3 and C at the
    mode gave sum_disp3 = 1.3e-52 against sum_disp1 = 4e-3 when the sweep read them — which the sums do not report.  The first order
    alone then meets the delivered records, residue included, to the bound of every other run."""
    ps = _spectra(zd, oracle, "file")[0]
    p = zd.make_params(64, q2LPT=1, q3LPT=1, qonemode=1, one_mode=(3, 5, -2))
    got = zd.lpt_power(p, ps)
    print("one mode: count", got["count"].sum(), "sum_disp1", got["sum_disp1"].sum(), "sum_disp2", got["sum_disp2"].sum(),
          "sum_disp3", got["sum_disp3"].sum())
    assert got["count"].sum() == 2 and got["sum_disp1"].sum() > 0
    assert np.all(got["sum_disp2"] == 0.0) and np.all(got["sum_disp3"] == 0.0)
    for key in ("sum_disp", "sum_vel"):  # (alpha = 1: the delivered power is the first order's)
        assert np.allclose(got[key], got["sum_disp1"], rtol=1e-14, atol=0), key
    sites = _sites(64)
    sums = zd.lpt_direct_sum(p, ps, sites)
    assert np.abs(sums[:, 0]).max() > 0 and np.all(sums[:, 1:] == 0.0)
    _check_records("one mode", sums, zd.generate(p, ps)["records"], sites)


# ---- 6. Parseval ----------------------------------------------------------------------------------------------------------------
def test_parseval_against_the_delivered_records(zd, oracle):
    n = 128
    ps = _spectra(zd, oracle, "file")[0]
    p = zd.make_params(n, q2LPT=1, q3LPT=1)
    rec = zd.generate(p, ps)["records"]
    got = zd.lpt_power(p, ps)
    for key, f in (("sum_disp", "d"), ("sum_vel", "v")):
        want = float((rec[f].astype(np.longdouble) ** 2).sum() / np.longdouble(n) ** 3)
        total = float(np.asarray(got[key], dtype=np.longdouble).sum())
        print(key, total, "N^-3 sum |%s|^2" % f, want, "relative difference", abs(total - want) / want)
        assert abs(total - want) <= 1e-10 * want, key


# ---- 7. command line ------------------------------------------------------------------------------------------------------------
PAR = """BoxSize = 720
CPD = 5
ICFormat = "%(fmt)s"
InitialConditionsDirectory = "%(out)s"
InitialRedshift = 49
NP = 32768
ZD_NumBlock = 2
ZD_Pk_filename = "%(pk)s"
ZD_Pk_norm = 8.0
ZD_Pk_scale = 1.0
ZD_Pk_sigma = 0.84
ZD_Pk_smooth = 0.0
ZD_Seed = 12346
ZD_Version = 2
"""
ON = "ZD_q2LPT = 1\nZD_q3LPT = 1\n"
LINE = re.compile(r"^lpt self-check: 8 sites, max \|record - direct sum\| / max\|q\| = (\S+), max\|psi2\| / max\|q\| = (\S+), "
                  r"max\|psi3\| / max\|q\| = (\S+) \(ZD_LPT_SelfCheck_tol = (\S+)\)$", re.M)


def _run(tmp_path, name, fmt, extra):
    out = tmp_path / name
    out.mkdir()
    par = tmp_path / (name + ".par")
    par.write_text(PAR % dict(fmt=fmt, out=out, pk=WMAP) + extra)
    return out, subprocess.run([EXE, str(par)], capture_output=True, text=True)


@pytest.mark.parametrize("fmt,tol", [("RVdoubleZel", 1e-10), ("RVZel", 1e-6)])
def test_cli_checks_itself_and_writes_its_power(zd, tmp_path, fmt, tol):
    n = 32
    plain, r = _run(tmp_path, "plain", fmt, ON)
    assert r.returncode == 0, r.stderr
    keys = 'ZD_LPT_SelfCheck = 8\nZD_LPT_SelfCheck_filename = "%s"\nZD_LPT_Pk_filename = "%s"\n' % (tmp_path / "sites.txt", tmp_path / "pk.txt")
    out, r = _run(tmp_path, "checked", fmt, ON + keys)
    assert r.returncode == 0, r.stderr
    m = LINE.search(r.stderr)
    assert m, r.stderr
    worst, r2, r3, bound = (float(v) for v in m.groups())
    print(fmt, m.group(0))
    assert worst <= tol and bound == tol and r2 > 1e-3 and r3 > 1e-4
    names = sorted(os.listdir(plain))
    assert names and names == sorted(os.listdir(out)) and all(nm.startswith("ic_") for nm in names)
    for nm in names:
        assert (plain / nm).read_bytes() == (out / nm).read_bytes(), nm
    # the site file: z y x, the record, the three orders; the record is their sum
    tab = np.loadtxt(tmp_path / "sites.txt")
    assert tab.shape == (8, 3 + 6 + 18) and tab[:, :3].min() >= 0 and tab[:, :3].max() < n
    tot = tab[:, 9:15] + tab[:, 15:21] + tab[:, 21:27]
    assert np.abs(tab[:, 3:9] - tot).max() <= tol * np.abs(tot[:, :3]).max()
    # the power table: the columns of lpt_power divided by the count, one line per non-empty shell
    ps = zd.PowerSpectrum.from_file(WMAP, BOX, Pk_sigma=SIGMA)
    got = zd.lpt_power(zd.make_params(n, q2LPT=1, q3LPT=1, icformat=fmt), ps)
    live = got["count"] > 0
    tab = np.loadtxt(tmp_path / "pk.txt")
    assert tab.shape == (live.sum(), 9) and np.array_equal(tab[:, 1], got["count"][live])
    assert np.allclose(tab[:, 0], got["k_mean"][live], rtol=1e-15, atol=0)
    for col, key in enumerate(zd.LPT_POWER_SUMS[1:], start=2):
        assert np.allclose(tab[:, col], got[key][live] / got["count"][live], rtol=1e-9, atol=0), key  # (double atomics: the order of the adds)
    # a bound nothing meets
    _o, r = _run(tmp_path, "tight", fmt, ON + "ZD_LPT_SelfCheck = 8\nZD_LPT_SelfCheck_tol = 1e-30\n")
    assert r.returncode == 1 and "lpt self-check FAILED" in r.stderr, r.stderr


CLI_REFUSALS = [
    ("ZD_LPT_SelfCheck = 8\n", "ZD_q2LPT = 1"),
    ('ZD_LPT_Pk_filename = "/tmp/unused.txt"\n', "ZD_q2LPT = 1"),
    ("ZD_SelfCheck = 4\nZD_LPT_SelfCheck = 8\n", "ZD_SelfCheck"),
    (ON + "ZD_SelfCheck = 4\nZD_LPT_SelfCheck = 8\n", "ZD_SelfCheck"),
    (ON + "ZD_SelfCheck = 4\n", "ZD_q2LPT"),  # as before this feature
    (ON + "ZD_LPT_SelfCheck = eight\n", "not an integer"),
    (ON + "ZD_LPT_SelfCheck = 8.5\n", "not an integer"),
    (ON + "ZD_LPT_SelfCheck = 65\n", "0 ... 64"),
    (ON + "ZD_LPT_SelfCheck = 8\nZD_LPT_SelfCheck_tol = tiny\n", "not a number"),
    (ON + "ZD_LPT_SelfCheck = 8\nZD_LPT_SelfCheck_tol = -1\n", ">= 0"),
]


def test_cli_refusals(tmp_path):
    for i, (extra, word) in enumerate(CLI_REFUSALS):
        _o, r = _run(tmp_path, "r%d" % i, "RVdoubleZel", extra)
        lines = [ln for ln in r.stderr.splitlines() if ln.strip()]
        if "ZD_LPT" not in extra:  # (the reader's refusal follows its own first line)
            lines = [ln for ln in lines if "Invalid Parameters" in ln]
        assert r.returncode == 1 and len(lines) == 1 and word in lines[0], (extra, r.stderr)


def test_plans_without_the_second_order_are_refused(zd, oracle, capfd):
    ps = _spectra(zd, oracle, "file")[0]
    plan = zd.Plan(zd.make_params(32), ps)
    try:
        capfd.readouterr()
        with pytest.raises(RuntimeError):
            plan.lpt_direct_sum([(0, 0, 0)])
        assert "ZD_q2LPT = 1" in capfd.readouterr().err
        with pytest.raises(RuntimeError):
            plan.lpt_power()
        assert "ZD_q2LPT = 1" in capfd.readouterr().err
    finally:
        plan.close()


# ---- 8. launch sites (after the tests above) ------------------------------------------------------------------------------------
def test_every_new_launch_site_was_launched(zd):
    """k_ds_lpt with and without the third order, k_pk_lpt in its eight forms (third order x power law x table arithmetic), through
    the library's launch accounting"""
    names = [name for (name, _l), cnt in zd.dispatch_report().items() if cnt > 0]
    for o3 in ("false", "true"):
        assert any("launch_ds_lpt_t" in nm and "O3 = %s" % o3 in nm for nm in names), "k_ds_lpt<%s> never launched" % o3
        for plaw in ("false", "true"):
            for fast in ("false", "true"):
                want = "O3 = %s, PLAW = %s, FAST = %s" % (o3, plaw, fast)
                assert any("launch_pk_lpt_t" in nm and want in nm for nm in names), "k_pk_lpt<%s> never launched" % want
    assert any("launch_ds_reduce" in nm for nm in names)
