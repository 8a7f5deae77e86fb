"""GPU: direct summation at sample sites (zd_direct_sum / zd_plan_direct_sum, csrc/zd_kernels_ds.hip) against the oracle's
mode-by-mode summation, a closed-form plane wave, the production path's own records, the committed full-size fixture, and through
the self-checking command line (ZD_SelfCheck).

Bounds.  Displacements and velocities: 1e-10 of max|q| over the sites, the project's parity bound; the density: 1e-10 of max|density|.
Where the density comes from the production path it is a float32 plane in every format (2^-24 = 6e-8 relative), so the direct sum
is rounded to float32 before it is compared: both sides are then roundings of two doubles 1e-10 apart, and the bound stays."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, WMAP

pytestmark = pytest.mark.gpu
BOX = 720.0
EXE = os.path.join(ROOT, "zeldovich_plt_amd", "csrc", "build", "zeldovich")
FIXTURE = json.load(open(os.path.join(GOLDEN, "direct_sum.json")))
PLT = dict(qPLT=1, qPLTrescale=1, PLT_target_z=5.0)


@pytest.fixture(scope="module")
def zd():
    import zeldovich_plt_amd.api as api
    api.load_library()
    return api


def sites9(n):
    """(0, 0, 0), the far corner, and coordinates on both sides of n / 2; 9 = 8 + 1 sites: a second launch group"""
    h = n // 2
    return [(0, 0, 0), (n - 1, n - 1, n - 1), (1, h - 1, h + 1), (h, h, h), (h + 1, 2, h - 1), (h - 1, h + 1, 3), (5, n - 2, h),
            (n - 3, 1, 7), (h // 2, h + h // 2, n - 4)]


def figures(got, want):
    q = np.abs(want[:, :3]).max()
    d = np.abs(want[:, 6]).max()
    return np.abs(got[:, :6] - want[:, :6]).max() / q, (np.abs(got[:, 6] - want[:, 6]).max() / d if d > 0 else 0.0)


def _spectra(zd, oracle, kind, fix=0):
    if kind == "plaw":
        return zd.PowerSpectrum.from_powerlaw(-1.5, BOX, fix_to_mean=fix), oracle.pk_from_powerlaw(-1.5, BOX, fix_to_mean=fix)
    return zd.PowerSpectrum.from_file(WMAP, BOX, fix_to_mean=fix), oracle.pk_from_file(WMAP, BOX, fix_to_mean=fix)


ORACLE_CASES = [
    ("za32", 32, "file", dict(), 0),
    ("za64", 64, "file", dict(), 0),
    ("za64_kcut2", 64, "file", dict(k_cutoff=2.0), 0),
    ("za64_fixed", 64, "file", dict(fix=1), 0),
    ("za32_plaw", 32, "plaw", dict(), 0),               # its own instantiation
    ("plt64_rescale", 64, "file", dict(PLT), 32),       # synthetic eigenmodes, interpolated (32 -> 64)
    ("plt32_plaw", 32, "plaw", dict(PLT), 32),          # the PLT power-law instantiations, exact stride
    ("za96", 96, "file", dict(), 0),                    # composite family
    ("za100", 100, "file", dict(), 0),                  # convolution family: the sweep is family-independent
]


@pytest.mark.parametrize("name,n,kind,kw,eig_ppd", ORACLE_CASES, ids=[c[0] for c in ORACLE_CASES])
def test_against_the_oracle(zd, oracle, name, n, kind, kw, eig_ppd):
    kw = dict(kw)
    fix = kw.pop("fix", 0)
    ps, opk = _spectra(zd, oracle, kind, fix)
    eig = oracle.synthetic_eigenmodes(eig_ppd) if eig_ppd else None
    sites = sites9(n)
    want = oracle.direct_sum(oracle.make_params(n, **kw), opk, sites, eig=eig)
    got = zd.direct_sum(zd.make_params(n, **kw), ps, sites, eig=eig)
    fq, fd = figures(got, want)
    print("%s: max |GPU - oracle| / max|q| = %.3g, density / max|density| = %.3g" % (name, fq, fd))
    assert got.shape == (9, 7) and np.abs(want[:, :3]).max() > 1e-4
    assert fq <= 1e-10 and fd <= 1e-10
    if kw.get("qPLT"):  # the velocity is its own field
        assert np.abs(got[:, 3:6] - got[:, :3]).max() > 1e-3 * np.abs(got[:, :3]).max()


def test_sixty_four_sites_in_one_call(zd, oracle):
    n = 32
    ps, opk = _spectra(zd, oracle, "file")
    rs = np.random.RandomState(5)
    sites = rs.randint(0, n, size=(64, 3))
    want = oracle.direct_sum(oracle.make_params(n), opk, sites)
    got = zd.direct_sum(zd.make_params(n), ps, sites)
    fq, fd = figures(got, want)
    print("64 sites: max |GPU - oracle| / max|q| = %.3g, density %.3g" % (fq, fd))
    assert fq <= 1e-10 and fd <= 1e-10


def test_one_mode_is_a_plane_wave(zd):
    """ZD_qonemode with (3, 5, -2) at PPD = 64: density = 2 Re(D e^{i t}), q_j = 2 Re(i s_j D e^{i t}) with s_j = k_j fundamental / k^2 and
    t = 2 pi k.x / N, D from zd_test_modes of that mode; v = q at f_cluster = 1"""
    n, k = 64, (3, 5, -2)
    ps = zd.PowerSpectrum.from_file(WMAP, BOX)
    D = zd.test_modes(zd.make_params(n), ps, [k])[0]
    sites = np.array(sites9(n))
    got = zd.direct_sum(zd.make_params(n, qonemode=1, one_mode=k), ps, sites)
    m = (k[0] * sites[:, 2] + k[1] * sites[:, 1] + k[2] * sites[:, 0]) % n  # sites are (z, y, x)
    e = np.exp(2j * np.pi * m / n)
    fund = 2 * np.pi / BOX
    want = np.zeros((9, 7))
    for j in range(3):
        want[:, j] = want[:, 3 + j] = 2 * (1j * k[j] / (fund * sum(c * c for c in k)) * D * e).real
    want[:, 6] = 2 * (D * e).real
    fq, fd = figures(got, want)
    print("one mode: max |GPU - plane wave| / max|q| = %.3g, density %.3g" % (fq, fd))
    assert abs(D) > 0 and fq <= 1e-10 and fd <= 1e-10


def records_at(zd, plan, n, sites, fmt="RVdoubleZel"):
    """records of a plan at the lattice sites [(z, y, x), ...]: only the passes that hold their planes are executed (staged API),
    only the picked records leave the GPU (the pattern of tests/test_gpu_direct_sum.py)"""
    import torch
    store = torch.empty(plan.exchange_bytes, dtype=torch.uint8, device="cuda")
    dt = zd.RECORD_DTYPES[fmt]
    step = plan.plane_step
    out = torch.empty(step * n * n * dt.itemsize, dtype=torch.uint8, device="cuda")
    where = {}
    for ps_ in range(plan.passes):
        for lp in range(plan.local_planes):
            where[plan.plane_z(ps_, lp)] = (ps_, lp)
    res = np.zeros((len(sites), 6))
    for z in sorted({s[0] for s in sites}, key=lambda z: where[z]):
        pass_, lp = where[z]
        plan.stage_z(pass_, store.data_ptr())
        plan.stage_y(store.data_ptr())
        first = lp // step * step
        plan.stage_x(pass_, store.data_ptr(), first, step, out.data_ptr())
        torch.cuda.synchronize()
        img = out.view(step, n, n, dt.itemsize)
        for i, (zz, y, x) in enumerate(sites):
            if zz == z:
                r = img[lp - first, y, x].cpu().numpy().view(dt)[0]
                assert tuple(int(v) for v in r["ijk"]) == (zz, y, x)
                res[i, :3] = np.array(r["d"])[::-1]  # records hold (qz, qy, qx)
                res[i, 3:] = np.array(r["v"])[::-1]
    del store, out
    torch.cuda.empty_cache()
    return res


PRODUCTION_CASES = [
    ("za256_R2_field_store", 256, dict(stream_factor=2), 0),
    ("plt512_fused", 512, dict(PLT), 32),
    ("fnl64", 64, dict(f_NL=100.0, n_s=0.96, Omega_M=0.31), 0),  # Plan.direct_sum against that plan's own records
]


@pytest.mark.parametrize("name,n,kw,eig_ppd", PRODUCTION_CASES, ids=[c[0] for c in PRODUCTION_CASES])
def test_against_the_production_path(zd, oracle, name, n, kw, eig_ppd):
    ps = zd.PowerSpectrum.from_file(WMAP, BOX)
    eig = oracle.synthetic_eigenmodes(eig_ppd) if eig_ppd else None
    sites = sites9(n)
    p = zd.make_params(n, **kw)
    if p.stream_factor <= 0:
        import torch
        free_b, _ = torch.cuda.mem_get_info()
        p.stream_factor = zd.load_library().zd_choose_stream_factor(C.byref(p), 1, int(free_b) - (24 << 30))
        assert p.stream_factor > 0
    plan = zd.Plan(p, ps, eig=eig)
    try:
        want = records_at(zd, plan, n, sites)
        got = plan.direct_sum(sites)
        info = (plan.store_mode, plan.R)
    finally:
        plan.close()
    scale = np.abs(got[:, :3]).max()
    fq = np.abs(got[:, :6] - want).max() / scale
    print("%s %r: max |record - direct sum| / max|q| = %.3g" % (name, info, fq))
    assert scale > 1e-4 and fq <= 1e-10
    if name.startswith("fnl"):  # the non-Gaussian term is really in the sums
        lin = zd.direct_sum(zd.make_params(n), ps, sites)
        assert np.abs(lin[:, :3] - got[:, :3]).max() > 1e-8 * scale


def test_density_column_against_the_production_path(zd):
    """PPD = 128 ZA with ZD_qdensity = 1 through zd_generate: records and the (float32) density plane at the sites"""
    n = 128
    ps = zd.PowerSpectrum.from_file(WMAP, BOX)
    sites = np.array(sites9(n))
    run = zd.generate(zd.make_params(n, qdensity=1), ps)
    got = zd.direct_sum(zd.make_params(n, qdensity=1), ps, sites)
    rec = run["records"][sites[:, 0], sites[:, 1], sites[:, 2]]
    want = np.concatenate([rec["d"][:, ::-1], rec["v"][:, ::-1]], axis=1)
    dens = run["density"][sites[:, 0], sites[:, 1], sites[:, 2]]
    fq = np.abs(got[:, :6] - want).max() / np.abs(got[:, :3]).max()
    dmax = np.abs(got[:, 6]).max()
    fd = np.abs(got[:, 6].astype(np.float32).astype(np.float64) - dens.astype(np.float64)).max() / dmax
    fd_raw = np.abs(got[:, 6] - dens).max() / dmax
    print("qdensity: max |record - direct sum| / max|q| = %.3g; density (as float32) / max|density| = %.3g (unrounded: %.3g)" % (fq, fd, fd_raw))
    assert dmax > 1e-3 and fq <= 1e-10 and fd <= 1e-10
    assert fd_raw <= 2.0 ** -24  # ... and the plane really is the float32 rounding of the sum


@pytest.mark.parametrize("case", ["ppd2048_plt_rescale", "ppd4096_za"])
def test_full_size_against_the_committed_fixture(zd, oracle, case):
    """the workload's own size, the point of the feature: the GPU direct sum at the fixture's 8 sites against the CPU oracle's values"""
    c = FIXTURE[case]
    n = c["ppd"]
    assert c["seed"] == 12346 and c["boxsize"] == 720.0
    ps = zd.PowerSpectrum.from_file(WMAP, BOX)
    eig = oracle.synthetic_eigenmodes(c["eig_ppd"]) if c["eig_ppd"] else None
    want = np.array(c["values"])
    got = zd.direct_sum(zd.make_params(n, **c["params"]), ps, c["sites"], eig=eig)
    scale = np.abs(want[:, :3]).max()
    fq = np.abs(got[:, :6] - want[:, :6]).max() / scale
    print("%s: max |GPU direct sum - fixture| / max|q| = %.3g" % (case, fq))
    assert len(c["sites"]) == 8 and scale > 1e-3 and fq <= 1e-10
    if want.shape[1] > 6:
        fd = np.abs(got[:, 6] - want[:, 6]).max() / np.abs(want[:, 6]).max()
        print("%s: density / max|density| = %.3g" % (case, fd))
        assert fd <= 1e-10


@pytest.mark.parametrize("nranks", [2, 4])
def test_rank_sums_add_up(zd, nranks):
    n = 64
    ps = zd.PowerSpectrum.from_file(WMAP, BOX)
    sites = sites9(n)
    one = zd.Plan(zd.make_params(n), ps)
    whole = one.direct_sum(sites)
    one.close()
    acc = np.zeros((9, 7), dtype=np.longdouble)
    for r in range(nranks):
        pl = zd.Plan(zd.make_params(n), ps, rank=r, nranks=nranks)
        part = pl.direct_sum(sites)
        pl.close()
        assert np.abs(part).max() > 0
        acc += part
    rel = np.abs(acc - whole).max(axis=0) / np.abs(whole).max(axis=0)
    print("%d ranks: largest |sum of the ranks - one rank| / max per column = %.3g" % (nranks, float(rel.max())))
    assert rel.max() <= 1e-12


def test_two_calls_return_the_same_bits(zd, oracle):
    ps = zd.PowerSpectrum.from_file(WMAP, BOX)
    for n, kw, eig in ((64, dict(), None), (64, dict(PLT), oracle.synthetic_eigenmodes(32))):
        plan = zd.Plan(zd.make_params(n, **kw), ps, eig=eig)
        a = plan.direct_sum(sites9(n))
        b = plan.direct_sum(sites9(n))
        plan.close()
        assert np.array_equal(a, b) and np.abs(a).max() > 0


def test_refusals(zd, capfd):
    ps = zd.PowerSpectrum.from_file(WMAP, BOX)
    for kw, word in ((dict(version=1), "ZD_Version = 1"), (dict(q2LPT=1), "ZD_q2LPT"), (dict(corner_modes=1, k_cutoff=2.0), "Nyquist")):
        capfd.readouterr()
        with pytest.raises(RuntimeError):
            zd.direct_sum(zd.make_params(64, **kw), ps, [(1, 2, 3)])
        err = capfd.readouterr().err
        assert word in err and "direct summation" in err, err
    # what api.direct_sum stops itself, handed to the library
    L = zd.load_library()
    p = zd.make_params(64)
    plan = zd.Plan(p, ps)
    for sites, word in (([(0, 0, 64)], "outside"), ([(64, 0, 0)], "outside"), ([(0, 0, 0)] * 65, "1 to 64 sites")):
        s = np.array(sites, dtype=np.int64)
        out = np.zeros((len(s), 7))
        capfd.readouterr()
        assert L.zd_direct_sum(C.byref(p), C.byref(ps.pk), None, 0, len(s), s.ctypes.data, out.ctypes.data) != 0
        assert word in capfd.readouterr().err
        assert L.zd_plan_direct_sum(plan.h, len(s), s.ctypes.data, out.ctypes.data, None) != 0
        assert word in capfd.readouterr().err and not out.any()
    assert L.zd_plan_direct_sum(plan.h, 0, s.ctypes.data, out.ctypes.data, None) != 0
    assert L.zd_plan_direct_sum(plan.h, 1, None, out.ctypes.data, None) != 0 and L.zd_plan_direct_sum(plan.h, 1, s.ctypes.data, None, None) != 0
    # ... and the plan still sums afterwards
    assert np.abs(plan.direct_sum([(1, 2, 3)])).max() > 0
    plan.close()


PAR = """BoxSize = 720
CPD = 5
ICFormat = "%(fmt)s"
InitialConditionsDirectory = "%(out)s"
InitialRedshift = 49
NP = %(np)d
ZD_NumBlock = 2
ZD_Pk_filename = "%(pk)s"
ZD_Pk_norm = 8.0
ZD_Pk_scale = 1.0
ZD_Pk_sigma = 0.0210839935761
ZD_Pk_smooth = 0.0
ZD_Seed = 12346
ZD_Version = 2
ZD_SelfCheck = 8
"""


def _cli(tmp_path, fmt, extra="", n=64):
    out = tmp_path / "ic"
    out.mkdir(exist_ok=True)
    table = tmp_path / "self_check.txt"
    par = tmp_path / "t.par"
    par.write_text(PAR % dict(fmt=fmt, out=out, pk=WMAP, np=n ** 3) + 'ZD_SelfCheck_filename = "%s"\n' % table + extra)
    r = subprocess.run([EXE, str(par)], capture_output=True, text=True)
    lines = [ln for ln in r.stderr.splitlines() if ln.startswith("self-check: 8 sites, max |record - direct sum| / max|q| = ")]
    figs = [float(v) for v in re.findall(r" = ([0-9.eE+-]+|nan|inf)[, )]", lines[0])] if lines else []
    tab = np.loadtxt(table) if table.exists() else None
    return r, lines, figs, tab


@pytest.mark.parametrize("fmt,bound,extra", [("RVdoubleZel", 1e-10, ""), ("RVZel", 1e-6, ""),
                                             ("RVdoubleZel", 1e-10, "ZD_qdensity = 1\nZD_NumGPU = 1\nZD_StreamFactor = 4\n")])
def test_cli_self_check(zd, tmp_path, fmt, bound, extra):
    n = 128 if extra else 64  # stream factor 4 needs z lines of 32 points
    r, lines, figs, tab = _cli(tmp_path, fmt, extra, n)
    print(r.stderr[-600:])
    assert r.returncode == 0, r.stderr
    assert len(lines) == 1 and len(figs) == (3 if extra else 2) and all(f <= bound for f in figs[:-1])
    assert figs[-1] == bound  # the bound the run applied: the format's default
    assert tab.shape == (8, 17)
    ps = zd.PowerSpectrum.from_file(WMAP, BOX)
    sites = tab[:, :3].astype(np.int64)
    want = zd.direct_sum(zd.make_params(n, icformat=fmt), ps, sites)
    assert np.array_equal(tab[:, 10:], want)  # the file holds the library's sums to the last bit (%.17g)
    ncol = 7 if extra else 6
    assert np.abs(tab[:, 3:3 + ncol] - want[:, :ncol]).max() <= (1e-6 if extra else bound) * np.abs(want).max()
    assert extra or np.isnan(tab[:, 9]).all()  # no density delivered: marked
    assert len(set(sites[:, 0] % 4)) >= 2, "the sites must span two z residues of the stream factor"
    assert len({tuple(s) for s in sites}) == 8


def test_cli_self_check_fails_a_run_that_misses_the_bound(tmp_path):
    """ZD_SelfCheck_tol = 1e-300: the failing branch, without corrupting anything"""
    r, lines, figs, tab = _cli(tmp_path, "RVdoubleZel", "ZD_SelfCheck_tol = 1e-300\n")
    assert r.returncode == 1 and len(lines) == 1 and 0 < figs[0] <= 1e-10 and "self-check FAILED" in r.stderr
    assert tab is not None and tab.shape == (8, 17)  # the table is written before the verdict


def test_every_launch_site_was_launched(zd):
    """every instantiation of the launcher's table — (PLT, PLAW) in the FAST and the general form — and the reduction have been
    launched by the tests of this file"""
    rep = zd.dispatch_report()
    names = [name for (name, _l), cnt in rep.items() if cnt > 0]
    txt = open(os.path.join(ROOT, "zeldovich_plt_amd", "csrc", "zd_kernels_ds.hip")).read()
    variants = re.findall(r"X\((true|false), (true|false)\)", re.search(r"#define DS_VARIANTS\(X\)(.*)", txt).group(1))
    assert len(variants) == 4
    for plt, plaw in variants:
        for fast in ("true", "false"):
            want = "PLT = %s, PLAW = %s, FAST = %s" % (plt, plaw, fast)
            assert any("launch_ds_t" in nm and want in nm for nm in names), "k_ds_sweep<%s> never launched" % want
    assert any("launch_ds_reduce" in nm for nm in names)
