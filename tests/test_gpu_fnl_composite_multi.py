"""ZD_f_NL on the composite grids (PPD = 2^a 3^b 5^c 7^d) on several ranks: the reference's arrays split over the ranks with the chunk
semantics of the power-of-two store (zd_device.h AnyChunks), every line through the composite transforms of zd_kernels_np2_ref.hip —
the z lines scattered into the chunked send store (k_refq_scatter), y columns gathered over the chunks of a ring slot (k_refq_ycols), the
phi round's x lines with phi + f_NL phi^2 (k_refq_xphi), the particle epilogue with the chunked row map (k_refq_emit).  Ranks share
this GPU (local transport; loopback: the RCCL branch on its in-process emulation)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, WMAP
from test_gpu_fnl_composite import _refq_sizes, _sample_planes

pytestmark = pytest.mark.gpu

TOL = 1e-10
FNL = dict(f_NL=2.0e4, n_s=0.96, Omega_M=0.31)
PLT = dict(qPLT=1, qPLTrescale=1, PLT_target_z=5.0, f_cluster=0.97)
NEW = ("launch_refq_scatter", "launch_refq_ycols_t", "launch_refq_xphi_t", "launch_refq_emit", "launch_refq_cols_t", "launch_refq_lines_t",
       "launch_refq_cols_oop_t")
OLD = ("launch_any_cols_t", "launch_any_lines_t", "launch_any_phi_nl", "launch_any_phik", "launch_any_scatter", "launch_any_emit")


@pytest.fixture(scope="module")
def zd():
    import zeldovich_plt_amd.api as api
    api.load_library()
    return api


@pytest.fixture(scope="module")
def ps(zd):
    return zd.PowerSpectrum.from_file(WMAP, 720.0)


def _rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _launches(zd, names, testing=False):
    return {k: sum(c for (nm, _l), c in zd.dispatch_report(testing).items() if k in nm) for k in names}


def _path_of(zd, run, testing=False):
    a0, b0 = _launches(zd, NEW, testing), _launches(zd, OLD, testing)
    out = run()
    a1, b1 = _launches(zd, NEW, testing), _launches(zd, OLD, testing)
    return out, {k: a1[k] - a0[k] for k in NEW}, {k: b1[k] - b0[k] for k in OLD}


def _oracle(oracle, n, kw, eig):
    opk = oracle.pk_from_file(WMAP, 720.0)
    oracle.lib().zdo_pk_set_primordial(C.byref(opk), FNL["n_s"])
    okw = {k: v for k, v in kw.items() if k not in ("stream_factor", "exchange_planes", "ngpu")}
    if "corner_modes" in okw:
        okw["CornerModes"] = okw.pop("corner_modes")
    return oracle.run(oracle.make_params(n, numblock=2, icformat="RVdoubleZel", **FNL, **okw), opk,
                      eig=eig, eig_ppd=0 if eig is None else eig.shape[0])


def _check(got, ref, n):
    assert np.array_equal(got["records"]["ijk"], ref["records"]["ijk"])
    for f in ("d", "v"):
        assert np.isfinite(got["records"][f]).all(), f
        for c in range(3):
            assert _rel(got["records"][f][..., c], ref["records"][f][..., c]) < TOL, (f, c)
    assert sorted(got["planes_seen"]) == list(range(n))
    assert abs(got["density_variance"] - ref["density_variance"]) <= TOL * ref["density_variance"]


CASES = [
    (2, 96, dict()),
    (4, 192, dict(stream_factor=2, exchange_planes=3)),           # several plane groups both ways, in the phi round and the main pass
    (2, 160, dict(plt=True, stream_factor=2)),
    (2, 224, dict(k_cutoff=2.0)),
    (4, 192, dict(k_cutoff=2.0, corner_modes=1)),
]


@pytest.mark.parametrize("ngpu,n,kw", CASES,
                         ids=["%dx%d-%s" % (g, n, "-".join("%s=%s" % i for i in kw.items()) or "default") for g, n, kw in CASES])
def test_fnl_composite_on_several_ranks(zd, oracle, ps, ngpu, n, kw):
    """every record, density_variance and the planes delivered against the oracle; the run goes through the chunked kernels and
    not one line through the convolution transforms or the one-rank store's scatter / epilogue"""
    kw = dict(kw)
    eig = None
    if kw.pop("plt", False):
        eig = oracle.synthetic_eigenmodes(24)
        kw.update(PLT)
    got, new, old = _path_of(zd, lambda: zd.generate(zd.make_params(n, icformat="RVdoubleZel", ngpu=ngpu, **FNL, **kw), ps, eig=eig))
    assert all(v > 0 for v in new.values()), new
    assert all(v == 0 for v in old.values()), old
    _check(got, _oracle(oracle, n, kw, eig), n)


def test_fnl_composite_rccl_branch_on_loopback(zd, oracle, ps):
    """the RCCL branch of the phi round's forward and reverse exchange and of the main pass (in-process emulation of its calls)"""
    n, kw = 192, dict(stream_factor=2, exchange_planes=5)
    got, new, old = _path_of(zd, lambda: zd.generate(zd.make_params(n, icformat="RVdoubleZel", ngpu=4, **FNL, **kw), ps, loopback=True),
                             testing=True)
    assert all(v > 0 for v in new.values()) and all(v == 0 for v in old.values()), (new, old)
    _check(got, _oracle(oracle, n, kw, None), n)


def test_fnl_composite_from_poisoned_memory(zd, oracle, ps):
    """stores, rings and the phi field start as NaN bytes (zd_test_poison): nothing unwritten is read — the twin slot of ky = 0 (the
    Nyquist row) included"""
    n = 160
    T = zd.load_testing_library()
    T.zd_test_poison(1)
    try:
        got = zd.generate(zd.make_params(n, icformat="RVdoubleZel", ngpu=2, **FNL), ps, testing=True)
    finally:
        T.zd_test_poison(0)
    _check(got, _oracle(oracle, n, {}, None), n)


@pytest.mark.parametrize("n,ngpu", [(1728, 2), (960, 4)])
def test_fnl_composite_several_ranks_equal_one_rank(zd, n, ngpu):
    """full-ish sizes: the same job on one rank (half-space phi round, the one-rank store) and on several: records of sample planes
    within 1e-12 of the field's maximum, density_variance to 1e-11"""
    zs, stride = [0, n // 2, n // 2 + 1, n - 1], 3
    kw = dict(icformat="RVdoubleZel", **FNL)
    a, oa = _sample_planes(zd, zd.make_params(n, **kw), zs, stride)
    (b, ob), new, old = _path_of(zd, lambda: _sample_planes(zd, zd.make_params(n, ngpu=ngpu, **kw), zs, stride))
    assert all(v > 0 for v in new.values()) and all(v == 0 for v in old.values()), (new, old)
    print("PPD=%d f_NL: 1 rank %.2f s, %d ranks on one GPU %.2f s" % (n, oa["seconds_total"], ngpu, ob["seconds_total"]))
    for z in zs:
        for f in ("d", "v"):
            assert np.abs(a[z][f]).max() > 0
            assert np.abs(a[z][f] - b[z][f]).max() <= 1e-12 * np.abs(a[z][f]).max(), (z, f)
    assert abs(oa["density_variance"] - ob["density_variance"]) <= 1e-11 * oa["density_variance"]


def test_chunked_y_columns_against_numpy(zd):
    """k_refq_ycols alone (zd_test_ycols) for every length of REFQ_SIZES at G = 2, 4, 8: the inverse transform with ky = N/2 read as
    zero (NaN there in the input) and every row written; and the phi round's second y transform, which writes the rows ky < N/2 only —
    checked as the forward transform it stands for (the conjugate of the inverse transform of the conjugate)"""
    T = zd.load_testing_library()
    rng = np.random.default_rng(11)
    bad = []
    for P, Q, W in _refq_sizes():
        n = P * Q
        ncols, nimg = 2 * W + 1, 2
        for G in (2, 4, 8):
            x = rng.standard_normal((nimg, n, ncols)) + 1j * rng.standard_normal((nimg, n, ncols))
            # mode 0: inverse, the Nyquist row never read
            xin = x.copy()
            xin[:, n // 2, :] = np.nan
            out = np.zeros_like(xin)
            assert T.zd_test_ycols(n, G, ncols, nimg, 0, xin.ctypes.data, out.ctypes.data) == 0, (n, G)
            x0 = x.copy()
            x0[:, n // 2, :] = 0
            ref = np.fft.ifft(x0, axis=1) * n
            err0 = np.abs(out - ref).max() / np.abs(ref).max()
            # mode 1 as the forward transform: conj(inverse(conj x)), rows ky < N/2
            xc = np.ascontiguousarray(np.conj(x))
            out = np.zeros_like(xc)
            assert T.zd_test_ycols(n, G, ncols, nimg, 1, xc.ctypes.data, out.ctypes.data) == 0, (n, G)
            ref = np.fft.fft(x, axis=1)[:, : n // 2]
            err1 = np.abs(np.conj(out[:, : n // 2]) - ref).max() / np.abs(ref).max()
            untouched = np.array_equal(out[:, n // 2:], xc[:, n // 2:])
            if not (err0 < 1e-12 and err1 < 1e-12 and untouched):
                bad.append((P, Q, W, G, err0, err1, untouched))
    assert not bad, bad


PAR = """BoxSize = 720
CPD = 7
ICFormat = "RVdoubleZel"
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
ZD_qdensity = 0
ZD_f_NL = 2e4
ZD_n_s = 0.96
Omega_M = 0.31
ZD_NumGPU = 2
"""


def test_cli_fnl_composite_on_two_gpus(tmp_path, oracle):
    """`zeldovich` on a .par with ZD_NumGPU = 2, PPD = 96 and ZD_f_NL = 2e4: the ic_* files against the oracle"""
    n, cpd = 96, 7
    out = tmp_path / "ic"
    out.mkdir()
    par = tmp_path / "t.par"
    par.write_text(PAR % dict(out=out, np=n ** 3, pk=WMAP))
    exe = os.path.join(ROOT, "zeldovich_plt_amd", "csrc", "build", "zeldovich")
    r = subprocess.run([exe, str(par)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    ref = _oracle(oracle, n, {}, None)
    dt = oracle.RECORD_DTYPES["RVdoubleZel"]
    files = sorted(int(f.name[3:]) for f in out.iterdir() if f.name.startswith("ic_"))
    assert files == sorted(set(z * cpd // n for z in range(n)))
    for f in files:
        zs = [z for z in range(n) if z * cpd // n == f]
        got = np.fromfile(out / ("ic_%d" % f), dtype=dt).reshape(len(zs), n, n)
        want = ref["records"][zs]
        assert np.array_equal(got["ijk"], want["ijk"])
        for fld in ("d", "v"):
            assert np.abs(got[fld] - want[fld]).max() <= TOL * np.abs(want[fld]).max(), (f, fld)


@pytest.mark.parametrize("n,kw,what", [(96, dict(store_mode="reference"), "ZD_StoreMode = reference"),
                                        (1000, dict(), "composite transforms")])
def test_fnl_composite_multi_refusals(zd, ps, capfd, n, kw, what):
    """configurations that keep the convolution transforms (ZD_StoreMode = reference; a PPD without composite transforms) run on one
    GPU only: several ranks refuse them at once, saying why"""
    import time
    t0 = time.time()
    with pytest.raises(RuntimeError):
        zd.generate(zd.make_params(n, icformat="RVdoubleZel", ngpu=2, **FNL, **kw), ps)
    assert time.time() - t0 < 10
    err = capfd.readouterr().err
    assert what in err and "one GPU" in err, err


def test_fnl_composite_oneslab_stays_one_gpu(zd, ps):
    """ZD_qoneslab finishes one slab on one GPU whatever ZD_NumGPU says (zd_generate): so it does with f_NL on a composite grid"""
    p = dict(icformat="RVdoubleZel", qoneslab=5, **FNL)
    a = zd.generate(zd.make_params(96, **p), ps)
    b = zd.generate(zd.make_params(96, ngpu=2, **p), ps)
    assert a["planes_seen"] == b["planes_seen"] == [5]
    assert a["records"][5].tobytes() == b["records"][5].tobytes()
