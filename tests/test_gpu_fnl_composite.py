"""ZD_f_NL on the composite grids (PPD = 2^a 3^b 5^c 7^d, one rank) through the composite-length transforms of the reference's
arrays (zd_kernels_np2_ref.hip: k_refq_cols / k_refq_lines) instead of the convolution (Bluestein) transforms of zd_kernels_any.hip.

The second f_NL pass keeps the Nyquist-plane modes live (D = PhiK * M on every mode but k = 0, src/zeldovich.cpp:393-400), so these
runs stay on the reference's two / four arrays and their twin rules; only the line transforms change.  Checked here: every record
against the CPU oracle, the launch sites the runs go through, the old path (forced by the tuning build's ZD_NO_NP2_FNL) against the
new one at full size, the staged API under the call orders of test_gpu_staged_api.py, and poisoned stores."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, WMAP, source_sha

pytestmark = pytest.mark.gpu

TOL = 1e-10
FNL = dict(f_NL=2.0e4, n_s=0.96, Omega_M=0.31)
PLT = dict(qPLT=1, qPLTrescale=1, PLT_target_z=5.0, f_cluster=0.97)
# the composite transforms and the phi round on half-space planes / the convolution transforms and the phi round on the full store
NEW = ("launch_refq_cols_t", "launch_refq_lines_t", "launch_refq_cols_oop_t", "launch_refq_yphi_t")
OLD = ("launch_any_cols_t", "launch_any_lines_t", "launch_any_phi_nl", "launch_any_phik")


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
    """launches of the composite (NEW) and the convolution (OLD) line transforms made by run()"""
    a0, b0 = _launches(zd, NEW, testing), _launches(zd, OLD, testing)
    out = run()
    a1, b1 = _launches(zd, NEW, testing), _launches(zd, OLD, testing)
    return out, {k: a1[k] - a0[k] for k in NEW}, {k: b1[k] - b0[k] for k in OLD}


CASES = [
    (96, dict()), (160, dict(stream_factor=2)), (192, dict()), (224, dict(stream_factor=2)),
    (192, dict(k_cutoff=2.0, stream_factor=4)), (192, dict(k_cutoff=2.0, corner_modes=1)), (160, dict(plt=True, stream_factor=2)),
]


@pytest.mark.parametrize("n,kw", CASES, ids=["%d-%s" % (n, "-".join("%s=%s" % i for i in kw.items()) or "default") for n, kw in CASES])
def test_fnl_composite_matches_the_oracle(zd, oracle, ps, n, kw):
    """every record and density_variance against the oracle, Q = 3, 5, 3, 7 (z lines of N and of N / R); the run goes through the
    composite transforms and not one line through the convolution ones"""
    kw = dict(kw)
    eig = None
    if kw.pop("plt", False):
        eig = oracle.synthetic_eigenmodes(24)
        kw.update(PLT)
    got, new, old = _path_of(zd, lambda: zd.generate(zd.make_params(n, icformat="RVdoubleZel", **FNL, **kw), ps, eig=eig))
    assert all(v > 0 for v in new.values()), new
    assert all(v == 0 for v in old.values()), old
    opk = oracle.pk_from_file(WMAP, 720.0)
    oracle.lib().zdo_pk_set_primordial(C.byref(opk), FNL["n_s"])
    okw = {k: v for k, v in kw.items() if k != "stream_factor"}
    if "corner_modes" in okw:
        okw["CornerModes"] = okw.pop("corner_modes")
    ref = oracle.run(oracle.make_params(n, numblock=2, icformat="RVdoubleZel", **FNL, **okw), opk,
                     eig=eig, eig_ppd=0 if eig is None else eig.shape[0])
    assert np.array_equal(got["records"]["ijk"], ref["records"]["ijk"])
    for f in ("d", "v"):
        for c in range(3):
            assert _rel(got["records"][f][..., c], ref["records"][f][..., c]) < TOL, (f, c)
    assert sorted(got["planes_seen"]) == list(range(n))
    assert abs(got["density_variance"] - ref["density_variance"]) <= TOL * ref["density_variance"]


def test_fnl_composite_dispatch_and_fallbacks(zd, ps):
    """the launch sites of a composite f_NL plan's phi round (composite transforms only), and the configurations that stay on the
    convolution transforms: ZD_StoreMode = reference (phi round and main pass), and a stream factor whose z lines (96 / 32 = 3) have no
    composite transform (the main pass; its phi round runs at stream factor 1) — with the same records as the composite run"""
    def plan_of(**kw):
        pl = zd.Plan(zd.make_params(96, icformat="RVdoubleZel", **FNL, **kw), ps)
        info = (pl.store_mode, pl.passes, pl.plane_step)
        pl.close()
        return info

    info, new, old = _path_of(zd, lambda: plan_of(stream_factor=2))
    assert info == ("reference", 2, 1), info
    assert new["launch_refq_yphi_t"] > 0 and new["launch_refq_cols_oop_t"] > 0 and new["launch_refq_lines_t"] > 0, new
    assert all(v == 0 for v in old.values()), old
    rep = zd.dispatch_report()
    assert any("launch_refq_yphi_t" in nm and "P = 32, E = 16, Q = 3," in nm and c > 0 for (nm, _l), c in rep.items())
    comp = zd.generate(zd.make_params(96, icformat="RVdoubleZel", stream_factor=2, **FNL), ps)
    for kw in (dict(stream_factor=2, store_mode="reference"), dict(stream_factor=32)):
        got, new, old = _path_of(zd, lambda: zd.generate(zd.make_params(96, icformat="RVdoubleZel", **FNL, **kw), ps))
        if "store_mode" in kw:
            assert all(v == 0 for v in new.values()), (kw, new)
        assert old["launch_any_cols_t"] > 0 and old["launch_any_lines_t"] > 0, (kw, old)
        for f in ("d", "v"):
            assert _rel(got["records"][f], comp["records"][f]) < 1e-12, (kw, f)
    # the library's own choice of stream factor for such a run is one the composite transforms take
    p = zd.make_params(96, icformat="RVdoubleZel", **FNL)
    R = zd.load_library().zd_choose_stream_factor(C.byref(p), 1, 1 << 40)
    assert R == 1


def _sample_planes(zd, params, zs, stride):
    got = {}

    def take(z, rec):
        if z in zs:
            got[z] = {f: np.array(rec[f][::stride, ::stride]) for f in ("d", "v")}

    out = zd.generate_planes(params, zd.PowerSpectrum.from_file(WMAP, 720.0), take)
    assert sorted(got) == sorted(zs)
    return got, out


_CHILD = r"""
import os, sys, json
import numpy as np
sys.path.insert(0, os.environ["ZD_ROOT"])
sys.path.insert(0, os.path.join(os.environ["ZD_ROOT"], "tests"))
import zeldovich_plt_amd.api as zd
from test_gpu_fnl_composite import FNL, _sample_planes, _launches, OLD, NEW
n, zs, stride = json.loads(os.environ["ZD_CHILD_ARGS"])
got, out = _sample_planes(zd, zd.make_params(n, icformat="RVdoubleZel", **FNL), zs, stride)
np.savez(os.environ["ZD_CHILD_OUT"], **{"%s_%d" % (f, z): got[z][f] for z in zs for f in ("d", "v")})
print(json.dumps(dict(seconds=out["seconds_total"], old=_launches(zd, OLD), new=_launches(zd, NEW))))
"""


def test_fnl_1728_composite_equals_convolution(zd, tmp_path):
    """PPD = 1728 = 64 * 27 with f_NL = 2e4: the composite path (this process, product library) against the convolution path (a child
    process on the tuning build with ZD_NO_NP2_FNL = 1) on sample planes of records, to 1e-10"""
    import json
    n, zs, stride = 1728, [3, 865, 1727], 3
    lib = os.path.join(ROOT, "zeldovich_plt_amd", "csrc", "build", "libzeldovich_hip_tuning.so")
    assert os.path.exists(lib), "tuning variant not built (make -C zeldovich_plt_amd/csrc tuning; build() does it)"
    assert open(lib + ".srcsha").read().split()[0] == source_sha(), "libzeldovich_hip_tuning.so is older than the kernel sources"
    (new, out), dnew, dold = _path_of(zd, lambda: _sample_planes(zd, zd.make_params(n, icformat="RVdoubleZel", **FNL), zs, stride))
    assert all(v > 0 for v in dnew.values()) and all(v == 0 for v in dold.values()), (dnew, dold)
    outf = str(tmp_path / "old.npz")
    env = dict(os.environ, ZD_LIB_PATH=lib, ZD_NO_NP2_FNL="1", ZD_ROOT=ROOT, ZD_CHILD_OUT=outf, ZD_CHILD_ARGS=json.dumps([n, zs, stride]))
    r = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stderr[-4000:]
    info = json.loads(r.stdout.strip().splitlines()[-1])
    assert all(v > 0 for v in info["old"].values()) and all(v == 0 for v in info["new"].values()), info
    old = np.load(outf)
    print("PPD=%d f_NL: composite %.2f s, convolution %.2f s" % (n, out["seconds_total"], info["seconds"]))
    for z in zs:
        for f in ("d", "v"):
            a, b = new[z][f], old["%s_%d" % (f, z)]
            assert np.abs(b).max() > 0
            assert np.abs(a - b).max() <= 1e-10 * np.abs(b).max(), (z, f)


def test_fnl_composite_staged_call_orders(zd, ps):
    """the staged API on a composite f_NL plan (PPD = 96, R = 2: z lines of 48) under the call orders O1 ... O6 of
    test_gpu_staged_api.py — byte-identical to O1 — and O1 byte-identical to zd_generate"""
    import test_gpu_staged_api as S
    fam = S.Family(96, "RVdoubleZel", dict(stream_factor=2, **FNL), False, 0, ("reference", 1, 2), False, None)
    p = zd.make_params(fam.n, icformat=fam.fmt, **fam.kw)
    plan, new, old = _path_of(zd, lambda: zd.Plan(p, ps))
    try:
        assert (plan.store_mode, plan.plane_step, plan.passes) == fam.expect
        o1, new, old = _path_of(zd, lambda: S._run(zd, plan, fam, "O1"))
        assert new["launch_refq_cols_t"] > 0 and new["launch_refq_lines_t"] > 0 and all(v == 0 for v in old.values()), (new, old)
        for order in ("O1", "O2", "O3", "O4", "O5", "O6"):
            S._same_as_o1(S._run(zd, plan, fam, order), o1, order)
        gen = zd.generate(p, ps)
        assert gen["records"].tobytes() == o1["rec"].cpu().numpy().tobytes()
        assert np.array_equal(gen["max_disp"], o1["stats"]["max_disp"])
        assert abs(gen["density_variance"] - o1["stats"]["density_variance"]) <= S.VAR_TOL * abs(o1["stats"]["density_variance"])
    finally:
        plan.close()


def test_fnl_composite_from_poisoned_memory(zd, ps):
    """PPD = 192, k_cutoff = 2 in the -DZD_TESTING library with stores, rings and the phi field starting as NaN bytes
    (zd_test_poison): finite records equal to the product library's run"""
    p = zd.make_params(192, icformat="RVdoubleZel", k_cutoff=2.0, stream_factor=2, **FNL)
    base = zd.generate(p, ps)
    T = zd.load_testing_library()
    T.zd_test_poison(1)
    try:
        got, new, old = _path_of(zd, lambda: zd.generate(p, ps, testing=True), testing=True)
    finally:
        T.zd_test_poison(0)
    assert all(v > 0 for v in new.values()) and all(v == 0 for v in old.values()), (new, old)
    for f in ("d", "v"):
        assert np.isfinite(got["records"][f]).all(), f
        assert _rel(got["records"][f], base["records"][f]) < 1e-13, f
    assert abs(got["density_variance"] - base["density_variance"]) <= 1e-12 * base["density_variance"]


def _refq_sizes():
    """(P, Q, W) of REFQ_SIZES (zd_kernels_np2_ref.hip)"""
    src = open(os.path.join(ROOT, "zeldovich_plt_amd", "csrc", "zd_kernels_np2_ref.hip")).read()
    body = src[src.index("#define REFQ_SIZES(X)"):]
    body = body[:body.index("\n\n")]
    sizes = [tuple(int(v) for v in m) for m in re.findall(r"X\((\d+), (\d+), (\d+)\)", body)]
    assert len(sizes) > 60
    return sizes


def test_every_composite_line_transform_against_numpy(zd):
    """every (P, Q, W) of REFQ_SIZES through k_refq_cols (strided lines, a ragged batch: 2 W + 1 columns) and k_refq_lines (three
    contiguous lines), against numpy's inverse DFT (zd_test_fft axis kinds 3 / 4 of the -DZD_TESTING library)"""
    T = zd.load_testing_library()
    rng = np.random.default_rng(7)
    bad = []
    for P, Q, W in _refq_sizes():
        n = P * Q
        for kind, lines in ((3, 2 * W + 1), (4, 3)):
            x = rng.standard_normal((lines, n)) + 1j * rng.standard_normal((lines, n))
            ref = np.fft.ifft(x, axis=1) * n
            hin = np.ascontiguousarray(x.T if kind == 3 else x)
            out = np.zeros_like(hin)
            assert T.zd_test_fft(n, lines, kind, hin.ctypes.data, out.ctypes.data) == 0, (n, kind)
            got = out.T if kind == 3 else out
            err = np.abs(got - ref).max() / np.abs(ref).max()
            if not err < 1e-12:
                bad.append((P, Q, W, kind, err))
    assert not bad, bad


@pytest.mark.parametrize("n", [2304, 2400])
def test_fnl_round_trip_identity_at_large_composite_sizes(zd, ps, n):
    """PPD = 2304 = 256 * 9 and 2400 = 32 * 75 with f_NL = 1e-300 on one GPU: the nonlinear term vanishes, and the second pass must
    reproduce the ordinary composite ZA run — records of sample planes to 1e-10.  The phi round holds half-space planes beside PhiK
    (~8 N^3 + 8 N^3 bytes: 222 GB at 2400); the full phi store of the convolution path (16 N^3 + 8 N^3: 334 GB at 2400) does not fit
    one MI355X at 2400 (at 2304 it peaks at 297 GB of the 309 GB).
    Not covered here: the phi^2 term itself (it vanishes with f_NL = 1e-300); test_gpu_fnl_closed_form.py checks it at 960 ... 2400
    against a closed form with a second wave as large as the first."""
    zs, stride = [3, n // 2 + 1, n - 1], 4
    kw = dict(icformat="RVdoubleZel", n_s=0.96, Omega_M=0.31)
    a, _ = _sample_planes(zd, zd.make_params(n, **kw), zs, stride)
    (b, out), new, old = _path_of(zd, lambda: _sample_planes(zd, zd.make_params(n, f_NL=1e-300, **kw), zs, stride))
    assert all(v > 0 for v in new.values()) and all(v == 0 for v in old.values()), (new, old)
    print("PPD=%d f_NL: %.2f s grid->displacements, R = %d" % (n, out["seconds_total"], out["stream_factor"]))
    for z in zs:
        for f in ("d", "v"):
            assert np.abs(a[z][f]).max() > 0
            assert np.abs(a[z][f] - b[z][f]).max() <= 1e-10 * np.abs(a[z][f]).max(), (z, f)
