"""GPU: the pair form of the field store's y stage and the paired ring rows (zd_device.h ring_pair_w, k_yfft_f PAIR, k_xfft_seq PW).

At PPD = 1024, 2048 and 4096 the ZA field store computes column x < N/2 and its mirror N - x from one fetch of the potentials,
    A(N - x) = conj FFT_y[(i kx + ky) U],    C(N - x) = conj FFT_y[i U0 + U1],
and writes the two side by side in the ring, which the x stage reads back by position.  A wrong sign, conjugate or position is an
error of order one in half of the columns, so everything here is compared at the suite's parity bound, 1e-10 of the field maximum
(float64 records), against the same job on the reference's arrays (ZD_StoreMode = reference: plain y / x kernels, no ring), against
closed-form plane waves (1e-12, the bound of the PPD = 4096 one-mode tests), and against the direct sum over every mode.

PPD = 1024 is the smallest size on the paired route (W = 8: four pairs per workgroup).  The W = 4 form (two pairs per workgroup)
otherwise runs at PPD = 4096 only — where the direct-sum fixture, the one-mode tests and the band-power test go through it — and is
run here at PPD = 1024 through zd_test_ring_pair_w of the -DZD_TESTING library."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_baseline_regime as regime
from conftest import WMAP, OneGroupApi
from test_gpu_baseline_regime import _planes
from test_gpu_parity import TOL, _rel
from test_gpu_site_sum import records_at

pytestmark = pytest.mark.gpu
BOX = 720.0
N = 1024
FMT = "RVdoubleZel"


@pytest.fixture(scope="module")
def zd():
    import zeldovich_plt_amd.api as api
    api.load_library()
    return OneGroupApi(api)


@pytest.fixture(scope="module")
def ps(zd):
    return zd.PowerSpectrum.from_file(WMAP, BOX)


@pytest.fixture(autouse=True, scope="module")
def _release_the_shared_store():
    yield
    regime._drop_store()


def _launched(zd, launcher, *words, testing=False):
    rep = zd.dispatch_report(testing=testing)
    return sum(cnt for (name, _l), cnt in rep.items() if launcher in name and all(w in name for w in words))


_REF = {}


def _reference(zd, ps, n, zs, R, **kw):
    """planes of the same job on the reference's arrays, computed once per job"""
    key = (n, tuple(zs), R, tuple(sorted(kw.items())))
    if key not in _REF:
        _REF[key], info = _planes(zd, ps, n, zs, fmt=FMT, stream_factor=R, store_mode="reference", **kw)
        assert info["narray"] != 3
    return _REF[key]


def _same_planes(got, want, zs, n):
    for z in zs:
        a, b = got[z], want[z]
        assert np.array_equal(a["ijk"], b["ijk"]) and np.array_equal(a["ijk"][..., 0], np.full((n, n), z))
        for f in ("d", "v"):
            assert np.abs(b[f]).max() > 0
            err = _rel(a[f], b[f])
            print("  plane %d, %s: max |paired - reference| / max = %.3g" % (z, f, err))
            assert err <= TOL, (z, f, err)


def _pass_planes(zd, ps, n, R):
    """two planes that share a store plane (the two z-residues of a pass), one of another pass where there is one, the last plane"""
    plan = zd.Plan(zd.make_params(n, icformat=FMT, stream_factor=R), ps)
    try:
        assert plan.store_mode == "fields" and plan.plane_step == 2
        zs = [plan.plane_z(0, 4), plan.plane_z(0, 5)]
        if plan.passes > 1:
            zs.append(plan.plane_z(1, 2))
    finally:
        plan.close()
    assert zs[0] % R != zs[1] % R
    return sorted(set(zs + [n - 1]))


@pytest.mark.parametrize("R", [2, 4])
def test_random_field_equals_the_reference_arrays(zd, ps, R):
    zs = _pass_planes(zd, ps, N, R)
    before = _launched(zd, "launch_yfft_f_t", "N = 1024, E = 16, W = 8,", "PAIR = true")
    got, info = _planes(zd, ps, N, zs, fmt=FMT, stream_factor=R)
    assert info["narray"] == 3 and info["R"] == R
    assert _launched(zd, "launch_yfft_f_t", "N = 1024, E = 16, W = 8,", "PAIR = true") > before
    assert _launched(zd, "launch_xfft_seq_t", "N = 1024, E = 16, PW = 8") > 0
    _same_planes(got, _reference(zd, ps, N, zs, R), zs, N)


def test_reductions_equal_the_reference_arrays(zd, ps):
    """sum delta^2, max_disp and its lattice site over every particle"""
    a = zd.generate(zd.make_params(N, icformat=FMT, stream_factor=2), ps, collect=False)
    b = zd.generate(zd.make_params(N, icformat=FMT, stream_factor=2, store_mode="reference"), ps, collect=False)
    print("density_variance", a["density_variance"], b["density_variance"], "max_disp", a["max_disp"], b["max_disp"], a["max_disp_index"])
    assert abs(a["density_variance"] - b["density_variance"]) <= TOL * b["density_variance"]
    assert _rel(a["max_disp"], b["max_disp"]) < TOL
    assert np.array_equal(a["max_disp_index"], b["max_disp_index"])


def test_k_cutoff_2_dead_tiles_and_half_dead_groups(zd, ps):
    """ZD_k_cutoff = 2: half of the tiles are dead, the x stage takes zeros for their columns, and the groups at the edge of the dead
    range are half dead; from a store that starts as NaN bytes"""
    zs = _pass_planes(zd, ps, N, 2)
    got, info = _planes(zd, ps, N, zs, fmt=FMT, stream_factor=2, k_cutoff=2.0)
    assert info["narray"] == 3
    _same_planes(got, _reference(zd, ps, N, zs, 2, k_cutoff=2.0), zs, N)


def _plane_wave(zd, ps, n, mode, z, **kw):
    """|record - closed form| / scale of a one-mode run, q_j(x) = -2 (k_j fund / k^2) (Re D sin t + Im D cos t), t = 2 pi k.x / N,
    v = q at f_cluster = 1 (the closed form of test_ppd6912_on_one_gpu_plane_waves), every site of plane z"""
    D = zd.test_modes(zd.make_params(n), ps, [mode])[0]
    got, info = _planes(zd, ps, n, [z], fmt=FMT, qonemode=1, one_mode=mode, stream_factor=2, **kw)
    assert info["narray"] == 3 and abs(D) > 0
    fund = 2 * np.pi / BOX
    k2 = sum(m * m for m in mode) * fund * fund
    yy, xx = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    t = 2 * np.pi * ((mode[0] * xx + mode[1] * yy + mode[2] * z) % n) / n
    wave = -2.0 * (D.real * np.sin(t) + D.imag * np.cos(t))
    scale = max(abs(m) for m in mode) * fund / k2 * np.abs(wave).max()
    err = 0.0
    for j in range(3):  # records hold (qz, qy, qx)
        want = mode[j] * fund / k2 * wave
        err = max(err, np.abs(got[z]["d"][..., 2 - j] - want).max() / scale, np.abs(got[z]["v"][..., 2 - j] - want).max() / scale)
    return err


MODES = [(5, 3, -7), (-5, 3, 7), (0, 2, 0), (1, 1, 0), (N // 2 - 1, 1, 1), (-(N // 2 - 1), 1, 1), (3, N // 2 - 1, 0)]


@pytest.mark.parametrize("mode", MODES, ids=["%d_%d_%d" % m for m in MODES])
def test_one_mode_is_its_plane_wave(zd, ps, mode):
    """+-kx pairs, the self-mirror column kx = 0, the last live columns beside the dead one, the last live row"""
    err = _plane_wave(zd, ps, N, mode, N // 2 + 5)
    print("mode", mode, "max |record - plane wave| / scale = %.3g" % err)
    assert err <= 1e-12


def test_records_equal_the_direct_sum_at_the_edges_of_the_pairing(zd, ps):
    """x on both sides of 0 and N/2 (column 0 and its mirror slot, the first and the last pair), y likewise, two planes of different
    residue: records against the sum over every mode"""
    h = N // 2
    sites = [(z, y, x) for z in (6, h + 1) for y in (0, 1, h, N - 1) for x in (0, 1, h - 1, h, h + 1, N - 1)]
    plan = zd.Plan(zd.make_params(N, icformat=FMT, stream_factor=2), ps)
    try:
        assert plan.store_mode == "fields"
        want = records_at(zd, plan, N, sites, fmt=FMT)
        got = plan.direct_sum(sites)
    finally:
        plan.close()
    scale = np.abs(got[:, :3]).max()
    fq = np.abs(got[:, :6] - want).max() / scale
    print("48 sites: max |record - direct sum| / max|q| = %.3g" % fq)
    assert len(sites) == 48 and scale > 1e-4 and fq <= TOL


def test_two_ranks_as_one_group(zd, ps):
    """ZD_NumGPU = 2 as ONE group on the in-process emulation of the RCCL calls: rows ky = rank mod 2, the ring filled from two chunks"""
    zs = _pass_planes(zd, ps, N, 2)
    T = zd.load_testing_library()
    p = zd.make_params(N, icformat=FMT, stream_factor=2, ngpu=2, exchange_planes=64)
    dt = zd.RECORD_DTYPES[FMT]
    kept = {}

    def _cb(user, z, nrec, recp, densp):
        if int(z) in zs and recp:
            buf = (C.c_char * (nrec * dt.itemsize)).from_address(recp)
            kept[int(z)] = np.frombuffer(buf, dtype=dt).reshape(N, N).copy()
        return 0

    st = zd.ZdStats()
    before = _launched(zd, "launch_yfft_f_t", "N = 1024, E = 16, W = 8,", "PAIR = true", testing=True)
    assert T.zd_test_generate_loopback(C.byref(p), C.byref(ps.pk), None, 0, zd.SLAB_CB(_cb), None, C.byref(st)) == 0
    assert _launched(zd, "launch_yfft_f_t", "N = 1024, E = 16, W = 8,", "PAIR = true", testing=True) > before
    assert sorted(kept) == zs
    _same_planes(kept, _reference(zd, ps, N, zs, 2), zs, N)


def _two_pairs_per_workgroup(zd, fn):
    T = zd.load_testing_library()
    T.zd_test_ring_pair_w(4)
    try:
        before = _launched(zd, "launch_yfft_f_t", "N = 1024, E = 16, W = 4,", "PAIR = true", testing=True)
        out = fn()
        assert _launched(zd, "launch_yfft_f_t", "N = 1024, E = 16, W = 4,", "PAIR = true", testing=True) > before
        assert _launched(zd, "launch_xfft_seq_t", "N = 1024, E = 16, PW = 4", testing=True) > 0
        return out
    finally:
        T.zd_test_ring_pair_w(0)


def test_two_pairs_per_workgroup_random_field(zd, ps):
    """the W = 4 form of PPD = 4096 at PPD = 1024 (the plans of _planes(poison=True) come from the -DZD_TESTING library)"""
    zs = _pass_planes(zd, ps, N, 2)
    got, info = _two_pairs_per_workgroup(zd, lambda: _planes(zd, ps, N, zs, fmt=FMT, stream_factor=2, poison=True))
    assert info["narray"] == 3
    _same_planes(got, _reference(zd, ps, N, zs, 2), zs, N)


def test_two_pairs_per_workgroup_plane_wave(zd, ps):
    err = _two_pairs_per_workgroup(zd, lambda: _plane_wave(zd, ps, N, (-5, 3, 7), N // 2 + 5, poison=True))
    print("W = 4, mode (-5, 3, 7): max |record - plane wave| / scale = %.3g" % err)
    assert err <= 1e-12


def test_random_field_at_2048(zd, ps):
    n, R = 2048, 16  # (R = 16: the reference's arrays of the comparison are 17 GB, allocated and filled in a second, not 137)
    zs = _pass_planes(zd, ps, n, R)
    got, info = _planes(zd, ps, n, zs, fmt=FMT, stream_factor=R)
    assert info["narray"] == 3 and _launched(zd, "launch_yfft_f_t", "N = 2048, E = 16, W = 8,", "PAIR = true") > 0
    _same_planes(got, _reference(zd, ps, n, zs, R), zs, n)


@pytest.mark.parametrize("n,w,R", [(1024, 8, 2), (2048, 8, 8), (4096, 4, 64)])  # (R: stores of 5, 20 and 40 GB)
def test_the_plain_form_still_serves_the_plt_field_store(zd, ps, oracle, n, w, R):
    """the unpaired instantiations at the paired sizes stay reachable through ZD_StoreMode = fields with PLT (six potentials, plain
    ring rows): one plane against the packed PLT arrays of the same job"""
    eig = oracle.synthetic_eigenmodes(32)
    kw = dict(qPLT=1, qPLTrescale=1, PLT_target_z=5.0, eig=eig, fmt=FMT, stream_factor=R)
    z = n // 2 + 3
    before = _launched(zd, "launch_yfft_f_t", "N = %d, E = 16, W = %d," % (n, w), "PAIR = false")
    got, info = _planes(zd, ps, n, [z], stride=4, store_mode="fields", **kw)
    assert _launched(zd, "launch_yfft_f_t", "N = %d, E = 16, W = %d," % (n, w), "PAIR = false") > before
    want, _ = _planes(zd, ps, n, [z], stride=4, **kw)
    for f in ("d", "v"):
        err = _rel(got[z][f], want[z][f])
        print("PPD %d PLT, %s: max |field store - packed arrays| / max = %.3g" % (n, f, err))
        assert np.abs(want[z][f]).max() > 0 and err <= TOL
