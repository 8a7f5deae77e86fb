"""Second-order displacements (ZD_q2LPT) without a GPU: the numpy restatement of the definition (tests/lpt2_ref.py) pinned by a
closed form, the three parameter keys, the defaults of the two coefficients, and the routing — what is refused, what is accepted,
and that nothing changes for a job without ZD_q2LPT."""
import ctypes as C

import numpy as np
import pytest

import lpt2_ref
from conftest import WMAP

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
ZD_Pk_sigma = 0.0210839935761
ZD_Pk_smooth = 0.0
ZD_Seed = 12346
ZD_Version = 2
"""


# ---- the numpy reference against a closed form ----------------------------------------------------------------------------
def _two_waves(n, boxsize, a, b, k1, k2):
    """psi1 = -grad phi for phi = a cos(k1.x) + b cos(k2.x) on the lattice, and the closed form of its source
    S = a b |k1 x k2|^2 cos(k1.x) cos(k2.x); k1, k2 integer wavevectors in array-axis order"""
    fund = 2.0 * np.pi / boxsize
    r = np.arange(n) * (boxsize / n)
    pos = np.meshgrid(r, r, r, indexing="ij")
    q = np.zeros((n, n, n, 3))
    th = []
    for amp, k in ((a, k1), (b, k2)):
        kp = np.array(k, dtype=np.float64) * fund
        t = kp[0] * pos[0] + kp[1] * pos[1] + kp[2] * pos[2]
        th.append(t)
        for j in range(3):
            q[..., j] += amp * kp[j] * np.sin(t)
    cr = np.cross(np.array(k1, dtype=np.float64) * fund, np.array(k2, dtype=np.float64) * fund)
    return q, a * b * np.dot(cr, cr) * np.cos(th[0]) * np.cos(th[1])


@pytest.mark.parametrize("k1,k2", [((1, 2, 0), (0, -1, 3)), ((3, 0, -1), (1, 1, 1)), ((2, -3, 1), (-1, 2, 3))])
def test_source_of_two_plane_waves_is_the_closed_form(k1, k2):
    """N = 16, 2 max|k| < N/2: the products alias nowhere, so the lattice source is the continuum one"""
    n, box = 16, 720.0
    assert 2 * max(map(abs, k1 + k2)) < n // 2
    q, want = _two_waves(n, box, 0.7, -1.3, k1, k2)
    got = lpt2_ref.source(q, box)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    # and the displacement: div psi2 = -gamma S, psi2 = i k gamma S / k^2 mode by mode (S has the modes k1 + k2 and k1 - k2)
    fund = 2.0 * np.pi / box
    r = np.arange(n) * (box / n)
    pos = np.meshgrid(r, r, r, indexing="ij")
    gamma = 3.0 / 7.0
    psi2 = np.zeros((n, n, n, 3))
    cr = np.cross(np.array(k1, dtype=np.float64) * fund, np.array(k2, dtype=np.float64) * fund)
    for sgn in (1, -1):
        kk = (np.array(k1) + sgn * np.array(k2)).astype(np.float64) * fund
        t = kk[0] * pos[0] + kk[1] * pos[1] + kk[2] * pos[2]
        for j in range(3):  # S = A (cos(k+ x) + cos(k- x)) / 2  ->  psi2_j = -gamma A/2 k_j sin(k x) / k^2
            psi2[..., j] += -gamma * 0.5 * 0.7 * -1.3 * np.dot(cr, cr) * kk[j] / np.dot(kk, kk) * np.sin(t)
    got2 = lpt2_ref.second_order(q, box, lpt2_ref.alive_mask(n, box))
    assert np.abs(got2 - psi2).max() <= 1e-12 * np.abs(psi2).max()


def test_source_of_a_single_wave_vanishes():
    n, box = 16, 720.0
    q, _ = _two_waves(n, box, 0.9, 0.0, (2, -1, 3), (0, 0, 0))
    s = lpt2_ref.source(q, box)
    grad_scale = (np.abs(q).max() * 2 * np.pi / box * 4) ** 2  # the size of the products that cancel
    assert np.abs(s).max() <= 1e-12 * grad_scale
    assert np.abs(lpt2_ref.second_order(q, box, lpt2_ref.alive_mask(n, box))).max() <= 1e-12 * np.abs(q).max()


def test_alive_mask_is_the_zero_rule():
    m = lpt2_ref.alive_mask(32, 720.0)
    assert not m[0, 0, 0] and not m[16].any() and not m[:, 16].any() and not m[:, :, 16].any()
    assert m[1, 0, 0] and m[15, 2, 31] and not m[15, 15, 15]       # the sphere |k| < N/2
    m2 = lpt2_ref.alive_mask(32, 720.0, k_cutoff=2.0)
    assert m2[7, 0, 0] and not m2[8, 0, 0] and not m2[6, 6, 0] and m2[5, 5, 0]
    assert lpt2_ref.alive_mask(32, 720.0, corner_modes=1)[15, 15, 15]


# ---- parameter reader -----------------------------------------------------------------------------------------------------
def _read(tmp_path, extra):
    import zeldovich_plt_amd.api as zd
    par = tmp_path / "t.par"
    par.write_text(PAR % dict(out=tmp_path / "ic", pk=WMAP) + extra)
    return zd.params_from_file(str(par))[0]


def test_parameter_keys(tmp_path):
    p = _read(tmp_path, "")
    assert (p.q2LPT, p.lpt2_ratio, p.lpt2_f2) == (0, 0.0, 0.0)
    p = _read(tmp_path, "ZD_q2LPT = 1\n")
    assert (p.q2LPT, p.lpt2_ratio, p.lpt2_f2) == (1, 0.0, 0.0)
    p = _read(tmp_path, "ZD_q2LPT = 1\nZD_2LPT_D2 = -0.4287\nZD_2LPT_f2 = 1.93\n")
    assert (p.q2LPT, p.lpt2_ratio, p.lpt2_f2) == (1, -0.4287, 1.93)


def test_make_params_mirrors_the_fields():
    import zeldovich_plt_amd.api as zd
    p = zd.make_params(64)
    assert (p.q2LPT, p.lpt2_ratio, p.lpt2_f2) == (0, 0.0, 0.0)
    p = zd.make_params(64, q2LPT=1, lpt2_ratio=-0.5, lpt2_f2=1.7)
    assert (p.q2LPT, p.lpt2_ratio, p.lpt2_f2) == (1, -0.5, 1.7)
    # appended at the end, behind pass_groups, with the C compiler's alignment of the two doubles
    assert zd.ZdParams.q2LPT.offset == zd.ZdParams.pass_groups.offset + 4
    assert zd.ZdParams.lpt2_ratio.offset == (zd.ZdParams.q2LPT.offset + 4 + 7) // 8 * 8
    assert C.sizeof(zd.ZdParams) == zd.ZdParams.lpt2_f2.offset + 8


def _coefficients(**kw):
    import zeldovich_plt_amd.api as zd
    T = zd.load_testing_library()
    out = (C.c_double * 3)()
    T.zd_test_lpt2_coefficients(C.byref(zd.make_params(64, q2LPT=1, **kw)), out)
    return tuple(out)


def test_default_coefficients():
    alpha, ratio, f2 = _coefficients()
    assert alpha == 1.0 and abs(ratio + 3.0 / 7.0) <= 1e-15 and f2 == 2.0
    alpha, ratio, f2 = _coefficients(f_cluster=0.9)
    a = (np.sqrt(1 + 24 * 0.9) - 1) / 4
    assert abs(alpha - a) <= 1e-15 and abs(ratio + (2 * a + 1) / (6 * a + 1)) <= 1e-15 and abs(f2 - 2 * a) <= 1e-15
    assert lpt2_ref.default_coefficients(0.9) == pytest.approx((alpha, ratio, f2), rel=1e-15)
    # the background's own equation: D2'' + D2'/2 - (3/2) f_cl D2 = -(3/2) f_cl D1^2 with D1 = a^alpha, D2 = ratio a^(2 alpha)
    assert abs(ratio * (4 * a * a + a - 1.35) + 1.35) <= 1e-14
    assert _coefficients(lpt2_ratio=-0.5, lpt2_f2=1.7, f_cluster=0.9)[1:] == (-0.5, 1.7)


# ---- routing --------------------------------------------------------------------------------------------------------------
BUDGET = 256 << 30


def _route_why(p, R=0, nranks=1):
    import zeldovich_plt_amd.api as zd
    T = zd.load_testing_library()
    v, why = (C.c_int32 * 12)(), C.create_string_buffer(512)
    T.zd_test_route.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_char_p, C.c_int64]
    rc = T.zd_test_route(C.byref(p), R, nranks, v, why, len(why))
    return rc, list(v), why.value.decode()


REFUSED = [
    ("PLT", dict(qPLT=1), 1, "ZD_qPLT"),
    ("f_NL", dict(f_NL=100.0), 1, "ZD_f_NL"),
    ("density", dict(qdensity=1), 1, "density"),
    ("density only", dict(qdensity=2), 1, "density"),
    ("version 1", dict(version=1), 1, "ZD_Version"),
    ("two ranks", dict(), 2, "one GPU"),
    ("two GPUs", dict(ngpu=2), 1, "one GPU"),
    ("composite PPD", dict(ppd=96), 1, "power of two"),
    ("convolution PPD", dict(ppd=100), 1, "power of two"),
    ("PPD 4096", dict(ppd=4096), 1, "power of two"),
    ("live Nyquist planes", dict(corner_modes=1, k_cutoff=2.0), 1, "Nyquist"),
]


@pytest.mark.parametrize("name,kw,nranks,word", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_combinations(name, kw, nranks, word):
    import zeldovich_plt_amd.api as zd
    L = zd.load_library()
    kw = dict(kw)
    p = zd.make_params(kw.pop("ppd", 128), q2LPT=1, **kw)
    assert L.zd_choose_stream_factor(C.byref(p), nranks, BUDGET) == -1
    rc, _, why = _route_why(p, 1, nranks)
    assert rc == 1 and "ZD_q2LPT" in why and word in why, why
    g, R = C.c_int32(), C.c_int32()
    assert L.zd_choose_pass_groups(C.byref(p), max(nranks, p.ngpu, 1), BUDGET, C.byref(g), C.byref(R)) != 0


def test_supported_jobs_are_accepted():
    import zeldovich_plt_amd.api as zd
    L = zd.load_library()
    for ppd in (32, 64, 128, 256, 512, 1024):
        p = zd.make_params(ppd, q2LPT=1)
        R = L.zd_choose_stream_factor(C.byref(p), 1, BUDGET)
        assert R == 1, (ppd, R)
        rc, v, why = _route_why(p, R)
        assert rc == 0 and why == "" and v[1:6] == [0, 4, 1, 1, 1], (v, why)  # reference arrays, four of them, one pass
    # every option of the supported set keeps the route: formats, k_cutoff, one mode, one slab, fixed amplitudes are not routing
    for kw in (dict(icformat="RVZel"), dict(icformat="Zeldovich"), dict(icformat="ZelSimple"), dict(k_cutoff=2.0), dict(corner_modes=1),
               dict(qonemode=1, one_mode=(1, 2, 3)), dict(qoneslab=5), dict(stream_factor=4), dict(store_mode="packed")):
        p = zd.make_params(128, q2LPT=1, **kw)
        assert L.zd_choose_stream_factor(C.byref(p), 1, BUDGET) == 1, kw
        assert _route_why(p, kw.get("stream_factor", 1))[0] == 0, kw
    # a given stream factor may leave a second-order job z lines of 16 points; every other job keeps the engine's 32
    for ppd, R in ((64, 4), (32, 2), (128, 8)):
        assert _route_why(zd.make_params(ppd, q2LPT=1, stream_factor=R), R)[0] == 0
        assert _route_why(zd.make_params(ppd, stream_factor=R), R)[0] == 1
        assert _route_why(zd.make_params(ppd, store_mode="reference", stream_factor=R), R)[0] == 1
    assert _route_why(zd.make_params(64, q2LPT=1, stream_factor=8), 8)[0] == 1
    # memory: the round peaks at 24 N^3 bytes (+ row padding), S(k) (8 N^3) stays beside the four arrays of a pass (64 N^3 / R)
    p = zd.make_params(1024, q2LPT=1)
    n3 = 1024 ** 3
    assert L.zd_choose_stream_factor(C.byref(p), 1, 80 * n3) == 1
    assert L.zd_choose_stream_factor(C.byref(p), 1, 60 * n3) == 2      # 8 + 64 (1 + 24 / 1024) does not fit, 8 + 32 does
    assert L.zd_choose_stream_factor(C.byref(p), 1, 26 * n3) == 4
    assert L.zd_choose_stream_factor(C.byref(p), 1, 24 * n3) == -1     # the round itself: 16 (1 + 24 / 1024) + 8
    p = zd.make_params(2048, q2LPT=1)
    assert L.zd_choose_stream_factor(C.byref(p), 1, (288 - 16) << 30) == 4


def test_jobs_without_2lpt_are_routed_as_before():
    """the table of tests/test_capi_symbols.py::test_choose_pass_groups_policy, with q2LPT = 0 spelled out, and the one-rank stream
    factors next to it"""
    import zeldovich_plt_amd.api as zd
    L = zd.load_library()
    budget = (288 - 32) << 30

    def choose(ppd, ngpu, **kw):
        p = zd.make_params(ppd, icformat="RVZel", numblock=64, q2LPT=0, lpt2_ratio=0.0, lpt2_f2=0.0, **kw)
        g, R = C.c_int32(), C.c_int32()
        assert L.zd_choose_pass_groups(C.byref(p), ngpu, budget, C.byref(g), C.byref(R)) == 0
        return g.value, R.value

    for ngpu, want in ((1, (1, 8)), (2, (2, 8)), (4, (4, 8)), (8, (8, 16))):
        assert choose(4096, ngpu) == want, ngpu
    g, R = choose(4096, 8, pass_groups=1)
    assert g == 1 and (R // 2) >= 4
    assert choose(4096, 8, pass_groups=8) == (8, 16)
    assert choose(4096, 8, stream_factor=8)[0] == 1
    assert choose(2048, 8)[0] == 1 and choose(2048, 2) == (2, 4)
    assert choose(4096, 8, qPLT=1, qPLTrescale=1) == (8, 16)
    assert choose(6912, 1) == (1, 32) and choose(6912, 2) == (2, 32) and choose(6912, 8) == (8, 32)
    for ppd, kw, want in ((2048, {}, 2), (2048, dict(qPLT=1), 2), (4096, {}, 8), (4096, dict(qPLT=1), 16), (1024, {}, 2),
                          (1024, dict(qPLT=1), 1), (1024, dict(f_NL=10.0), 1), (3456, {}, 4)):
        p = zd.make_params(ppd, icformat="RVZel", numblock=64, **kw)
        assert L.zd_choose_stream_factor(C.byref(p), 1, budget) == want, (ppd, kw)
