"""Third-order displacements (ZD_q3LPT) without a GPU: the numpy restatement of the definition (tests/lpt3_ref.py) held to the
equation of motion it is meant to solve — the EdS Lagrangian equation and the Cauchy invariants close one order higher with the third
order than without, and only with the right sign of the transverse term —, the parameter keys, and the routing: what is refused,
what is accepted, what the choosers count."""
import ctypes as C

import numpy as np
import pytest

import lpt2_ref
import lpt3_ref
from conftest import WMAP

BOX = 720.0
BUDGET = 256 << 30
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


def _route_why(p, R=0, nranks=1):
    """the route test hook of the testing library: (refused, shape, the one-line reason)"""
    import zeldovich_plt_amd.api as zd
    T = zd.load_testing_library()
    v, why = (C.c_int32 * 12)(), C.create_string_buffer(512)
    T.zd_test_route.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_char_p, C.c_int64]
    rc = T.zd_test_route(C.byref(p), R, nranks, v, why, len(why))
    return rc, list(v), why.value.decode()


# ---- the numpy reference -----------------------------------------------------------------------------------------------------
def _band_limited_field(n=32, k2max=4.5, seed=7):
    """a fixed random first-order field with |k|^2 <= k2max (integer wavenumbers), max |grad psi1| = 1: q[z, y, x, 3]"""
    rng = np.random.default_rng(seed)
    dk = np.fft.fftn(rng.standard_normal((n, n, n)))
    k = lpt2_ref.wavenumbers(n)
    kz, ky, kx = np.meshgrid(k, k, k, indexing="ij")
    k2i = kx * kx + ky * ky + kz * kz
    dk[(k2i > k2max) | (k2i == 0)] = 0.0
    kv = lpt2_ref._kvec(n, BOX)
    k2 = kv[0] ** 2 + kv[1] ** 2 + kv[2] ** 2
    k2[0, 0, 0] = 1.0
    q = np.stack([np.real(np.fft.ifftn(1j * kv[j] * dk / k2)) for j in range(3)], axis=-1)
    return q / max(np.abs(_grad(q[..., b], a)).max() for a in range(3) for b in range(3))


def _grad(f, a):
    n = f.shape[0]
    return np.real(np.fft.ifftn(1j * lpt2_ref._kvec(n, BOX)[a] * np.fft.fftn(f)))


def _jac(v):
    """d v_l / d q_j as [z, y, x, l, j]"""
    return np.stack([np.stack([_grad(v[..., l], j) for j in range(3)], axis=-1) for l in range(3)], axis=-2)


def _orders(q1, eps, g3c_sign=1.0):
    """(psi1, psi2, psi3) of the field eps q1 at f_cluster = 1: defaults of both orders"""
    q = eps * q1
    mask = lpt2_ref.alive_mask(q.shape[0], BOX)
    psi2 = lpt2_ref.second_order(q, BOX, mask)
    psi3 = lpt3_ref.combine(lpt3_ref.third_order(q, BOX, mask), g3c=g3c_sign * lpt3_ref.DEFAULTS["g3c"])
    return q, psi2, psi3


def _residuals(psi, upto):
    """max |EdS equation-of-motion residual| and max |Cauchy invariant| of x = q + sum_n a^n psi_n at a = 1, orders 1 .. upto.
    T = d^2/da^2 + (3 / 2a) d/da gives T a^n = n (n + 1/2) a^(n-2); the residual is J tr[(dx/dq)^-1 d(T x)/dq] - (3/2)(J - 1)."""
    disp = sum(psi[:upto])
    tx = sum((n + 1) * (n + 1.5) * psi[n] for n in range(upto))
    xdot = sum((n + 1) * psi[n] for n in range(upto))
    a = np.eye(3) + _jac(disp)
    det = np.linalg.det(a)
    eom = det * np.trace(np.linalg.solve(a, _jac(tx)), axis1=-2, axis2=-1) - 1.5 * (det - 1.0)
    jd = _jac(xdot)
    cauchy = 0.0
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        cauchy = max(cauchy, np.abs(sum(a[..., l, j] * jd[..., l, k] - a[..., l, k] * jd[..., l, j] for l in range(3))).max())
    return np.abs(eom).max(), cauchy


def test_the_restated_second_order_source_is_lpt2_refs():
    q = 0.05 * _band_limited_field()
    td = lpt3_ref.hessian(lpt3_ref.first_order_modes(q, BOX), BOX)
    want = lpt2_ref.source(q, BOX)
    assert np.abs(lpt3_ref.second_order_source(td) - want).max() <= 1e-12 * np.abs(want).max()
    # T_ab[D] = -psi1_{a,b}, and tr T[D] is the inverse transform of D = -div psi1
    assert np.abs(td[(0, 1)] + _grad(q[..., 1], 0)).max() <= 1e-12 * np.abs(td[(0, 1)]).max()
    # div C = 0 (to rounding: nothing aliases in this band)
    _, _, c, _ = lpt3_ref.sources(q, BOX, lpt2_ref.alive_mask(32, BOX))
    div = sum(_grad(c[a], a) for a in range(3))
    scale = max(np.abs(_grad(c[a], b)).max() for a in range(3) for b in range(3))
    assert np.abs(div).max() <= 1e-10 * scale


def test_equation_of_motion_and_cauchy_invariants_close_one_order_higher():
    """one fixed band-limited field (32^3, |k|^2 <= 4.5) at eps and eps / 2: the residuals fall as eps^3 with orders 1 + 2 and as
    eps^4 with 1 + 2 + 3; with the sign of g3c flipped the Cauchy invariants stay at eps^3"""
    q1 = _band_limited_field()
    eps = 0.02
    res = {}
    for e in (eps, eps / 2):
        psi = _orders(q1, e)
        res[e] = (_residuals(psi, 1), _residuals(psi, 2), _residuals(psi, 3), _residuals(_orders(q1, e, -1.0), 3))
    ratio = [[res[eps][o][i] / res[eps / 2][o][i] for i in range(2)] for o in range(4)]
    print("residuals at eps:", res[eps], "\nratios eps : eps/2 (equation of motion, Cauchy) by order 1, 1+2, 1+2+3, 1+2+3 with -g3c:", ratio)
    assert 3.0 <= ratio[0][0] <= 5.0                   # first order alone: eps^2
    assert ratio[1][0] <= 10.0 and ratio[1][1] <= 10.0  # 1 + 2: eps^3
    assert ratio[2][0] >= 12.0 and ratio[2][1] >= 12.0  # 1 + 2 + 3: eps^4 (or better)
    assert 6.0 <= ratio[3][1] <= 10.0                   # wrong sign of the transverse term: the invariants stay at eps^3 ...
    assert res[eps][3][1] >= 0.5 * res[eps][1][1]       # ... at the level of orders 1 + 2


def test_a_single_plane_wave_has_no_third_order():
    n = 16
    fund = 2.0 * np.pi / BOX
    r = np.arange(n) * (BOX / n)
    pos = np.meshgrid(r, r, r, indexing="ij")
    kp = np.array((2, -1, 3), dtype=np.float64) * fund
    t = kp[0] * pos[0] + kp[1] * pos[1] + kp[2] * pos[2]
    q = np.stack([0.9 * kp[j] * np.sin(t) for j in range(3)], axis=-1)
    parts = lpt3_ref.third_order(q, BOX, lpt2_ref.alive_mask(n, BOX))
    for part in parts:
        assert np.abs(part).max() <= 1e-12 * np.abs(q).max()


# ---- parameter reader, make_params --------------------------------------------------------------------------------------------
def _read(tmp_path, extra):
    import zeldovich_plt_amd.api as zd
    par = tmp_path / "t.par"
    par.write_text(PAR % dict(out=tmp_path / "ic", pk=WMAP) + extra)
    return zd.params_from_file(str(par))[0]


def _fields(p):
    return (p.q3LPT, p.lpt3_g3a, p.lpt3_g3b, p.lpt3_g3c, p.lpt3_f3, p.lpt3_terms)


def test_parameter_keys(tmp_path):
    assert _fields(_read(tmp_path, "")) == (0, 0.0, 0.0, 0.0, 0.0, 0)
    assert _fields(_read(tmp_path, "ZD_q2LPT = 1\nZD_q3LPT = 1\n")) == (1, 0.0, 0.0, 0.0, 0.0, 0)
    p = _read(tmp_path, "ZD_q2LPT = 1\nZD_q3LPT = 1\nZD_3LPT_D3a = -0.3\nZD_3LPT_D3b = 0.47\nZD_3LPT_D3c = 0.14\nZD_3LPT_f3 = 2.9\nZD_3LPT_terms = 5\n")
    assert _fields(p) == (1, -0.3, 0.47, 0.14, 2.9, 5) and p.q2LPT == 1


def test_make_params_mirrors_the_fields():
    import zeldovich_plt_amd.api as zd
    assert _fields(zd.make_params(64)) == (0, 0.0, 0.0, 0.0, 0.0, 0)
    p = zd.make_params(64, q2LPT=1, q3LPT=1, lpt3_g3a=-0.3, lpt3_g3b=0.47, lpt3_g3c=0.14, lpt3_f3=2.9, lpt3_terms=6)
    assert _fields(p) == (1, -0.3, 0.47, 0.14, 2.9, 6)
    # between lpt2_ratio and lpt2_f2: lpt2_f2 stays the last member (tests/test_lpt2.py pins it), nothing in front of lpt2_ratio moves
    Z = zd.ZdParams
    assert Z.q3LPT.offset == Z.lpt2_ratio.offset + 8 and Z.lpt3_terms.offset == Z.q3LPT.offset + 4
    assert [getattr(Z, f).offset - Z.q3LPT.offset for f in ("lpt3_g3a", "lpt3_g3b", "lpt3_g3c", "lpt3_f3", "lpt2_f2")] == [8, 16, 24, 32, 40]
    assert C.sizeof(Z) == Z.lpt2_f2.offset + 8


# ---- routing ------------------------------------------------------------------------------------------------------------------
REFUSED = [
    ("without the second order", dict(q2LPT=0), "ZD_q3LPT = 1 needs ZD_q2LPT = 1"),
    ("de-aliased second order", dict(lpt2_dealias=1), "ZD_2LPT_dealias"),
    ("PPD 2048", dict(ppd=2048), "PPD <= 1024"),
    ("q3LPT = 2", dict(q3LPT=2), "must be 0 or 1"),
    ("terms = 8", dict(lpt3_terms=8), "ZD_3LPT_terms"),
    ("terms = -1", dict(lpt3_terms=-1), "ZD_3LPT_terms"),
    ("f_cluster without coefficients", dict(f_cluster=0.9), "ZD_f_cluster"),
    ("f_cluster without f3", dict(f_cluster=0.9, lpt3_g3a=-0.3, lpt3_g3b=0.4, lpt3_g3c=0.1), "ZD_f_cluster"),
    ("f_cluster without an enabled term's coefficient", dict(f_cluster=0.9, lpt3_g3a=-0.3, lpt3_g3b=0.4, lpt3_f3=2.8, lpt3_terms=5), "ZD_f_cluster"),
    # inherited from the second order
    ("PLT", dict(qPLT=1), "ZD_qPLT"),
    ("f_NL", dict(f_NL=100.0), "ZD_f_NL"),
    ("density", dict(qdensity=1), "density"),
    ("version 1", dict(version=1), "ZD_Version"),
    ("two GPUs", dict(ngpu=2), "one GPU"),
    ("composite PPD", dict(ppd=96), "power of two"),
    ("live Nyquist planes", dict(corner_modes=1, k_cutoff=2.0), "Nyquist"),
]


@pytest.mark.parametrize("name,kw,word", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_combinations(name, kw, word):
    import zeldovich_plt_amd.api as zd
    L = zd.load_library()
    kw = dict(dict(q2LPT=1, q3LPT=1), **kw)
    p = zd.make_params(kw.pop("ppd", 128), **kw)
    assert L.zd_choose_stream_factor(C.byref(p), 1, BUDGET) == -1
    rc, _, why = _route_why(p, 1, 1)
    assert rc == 1 and "\n" not in why and word in why, why
    assert "ZD_q3LPT" in why or "ZD_q2LPT" in why, why  # (a refusal of the second order names the second order)
    g, R = C.c_int32(), C.c_int32()
    assert L.zd_choose_pass_groups(C.byref(p), max(p.ngpu, 1), BUDGET, C.byref(g), C.byref(R)) != 0


def test_supported_jobs_are_accepted():
    import zeldovich_plt_amd.api as zd
    L = zd.load_library()
    for ppd in (32, 64, 128, 256, 512, 1024):
        p = zd.make_params(ppd, q2LPT=1, q3LPT=1)
        R = L.zd_choose_stream_factor(C.byref(p), 1, BUDGET)
        assert R == 1, (ppd, R)
        rc, v, why = _route_why(p, R)
        assert rc == 0 and why == "" and v[1:6] == [0, 4, 1, 1, 1], (v, why)  # the second order's route: four reference arrays
    for kw in (dict(icformat="RVZel"), dict(k_cutoff=2.0), dict(qonemode=1, one_mode=(1, 2, 3)), dict(qoneslab=5), dict(stream_factor=4),
               dict(lpt3_terms=4), dict(f_cluster=0.9, lpt3_g3a=-0.3, lpt3_g3b=0.4, lpt3_g3c=0.1, lpt3_f3=2.8),
               dict(f_cluster=0.9, lpt3_g3c=0.1, lpt3_f3=2.8, lpt3_terms=4)):
        p = zd.make_params(128, q2LPT=1, q3LPT=1, **kw)
        assert L.zd_choose_stream_factor(C.byref(p), 1, BUDGET) == 1, kw
        assert _route_why(p, kw.get("stream_factor", 1))[0] == 0, kw
    assert _route_why(zd.make_params(64, q2LPT=1, q3LPT=1, stream_factor=4), 4)[0] == 0  # z lines of 16 points, as for the second order
    # q3LPT = 0: the other keys are not read
    assert _route_why(zd.make_params(128, q2LPT=1, lpt3_terms=9, lpt2_dealias=1), 1)[0] == 0
    # memory: the round peaks at 120 N^3 bytes (+ row padding); S, P3, C_x,y,z (40 N^3) stay beside the four arrays of a pass (64 N^3 / R)
    p = zd.make_params(1024, q2LPT=1, q3LPT=1)
    n3 = 1024 ** 3
    assert L.zd_choose_stream_factor(C.byref(p), 1, 119 * n3) == -1
    assert L.zd_choose_stream_factor(C.byref(p), 1, 121 * n3) == 1
    p = zd.make_params(512, q2LPT=1, q3LPT=1)
    n3 = 512 ** 3
    assert L.zd_choose_stream_factor(C.byref(p), 1, 124 * n3) == 1      # round 120 (1 + ...), then 40 + 64 (1 + 24 / 512)
    p2 = zd.make_params(512, q2LPT=1)
    assert L.zd_choose_stream_factor(C.byref(p2), 1, 100 * n3) == 1 and L.zd_choose_stream_factor(C.byref(p), 1, 100 * n3) == -1
