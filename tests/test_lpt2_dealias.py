"""The de-aliased second-order source (ZD_2LPT_dealias) without a GPU: the numpy restatement of step 2' (tests/lpt2_dealias_ref.py)
pinned by a closed form that aliases on the N lattice, its agreement with tests/lpt2_ref.py where nothing aliases, the parameter
key, and the routing — what is refused, what is accepted, what fits."""
import ctypes as C

import numpy as np
import pytest

import lpt2_dealias_ref
import lpt2_ref
from conftest import WMAP
from test_lpt2 import PAR

BOX = 720.0


# ---- 1. a closed form that aliases ------------------------------------------------------------------------------------------
def _two_waves(n, a, b, k1, k2):
    """psi1 = -grad phi for phi = a cos(k1.x) + b cos(k2.x) on the lattice (k in array-axis order) and A = a b |k1 x k2|^2 of its
    source S = A cos(k1.x) cos(k2.x) = (A / 2) [cos((k1 + k2).x) + cos((k1 - k2).x)]"""
    fund = 2.0 * np.pi / BOX
    r = np.arange(n) * (BOX / n)
    pos = np.meshgrid(r, r, r, indexing="ij")
    q = np.zeros((n, n, n, 3))
    for amp, k in ((a, k1), (b, k2)):
        kp = np.array(k, dtype=np.float64) * fund
        t = kp[0] * pos[0] + kp[1] * pos[1] + kp[2] * pos[2]
        for j in range(3):
            q[..., j] += amp * kp[j] * np.sin(t)
    cr = np.cross(np.array(k1, dtype=np.float64) * fund, np.array(k2, dtype=np.float64) * fund)
    return q, a * b * np.dot(cr, cr)


@pytest.mark.parametrize("k1,k2,axis", [((5, 1, 0), (4, 0, 2), 0), ((1, -6, 2), (0, -5, 1), 1), ((2, 1, 7), (-1, 3, 6), 2)])
def test_two_waves_whose_sum_leaves_the_band(k1, k2, axis):
    n = 16
    ks, kd = np.array(k1) + np.array(k2), np.array(k1) - np.array(k2)
    assert abs(ks[axis]) > n // 2 and np.abs(kd).max() < n // 2 and max(map(abs, k1 + k2)) < n // 2
    q, A = _two_waves(n, 0.7, -1.3, k1, k2)
    folded = ks.copy()
    folded[axis] -= n * np.sign(ks[axis])
    # the plain source carries the sum wave at its folded wavenumber ...
    plain = np.fft.fftn(lpt2_ref.source(q, BOX)) / n ** 3
    assert abs(plain[tuple(folded % n)] - A / 4) <= 1e-12 * abs(A)
    # ... the de-aliased one does not: it is the analytic source restricted to |k_i| < N/2, the difference wave alone
    want = np.zeros((n, n, n), dtype=np.complex128)
    want[tuple(kd % n)] = want[tuple(-kd % n)] = A / 4
    got = lpt2_dealias_ref.source_k(q, BOX)
    assert abs(got[tuple(folded % n)]) <= 1e-12 * abs(A)
    assert np.abs(got - want).max() <= 1e-12 * abs(A)


# ---- 2. nothing aliases, nothing changes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("k_cutoff", [1.5, 2.0])
def test_agrees_with_the_plain_definition_where_nothing_aliases(oracle, k_cutoff):
    n = 32
    pk = oracle.pk_from_file(WMAP, BOX, Pk_sigma=0.42)
    q = np.ascontiguousarray(oracle.run(oracle.make_params(n, k_cutoff=k_cutoff), pk)["records"]["d"], dtype=np.float64)
    mask = lpt2_ref.alive_mask(n, BOX, k_cutoff)
    a, b = lpt2_ref.second_order(q, BOX, mask), lpt2_dealias_ref.second_order(q, BOX, mask)
    err = np.abs(a - b).max() / np.abs(a).max()
    print("k_cutoff", k_cutoff, "plain against de-aliased:", err)
    assert np.abs(a).max() > 0 and err <= 1e-12


def test_differs_from_the_plain_definition_at_k_cutoff_1(oracle):
    n = 32
    pk = oracle.pk_from_file(WMAP, BOX, Pk_sigma=0.42)
    q = np.ascontiguousarray(oracle.run(oracle.make_params(n), pk)["records"]["d"], dtype=np.float64)
    mask = lpt2_ref.alive_mask(n, BOX)
    a, b = lpt2_ref.second_order(q, BOX, mask), lpt2_dealias_ref.second_order(q, BOX, mask)
    assert np.abs(a - b).max() >= 0.05 * np.abs(b).max()


# ---- 3. the key, the struct, the route --------------------------------------------------------------------------------------
def _read(tmp_path, extra):
    import zeldovich_plt_amd.api as zd
    par = tmp_path / "t.par"
    par.write_text(PAR % dict(out=tmp_path / "ic", pk=WMAP) + extra)
    return zd.params_from_file(str(par))[0]


def test_parameter_key(tmp_path):
    import zeldovich_plt_amd.api as zd
    assert _read(tmp_path, "ZD_q2LPT = 1\n").lpt2_dealias == 0
    p = _read(tmp_path, "ZD_q2LPT = 1\nZD_2LPT_dealias = 1\n")
    assert (p.q2LPT, p.lpt2_dealias) == (1, 1)
    assert zd.make_params(64).lpt2_dealias == 0 and zd.make_params(64, q2LPT=1, lpt2_dealias=1).lpt2_dealias == 1
    # a job without the key: the struct is byte for byte what it is without the field (which sits in the former alignment gap)
    a, b = _read(tmp_path, "ZD_q2LPT = 1\n"), _read(tmp_path, "ZD_q2LPT = 1\nZD_2LPT_dealias = 0\n")
    assert bytes(a) == bytes(b)
    assert zd.ZdParams.lpt2_dealias.offset == zd.ZdParams.q2LPT.offset + 4 and zd.ZdParams.lpt2_ratio.offset == zd.ZdParams.lpt2_dealias.offset + 4
    assert bytes(a)[zd.ZdParams.lpt2_dealias.offset:zd.ZdParams.lpt2_ratio.offset] == b"\0\0\0\0"
    assert bytes(zd.make_params(64, q2LPT=1)) == bytes(zd.make_params(64, q2LPT=1, lpt2_dealias=0))


def _route_why(p, R=1, nranks=1):
    import zeldovich_plt_amd.api as zd
    T = zd.load_testing_library()
    v, why = (C.c_int32 * 12)(), C.create_string_buffer(512)
    T.zd_test_route.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_char_p, C.c_int64]
    rc = T.zd_test_route(C.byref(p), R, nranks, v, why, len(why))
    return rc, list(v), why.value.decode()


BUDGET = 272 << 30

REFUSED = [
    ("value 2", dict(q2LPT=1, lpt2_dealias=2), "0 or 1"),
    ("without ZD_q2LPT", dict(lpt2_dealias=1), "ZD_q2LPT = 1"),
    ("corner modes", dict(q2LPT=1, lpt2_dealias=1, corner_modes=1), "ZD_CornerModes"),
]


@pytest.mark.parametrize("name,kw,word", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_combinations(name, kw, word):
    import zeldovich_plt_amd.api as zd
    L = zd.load_library()
    p = zd.make_params(128, **kw)
    rc, _, why = _route_why(p)
    assert rc == 1 and "ZD_2LPT_dealias" in why and word in why and "\n" not in why, why
    assert L.zd_choose_stream_factor(C.byref(p), 1, BUDGET) == -1
    g, R = C.c_int32(), C.c_int32()
    assert L.zd_choose_pass_groups(C.byref(p), 1, BUDGET, C.byref(g), C.byref(R)) != 0


def test_what_2lpt_refuses_stays_refused_with_its_message():
    import zeldovich_plt_amd.api as zd
    for kw, word in ((dict(qPLT=1), "ZD_qPLT"), (dict(f_NL=10.0), "ZD_f_NL"), (dict(qdensity=1), "density"), (dict(version=1), "ZD_Version"),
                     (dict(ngpu=2), "one GPU"), (dict(ppd=96), "power of two"), (dict(ppd=4096), "power of two")):
        kw = dict(kw)
        ppd = kw.pop("ppd", 128)
        plain = _route_why(zd.make_params(ppd, q2LPT=1, **kw))
        both = _route_why(zd.make_params(ppd, q2LPT=1, lpt2_dealias=1, **kw))
        assert plain[0] == 1 and both[0] == 1 and both[2] == plain[2] and "ZD_q2LPT" in both[2] and word in both[2]


def test_accepted_jobs_and_memory():
    import zeldovich_plt_amd.api as zd
    L = zd.load_library()
    for ppd in (32, 64, 128, 256, 512, 1024):
        p = zd.make_params(ppd, q2LPT=1, lpt2_dealias=1)
        assert L.zd_choose_stream_factor(C.byref(p), 1, BUDGET) == 1, ppd
        rc, v, why = _route_why(p)
        plain = _route_why(zd.make_params(ppd, q2LPT=1))
        assert rc == 0 and why == "" and v == plain[1], (ppd, v, why)  # the final pass is the plain job's
    for kw in (dict(k_cutoff=2.0), dict(k_cutoff=1.5), dict(qoneslab=3), dict(stream_factor=4), dict(icformat="RVZel"),
               dict(qonemode=1, one_mode=(1, 2, 3))):
        assert _route_why(zd.make_params(128, q2LPT=1, lpt2_dealias=1, **kw), kw.get("stream_factor", 1))[0] == 0, kw
    # memory: the round peaks at (16 + 8) (3 N / 2)^3 = 81 N^3 bytes (+ the row pad): 87 GB at 1024, 696 GB at 2048
    p = zd.make_params(2048, q2LPT=1, lpt2_dealias=1)
    rc, _, why = _route_why(p)                                         # (the lattice 3072 has line transforms, but no k_xlpt2q / k_lpt2q_zsrc)
    assert rc == 1 and "no kernel for the second-order round: x stage of this job (launch_lpt2q_xsrc_t, n = 3072)" in why, why
    assert L.zd_choose_stream_factor(C.byref(p), 1, BUDGET) == -1
    assert L.zd_choose_stream_factor(C.byref(zd.make_params(2048, q2LPT=1)), 1, BUDGET) > 0
    p = zd.make_params(1024, q2LPT=1, lpt2_dealias=1)
    n3 = 1024 ** 3
    assert L.zd_choose_stream_factor(C.byref(p), 1, 84 * n3) >= 1
    assert L.zd_choose_stream_factor(C.byref(p), 1, 81 * n3) == -1     # 81 N^3 + the row pad of 24 elements
    assert L.zd_choose_stream_factor(C.byref(zd.make_params(1024, q2LPT=1)), 1, 81 * n3) == 1
