"""GPU: every device buffer, pinned buffer, event, stream and plan the host layer makes is given back, however a call ends.

The owning handles of csrc/zd_own.h count themselves in the -DZD_TESTING library (zd_test_live_handles: live handles + live plans).
Each test below runs one path of the library at the smallest grid that path accepts — success paths, consumers that fail, a rank that
fails before its first pass, a refusal after the second-order round's check, the device test hooks — and asserts the count is 0
afterwards.  The failures are host-side error returns; nothing here provokes a GPU fault."""
import gc

import numpy as np
import pytest

from conftest import WMAP

pytestmark = pytest.mark.gpu

FNL = dict(f_NL=2.0e4, n_s=0.96, Omega_M=0.31)
PLT = dict(qPLT=1, qPLTrescale=1, PLT_target_z=5.0, z_initial=49.0)


@pytest.fixture
def zd(monkeypatch):
    """the API with every call — generate_planes and the staged API included — on the testing library, where the counter lives"""
    import zeldovich_plt_amd.api as api
    monkeypatch.setattr(api, "load_library", api.load_testing_library)
    return api


@pytest.fixture
def live(zd):
    L = zd.load_testing_library()
    gc.collect()  # (a Plan object an earlier test dropped without close())
    assert L.zd_test_live_handles() == 0
    return L.zd_test_live_handles


@pytest.fixture(scope="module")
def ps():
    import zeldovich_plt_amd.api as api
    return api.PowerSpectrum.from_file(WMAP, 720.0)


RUNS = {
    "za-callback": (64, dict(icformat="RVZel", stream_factor=2), dict()),  # stream factor 2: z lines of 32, the engine's shortest
    "za-null-sink": (64, dict(icformat="RVZel", stream_factor=2), dict(collect=False)),
    "plt": (64, dict(PLT), dict(eig=32)),
    "fnl-pow2": (64, dict(FNL), dict()),
    "fnl-composite": (96, dict(FNL), dict()),
    "q2lpt": (32, dict(q2LPT=1), dict()),
    "q2lpt-dealias": (32, dict(q2LPT=1, lpt2_dealias=1), dict()),  # its rounds run on the 48 lattice
    "qdensity": (32, dict(qdensity=1), dict()),
    "two-ranks-local": (64, dict(icformat="RVZel", stream_factor=2, ngpu=2, pass_groups=1), dict()),
    "two-ranks-loopback": (64, dict(icformat="RVZel", stream_factor=2, ngpu=2, pass_groups=1), dict(loopback=True)),
}


@pytest.mark.parametrize("name", list(RUNS))
def test_a_run_gives_everything_back(zd, oracle, ps, live, name):
    n, pkw, gkw = RUNS[name]
    gkw = dict(gkw)
    if "eig" in gkw:
        gkw["eig"] = oracle.synthetic_eigenmodes(gkw["eig"])
    out = zd.generate(zd.make_params(n, **pkw), ps, testing=True, **gkw)
    if gkw.get("collect", True):
        assert sorted(out["planes_seen"]) == list(range(n))
    assert live() == 0


def _fails_on_third_plane():
    seen = []

    def on_plane(z, rec):
        seen.append(z)
        return 1 if len(seen) == 3 else 0

    return seen, on_plane


@pytest.mark.parametrize("ngpu", [1, 2])
def test_a_failing_consumer_gives_everything_back(zd, ps, live, ngpu):
    """the consumer returns 1 on its third plane: one rank (the writer thread of zd_generate), and two ranks on the local transport
    (every rank thread leaves, the first one aborts the job before its buffers go)"""
    seen, on_plane = _fails_on_third_plane()
    kw = dict(ngpu=2, pass_groups=1, exchange_planes=3) if ngpu == 2 else dict()
    with pytest.raises(RuntimeError):
        zd.generate_planes(zd.make_params(64, icformat="RVZel", stream_factor=2, **kw), ps, on_plane)
    assert len(seen) == 3
    assert live() == 0


def test_a_rank_failing_before_its_first_pass_gives_everything_back(zd, ps, live):
    L = zd.load_testing_library()
    L.zd_test_fail_rank(1)
    try:
        with pytest.raises(RuntimeError):
            zd.generate(zd.make_params(64, icformat="RVZel", stream_factor=2, ngpu=2, pass_groups=1), ps, loopback=True)
    finally:
        L.zd_test_fail_rank(-1)
    assert live() == 0


def test_a_refusal_after_the_second_order_check_gives_everything_back(zd, ps, live, capfd):
    with pytest.raises(RuntimeError):
        zd.generate(zd.make_params(32, q2LPT=1, qdensity=1), ps, testing=True)
    assert "ZD_q2LPT = 1" in capfd.readouterr().err
    assert live() == 0


def test_the_staged_api_counts_its_plan(zd, ps, live):
    """the counter is alive: above zero while a plan exists, back where it was after zd_plan_destroy"""
    before = live()
    plan = zd.Plan(zd.make_params(32), ps, testing=True)
    try:
        assert live() > before
    finally:
        plan.close()
    assert live() == before == 0


def test_every_device_hook_gives_everything_back(zd, ps, live):
    """each zd_test_* hook that touches the device, once, at its smallest legal shape"""
    L = zd.load_testing_library()
    k = np.array([[1, 2, 3], [0, 1, -2]], dtype=np.int32)
    zd.test_draws(12346, k)
    assert live() == 0
    zd.test_modes(zd.make_params(32), ps, k)
    assert live() == 0
    zd.test_modes_table(zd.make_params(32), ps, k)
    assert live() == 0
    zd.test_v1_words(5, 1)
    assert live() == 0
    rng = np.random.default_rng(3)
    # zd_test_fft: power of two (both layouts), composite, convolution, and the composite transforms of the reference's arrays
    for n, lines, kind in ((32, 64, 0), (32, 64, 1), (24, 8, 0), (10, 7, 0), (48, 3, 3), (48, 3, 4)):
        x = rng.standard_normal((lines, n)) + 1j * rng.standard_normal((lines, n))
        hin = np.ascontiguousarray(x.T if kind in (1, 3) else x)
        out = np.zeros_like(hin)
        assert L.zd_test_fft(n, lines, kind, hin.ctypes.data, out.ctypes.data) == 0, (n, kind)
        got = out.T if kind in (1, 3) else out
        ref = np.fft.ifft(x, axis=1) * n
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max(), (n, kind)
        assert live() == 0, (n, kind)
    x = rng.standard_normal((2, 48, 3)) + 1j * rng.standard_normal((2, 48, 3))
    x[:, 24, :] = 0
    out = np.zeros_like(x)
    assert L.zd_test_ycols(48, 2, 3, 2, 0, x.ctypes.data, out.ctypes.data) == 0
    ref = np.fft.ifft(x, axis=1) * 48
    assert np.abs(out - ref).max() <= 1e-12 * np.abs(ref).max()
    assert live() == 0
    # ... and a hook that refuses its arguments after nothing was made
    assert L.zd_test_fft(48, 0, 3, x.ctypes.data, out.ctypes.data) != 0
    assert live() == 0
