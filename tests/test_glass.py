"""CPU: the definition of the off-lattice interpolation (zeldovich_plt_amd/csrc/zd_kernels_glass.hip) restated in numpy
(tests/glass_ref.py) — weight identities, exactness at lattice sites, convergence under oversampling against the oracle's exact
band-limited field, the tiling formula — and the host side of the new entry points: symbols, argument refusals before a plan or the
GPU is touched, unchanged struct sizes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import glass_ref as gr
from conftest import ROOT, WMAP

BOX = 720.0
NEW_SYMBOLS = ("zd_interp_create", "zd_interp_add_plane", "zd_interp_result", "zd_interp_destroy", "zd_plan_interp", "zd_displace")


# ---- the definition -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 3])
def test_weight_identities(order):
    """the weights reproduce polynomials up to their order: sum w = 1, sum w j = tau (both), sum w j^2 = tau^2, sum w j^3 = tau^3 (3)"""
    tau = np.concatenate([np.random.default_rng(3).random(2000), [0.0, 0.5, 1.0 - 2.0 ** -53]])
    w, j = gr.weights(tau, order), gr.offsets(order).astype(np.float64)[:, None]
    assert np.abs(w.sum(axis=0) - 1.0).max() <= 4e-16
    assert np.abs((w * j).sum(axis=0) - tau).max() <= 8e-16
    if order == 3:
        assert np.abs((w * j ** 2).sum(axis=0) - tau ** 2).max() <= 2e-15
        assert np.abs((w * j ** 3).sum(axis=0) - tau ** 3).max() <= 4e-15
    # at tau = 0 every weight is exactly 0 or 1
    w0 = gr.weights(np.zeros(1), order)[:, 0]
    assert sorted(np.abs(w0).tolist()) == [0.0] * order + [1.0]


@pytest.fixture(scope="module")
def runs(oracle):
    """oracle runs (ppd, k_cutoff) -> fields [z, y, x, 6], made once and kept read-only"""
    pk = oracle.pk_from_file(WMAP, BOX)
    cache = {}

    def get(ppd, k_cutoff, icformat="RVdoubleZel"):
        key = (ppd, k_cutoff, icformat)
        if key not in cache:
            rec = oracle.run(oracle.make_params(ppd, k_cutoff=float(k_cutoff), icformat=icformat), pk)["records"]
            f = gr.fields_of_records(rec)
            f.setflags(write=False)
            cache[key] = (rec, f)
        return cache[key]

    return get


def _site_positions(n, m):
    """every site of the lattice of m points per side, as positions (x, y, z) in (z, y, x) index order"""
    z, y, x = np.meshgrid(np.arange(m), np.arange(m), np.arange(m), indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1) / float(m)


@pytest.mark.parametrize("order", [1, 3])
@pytest.mark.parametrize("fmt", ["RVdoubleZel", "ZelSimple"])
def test_lattice_sites_reproduce_the_records_bit_for_bit(runs, order, fmt):
    n = 32
    rec, f = runs(n, 1, fmt)
    got = gr.interpolate(f, _site_positions(n, n), order).reshape(n, n, n, 6)
    assert np.array_equal(got[..., :3], rec["d"][..., ::-1].astype(np.float64))
    if "v" in rec.dtype.names:
        assert np.array_equal(got[..., 3:], rec["v"][..., ::-1]) and np.abs(got[..., 3:]).max() > 0
    else:
        assert not got[..., 3:].any()


# max |psi_interp - psi_exact| / max|q| with wmap1new.pow and default parameters, particles at every site of the 2N lattice, the truth
# the oracle's 2N run with k_cutoff doubled: (N, k_cutoff) -> (order 1, order 3)
CONVERGENCE = {(32, 2): (0.1027, 0.0205), (32, 4): (0.0344, 0.00155), (64, 2): (0.0851, 0.0161), (64, 4): (0.0269, 0.00147)}


@pytest.mark.parametrize("n,kc", sorted(CONVERGENCE))
def test_oversampled_field_is_the_same_field_and_interpolation_converges_to_it(runs, n, kc):
    _rec, a = runs(n, kc)
    _rec, b = runs(2 * n, 2 * kc)
    assert np.array_equal(b[::2, ::2, ::2], a)  # the oversampling link: B[::2, ::2, ::2] - A is exactly 0.0
    qmax = np.abs(b[..., :3]).max()
    pos = _site_positions(n, 2 * n)
    err = {}
    for order in (1, 3):
        got = gr.interpolate(a[..., :3], pos, order).reshape(2 * n, 2 * n, 2 * n, 3)
        err[order] = np.abs(got - b[..., :3]).max() / qmax
    print("N = %d, k_cutoff = %d: order 1 %.4g, order 3 %.4g (tabulated %r)" % (n, kc, err[1], err[3], CONVERGENCE[(n, kc)]))
    assert err[3] <= 2.0 * CONVERGENCE[(n, kc)][1]  # (the margin covers libm and FFT rounding only)
    assert err[1] >= 4.0 * err[3]


def test_tiling_formula():
    rng = np.random.default_rng(5)
    p = rng.random((7, 3))
    t = 3
    full = gr.tiled(p, t)
    assert full.shape == (7 * t ** 3, 3) and full.min() >= 0.0 and full.max() < 1.0
    for a in range(t):
        for b in range(t):
            for c in range(t):
                for i in (0, 3, 6):
                    g = ((a * t + b) * t + c) * 7 + i
                    assert np.array_equal(full[g], (p[i] + np.array([c, b, a], dtype=np.float64)) / t)
    assert np.array_equal(gr.tiled(p, 1), p)
    # a periodic field sampled by the tiled load = the field of the one tile seen t times: positions differ by multiples of 1 / t
    assert np.abs((full.reshape(t ** 3, 7, 3) * t) % 1.0 - p[None]).max() <= 4e-16 * t


# ---- the built library, no GPU ------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_listed():
    import zeldovich_plt_amd.api as api
    header = open(os.path.join(ROOT, "include", "zeldovich_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = api.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), "%s is not declared in the header" % name
        assert name in api.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    assert os.path.exists(os.path.join(ROOT, "zeldovich_plt_amd", "csrc", "zd_kernels_glass.hip"))
    assert callable(api.displace) and callable(api.Plan.interp) and callable(api.Interp)


def test_struct_sizes_are_unchanged():
    """the feature arrives through entry points and keys read with zd_param_file_string: no ABI struct has a new member"""
    import zeldovich_plt_amd.api as api
    assert (C.sizeof(api.ZdParams), len(api.ZdParams._fields_)) == (240, 40)
    assert (C.sizeof(api.ZdParamStrings), len(api.ZdParamStrings._fields_)) == (6312, 22)
    assert (C.sizeof(api.ZdStats), len(api.ZdStats._fields_)) == (184, 10)


def _one_line(capfd, word):
    lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("zeldovich_hip: ") and word in lines[0], (word, lines)


@pytest.fixture(scope="module")
def lib_and_ps():
    import zeldovich_plt_amd.api as api
    return api, api.load_library(), api.PowerSpectrum.from_file(WMAP, BOX)


GOOD = np.array([[0.25, 0.5, 0.75], [0.0, 0.0, 0.0]], dtype=np.float64)
BAD_POSITIONS = [("one", 1.0), ("negative", -1e-300), ("nan", np.nan), ("inf", np.inf), ("two", 2.0)]


def test_displace_refuses_its_arguments_before_a_plan_or_the_gpu(lib_and_ps, capfd):
    api, L, ps = lib_and_ps
    seen = []
    cb = api.PARTICLE_CB(lambda user, first, n, out: seen.append(first) or 0)

    def call(p=None, pk=True, order=3, npart=2, pos=GOOD, tile=1, sweep=0, cb_=cb, **kw):
        p = api.make_params(32, **kw) if p is None else p
        return L.zd_displace(C.byref(p) if p is not False else None, C.byref(ps.pk) if pk else None, None, 0, order, npart,
                             pos.ctypes.data if pos is not None else None, tile, sweep, cb_, None, None)

    capfd.readouterr()
    for order in (0, 2, 4, -1):
        assert call(order=order) != 0
        _one_line(capfd, "order")
    for npart in (0, -5):
        assert call(npart=npart) != 0
        _one_line(capfd, "npart")
    for tile in (0, -1):
        assert call(tile=tile) != 0
        _one_line(capfd, "tile")
    assert call(pos=None) != 0
    _one_line(capfd, "pos_xyz")
    assert call(p=False) != 0
    _one_line(capfd, "parameters")
    assert call(pk=False) != 0
    _one_line(capfd, "power spectrum")
    assert call(cb_=api.PARTICLE_CB()) != 0
    _one_line(capfd, "cb")
    assert call(sweep=-1) != 0
    _one_line(capfd, "max_particles_per_sweep")
    for _name, v in BAD_POSITIONS:
        for axis in range(3):
            pos = GOOD.copy()
            pos[1, axis] = v
            assert call(pos=pos) != 0
            _one_line(capfd, "particle 1")
    assert call(qoneslab=3) != 0
    _one_line(capfd, "ZD_qoneslab")
    assert call(qdensity=2) != 0
    _one_line(capfd, "ZD_qdensity = 2")
    assert call(ngpu=2) != 0
    _one_line(capfd, "ngpu")
    assert not seen
    # the Python layer: the shape of the array is its own check, everything else the library's
    for bad in ([], [[0.5, 0.5]], [0.5, 0.5, 0.5]):
        with pytest.raises(ValueError):
            api.displace(api.make_params(32), ps, bad)
    with pytest.raises(RuntimeError):
        api.displace(api.make_params(32), ps, [[0.5, 0.5, 1.0]])
    _one_line(capfd, "outside [0, 1)")
    with pytest.raises(RuntimeError):
        api.displace(api.make_params(32), ps, GOOD, order=2)
    _one_line(capfd, "order")


def test_interp_create_refuses_its_arguments_before_the_gpu(lib_and_ps, capfd):
    api, L, _ps = lib_and_ps
    h = C.c_void_p()

    def call(ppd=32, fmt=2, order=3, npart=2, pos=GOOD, out=True):
        return L.zd_interp_create(ppd, fmt, order, npart, pos.ctypes.data if pos is not None else None, C.byref(h) if out else None)

    capfd.readouterr()
    for kw, word in ((dict(order=2), "order"), (dict(order=0), "order"), (dict(npart=0), "npart"), (dict(npart=-1), "npart"),
                     (dict(pos=None), "pos_xyz"), (dict(out=False), "out"), (dict(ppd=2), "ppd"), (dict(ppd=1 << 20), "ppd"),
                     (dict(fmt=4), "icformat"), (dict(fmt=-1), "icformat")):
        assert call(**kw) != 0
        _one_line(capfd, word)
        assert not h.value
    for _name, v in BAD_POSITIONS:
        pos = GOOD.copy()
        pos[0, 2] = v
        assert call(pos=pos) != 0
        _one_line(capfd, "particle 0")
    # misuse of the other entry points without an object
    assert L.zd_interp_add_plane(None, 0, None, None) != 0
    _one_line(capfd, "object")
    assert L.zd_interp_result(None, None) != 0
    _one_line(capfd, "object")
    assert L.zd_plan_interp(None, None, None) != 0
    _one_line(capfd, "plan")
    L.zd_interp_destroy(None)
    with pytest.raises(RuntimeError):
        api.Interp(32, "RVdoubleZel", [[0.5, 0.5, -0.5]])
    _one_line(capfd, "outside [0, 1)")
