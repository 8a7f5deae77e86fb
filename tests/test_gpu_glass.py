"""GPU: displacements and velocities at off-lattice positions (zd_displace, zd_plan_interp, zd_interp_*; definition in
zeldovich_plt_amd/csrc/zd_kernels_glass.hip).

THE PIN is tests/glass_ref.py — the definition in numpy — applied to the records zd.generate(..., collect=True) delivers for the same
parameters on the same GPU; those records are held to the oracle by the rest of the suite.  BOUND 1e-12 max|q|: at most 64 products of
magnitude <= 1.25^3 max|q| are summed in another order, about 3e-14.

The stream factors: the route takes no z lines shorter than 32, so PPD 32 runs at R = 1 only (R = 2 with ZD_q2LPT); R = 1, 2 and 4 — the
z stencil across residue classes, the two-residue passes of the packed and the field store, the reference arrays — run at PPD 128, the
smallest size that accepts all three."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import glass_ref as gr
from conftest import ROOT, WMAP

pytestmark = pytest.mark.gpu
BOX = 720.0
BOUND = 1e-12
EXE = os.path.join(ROOT, "zeldovich_plt_amd", "csrc", "build", "zeldovich")
BELOW_ONE = 1.0 - 2.0 ** -53  # the largest double below 1


@pytest.fixture(scope="module")
def zd():
    import zeldovich_plt_amd.api as api
    return api


@pytest.fixture(scope="module")
def ps(zd):
    return zd.PowerSpectrum.from_file(WMAP, BOX)


@pytest.fixture(scope="module")
def fields(zd, ps):
    """(ppd, make_params keywords) -> (records, float64 fields [z, y, x, 6]) of zd.generate, made once, read-only"""
    cache = {}

    def get(n, eig=None, **kw):
        key = (n, tuple(sorted(kw.items())))
        if key not in cache:
            rec = zd.generate(zd.make_params(n, **kw), ps, eig=eig)["records"]
            f = gr.fields_of_records(rec)
            f.setflags(write=False)
            cache[key] = (rec, f)
        return cache[key]

    return get


def load(n, nrandom=20000, seed=11):
    """uniform random positions plus the chosen ones: lattice sites, p = 0, the largest double below 1 on each axis, the cells N - 2 and
    N - 1 (stencil wrap in x, y and z), 1000 particles inside one cell"""
    rng = np.random.default_rng(seed)
    sites = rng.integers(0, n, size=(500, 3)) / float(n)
    edge = np.array([[0.0, 0.0, 0.0], [BELOW_ONE, 0.3, 0.4], [0.3, BELOW_ONE, 0.4], [0.3, 0.4, BELOW_ONE], [BELOW_ONE] * 3])
    wrap = (rng.integers(n - 2, n, size=(600, 3)) + rng.random((600, 3))) / n
    wrap[:200, 1:] = rng.random((200, 2))       # x wraps alone
    wrap[200:400, ::2] = rng.random((200, 2))   # y alone
    wrap[400:500, :2] = rng.random((100, 2))    # z alone; the last 100 wrap in all three
    one_cell = (np.array([5, n - 1, 3]) + rng.random((1000, 3))) / n
    pos = np.concatenate([rng.random((nrandom, 3)), sites, edge, np.minimum(wrap, BELOW_ONE), np.minimum(one_cell, BELOW_ONE)])
    assert pos.min() >= 0.0 and pos.max() < 1.0
    return pos, slice(nrandom, nrandom + 500)


def check(got, f, pos, order, what=""):
    want = gr.interpolate(f, pos, order)
    qmax = np.abs(f[..., :3]).max()
    err = np.abs(got - want).max() / qmax
    print("%s order %d: max |displace - numpy| / max|q| = %.3g (%d particles)" % (what, order, err, pos.shape[0]))
    assert err <= BOUND, (what, order, err)
    return err


@pytest.mark.parametrize("order", [1, 3])
@pytest.mark.parametrize("fmt", ["RVdoubleZel", "RVZel", "Zeldovich", "ZelSimple"])
def test_every_format_at_ppd_32(zd, ps, fields, fmt, order):
    """float32 records are compared against numpy on the same float32 records; formats without velocities return exact zeros; lattice
    sites return the delivered records exactly; a second call returns the same bits"""
    n = 32
    rec, f = fields(n, icformat=fmt)
    pos, at_sites = load(n)
    p = zd.make_params(n, icformat=fmt)
    got = zd.displace(p, ps, pos, order=order)
    check(got, f, pos, order, fmt)
    if "v" in rec.dtype.names:
        assert np.abs(got[:, 3:]).max() > 0
    else:
        assert not got[:, 3:].any()
    cell = np.rint(pos[at_sites] * n).astype(int)
    assert np.array_equal(got[at_sites], f[cell[:, 2], cell[:, 1], cell[:, 0]])
    assert not pos[at_sites.stop].any() and np.array_equal(got[at_sites.stop], f[0, 0, 0])  # p = 0
    assert np.array_equal(zd.displace(p, ps, pos, order=order), got)
    # a particle's result does not depend on the rest of the load: the same bits in a load of 300
    assert np.array_equal(zd.displace(p, ps, pos[at_sites.start - 100:at_sites.start + 200], order=order), got[at_sites.start - 100:at_sites.start + 200])


@pytest.mark.parametrize("order", [1, 3])
def test_stream_factors_and_stores_at_ppd_128(zd, ps, fields, order):
    """R = 1 against 2 against 4 and the stores: every plane order (residue order, pairs z, z + R / 2) gives the pin within the bound"""
    n = 128
    pos, _ = load(n)
    _rec, f = fields(n)
    res = {}
    for R, store in ((1, "auto"), (2, "auto"), (4, "auto"), (4, "packed"), (4, "fields"), (2, "reference")):
        p = zd.make_params(n, stream_factor=R, store_mode=store)
        st = {}
        res[(R, store)] = zd.displace(p, ps, pos, order=order, stats=st)
        assert st["stream_factor"] == R and st["sweeps"] == 1
        qmax = np.abs(f[..., :3]).max()
        err = np.abs(res[(R, store)] - gr.interpolate(f, pos, order)).max() / qmax if (R, store) == (1, "auto") else \
            np.abs(res[(R, store)] - res[(1, "auto")]).max() / qmax
        print("R = %d, %s store, order %d: %.3g" % (R, store, order, err))
        assert err <= BOUND, (R, store, err)


def test_one_particle_and_a_load_that_leaves_most_z_bins_empty(zd, ps, fields):
    n = 32
    _rec, f = fields(n)
    p = zd.make_params(n)
    for order in (1, 3):
        one = np.array([[0.123, 0.987, 0.5001]])
        check(zd.displace(p, ps, one, order=order), f, one, order, "npart = 1")
        rng = np.random.default_rng(2)
        thin = rng.random((3000, 3))
        thin[:, 2] = (np.array([3, 30])[rng.integers(0, 2, 3000)] + rng.random(3000)) / n  # two z cells hold everything
        check(zd.displace(p, ps, thin, order=order), f, thin, order, "two z bins")


def test_sweeps_and_tiling(zd, ps, fields):
    """max_particles_per_sweep forcing three sweeps returns the bits of one sweep; a tiled load returns the bits of the explicitly
    expanded one"""
    n = 32
    _rec, f = fields(n)
    p = zd.make_params(n)
    pos, _ = load(n, nrandom=3000)
    st1, st3 = {}, {}
    one = zd.displace(p, ps, pos, order=3, stats=st1)
    three = zd.displace(p, ps, pos, order=3, max_particles_per_sweep=(pos.shape[0] + 2) // 3, stats=st3)
    assert (st1["sweeps"], st3["sweeps"]) == (1, 3)
    assert np.array_equal(one, three)
    base = np.random.default_rng(9).random((700, 3))
    for order in (1, 3):
        full = gr.tiled(base, 3)
        tiled = zd.displace(p, ps, base, order=order, tile=3)
        assert tiled.shape == (700 * 27, 6)
        assert np.array_equal(tiled, zd.displace(p, ps, full, order=order))
        assert np.array_equal(tiled, zd.displace(p, ps, base, order=order, tile=3, max_particles_per_sweep=5000))  # sweeps across tiles
        check(tiled, f, full, order, "tile = 3")


def test_plt_rescale_with_four_arrays_at_ppd_64(zd, ps, fields, oracle):
    n = 64
    eig = oracle.synthetic_eigenmodes(32)
    kw = dict(qPLT=1, qPLTrescale=1, PLT_target_z=5.0, store_mode="reference")
    _rec, f = fields(n, eig=eig, **kw)
    pos, _ = load(n)
    for order in (1, 3):
        check(zd.displace(zd.make_params(n, **kw), ps, pos, order=order, eig=eig), f, pos, order, "PLT + rescale")


@pytest.mark.parametrize("n,what", [(96, "composite"), (50, "convolution")])
def test_composite_and_convolution_grids(zd, ps, fields, n, what):
    _rec, f = fields(n)
    pos, _ = load(n)
    for order in (1, 3):
        check(zd.displace(zd.make_params(n), ps, pos, order=order), f, pos, order, "PPD %d (%s)" % (n, what))


@pytest.mark.parametrize("kw", [dict(q2LPT=1), dict(qdensity=1)], ids=["2LPT", "qdensity"])
def test_second_order_and_density_runs_at_ppd_32(zd, ps, fields, kw):
    """ZD_q2LPT = 1: the records hold both orders; ZD_qdensity = 1: accepted, the density plane ignored"""
    n = 32
    _rec, f = fields(n, **kw)
    pos, _ = load(n)
    for order in (1, 3):
        check(zd.displace(zd.make_params(n, **kw), ps, pos, order=order), f, pos, order, str(kw))


def test_mid_size_ppd_256_with_a_tiled_load_of_a_million(zd, ps, fields):
    """bins of 8 x 8 cells over 32 tiles per side, thousands of workgroups per plane: a 50^3 random load at tile = 2"""
    n = 256
    _rec, f = fields(n, icformat="Zeldovich")
    base = np.random.default_rng(4).random((50 ** 3, 3))
    got = zd.displace(zd.make_params(n, icformat="Zeldovich"), ps, base, order=3, tile=2)
    assert got.shape == (10 ** 6, 6)
    check(got[:, :3], f[..., :3], gr.tiled(base, 2), 3, "PPD 256, 10^6 particles")


def test_plan_interp_and_planes_fed_by_hand(zd, ps, fields):
    """Plan.interp (zd_plan_interp) returns the bits of displace; the consumer object fed plane by plane from device copies of the
    delivered records returns them too when the planes come in the plan's order (z = 0, 1, ... at R = 1), and stays within the bound
    in a scrambled order (a particle's sum over its z planes is then added in another order)"""
    import torch
    n = 32
    rec, f = fields(n)
    pos, _ = load(n, nrandom=4000)
    p = zd.make_params(n)
    want = zd.displace(p, ps, pos, order=3)
    pl = zd.Plan(p, ps)
    assert np.array_equal(pl.interp(pos, order=3), want)
    check(pl.interp(pos, order=1), f, pos, 1, "Plan.interp")
    pl.close()
    dev = torch.from_numpy(rec.view(np.uint8).reshape(n, -1).copy()).cuda()
    it = zd.Interp(n, "RVdoubleZel", pos, order=3)
    for z in range(n):
        it.add_plane(z, dev[z].data_ptr())
    assert np.array_equal(it.result(), want)
    assert np.array_equal(it.result(), want)  # (the result can be taken again)
    it.close()
    it = zd.Interp(n, "RVdoubleZel", pos, order=3)
    for z in np.random.default_rng(1).permutation(n):
        it.add_plane(int(z), dev[int(z)].data_ptr())
    check(it.result(), f, pos, 3, "scrambled planes")
    it.close()


def test_misuse_of_the_consumer_object(zd, ps, fields, capfd):
    """a plane fed twice, a plane missing at result, a z out of range: non-zero with one line, no fault"""
    import torch
    n = 32
    rec, _f = fields(n)
    dev = torch.from_numpy(rec.view(np.uint8).reshape(n, -1).copy()).cuda()
    pos = np.random.default_rng(3).random((100, 3))
    it = zd.Interp(n, "RVdoubleZel", pos, order=3)
    other = zd.Interp(64, "RVdoubleZel", pos, order=3)
    pl = zd.Plan(zd.make_params(n), ps)
    L, out = zd.load_library(), np.zeros((100, 6))
    capfd.readouterr()

    def one_line(word):
        lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.strip()]
        assert len(lines) == 1 and lines[0].startswith("zeldovich_hip: ") and word in lines[0], lines

    for z in (-1, n, n + 5):
        assert L.zd_interp_add_plane(it.h, z, dev[0].data_ptr(), None) != 0
        one_line("outside [0, 32)")
    assert L.zd_interp_add_plane(it.h, 3, None, None) != 0
    one_line("null pointer")
    it.add_plane(3, dev[3].data_ptr())
    assert L.zd_interp_add_plane(it.h, 3, dev[3].data_ptr(), None) != 0
    one_line("added before")
    assert L.zd_interp_result(it.h, out.ctypes.data) != 0
    one_line("31 of 32 planes have not been added")
    for z in range(n):
        if z != 3 and z != 17:
            it.add_plane(z, dev[z].data_ptr())
    assert L.zd_interp_result(it.h, out.ctypes.data) != 0
    one_line("z = 17")
    assert L.zd_interp_result(it.h, None) != 0
    one_line("out6")
    it.add_plane(17, dev[17].data_ptr())
    assert L.zd_interp_result(it.h, out.ctypes.data) == 0 and np.abs(out).max() > 0
    # a plan that cannot feed the object
    assert L.zd_plan_interp(pl.h, other.h, None) != 0
    one_line("made for ppd = 64")
    for o in (it, other, pl):
        o.close()


def test_oversampling_on_the_gpu(zd, ps, fields):
    """PPD 64 with k_cutoff 4 against PPD 128 with k_cutoff 8: order 3 at every site of the 128 lattice meets the 128 run's records
    within twice the CPU figure of tests/test_glass.py (0.00147)"""
    n = 64
    _rec, b = fields(2 * n, k_cutoff=8.0)
    m = 2 * n
    z, y, x = np.meshgrid(np.arange(m), np.arange(m), np.arange(m), indexing="ij")
    pos = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1) / float(m)
    got = zd.displace(zd.make_params(n, k_cutoff=4.0), ps, pos, order=3).reshape(m, m, m, 6)
    err = np.abs(got[..., :3] - b[..., :3]).max() / np.abs(b[..., :3]).max()
    print("oversampling 64 -> 128, order 3: %.4g" % err)
    assert err <= 2 * 0.00147


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
ZD_qdensity = 0
"""


def test_command_line(zd, ps, tmp_path):
    out = tmp_path / "ic"
    out.mkdir()
    base = np.random.default_rng(8).random((900, 3))
    glass = tmp_path / "glass.f64"
    base.tofile(glass)
    par = tmp_path / "g.par"
    par.write_text(PAR % dict(out=out, pk=WMAP) + 'ZD_Glass_filename = "%s"\nZD_Glass_tile = 2\n' % glass)
    r = subprocess.run([EXE, str(par)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "glass: 7200 particles, order 3, 1 sweeps" in r.stderr.splitlines(), r.stderr
    assert sorted(f.name for f in out.iterdir()) == ["ic_glass"]  # no lattice file
    got = np.fromfile(out / "ic_glass", dtype=np.float64).reshape(-1, 9)
    assert np.array_equal(got[:, :3], gr.tiled(base, 2))
    assert np.array_equal(got[:, 3:], zd.displace(zd.make_params(32, cpd=5), ps, base, order=3, tile=2))
    # order and output file of one's own
    par.write_text(PAR % dict(out=out, pk=WMAP) + 'ZD_Glass_filename = "%s"\nZD_Glass_order = 1\nZD_Glass_output = "%s"\n' % (glass, tmp_path / "o1"))
    r = subprocess.run([EXE, str(par)], capture_output=True, text=True)
    assert r.returncode == 0 and "glass: 900 particles, order 1, 1 sweeps" in r.stderr.splitlines(), r.stderr
    got = np.fromfile(tmp_path / "o1", dtype=np.float64).reshape(-1, 9)
    assert np.array_equal(got[:, 3:], zd.displace(zd.make_params(32, cpd=5), ps, base, order=1))

    def refused(extra, word):
        par.write_text(PAR % dict(out=out, pk=WMAP) + extra)
        r = subprocess.run([EXE, str(par)], capture_output=True, text=True)
        lines = [ln for ln in r.stderr.splitlines() if ln.strip()]
        assert r.returncode == 1 and len(lines) == 1 and word in lines[0], (r.returncode, lines)

    refused("ZD_Glass_tile = 2\n", "ZD_Glass_tile needs ZD_Glass_filename")
    odd = tmp_path / "odd.f64"
    odd.write_bytes(b"\0" * 100)
    refused('ZD_Glass_filename = "%s"\n' % odd, "multiple of 24")
    bad = base.copy()
    bad[5, 1] = 1.0
    bad.tofile(tmp_path / "bad.f64")
    refused('ZD_Glass_filename = "%s"\n' % (tmp_path / "bad.f64"), "particle 5")
    refused('ZD_Glass_filename = "%s"\nZD_Glass_order = 2\n' % glass, "ZD_Glass_order")


def test_every_new_launch_site_was_reached(zd):
    """every launch site of zd_kernels_glass.hip, and every (order, format) instantiation of the accumulate kernel, is in
    zd_dispatch_report with a count after the tests above"""
    src = open(os.path.join(ROOT, "zeldovich_plt_amd", "csrc", "zd_kernels_glass.hip")).read().splitlines()
    lines = [i + 1 for i, ln in enumerate(src) if "ZD_LAUNCH_CHECK();" in ln]
    assert len(lines) == 8
    rep = {k: v for k, v in zd.dispatch_report().items() if re.search(r"launch_glass_|launch_interp_plane_t", k[0])}
    for ln in lines:
        assert any(line == ln and cnt > 0 for (_name, line), cnt in rep.items()), "launch site at line %d never reached" % ln
    names = [name for (name, _line), cnt in rep.items() if "launch_interp_plane_t" in name and cnt > 0]
    for order in (1, 3):
        for fmt in range(4):
            assert any("ORDER = %d, FMT = %d" % (order, fmt) in nm for nm in names), (order, fmt, names)
