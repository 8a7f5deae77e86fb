"""GPU: a run on a caller-supplied density or white-noise field (generate_field, Plan.from_field, ZD_Field_filename; definition in
zeldovich_plt_amd/csrc/zd_kernels_field.hip).

The yardstick is tests/field_ref.py, the definition restated with numpy.fft and held to the oracle's records in tests/test_field.py.
The tolerance is the project's parity bound, 1e-10 of max|q|, wherever no other bound is stated; every test prints its figures before
it asserts."""
import os
import re
import subprocess

import numpy as np
import pytest

import field_ref
from conftest import ROOT, WMAP

pytestmark = pytest.mark.gpu

BOX = 720.0
TOL = 1e-10
PLT = dict(qPLT=1, qPLTrescale=1, PLT_target_z=5.0, f_cluster=0.97)
EXE = os.path.join(ROOT, "zeldovich_plt_amd", "csrc", "build", "zeldovich")


@pytest.fixture(scope="module")
def zd():
    import zeldovich_plt_amd.api as api
    return api


@pytest.fixture(scope="module")
def ps(zd):
    return zd.PowerSpectrum.from_file(WMAP, BOX)


_NOISE = {}


def _noise(n):
    """default_rng(1).standard_normal((n, n, n)): Nyquist and corner content that the zero rule must remove (shared, read-only)"""
    if n not in _NOISE:
        a = np.random.default_rng(1).standard_normal((n, n, n))
        a.setflags(write=False)
        _NOISE[n] = a
    return _NOISE[n]


def _check(rec, q, v, label, tol=TOL):
    scale = np.abs(q).max()
    assert scale > 0, label
    ed = np.abs(rec["d"] - q).max() / scale
    ev = np.abs(rec["v"] - v).max() / max(np.abs(v).max(), 1e-300)
    print(label, "max|q| =", scale, "displacement error", ed, "velocity error", ev)
    assert ed <= tol and ev <= tol, (label, ed, ev)


def _check_ijk(rec):
    n = rec.shape[0]
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    assert np.array_equal(rec["ijk"], np.stack([z, y, x], axis=-1).astype(rec["ijk"].dtype))


# ---- 1. against the reference, where the mask matters ------------------------------------------------------------------------
CASES = [(32, {}), (64, {}), (128, {}), (64, dict(k_cutoff=2.0)), (64, dict(k_cutoff=2.0, corner_modes=1)),
         (64, dict(qonemode=1, one_mode=(3, 2, -4))), (64, dict(qonemode=1, one_mode=(-5, 0, 7)))]


@pytest.mark.parametrize("n,kw", CASES, ids=["%d-%s" % (n, "-".join("%s%s" % kv for kv in kw.items()) or "plain") for n, kw in CASES])
def test_records_against_numpy(zd, ps, n, kw):
    p = zd.make_params(n, boxsize=BOX, **kw)
    q, v, _dens = field_ref.displace(_noise(n), p)
    got = zd.generate_field(p, ps, _noise(n))
    assert sorted(got["planes_seen"]) == list(range(n))
    _check_ijk(got["records"])
    _check(got["records"], q, v, "PPD %d %r" % (n, kw))


# ---- 2. seeds and fields meet --------------------------------------------------------------------------------------------------
_SEEDED = {}


def _seeded(zd, ps, n):
    """an ordinary seeded ZA run and the density its displacement belongs to, once per size"""
    if n not in _SEEDED:
        rec = zd.generate(zd.make_params(n, boxsize=BOX), ps)["records"]
        delta = field_ref.delta_from_za(rec, BOX)
        delta.setflags(write=False)
        _SEEDED[n] = (rec, delta)
    return _SEEDED[n]


def test_the_density_of_a_seeded_run_returns_its_records(zd, ps):
    rec, delta = _seeded(zd, ps, 64)
    got = zd.generate_field(zd.make_params(64, boxsize=BOX, seed=999), ps, delta)["records"]  # (ZD_Seed is ignored)
    _check(got, rec["d"], rec["v"], "PPD 64 ZA, seeded run")


def test_the_same_density_with_plt_returns_the_seeded_plt_run(zd, ps, oracle):
    _rec, delta = _seeded(zd, ps, 64)
    eig = oracle.synthetic_eigenmodes(128)
    ref = zd.generate(zd.make_params(64, boxsize=BOX, **PLT), ps, eig=eig)["records"]
    got = zd.generate_field(zd.make_params(64, boxsize=BOX, **PLT), ps, delta, eig=eig)["records"]
    _check(got, ref["d"], ref["v"], "PPD 64 PLT + rescale, seeded run")


@pytest.mark.parametrize("R", [1, 2, 4])
def test_every_stream_factor(zd, ps, R):
    rec, delta = _seeded(zd, ps, 128)
    got = zd.generate_field(zd.make_params(128, boxsize=BOX, stream_factor=R), ps, delta)
    assert got["stream_factor"] == R and sorted(got["planes_seen"]) == list(range(128))
    _check(got["records"], rec["d"], rec["v"], "PPD 128 ZA, stream factor %d" % R)


# ---- 3. ZD_qdensity ------------------------------------------------------------------------------------------------------------
def test_density_output(zd, ps):
    """the delivered float32 density is float32(masked field): one float32 rounding plus the compute bound, 2^-23 max|delta|"""
    n = 64
    p1 = zd.make_params(n, boxsize=BOX, qdensity=1)
    q, v, dens = field_ref.displace(_noise(n), p1)
    scale = np.abs(dens).max()
    got = zd.generate_field(p1, ps, _noise(n))
    err = np.abs(got["density"].astype(np.float64) - dens.astype(np.float32).astype(np.float64)).max() / scale
    print("ZD_qdensity = 1: max|delta| =", scale, "density error / max|delta| =", err, "bound", 2.0 ** -23)
    assert got["density"].dtype == np.float32 and err <= 2.0 ** -23
    _check(got["records"], q, v, "PPD 64 with ZD_qdensity = 1")
    only = zd.generate_field(zd.make_params(n, boxsize=BOX, qdensity=2), ps, _noise(n))
    assert only["records"] is None
    err2 = np.abs(only["density"].astype(np.float64) - dens.astype(np.float32).astype(np.float64)).max() / scale
    print("ZD_qdensity = 2: density error / max|delta| =", err2)
    assert err2 <= 2.0 ** -23


# ---- 4. input forms ------------------------------------------------------------------------------------------------------------
def test_input_forms_give_identical_bits(zd, ps):
    import torch
    n = 64
    a64 = _noise(n).astype(np.float32).astype(np.float64)  # float64 values that float32 holds exactly
    a32 = a64.astype(np.float32)
    assert np.array_equal(a32.astype(np.float64), a64)
    p = zd.make_params(n, boxsize=BOX)
    forms = {"host float64": a64, "host float32": a32, "device float64": torch.from_numpy(a64).cuda(), "device float32": torch.from_numpy(a32).cuda()}
    base = zd.generate_field(p, ps, a64)["records"].tobytes()
    for name, f in forms.items():
        assert zd.generate_field(p, ps, f)["records"].tobytes() == base, name
    assert zd.generate_field(p, ps, forms["device float32"])["records"].tobytes() == base  # (and twice the same)


# ---- 5. white noise ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spectrum", ["tabulated", "powerlaw"])
def test_white_noise_is_the_coloured_density(zd, ps, spectrum):
    n = 64
    pw = ps if spectrum == "tabulated" else zd.PowerSpectrum.from_powerlaw(-1.5, BOX)
    p = zd.make_params(n, boxsize=BOX)
    a = zd.generate_field(p, pw, _noise(n), kind="white")["records"]
    b = zd.generate_field(p, pw, field_ref.white_to_density(_noise(n), pw, p), kind="density")["records"]
    _check(a, b["d"], b["v"], "PPD 64 white, %s spectrum" % spectrum)


# ---- 6. the four ICFormats -----------------------------------------------------------------------------------------------------
def test_record_formats(zd, ps):
    n = 32
    ref = zd.generate_field(zd.make_params(n, boxsize=BOX), ps, _noise(n))["records"]
    for fmt in ("RVZel", "Zeldovich", "ZelSimple"):
        got = zd.generate_field(zd.make_params(n, boxsize=BOX, icformat=fmt), ps, _noise(n))["records"]
        if "ijk" in got.dtype.names:
            assert np.array_equal(got["ijk"], ref["ijk"])
        for f in ("d", "v"):
            if f in got.dtype.names:  # (cast as the parity tests cast: 1e-6 for the float32 members)
                tol = TOL if got[f].dtype == np.float64 else 1e-6
                err = np.abs(got[f] - ref[f]).max() / np.abs(ref[f]).max()
                print(fmt, f, "error", err)
                assert err <= tol, (fmt, f, err)


# ---- 7. every instantiated length ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,R", [(256, 1), (512, 2), (1024, 4), (2048, 8)])
def test_every_length_against_plane_waves(zd, ps, n, R):
    """three waves built ON THE DEVICE (one with ky = 0, one with negative components, one with |kx| = N/2 - 1), compared at 4200
    sites of three planes through the staged calls: neither the records nor the field ever come to the host.  (2048: the float64
    field, PhiK and the workspace are 138 GB; the field is released before the store of the pass, stream factor 8, is allocated.)"""
    import torch
    waves = [((5, 0, 3), 1.0, 0.3), ((-7, 11, -2), 0.7, 1.1), ((n // 2 - 1, 4, 9), 0.4, -0.6)]
    p = zd.make_params(n, boxsize=BOX, stream_factor=R)
    plan_probe_planes = [0, (n // R) // 3, n // R - 1]  # local planes of pass 0
    rng = np.random.default_rng(n)
    yx = rng.integers(0, n, (3, 1400, 2))
    field = field_ref.plane_waves(n, waves, BOX, [(0, 0, 0)], xp=torch, device="cuda")[0]
    plan = zd.Plan.from_field(p, ps, field)
    del field
    torch.cuda.empty_cache()
    try:
        assert plan.R == R and plan.record_size == 56
        store = torch.empty(plan.exchange_bytes, dtype=torch.uint8, device="cuda")
        rec = torch.empty(n * n * 56, dtype=torch.uint8, device="cuda")
        plan.stage_z(0, store.data_ptr())
        plan.stage_y(store.data_ptr())
        worst, scale = 0.0, 0.0
        for i, lp in enumerate(plan_probe_planes):
            z = plan.plane_z(0, lp)
            plan.stage_x(0, store.data_ptr(), lp, 1, rec.data_ptr())
            torch.cuda.synchronize()
            rows = torch.from_numpy(yx[i, :, 0] * n + yx[i, :, 1]).cuda()
            got = rec.view(n * n, 56)[rows].cpu().numpy().view(zd.RECORD_DTYPES["RVdoubleZel"]).reshape(-1)
            sites = np.column_stack([np.full(1400, z), yx[i]])
            _none, q, v = field_ref.plane_waves(n, waves, BOX, sites, xp=None)
            assert np.array_equal(got["ijk"], sites.astype(got["ijk"].dtype))
            scale = max(scale, np.abs(q).max())
            worst = max(worst, np.abs(got["d"] - q).max(), np.abs(got["v"] - v).max())
        print("PPD", n, "stream factor", R, "max|q| =", scale, "worst error / max|q| =", worst / scale)
        assert worst <= TOL * scale
    finally:
        plan.close()


# ---- 8. the plan is a plan -----------------------------------------------------------------------------------------------------
def test_the_plan_is_a_plan(zd, ps):
    n = 64
    p = zd.make_params(n, boxsize=BOX)
    rec = zd.generate_field(p, ps, _noise(n))["records"]
    scale = np.abs(rec["d"]).max()
    plan = zd.Plan.from_field(p, ps, _noise(n))
    try:
        sites = np.random.default_rng(5).integers(0, n, (8, 3))
        at = (sites[:, 0], sites[:, 1], sites[:, 2])
        ds = plan.direct_sum(sites)  # qx, qy, qz, vx, vy, vz, density; the records hold (qz, qy, qx)
        e1 = max(np.abs(ds[:, 2::-1] - rec["d"][at]).max(), np.abs(ds[:, 5:2:-1] - rec["v"][at]).max()) / scale
        print("direct_sum at 8 sites: error / max|q| =", e1)
        assert e1 <= TOL
        # band power: numpy's binning of the masked |D|^2 over all N^3 wavevectors
        D = np.fft.fftn(_noise(n)) / n ** 3 * field_ref.alive_mask(p)
        k = field_ref.wavenumbers(n)
        kz, ky, kx = np.meshgrid(k, k, k, indexing="ij")
        shell = np.floor(np.sqrt((kx * kx + ky * ky + kz * kz).astype(np.float64))).astype(np.int64)
        pw = plan.measure_power(1)
        want = np.bincount(shell.ravel(), weights=(np.abs(D) ** 2).ravel(), minlength=len(pw["sum_dens"]))[:len(pw["sum_dens"])]
        e2 = np.abs(pw["sum_dens"] - want).max() / want.max()
        print("measure_power: worst shell error / largest shell =", e2)
        assert e2 <= 1e-12
        pos = sites[:, ::-1] / float(n)  # (x, y, z) in box units: lattice sites
        it = plan.interp(pos, order=3)
        e3 = max(np.abs(it[:, 2::-1] - rec["d"][at]).max(), np.abs(it[:, 5:2:-1] - rec["v"][at]).max()) / scale
        print("interp at lattice sites: error / max|q| =", e3)
        assert e3 <= TOL
    finally:
        plan.close()


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------
PAR = """BoxSize = 720
CPD = 5
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
ZD_qdensity = 0
"""
REFUSED = [  # (make_params arguments, spectrum arguments, lines of the parameter file, the option the line names)
    (dict(f_NL=50.0), {}, "ZD_f_NL = 50\nZD_n_s = 0.96\nOmega_M = 0.3\n", "ZD_f_NL"),
    (dict(q2LPT=1), {}, "ZD_q2LPT = 1\n", "ZD_q2LPT"),
    (dict(q2LPT=1, q3LPT=1), {}, "ZD_q2LPT = 1\nZD_q3LPT = 1\n", "ZD_q3LPT"),
    (dict(version=1), {}, "ZD_Version = 1\n", "ZD_Version"),
    ({}, dict(fix_to_mean=1), "ZD_qPk_fix_to_mean = 1\n", "ZD_qPk_fix_to_mean"),
    (dict(ngpu=2), {}, "ZD_NumGPU = 2\n", "ZD_NumGPU"),
    (dict(ppd=48), {}, None, "PPD"),
]


def _one_field_line(err, word):
    lines = [ln for ln in err.splitlines() if ln.startswith("zeldovich_hip: ZD_Field")]
    assert len(lines) == 1 and word in lines[0], (word, err)


@pytest.mark.parametrize("kw,pkw,par,word", REFUSED, ids=[r[3] for r in REFUSED])
def test_refusals(zd, capfd, tmp_path, kw, pkw, par, word):
    kw = dict(kw)
    n = kw.pop("ppd", 32)
    field = np.zeros((n, n, n), dtype=np.float32)
    field[1, 2, 3] = 1.0
    pw = zd.PowerSpectrum.from_file(WMAP, BOX, **pkw)
    p = zd.make_params(n, boxsize=BOX, **kw)
    capfd.readouterr()
    with pytest.raises(RuntimeError):
        zd.generate_field(p, pw, field)
    _one_field_line(capfd.readouterr().err, word)
    with pytest.raises(RuntimeError):
        zd.Plan.from_field(p, pw, field)
    _one_field_line(capfd.readouterr().err, word)
    # ... and through the command line
    out = tmp_path / "ic"
    out.mkdir()
    field.tofile(tmp_path / "field.f32")
    text = PAR % dict(out=out, pk=WMAP, np=n ** 3) + 'ZD_Field_filename = "%s"\n' % (tmp_path / "field.f32") + (par or "")
    if "ZD_Version" not in text:
        text += "ZD_Version = 2\n"
    (tmp_path / "f.par").write_text(text)
    r = subprocess.run([EXE, str(tmp_path / "f.par")], capture_output=True, text=True)
    assert r.returncode == 1, (r.returncode, r.stderr)
    _one_field_line(r.stderr, word)


def test_arrays_python_refuses(zd, ps):
    import torch
    n = 32
    p = zd.make_params(n, boxsize=BOX)
    good = np.zeros((n, n, n))
    bad = [good[:, :, :31], good.astype(np.int32), good.astype(np.float16), good.transpose(2, 1, 0), good[::1, ::1, ::-1], good.tolist(),
           torch.zeros((n, n, n), dtype=torch.float64), torch.zeros((n, n, n), dtype=torch.int32, device="cuda"),
           torch.zeros((n, n, 2 * n), dtype=torch.float64, device="cuda")[:, :, ::2], torch.zeros((n, n), dtype=torch.float64, device="cuda")]
    for f in bad:
        with pytest.raises((TypeError, ValueError)):
            zd.generate_field(p, ps, f)
        with pytest.raises((TypeError, ValueError)):
            zd.Plan.from_field(p, ps, f)
    with pytest.raises(ValueError):
        zd.generate_field(p, ps, good, kind="pink")


# ---- 10. command line ----------------------------------------------------------------------------------------------------------
def test_command_line(zd, ps, tmp_path):
    n = 32
    a32 = _noise(n).astype(np.float32)
    a64 = a32.astype(np.float64)
    a32.tofile(tmp_path / "a.f32")
    a64.tofile(tmp_path / "a.f64")
    out = tmp_path / "ic"
    out.mkdir()
    par = tmp_path / "f.par"
    head = PAR % dict(out=out, pk=WMAP, np=n ** 3) + "ZD_Version = 2\n"

    def run(extra):
        par.write_text(head + extra)
        return subprocess.run([EXE, str(par)], capture_output=True, text=True)

    def files():
        return b"".join((out / ("ic_%d" % i)).read_bytes() for i in range(5))

    want = zd.generate_field(zd.make_params(n, boxsize=BOX, cpd=5), ps, a64)["records"].tobytes()
    for name, dtype in (("a.f64", "float64"), ("a.f32", "float32")):
        r = run('ZD_Field_filename = "%s"\n' % (tmp_path / name))
        assert r.returncode == 0, r.stderr
        assert "field: density, %s, PPD 32" % dtype in r.stderr.splitlines(), r.stderr
        assert sorted(f.name for f in out.iterdir()) == ["ic_%d" % i for i in range(5)]
        assert files() == want, name
    r = run('ZD_Field_filename = "%s"\nZD_Field_kind = "white"\n' % (tmp_path / "a.f32"))
    assert r.returncode == 0 and "field: white, float32, PPD 32" in r.stderr.splitlines(), r.stderr
    assert files() == zd.generate_field(zd.make_params(n, boxsize=BOX, cpd=5), ps, a32, kind="white")["records"].tobytes()

    def refused(extra, *words):
        r = run(extra)
        lines = [ln for ln in r.stderr.splitlines() if ln.startswith("zeldovich_hip: ZD_Field")]
        assert r.returncode == 1 and len(lines) == 1 and all(w in lines[0] for w in words), (r.returncode, r.stderr)

    (tmp_path / "odd").write_bytes(b"\0" * 1000)
    refused('ZD_Field_filename = "%s"\n' % (tmp_path / "odd"), "1000 bytes", str(4 * n ** 3), str(8 * n ** 3))
    refused('ZD_Field_kind = "white"\n', "ZD_Field_kind needs ZD_Field_filename")
    refused('ZD_Field_filename = "%s"\nZD_Field_kind = "pink"\n' % (tmp_path / "a.f32"), "ZD_Field_kind")
    refused('ZD_Field_filename = "%s"\n' % (tmp_path / "missing"), "cannot be read")


# ---- 11. launch sites (after the tests above) ----------------------------------------------------------------------------------
def test_every_launch_site_was_launched(zd):
    """the three stages at every length of the intake's table have been launched by the tests of this file"""
    txt = open(os.path.join(ROOT, "zeldovich_plt_amd", "csrc", "zd_kernels_field.hip")).read()
    assert txt.count("ZD_LAUNCH_CHECK();") == 3
    sizes = re.findall(r"X\((\d+), (\d+), (\d+), (\d+)\)", re.search(r"#define FIELD_SIZES\(X\)(.*)", txt).group(1))
    assert [int(s[0]) for s in sizes] == [32, 64, 128, 256, 512, 1024, 2048]
    names = [name for (name, _l), cnt in zd.dispatch_report().items() if cnt > 0]
    for N, E, W, ROWS in sizes:
        for launcher, want in (("launch_field_x_t", "N = %s, E = %s, ROWS = %s" % (N, E, ROWS)), ("launch_field_y_t", "N = %s, E = %s, W = %s" % (N, E, W)),
                               ("launch_field_z_t", "N = %s, E = %s, W = %s" % (N, E, W))):
            assert any(launcher in nm and want in nm for nm in names), "%s<%s> never launched" % (launcher, want)
