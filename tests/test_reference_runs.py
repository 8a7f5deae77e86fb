"""CPU: the oracle against records the COMPLETE reference program wrote (tests/golden/reference_runs/, written by
tests/golden/make_reference_runs.py from oracle/_ref/zeldovich_ref), and this project's stand-ins for GSL, FFTW3 and
ParseHeader -- the three things that program is linked against here -- against independent truths.  Until these fixtures
existed the oracle's mode loop, zero rule, PLT algebra, transforms, epilogue, ZD_Version = 1 streams and f_NL round were
checked only against restatements by the same reader of the same source.

Bound for float64 fields, fixed before the comparison was first asserted: the worst |oracle - reference| / max|field| over
the kept planes of all 27 configurations was measured once (figures per configuration in DESIGN.md section 6; worst 5.6e-16,
the f_NL run), ten times that rounded up to a decade is 1e-14, tighter than the 1e-12 the project uses between two of its own
double routes.  float32 fields: the project's 1e-6.  Signed sums: |delta| <= tol n^2 max|field|."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import reference_runs as rr
from conftest import ROOT, WMAP

TOL64 = 1e-14
TOL32 = 1e-6
SHIMS = os.path.join(ROOT, "oracle", "_build", "libzd_shims.so")
needs_reference = pytest.mark.skipif(not os.path.exists(rr.REF_EXE),
                                     reason="oracle/_ref/zeldovich_ref is built only where the reference's sources are mounted")


@pytest.fixture(scope="module")
def api():
    import zeldovich_plt_amd.api as api
    api.load_library()
    return api


@pytest.fixture(scope="module")
def shims(oracle):
    if not os.path.exists(SHIMS):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "_build/libzd_shims.so"])
    L = C.CDLL(SHIMS)
    L.shim_mt_words.argtypes = [C.c_ulong, C.c_int, C.c_void_p, C.c_void_p]
    L.shim_dft.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.shim_parse.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]
    return L


def tol_of(par):
    return TOL64 if rr.par_value(par, "ICFormat") in ("RVdoubleZel", "Zeldovich") else TOL32


def oracle_run(zdo, api, par, tmp):
    """zdo.run with the parameters the PRODUCT's reader takes from the parameter text: returns ({z: records}, {z: density} or
    None, expected file listing, max_disp, rms density, sha-256 of the eigenmode file)"""
    eig, sha = rr.write_eigenmodes(os.path.join(tmp, "eigmodes"), zdo)
    parfile = os.path.join(tmp, "oracle.par")
    with open(parfile, "w") as f:
        f.write(rr.fill(par, os.path.join(tmp, "unused_out"), WMAP, os.path.join(tmp, "eigmodes")))
    p, s = api.params_from_file(parfile)
    fmt = s.ICFormat.decode()
    n = int(p.ppd)
    op = zdo.make_params(n, numblock=p.numblock, boxsize=p.boxsize, seed=p.seed, k_cutoff=p.k_cutoff, qPLT=p.qPLT,
                         qPLTrescale=p.qPLTrescale, PLT_target_z=p.PLT_target_z, z_initial=p.z_initial, f_cluster=p.f_cluster,
                         icformat=fmt, qdensity=p.qdensity, qoneslab=p.qoneslab, qonemode=p.qonemode, one_mode=tuple(p.one_mode),
                         CornerModes=p.corner_modes, cpd=p.cpd, f_NL=p.f_NL, n_s=p.n_s, Omega_M=p.Omega_M)
    op.version = p.version      # the reader has scaled NumBlock by ZD_k_cutoff for ZD_Version = 1 already
    if s.Pk_filename:
        pk = zdo.pk_from_file(s.Pk_filename.decode(), p.boxsize, s.Pk_scale, s.Pk_norm, s.Pk_sigma, s.Pk_sigma_ratio, s.Pk_smooth,
                              s.qPk_fix_to_mean)
    else:
        pk = zdo.pk_from_powerlaw(s.Pk_powerlaw_index, p.boxsize, s.Pk_norm, s.Pk_sigma, s.Pk_sigma_ratio, s.Pk_smooth,
                                  s.qPk_fix_to_mean)
    if p.f_NL != 0.0:
        zdo.lib().zdo_pk_set_primordial(C.byref(pk), p.n_s)
    r = zdo.run(op, pk, eig=eig if p.qPLT else None, eig_ppd=rr.EIG_PPD if p.qPLT else 0, want_density=bool(p.qdensity))
    zs = [z for z in range(n) if p.qoneslab < 0 or z == p.qoneslab]
    planes = {z: r["records"][z] for z in zs} if p.qdensity != 2 else {}
    dens = {z: r["density"][z] for z in zs} if p.qdensity else None
    files = {}
    if p.qdensity != 2:
        for z in zs:
            name = "ic_%d" % (z * p.cpd // n)
            files[name] = files.get(name, 0) + n * n * zdo.RECORD_DTYPES[fmt].itemsize
    if p.qdensity:
        files["density%d" % n] = len(zs) * n * n * 4
    return planes, dens, sorted(files.items()), r["max_disp"], float(np.sqrt(r["density_variance"] / float(n) ** 3)), sha


def check_against_fixture(fx, planes, dens, files, max_disp, rms, tol):
    worst = rr.compare(fx, planes, dens, tol)
    print("worst / bound: planes %.3g sums %.3g density %.3g (tol %g)" % (worst["planes"], worst["sums"], worst["dens"], tol))
    assert worst["planes"] <= 1.0 and worst["sums"] <= 1.0 and worst["dens"] <= 1.0, worst
    assert files == fx["files"]
    # the reference prints max_disp with 6 significant digits and the rms density with 6 decimals
    if "ZD_qonemode = 1" in fx["par"]:
        # a plane wave on the lattice takes its extreme value at sites half a period apart with opposite signs, equal but for
        # the last bit: which of them output.cpp:190-193 keeps, and so the sign printed, is decided by rounding
        max_disp, fx = np.abs(max_disp), dict(fx, max_disp=np.abs(fx["max_disp"]))
    for got, want in zip(max_disp, fx["max_disp"]):
        # half a unit of the sixth digit printed; a component that is zero but for rounding (ky = 0 mode) is held to the
        # field's own bound instead of to its own digits
        assert abs(got - want) <= 0.5001 * 10.0 ** (np.floor(np.log10(abs(want))) - 5) + TOL64 * np.abs(fx["max_disp"]).max(), (max_disp, fx["max_disp"])
    assert abs(rms - float(fx["rms_density"])) <= 0.5001e-6


@pytest.mark.parametrize("name", rr.fixture_names())
def test_oracle_matches_reference_run(oracle, api, tmp_path, name):
    fx = rr.load_fixture(name)
    assert fx["par"] == rr.par_text(name)     # the committed text is the one the configuration table gives
    planes, dens, files, max_disp, rms, sha = oracle_run(oracle, api, fx["par"], str(tmp_path))
    if fx["eig_sha256"]:
        assert sha == fx["eig_sha256"]        # the eigenmode table the reference read is the one regenerated here
    check_against_fixture(fx, planes, dens, files, max_disp if fx["max_disp"].size else [], rms, tol_of(fx["par"]))


def test_fixtures_respect_the_size_limit_and_keep_planes():
    for name in rr.fixture_names():
        assert os.path.getsize(os.path.join(rr.FIXDIR, name + ".npz")) <= rr.MAX_FIXTURE_BYTES
        fx = rr.load_fixture(name)
        n = rr.par_ppd(fx["par"])
        assert len(fx["kept_z"]) >= 1 and len(fx["sum_z"]) == (1 if "qoneslab" in fx["par"] else n)


def test_signed_sum_weights():
    """the weights are +-1, differ between planes, components and patterns, and their first word is splitmix64's published
    first output for state 0 when the key is made so"""
    assert int(rr.splitmix64(np.uint64(0))) == 0xE220A8397B1DCDAF     # first output of splitmix64 seeded with 0
    w = np.array([rr.weights(z, c, p, 1024) for z in (0, 1) for c in (0, 1) for p in range(4)])
    assert set(np.unique(w)) == {-1.0, 1.0}
    assert all(not np.array_equal(w[i], w[j]) for i in range(len(w)) for j in range(i))
    assert np.abs(w.sum(axis=1)).max() < 5 * 32     # balanced: |sum| of 1024 fair signs stays below 5 sigma


# ---- the stand-ins against independent truths ------------------------------------------------------------------------------

SEEDS = (0, 1, 5489, 12346, 2 ** 32 - 1, 2 ** 32 + 7)      # those of test_gpu_parity.py::test_v1_stream_words


def _mt(shims, seed, n=1000):
    words, uni = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.float64)
    shims.shim_mt_words(seed, n, words.ctypes.data, uni.ctypes.data)
    return words, uni


def test_standin_mt19937(shims):
    """first word of seed 5489 (the value every MT19937 implementation documents), numpy's MT19937 -- an independent
    implementation with the same init_genrand seeding -- for the seeds of test_v1_stream_words, seed 0 -> 4357, uniform = word / 2^32"""
    assert _mt(shims, 5489)[0][0] == 3499211612
    for seed in SEEDS:
        words, uni = _mt(shims, seed)
        rs = np.random.RandomState(4357 if seed == 0 else seed & 0xffffffff)   # init_genrand seeding; GSL maps 0 to 4357 and keeps 32 bits
        want = rs.randint(0, 2 ** 32, size=1000, dtype=np.uint64).astype(np.uint32)
        assert np.array_equal(words, want), seed
        assert np.array_equal(uni, words / 4294967296.0)
    assert np.array_equal(_mt(shims, 0)[0], _mt(shims, 4357)[0])


def test_standin_mt19937_against_the_oracles_streams(shims, oracle):
    """the oracle's own mt19937 (ZD_Version = 1 streams): the first draws of stream i of seed s are gsl_rng_uniform of seed s + i"""
    L = oracle.lib()
    st = (C.c_uint64 * 640)()        # room for a zdo_mt (624 words and a position)
    L.zdo_mt_seed.argtypes = [C.c_void_p, C.c_ulong]
    L.zdo_mt_next.argtypes = [C.c_void_p]
    L.zdo_mt_next.restype = C.c_uint32
    for seed in SEEDS:
        L.zdo_mt_seed(st, seed)
        got = np.array([L.zdo_mt_next(st) for _ in range(1000)], dtype=np.uint32)
        assert np.array_equal(got, _mt(shims, seed)[0])


@pytest.mark.parametrize("n", [2, 3, 32, 48, 50])
def test_standin_dft(shims, n):
    """unnormalised, FFTW's sign convention (-1 forward = numpy.fft.fft, +1 = n * ifft), 1-D and 2-D (rows then columns = fft2),
    in place, planned on NULL: against numpy.fft (pocketfft, double) to a few ulp of the largest output"""
    rng = np.random.default_rng(n)
    for rank in (1, 2):
        shape = (n,) if rank == 1 else (n, n)
        x = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
        for sign in (-1, +1):
            buf = np.ascontiguousarray(x.copy())
            assert shims.shim_dft(rank, n, n, sign, buf.ctypes.data) == 0
            f = np.fft.fftn if sign < 0 else (lambda a: np.fft.ifftn(a) * a.size)
            want = f(x)
            # numpy's own error is ~ eps log2(n) of the rms output; the stand-in's is half an ulp of each output
            assert np.abs(buf - want).max() <= 8 * np.finfo(float).eps * np.log2(max(n * n if rank == 2 else n, 2)) * np.abs(want).max()
    # a 2-D plan that is not square: rows of n1, then columns of n0
    x = rng.standard_normal((3, n)) + 1j * rng.standard_normal((3, n))
    buf = np.ascontiguousarray(x.copy())
    assert shims.shim_dft(2, 3, n, -1, buf.ctypes.data) == 0
    assert np.abs(buf - np.fft.fft2(x)).max() <= 1e-13 * np.abs(x).max() * n


MUST = "BoxSize ZD_Pk_scale NP ZD_NumBlock CPD ZD_Seed ZD_Pk_norm ZD_Pk_smooth InitialConditionsDirectory InitialRedshift ICFormat"


def _parse(shims, text, must=MUST):
    out = C.create_string_buffer(8192)
    rc = shims.shim_parse(text.encode(), must.encode(), out, len(out))
    return rc, out.value.decode()


def test_standin_parser_on_the_committed_texts(shims):
    """every committed parameter text: what the stand-in hands the reference is what the text says (read here by a regular
    expression per key)"""
    for name in rr.fixture_names():
        par = rr.load_fixture(name)["par"]
        rc, out = _parse(shims, par)
        assert rc == 0, out
        got = dict(line.split("=", 1) for line in out.splitlines())
        for key in ("NP", "ZD_NumBlock", "CPD", "ZD_Seed", "ICFormat", "ZD_qPLT", "ZD_qPLT_rescale", "ZD_Version", "ZD_one_mode",
                    "ZD_Pk_filename", "InitialConditionsDirectory", "ZD_PLT_filename", "ZD_CornerModes", "ZD_qdensity", "ZD_qoneslab"):
            want = rr.par_value(par, key)
            if want is not None:
                assert got[key] == want, (name, key)
        for key, default in (("BoxSize", None), ("ZD_Pk_sigma", 0.0), ("ZD_Pk_sigma_ratio", 0.0), ("ZD_Pk_smooth", 0.0), ("ZD_k_cutoff", 1.0),
                             ("ZD_f_cluster", 1.0), ("ZD_f_NL", 0.0), ("ZD_Pk_powerlaw_index", 1000.0)):
            want = rr.par_value(par, key, default)
            assert float(got[key]) == float(want), (name, key)


def test_standin_parser_grammar_and_refusals(shims):
    base = rr.par_text("base")
    rc, out = _parse(shims, base + '  # a comment line\nZD_one_mode = 1   -2\t3   # trailing\nZD_Pk_sigma_ratio = 1.5D-1\n'
                     'ZD_density_filename = "dens # not a comment"\n')
    assert rc == 0 and "ZD_one_mode=1 -2 3\n" in out and "ZD_Pk_sigma_ratio=0.15\n" in out
    for bad, why in [(base.replace("BoxSize = 720\n", ""), "must be defined"),          # MUST_DEFINE
                     (base + "ZD_Sed = 3\n", "not a registered parameter"),              # a typo cannot fall back to a default
                     (base + "ZD_Seed = 3\n", "defined twice"),
                     (base.replace("NP = 32768", "NP = 32768.5"), "not an integer"),
                     (base.replace("BoxSize = 720", "BoxSize = 7x0"), "not a number"),
                     (base.replace('"RVdoubleZel"', "RVdoubleZel"), "needs a quoted string"),
                     (base.replace("ZD_Seed = 12346", 'ZD_Seed = "12346"'), "cannot take a quoted string"),
                     (base.replace("ZD_Seed = 12346", "ZD_Seed = 1 2"), "takes one value"),
                     (base.replace("ZD_Seed = 12346", "ZD_Seed 12346"), "no '='"),
                     (base.replace('"RVdoubleZel"', '"RVdoubleZel'), "unterminated")]:
        rc, out = _parse(shims, bad)
        assert rc == 1 and why in out, (why, out)


# ---- live: only where the reference binary exists --------------------------------------------------------------------------

def _reference_run(zdo, par, tmp):
    out = os.path.join(tmp, "ref_out")
    rr.write_eigenmodes(os.path.join(tmp, "eigmodes"), zdo)
    with open(os.path.join(tmp, "ref.par"), "w") as f:
        f.write(rr.fill(par, out, WMAP, os.path.join(tmp, "eigmodes")))
    r = subprocess.run([rr.REF_EXE, os.path.join(tmp, "ref.par")], cwd=tmp, capture_output=True, text=True,
                       env=dict(os.environ, OMP_NUM_THREADS="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    fmt, qd = rr.par_value(par, "ICFormat"), int(rr.par_value(par, "ZD_qdensity", "0"))
    planes = rr.read_planes(out, par, zdo.RECORD_DTYPES[fmt]) if qd != 2 else {}
    return planes, rr.read_density(out, par), rr.list_files(out), r.stderr


@needs_reference
@pytest.mark.parametrize("name", rr.ROT_CONFIGS)
def test_fixtures_do_not_rot(oracle, tmp_path, name):
    """a fresh run of the reference program (one OpenMP thread, as the generator runs it) gives the committed planes and sums
    bit for bit"""
    fx = rr.load_fixture(name)
    planes, dens, files, stderr = _reference_run(oracle, fx["par"], str(tmp_path))
    assert files == fx["files"]
    for z in fx["kept_z"]:
        for f in fx["plane_%d" % z].dtype.names:
            if f != "pad":       # padding bytes are indeterminate in the reference
                assert np.array_equal(planes[int(z)][f], fx["plane_%d" % z][f]), (z, f)
    assert np.array_equal(np.array([rr.signed_sums(int(z), planes[int(z)]) for z in fx["sum_z"]]), fx["sums"])


def _random_par(rng):
    n = int(rng.choice([8, 16, 32]))
    fmt = str(rng.choice(["RVdoubleZel", "RVZel", "Zeldovich", "ZelSimple"]))
    plt = int(rng.random() < 0.35)
    if plt and not fmt.startswith("RV"):
        fmt = "RVdoubleZel"
    kv = [("BoxSize", "%r" % float(rng.choice([720.0, 100.0, 1234.5]))), ("CPD", "%d" % rng.integers(1, 3 * n)), ("ICFormat", '"%s"' % fmt),
          ("InitialConditionsDirectory", '"@OUT@"'), ("InitialRedshift", "%r" % float(rng.choice([49.0, 99.0, 10.5]))), ("NP", "%d" % n ** 3),
          ("ZD_NumBlock", "%d" % rng.choice([2, 4] if n > 8 else [2])), ("ZD_Pk_norm", "8.0"), ("ZD_Pk_scale", "%r" % float(rng.choice([1.0, 1.3]))),
          ("ZD_Pk_smooth", "%r" % float(rng.choice([0.0, 0.0, 25.0]))), ("ZD_Seed", "%d" % rng.integers(1, 2 ** 31 - 64)),
          ("ZD_Version", "%d" % (1 if rng.random() < 0.25 else 2)), ("ZD_k_cutoff", "%r" % float(rng.choice([1.0, 1.0, 2.0, 4.0] if n > 8 else [1.0, 2.0]))),
          ("ZD_CornerModes", "%d" % (rng.random() < 0.3)), ("ZD_qPk_fix_to_mean", "%d" % (rng.random() < 0.3)),
          ("ZD_f_cluster", "%r" % float(rng.choice([1.0, 1.0, 0.9, 0.5]))), ("ZD_qdensity", "%d" % (rng.random() < 0.3))]
    kv.append(("ZD_Pk_sigma", "0.0210839935761") if rng.random() < 0.7 else ("ZD_Pk_sigma_ratio", "1.25"))
    kv.append(("ZD_Pk_filename", '"@PK@"') if rng.random() < 0.7 else ("ZD_Pk_powerlaw_index", "%r" % float(rng.choice([-1.0, -2.5, 0.0]))))
    if plt:
        kv += [("ZD_qPLT", "1"), ("ZD_PLT_filename", '"@EIG@"'), ("ZD_qPLT_rescale", "%d" % (rng.random() < 0.5)), ("ZD_PLT_target_z", "5.0")]
    if rng.random() < 0.15:
        kv += [("ZD_qonemode", "1"), ("ZD_one_mode", "%d %d %d" % tuple(rng.integers(-n // 2 + 1, n // 2, size=3)))]
    if rng.random() < 0.15:
        kv.append(("ZD_qoneslab", "%d" % rng.integers(0, n)))
    return "".join("%s = %s\n" % t for t in kv)


@needs_reference
@pytest.mark.parametrize("seed", range(30))
def test_live_sweep_oracle_against_a_fresh_reference_run(oracle, api, tmp_path, seed):
    """seeded random option mixes at PPD 8, 16, 32: every record of a fresh reference run against the oracle"""
    par = _random_par(np.random.default_rng(1000 + seed))
    msg = "seed %d:\n%s" % (seed, par)
    want_planes, want_dens, want_files, stderr = _reference_run(oracle, par, str(tmp_path))
    planes, dens, files, max_disp, rms, _ = oracle_run(oracle, api, par, str(tmp_path))
    assert files == want_files, msg
    tol = tol_of(par)
    assert sorted(planes) == sorted(want_planes), msg
    if planes:
        dmax = max(float(np.abs(p["d"]).max()) for p in want_planes.values())
        vmax = max([float(np.abs(p["v"]).max()) for p in want_planes.values() if "v" in p.dtype.names], default=0.0)
        for z, want in want_planes.items():
            got = planes[z]
            if "ijk" in want.dtype.names:
                assert np.array_equal(got["ijk"], want["ijk"]), msg
            assert np.abs(got["d"].astype(np.float64) - want["d"]).max() <= tol * dmax, msg
            if "v" in want.dtype.names:
                assert np.abs(got["v"].astype(np.float64) - want["v"]).max() <= tol * vmax, msg
    if want_dens is not None:
        densmax = max(float(np.abs(d).max()) for d in want_dens.values())
        for z, want in want_dens.items():
            assert np.abs(dens[z].astype(np.float64) - want).max() <= TOL32 * densmax, msg
    md, want_rms = rr.printed_figures(stderr)
    assert abs(rms - want_rms) <= 0.5001e-6, msg
