"""Shared by tests/golden/make_reference_runs.py (which writes tests/golden/reference_runs/) and the tests that read those
fixtures (test_reference_runs.py, test_gpu_reference_runs.py): the configurations, the parameter texts, the signed-sum
weights and the readers of what a run leaves in its output directory.

A fixture is one .npz written from a run of the complete reference program (oracle/_ref/zeldovich_ref: the reference's sources
compiled where they lie against this project's stand-ins for GSL, FFTW3 and ParseHeader, oracle/ref_shim/).  It holds

  par          the parameter text as the reference read it; @OUT@, @PK@ and @EIG@ stand for the output directory, the P(k) file
               and the eigenmode file
  kept_z       the planes kept whole;  plane_<z>: their records exactly as read from ic_*;  dens_<z>: their density planes
  sums         float64 [n][ncomp][4]: four signed sums per plane and component (d0 d1 d2, then v0 v1 v2 where the format has them)
  dens_sums    float64 [n][4] where a density file was written
  files        names and sizes of every file the run left in its output directory
  max_disp, rms_density    the figures the reference printed (6 significant digits / 6 decimals)
  eig_sha256   of the eigenmode file (PLT runs): oracle.synthetic_eigenmodes(16) in the layout the reference reads
"""
import hashlib
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXDIR = os.path.join(HERE, "golden", "reference_runs")
REF_EXE = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "zeldovich_ref")
EIG_PPD = 16
NPATTERN = 4
MAX_FIXTURE_BYTES = 256 * 1024

# the keys of the reference's example.par, at NP = 32^3, ZD_NumBlock = 2, RVdoubleZel, ZD_qPLT = 0
BASE = [("BoxSize", "720"), ("CPD", "375"), ("ICFormat", '"RVdoubleZel"'), ("InitialConditionsDirectory", '"@OUT@"'),
        ("InitialRedshift", "49"), ("NP", "32768"), ("ZD_NumBlock", "2"), ("ZD_PLT_filename", '"@EIG@"'),
        ("ZD_PLT_target_z", "5"), ("ZD_Pk_filename", '"@PK@"'), ("ZD_Pk_norm", "8.0"), ("ZD_Pk_scale", "1.0"),
        ("ZD_Pk_sigma", "0.0210839935761"), ("ZD_Pk_smooth", "0.0"), ("ZD_Seed", "12346"), ("ZD_k_cutoff", "1.0"),
        ("ZD_qPLT", "0"), ("ZD_qPLT_rescale", "0"), ("ZD_qPk_fix_to_mean", "0"), ("ZD_Version", "2"), ("ZD_f_NL", "0")]

# name -> what differs from BASE (None removes a key).  One setting away from the base each, so that a failure names its row
# of DESIGN.md section 6; the *_64 ones repeat a setting at PPD = 64 for the store sweep of test_gpu_reference_runs.py.
CONFIGS = {
    "base": {},
    "fmt_rvzel": {"ICFormat": '"RVZel"'},
    "fmt_zeldovich": {"ICFormat": '"Zeldovich"'},
    "fmt_zelsimple": {"ICFormat": '"ZelSimple"'},
    "k_cutoff2": {"ZD_k_cutoff": "2"},
    "corner_modes": {"ZD_CornerModes": "1"},
    "fix_to_mean": {"ZD_qPk_fix_to_mean": "1"},
    "powerlaw": {"ZD_Pk_filename": None, "ZD_Pk_powerlaw_index": "-1"},
    "pk_smooth": {"ZD_Pk_smooth": "30.0"},
    "f_cluster": {"ZD_f_cluster": "0.9"},
    "sigma_ratio": {"ZD_Pk_sigma": None, "ZD_Pk_sigma_ratio": "0.75"},
    "one_mode": {"ZD_qonemode": "1", "ZD_one_mode": "1 2 3"},
    "one_mode_ky0": {"ZD_qonemode": "1", "ZD_one_mode": "3 0 2"},
    "qdensity1": {"ZD_qdensity": "1"},
    "qdensity2": {"ZD_qdensity": "2"},
    "oneslab5": {"ZD_qoneslab": "5"},
    "plt": {"ZD_qPLT": "1"},
    "plt_rescale": {"ZD_qPLT": "1", "ZD_qPLT_rescale": "1"},
    "plt_f_cluster": {"ZD_qPLT": "1", "ZD_f_cluster": "0.9"},     # f_cluster inside the PLT growth rate, not in the epilogue
    "v1_nb2": {"ZD_Version": "1"},
    "v1_nb4_kc2": {"ZD_Version": "1", "ZD_NumBlock": "4", "ZD_k_cutoff": "2"},
    "fnl_64": {"NP": "262144", "ZD_f_NL": "100", "ZD_n_s": "0.96", "Omega_M": "0.31"},
    "ppd64_nb4_cpd5": {"NP": "262144", "ZD_NumBlock": "4", "CPD": "5"},
    "k_cutoff2_64": {"NP": "262144", "ZD_k_cutoff": "2"},           # PPD = 64: the smallest size at which every store exists
    "plt_rescale_64": {"NP": "262144", "ZD_qPLT": "1", "ZD_qPLT_rescale": "1"},
    "ppd48_cpd7": {"NP": "110592", "CPD": "7"},
    "ppd50": {"NP": "125000"},
}
ROT_CONFIGS = ("base", "plt_rescale")   # rerun against the reference binary wherever it exists


def par_text(name):
    over = dict(CONFIGS[name])
    lines = []
    for k, v in BASE:
        v = over.pop(k, v)
        if v is not None:
            lines.append("%s = %s\n" % (k, v))
    lines += ["%s = %s\n" % kv for kv in over.items()]
    return "# %s\n" % name + "".join(lines)


def fill(par, out, pk, eig):
    return par.replace("@OUT@", str(out)).replace("@PK@", str(pk)).replace("@EIG@", str(eig))


def par_value(par, key, default=None):
    m = re.search(r"^%s\s*=\s*(.*?)\s*(#.*)?$" % re.escape(key), par, re.M)
    return m.group(1).strip('"') if m else default


def par_ppd(par):
    return int(round(int(par_value(par, "NP")) ** (1.0 / 3.0)))


# ---- signed sums -----------------------------------------------------------------------------------------------------------

_GOLDEN = np.uint64(0x9E3779B97F4A7C15)


def splitmix64(x):
    """the output function of splitmix64 (Steele, Lea, Flood 2014) on uint64 states, vectorised"""
    with np.errstate(over="ignore"):
        z = np.asarray(x, dtype=np.uint64) + _GOLDEN
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def weights(z, comp, pattern, count):
    """+-1 float64 [count]: the bits (least significant first) of the splitmix64 stream whose state starts at
    splitmix64(z << 16 | comp << 8 | pattern)"""
    nwords = (count + 63) // 64
    with np.errstate(over="ignore"):
        seed = splitmix64(np.uint64((int(z) << 16) | (int(comp) << 8) | int(pattern)))
        words = splitmix64(seed + np.arange(nwords, dtype=np.uint64) * _GOLDEN)
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:count]
    return 1.0 - 2.0 * bits.astype(np.float64)


def components(plane):
    """float64 [ncomp][n*n] of one plane of records: d0 d1 d2 (v0 v1 v2)"""
    cols = [plane["d"][..., c] for c in range(3)]
    if "v" in plane.dtype.names:
        cols += [plane["v"][..., c] for c in range(3)]
    return np.array([np.asarray(c, dtype=np.float64).ravel() for c in cols])


def signed_sums(z, plane):
    comps = components(plane)
    return np.array([[np.dot(weights(z, c, p, comps.shape[1]), comps[c]) for p in range(NPATTERN)] for c in range(comps.shape[0])])


def density_signed_sums(z, dens):
    d = np.asarray(dens, dtype=np.float64).ravel()
    return np.array([np.dot(weights(z, 255, p, d.size), d) for p in range(NPATTERN)])


# ---- what a run leaves behind ----------------------------------------------------------------------------------------------

def write_eigenmodes(path, zdo):
    """oracle.synthetic_eigenmodes(16) in the file layout of the reference (int32 ppd, then ppd^2 (ppd/2 + 1) 4 doubles); returns
    (table, sha-256 of the file)"""
    eig = np.ascontiguousarray(zdo.synthetic_eigenmodes(EIG_PPD), dtype=np.float64)
    blob = np.int32(EIG_PPD).tobytes() + eig.tobytes()
    with open(path, "wb") as f:
        f.write(blob)
    return eig, hashlib.sha256(blob).hexdigest()


def list_files(out):
    """sorted (name, size) of the regular files in an output directory"""
    return sorted((f, os.path.getsize(os.path.join(out, f))) for f in os.listdir(out) if os.path.isfile(os.path.join(out, f)))


def read_planes(out, par, dtype):
    """{z: records [n][n]} for every plane found in the ic_* files of `out` (planes lie in a file in increasing z)"""
    n, cpd = par_ppd(par), int(par_value(par, "CPD"))
    oneslab = int(par_value(par, "ZD_qoneslab", "-1"))
    zs = [z for z in range(n) if oneslab < 0 or z == oneslab]
    planes = {}
    for f in sorted(set(z * cpd // n for z in zs)):
        mine = [z for z in zs if z * cpd // n == f]
        rec = np.fromfile(os.path.join(out, "ic_%d" % f), dtype=dtype)
        assert rec.size == len(mine) * n * n, "ic_%d holds %d records, expected %d planes" % (f, rec.size, len(mine))
        for i, z in enumerate(mine):
            planes[z] = rec[i * n * n:(i + 1) * n * n].reshape(n, n)
    return planes


def read_density(out, par):
    """{z: float32 [n][n]} from the density file (planes appended in the order they were written), or None"""
    if int(par_value(par, "ZD_qdensity", "0")) == 0:
        return None
    n = par_ppd(par)
    oneslab = int(par_value(par, "ZD_qoneslab", "-1"))
    zs = [z for z in range(n) if oneslab < 0 or z == oneslab]
    d = np.fromfile(os.path.join(out, "density%d" % n), dtype=np.float32)
    assert d.size == len(zs) * n * n
    return {z: d[i * n * n:(i + 1) * n * n].reshape(n, n) for i, z in enumerate(zs)}


def printed_figures(stderr):
    """(max_disp [3] or None, rms density or None) as the program printed them"""
    m = re.search(r"maximum component-wise displacements are \(([^)]*)\)", stderr)
    md = np.array([float(t) for t in m.group(1).split(",")]) if m else None
    m = re.search(r"rms density variation of the pixels is ([-+0-9.eEna]+)", stderr)
    return md, (float(m.group(1)) if m else None)


def fixture_names():
    return list(CONFIGS)


def load_fixture(name):
    with np.load(os.path.join(FIXDIR, name + ".npz"), allow_pickle=False) as z:
        fx = {k: z[k] for k in z.files}
    fx["par"] = str(fx["par"])
    fx["files"] = [(str(a), int(b)) for a, b in zip(fx["file_names"], fx["file_sizes"])]
    fx["eig_sha256"] = str(fx["eig_sha256"])
    return fx


# ---- comparing a run with a fixture ----------------------------------------------------------------------------------------

def field_max(fx):
    """max |d| and max |v| over the fixture's kept planes (the scale the bounds are stated against)"""
    kept = [fx["plane_%d" % z] for z in fx["kept_z"] if "plane_%d" % z in fx]
    dmax = max([float(np.abs(p["d"]).max()) for p in kept], default=0.0)
    vmax = max([float(np.abs(p["v"]).max()) for p in kept if "v" in p.dtype.names], default=0.0)
    return dmax, vmax


def compare(fx, planes, density, tol, tol_dens=1e-6):
    """worst ratios of a run ({z: records}, {z: density plane} or None) against a fixture, each divided by its bound so that <= 1
    passes: kept planes record by record (indices exactly), signed sums on every plane with |delta| <= tol n^2 max|field|.
    Returns dict(planes=, sums=, dens=) and asserts nothing but the indices and the plane set."""
    par = fx["par"]
    n = par_ppd(par)
    dmax, vmax = field_max(fx)
    worst = dict(planes=0.0, sums=0.0, dens=0.0)
    has_records = fx["sums"].size > 0      # ZD_qdensity = 2 writes the density alone
    if has_records:
        assert sorted(planes) == [int(z) for z in fx["sum_z"]], "planes delivered: %s" % sorted(planes)
    for z in fx["kept_z"] if has_records else []:
        want, got = fx["plane_%d" % z], planes[int(z)]
        assert got.dtype == want.dtype
        if "ijk" in want.dtype.names:
            assert np.array_equal(got["ijk"], want["ijk"]), "indices of plane %d" % z
        worst["planes"] = max(worst["planes"], float(np.abs(got["d"].astype(np.float64) - want["d"]).max()) / (tol * dmax))
        if "v" in want.dtype.names:
            worst["planes"] = max(worst["planes"], float(np.abs(got["v"].astype(np.float64) - want["v"]).max()) / (tol * vmax))
    for i, z in enumerate(fx["sum_z"] if has_records else []):
        s = signed_sums(int(z), planes[int(z)])
        scale = np.array([dmax] * 3 + [vmax] * 3)[:s.shape[0], None]
        worst["sums"] = max(worst["sums"], float((np.abs(s - fx["sums"][i]) / (tol * n * n * scale)).max()))
    if "dens_sums" in fx:
        densmax = max(float(np.abs(fx["dens_%d" % z]).max()) for z in fx["kept_z"])
        for z in fx["kept_z"]:
            worst["dens"] = max(worst["dens"], float(np.abs(density[int(z)].astype(np.float64) - fx["dens_%d" % z]).max()) / (tol_dens * densmax))
        for i, z in enumerate(fx["sum_z"]):
            s = density_signed_sums(int(z), density[int(z)])
            worst["dens"] = max(worst["dens"], float(np.abs(s - fx["dens_sums"][i]).max() / (tol_dens * n * n * densmax)))
    return worst
