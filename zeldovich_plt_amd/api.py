"""ctypes binding of include/zeldovich_hip.h — the host-side mirror of the reference's call sites
(Parameters / PowerSpectrum / ZeldovichZ + ZeldovichXY, src/zeldovich.cpp:848-1032).

This module is plumbing only: every number is produced by libzeldovich_hip.so (HIP, gfx950).  There is
no CPU fallback — if the library is missing, or no GPU is present when a compute entry point is
called, it fails loudly.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# ZD_LIB_PATH: A/B-testing another build of the same library (tuning only)
LIB_PATH = os.environ.get("ZD_LIB_PATH") or os.path.join(_HERE, "csrc", "build", "libzeldovich_hip.so")

ICFORMATS = {"Zeldovich": 0, "RVZel": 1, "RVdoubleZel": 2, "ZelSimple": 3}
RECORD_DTYPES = {
    "Zeldovich": np.dtype([("ijk", "<u2", 3), ("pad", "<u2"), ("d", "<f8", 3)]),
    "RVZel": np.dtype([("ijk", "<u2", 3), ("pad", "<u2"), ("d", "<f4", 3), ("v", "<f4", 3)]),
    "RVdoubleZel": np.dtype([("ijk", "<u2", 3), ("pad", "<u2"), ("d", "<f8", 3), ("v", "<f8", 3)]),
    "ZelSimple": np.dtype([("d", "<f4", 3)]),
}
KERNEL_NAMES = ("k_gen", "k_zfft", "k_yfft", "k_xfft", "z_stage", "exchange_wait")


class ZdParams(C.Structure):
    _fields_ = [
        ("ppd", C.c_int64), ("numblock", C.c_int32), ("cpd", C.c_int32), ("boxsize", C.c_double),
        ("fundamental", C.c_double), ("nyquist", C.c_double), ("k_cutoff", C.c_double),
        ("f_cluster", C.c_double), ("z_initial", C.c_double), ("PLT_target_z", C.c_double),
        ("seed", C.c_int64), ("corner_modes", C.c_int32), ("qdensity", C.c_int32),
        ("qoneslab", C.c_int32), ("qonemode", C.c_int32), ("one_mode", C.c_int32 * 3),
        ("qPLT", C.c_int32), ("qPLTrescale", C.c_int32), ("icformat", C.c_int32),
        ("stream_factor", C.c_int32), ("profile", C.c_int32),
        ("store_mode", C.c_int32), ("serial_z", C.c_int32), ("ngpu", C.c_int32), ("exchange_planes", C.c_int32),
        ("f_NL", C.c_double), ("n_s", C.c_double), ("Omega_M", C.c_double),
        ("version", C.c_int32), ("pass_groups", C.c_int32),
        ("q2LPT", C.c_int32), ("lpt2_dealias", C.c_int32), ("lpt2_ratio", C.c_double),
        ("q3LPT", C.c_int32), ("lpt3_terms", C.c_int32), ("lpt3_g3a", C.c_double), ("lpt3_g3b", C.c_double),
        ("lpt3_g3c", C.c_double), ("lpt3_f3", C.c_double),
        ("lpt2_f2", C.c_double),  # (stays the last member)
    ]


class ZdPk(C.Structure):
    _fields_ = [
        ("n", C.c_int32), ("x", C.POINTER(C.c_double)), ("y", C.POINTER(C.c_double)),
        ("y2", C.POINTER(C.c_double)), ("normalization", C.c_double), ("Pk_smooth2", C.c_double),
        ("fixed_power", C.c_int32), ("is_powerlaw", C.c_int32), ("powerlaw_index", C.c_double),
        ("kmax", C.c_double), ("kmin", C.c_double),
    ]


class ZdStats(C.Structure):
    _fields_ = [
        ("max_disp", C.c_double * 3), ("density_variance", C.c_double), ("seconds_total", C.c_double),
        ("kernel_ms", C.c_double * 6), ("kernel_launches", C.c_int64 * 6),
        ("bytes_intermediate", C.c_int64), ("stream_factor", C.c_int32), ("modes_cached", C.c_int32),
        ("bytes_sent", C.c_int64), ("max_disp_index", C.c_int64 * 3),
    ]


class ZdParamStrings(C.Structure):
    _fields_ = [
        ("Pk_filename", C.c_char * 1024), ("output_dir", C.c_char * 1024),
        ("density_filename", C.c_char * 1024), ("PLT_filename", C.c_char * 1024),
        ("ICFormat", C.c_char * 64),
        ("Pk_scale", C.c_double), ("Pk_norm", C.c_double), ("Pk_sigma", C.c_double),
        ("Pk_sigma_ratio", C.c_double), ("Pk_smooth", C.c_double), ("Pk_powerlaw_index", C.c_double),
        ("qPk_fix_to_mean", C.c_int32), ("version", C.c_int32),
        ("f_NL", C.c_double), ("n_s", C.c_double), ("Omega_M", C.c_double), ("np", C.c_int64),
        ("Pk_measured_filename", C.c_char * 1024),
        ("SelfCheck_tol", C.c_double), ("SelfCheck", C.c_int32), ("SelfCheck_filename", C.c_char * 1024),
        ("PLT_compute_ppd", C.c_int32),
    ]


SLAB_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p)
GROUP_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p)
PASS_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p)
PARTICLE_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p)

# every symbol include/zeldovich_hip.h declares (checked by tests/test_capi_symbols.py)
EXPORTED_SYMBOLS = [
    "zd_generate", "zd_choose_stream_factor", "zd_plan_create", "zd_plan_destroy", "zd_plan_narray", "zd_plan_store_mode",
    "zd_plan_stream_factor", "zd_plan_passes", "zd_plan_plane_step", "zd_plan_record_size", "zd_plan_exchange_bytes", "zd_plan_local_planes",
    "zd_plan_plane_z", "zd_plan_stage_z", "zd_plan_stage_y", "zd_plan_stage_x", "zd_plan_stats", "zd_comm_unique_id", "zd_comm_create", "zd_comm_destroy", "zd_plan_ring_bytes", "zd_plan_run_pass",
    "zd_params_from_file", "zd_pk_create_from_file", "zd_pk_create_powerlaw", "zd_pk_power",
    "zd_pk_sigmaR", "zd_pk_destroy", "zd_load_eigmodes", "zd_free", "zd_comm_abort", "zd_comm_traffic", "zd_choose_pass_groups", "zd_plan_run_passes", "zd_comm_probe", "zd_choose_pass_groups_measured",
    "zd_dispatch_report", "zd_power_nbins", "zd_plan_measure_power", "zd_measure_power",
    "zd_plan_direct_sum", "zd_direct_sum", "zd_make_eigenmodes", "zd_write_eigmodes", "zd_param_file_string",
    "zd_plan_lpt_direct_sum", "zd_lpt_direct_sum", "zd_plan_lpt_power", "zd_lpt_power",
    "zd_interp_create", "zd_interp_add_plane", "zd_interp_result", "zd_interp_destroy", "zd_plan_interp", "zd_displace",
    "zd_plan_create_field", "zd_generate_field", "zd_field_vjp", "zd_plan_create_field_lpt", "zd_generate_field_lpt",
]
# test scaffolding: exists only in the -DZD_TESTING library (csrc/zd_testing.h, `make testing`), never in the product
TESTING_SYMBOLS = ["zd_test_draws", "zd_test_modes", "zd_test_modes_table", "zd_test_v1_words", "zd_test_generate_loopback", "zd_test_fail_rank",
                   "zd_test_fft", "zd_test_ycols", "zd_test_poison", "zd_test_route", "zd_test_route_kernels", "zd_test_lpt2_coefficients", "zd_test_live_handles", "zd_test_plt_matrix",
                   "zd_test_ring_pair_w"]
STORE_MODES = {"auto": 0, "reference": 1, "packed": 2, "fields": 3}  # zd_params.store_mode (ZD_STORE_*)

_lib = None
_testing_lib = None
TESTING_LIB_PATH = os.environ.get("ZD_TESTING_LIB_PATH") or os.path.join(_HERE, "csrc", "build", "libzeldovich_hip_testing.so")


def load_library():
    """Load libzeldovich_hip.so; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        _lib = _load(LIB_PATH, testing=False)
    return _lib


def load_testing_library():
    """The -DZD_TESTING build of the same sources: the product plus the device test hooks (zd_test_*) and the in-process
    emulation of the RCCL calls.  Only tests/ use it."""
    global _testing_lib
    if _testing_lib is None:
        _testing_lib = _load(TESTING_LIB_PATH, testing=True)
    return _testing_lib


def _load(path, testing):
    if not os.path.exists(path):
        raise RuntimeError(
            "zeldovich_plt_amd: %s is missing — run `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C zeldovich_plt_amd/csrc%s`; there is no CPU fallback." % (path, " testing" if testing else ""))
    try:
        # torch bundles its own HIP runtime; it must be the first one initialised in the process,
        # otherwise torch later reports "No HIP GPUs are available" (measured on the MI355X box)
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(path)
    vp, i32, i64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    L.zd_generate.argtypes = [C.POINTER(ZdParams), C.POINTER(ZdPk), vp, i64, SLAB_CB, vp, C.POINTER(ZdStats)]
    if testing:
        L.zd_test_generate_loopback.argtypes = L.zd_generate.argtypes
        L.zd_test_draws.argtypes = [i64, i64, vp, vp]
        L.zd_test_modes.argtypes = [C.POINTER(ZdParams), C.POINTER(ZdPk), i64, vp, vp]
        L.zd_test_modes_table.argtypes = [C.POINTER(ZdParams), C.POINTER(ZdPk), i64, vp, vp]
        L.zd_test_v1_words.argtypes = [i64, C.c_int32, vp]
        L.zd_test_fft.argtypes = [i32, i64, i32, vp, vp]
        L.zd_test_ycols.argtypes = [i32, i32, i32, i32, i32, vp, vp]
        L.zd_test_poison.argtypes = [C.c_int]
        L.zd_test_poison.restype = None
        L.zd_test_ring_pair_w.argtypes = [C.c_int]
        L.zd_test_ring_pair_w.restype = None
        L.zd_test_lpt2_coefficients.argtypes = [C.POINTER(ZdParams), vp]
        L.zd_test_lpt2_coefficients.restype = None
        L.zd_test_live_handles.argtypes = []
        L.zd_test_live_handles.restype = i64
        L.zd_test_plt_matrix.argtypes = [i64, dbl, i32, i64, vp, vp]
        L.zd_test_route_kernels.argtypes = [C.POINTER(ZdParams), i32, i32, i32, C.c_char_p, i64]
    L.zd_choose_stream_factor.argtypes = [C.POINTER(ZdParams), C.c_int, i64]
    L.zd_choose_pass_groups.argtypes = [C.POINTER(ZdParams), C.c_int, i64, C.POINTER(i32), C.POINTER(i32)]
    L.zd_plan_create.argtypes = [C.POINTER(ZdParams), C.POINTER(ZdPk), vp, i64, C.c_int, C.c_int, C.POINTER(vp)]
    L.zd_plan_destroy.argtypes = [vp]
    L.zd_plan_destroy.restype = None
    for name in ("zd_plan_narray", "zd_plan_store_mode", "zd_plan_stream_factor", "zd_plan_record_size", "zd_plan_passes", "zd_plan_plane_step"):
        getattr(L, name).argtypes = [vp]
        getattr(L, name).restype = i32
    for name in ("zd_plan_exchange_bytes", "zd_plan_local_planes"):
        getattr(L, name).argtypes = [vp]
        getattr(L, name).restype = i64
    L.zd_plan_plane_z.argtypes = [vp, C.c_int, i64]
    L.zd_plan_plane_z.restype = i64
    L.zd_plan_stage_z.argtypes = [vp, C.c_int, vp, vp]
    L.zd_plan_stage_y.argtypes = [vp, vp, vp]
    L.zd_plan_stage_x.argtypes = [vp, C.c_int, vp, i64, i64, vp, vp, vp]
    L.zd_plan_stats.argtypes = [vp, C.POINTER(ZdStats)]
    L.zd_comm_unique_id.argtypes = [vp]
    L.zd_comm_create.argtypes = [C.c_int, C.c_int, vp, C.POINTER(vp)]
    L.zd_comm_destroy.argtypes = [vp]
    L.zd_comm_destroy.restype = None
    L.zd_comm_abort.argtypes = [vp]
    L.zd_comm_abort.restype = None
    L.zd_comm_probe.argtypes = [vp, i64, i32, C.POINTER(C.c_double)]
    L.zd_choose_pass_groups_measured.argtypes = [C.POINTER(ZdParams), C.c_int, i64, C.c_double, C.POINTER(i32), C.POINTER(i32), C.POINTER(C.c_double)]
    L.zd_comm_traffic.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.c_int]
    L.zd_comm_traffic.restype = None
    L.zd_plan_ring_bytes.argtypes = [vp, C.POINTER(i32)]
    L.zd_plan_ring_bytes.restype = i64
    L.zd_plan_run_pass.argtypes = [vp, vp, C.c_int, vp, vp, i64, GROUP_CB, vp, vp]
    L.zd_plan_run_passes.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp, i64, PASS_CB, vp, vp]
    L.zd_params_from_file.argtypes = [C.c_char_p, C.POINTER(ZdParams), C.POINTER(ZdParamStrings)]
    L.zd_param_file_string.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, i64]
    L.zd_pk_create_from_file.argtypes = [C.c_char_p, dbl, dbl, dbl, dbl, dbl, C.c_int, dbl, C.POINTER(vp), C.POINTER(ZdPk)]
    L.zd_pk_create_powerlaw.argtypes = [dbl, dbl, dbl, dbl, dbl, C.c_int, dbl, C.POINTER(vp), C.POINTER(ZdPk)]
    L.zd_pk_power.argtypes = [C.POINTER(ZdPk), dbl]
    L.zd_pk_power.restype = dbl
    L.zd_pk_sigmaR.argtypes = [C.POINTER(ZdPk), dbl]
    L.zd_pk_sigmaR.restype = dbl
    L.zd_pk_destroy.argtypes = [vp]
    L.zd_pk_destroy.restype = None
    L.zd_load_eigmodes.argtypes = [C.c_char_p, C.POINTER(vp), C.POINTER(i64)]
    L.zd_free.argtypes = [vp]
    L.zd_free.restype = None
    L.zd_write_eigmodes.argtypes = [C.c_char_p, vp, i64]
    L.zd_make_eigenmodes.argtypes = [i64, vp]
    L.zd_power_nbins.argtypes = [i64, i32]
    L.zd_power_nbins.restype = i64
    L.zd_plan_measure_power.argtypes = [vp, i32, i64, vp, vp, vp, vp, vp, vp, vp]
    L.zd_measure_power.argtypes = [C.POINTER(ZdParams), C.POINTER(ZdPk), vp, i64, i32, i64, vp, vp, vp, vp, vp, vp]
    L.zd_plan_direct_sum.argtypes = [vp, i64, vp, vp, vp]
    L.zd_direct_sum.argtypes = [C.POINTER(ZdParams), C.POINTER(ZdPk), vp, i64, i64, vp, vp]
    L.zd_plan_lpt_direct_sum.argtypes = [vp, i64, vp, vp, vp]
    L.zd_lpt_direct_sum.argtypes = [C.POINTER(ZdParams), C.POINTER(ZdPk), i64, vp, vp]
    L.zd_plan_lpt_power.argtypes = [vp, i32, i64, vp, vp, vp]
    L.zd_lpt_power.argtypes = [C.POINTER(ZdParams), C.POINTER(ZdPk), i32, i64, vp, vp]
    L.zd_interp_create.argtypes = [i64, i32, i32, i64, vp, C.POINTER(vp)]
    L.zd_interp_add_plane.argtypes = [vp, i64, vp, vp]
    L.zd_interp_result.argtypes = [vp, vp]
    L.zd_interp_destroy.argtypes = [vp]
    L.zd_interp_destroy.restype = None
    L.zd_plan_interp.argtypes = [vp, vp, vp]
    L.zd_displace.argtypes = [C.POINTER(ZdParams), C.POINTER(ZdPk), vp, i64, i32, i64, vp, i64, i64, PARTICLE_CB, vp, C.POINTER(ZdStats)]
    L.zd_plan_create_field.argtypes = [C.POINTER(ZdParams), C.POINTER(ZdPk), vp, i64, i32, i32, vp, i32, C.POINTER(vp)]
    L.zd_generate_field.argtypes = [C.POINTER(ZdParams), C.POINTER(ZdPk), vp, i64, i32, i32, vp, i32, SLAB_CB, vp, C.POINTER(ZdStats)]
    L.zd_plan_create_field_lpt.argtypes = [C.POINTER(ZdParams), C.POINTER(ZdPk), i32, i32, vp, i32, i32, C.POINTER(vp)]
    L.zd_generate_field_lpt.argtypes = [C.POINTER(ZdParams), C.POINTER(ZdPk), i32, i32, vp, i32, i32, SLAB_CB, vp, C.POINTER(ZdStats)]
    L.zd_field_vjp.argtypes = [C.POINTER(ZdParams), C.POINTER(ZdPk), vp, i64, i32, i32, vp, vp, vp, i32, vp, i32, C.POINTER(ZdStats)]
    L.zd_dispatch_report.argtypes = [C.c_char_p, i64]
    L.zd_dispatch_report.restype = i64
    return L


def dispatch_report(testing=False):
    """{(launcher with its template arguments, source line): launches so far} of the product library (testing=True: of the
    -DZD_TESTING library, which counts its own launches) — zd_dispatch_report"""
    L = load_testing_library() if testing else load_library()
    n = L.zd_dispatch_report(None, 0)
    buf = C.create_string_buffer(int(n) + 4096)
    L.zd_dispatch_report(buf, len(buf))
    out = {}
    for line in buf.value.decode().splitlines():
        cnt, ln, name = line.split("\t", 2)
        out[(name, int(ln))] = out.get((name, int(ln)), 0) + int(cnt)
    return out


def make_params(ppd, numblock=2, boxsize=720.0, seed=12346, k_cutoff=1.0, qPLT=0, qPLTrescale=0,
                PLT_target_z=0.0, z_initial=49.0, f_cluster=1.0, icformat="RVdoubleZel", qdensity=0,
                qoneslab=-1, qonemode=0, one_mode=(0, 0, 0), corner_modes=0, cpd=None, stream_factor=0,
                profile=0, f_NL=0.0, n_s=1.0, Omega_M=1.0, store_mode="auto", serial_z=0, ngpu=0, exchange_planes=0,
                version=2, pass_groups=0, q2LPT=0, lpt2_ratio=0.0, lpt2_f2=0.0, lpt2_dealias=0,
                q3LPT=0, lpt3_g3a=0.0, lpt3_g3b=0.0, lpt3_g3c=0.0, lpt3_f3=0.0, lpt3_terms=0):
    """Parameters with the derived quantities of Parameters::setup (src/parameters.cpp:172-174); version = 1 (legacy
    mt19937 streams) adjusts NumBlock by k_cutoff as the reader does (src/parameters.cpp:129-141).  q2LPT = 1 adds the
    second-order displacements (csrc/zd_kernels_lpt2.hip); lpt2_ratio = D2 / D1^2 and lpt2_f2: 0 = the f_cluster background's;
    lpt2_dealias = 1 forms its source on the 3 PPD / 2 lattice (Orszag's 3/2 rule, csrc/zd_kernels_lpt2q.hip).  q3LPT = 1 (with q2LPT = 1) adds
    the third-order displacements (csrc/zd_kernels_lpt3.hip); lpt3_g3a, lpt3_g3b, lpt3_g3c and lpt3_f3: 0 = the defaults of f_cluster = 1
    (-1/3, 10/21, 1/7, 3); lpt3_terms leaves terms out (bit 1 = 3a, 2 = 3b, 4 = 3c; 0 = all)."""
    p = ZdParams()
    p.ppd = ppd
    if version == 1 and k_cutoff != 1.0:
        numblock = int(numblock * k_cutoff + .5)
    p.version = version
    p.numblock = numblock
    p.cpd = cpd if cpd is not None else ppd
    p.boxsize = boxsize
    p.fundamental = 2.0 * np.pi / boxsize
    p.nyquist = np.pi / (boxsize / ppd)
    p.k_cutoff = k_cutoff
    p.f_cluster = f_cluster
    p.z_initial = z_initial
    p.PLT_target_z = PLT_target_z
    p.seed = int(seed)
    p.corner_modes = corner_modes
    p.qdensity = qdensity
    p.qoneslab = qoneslab
    p.qonemode = qonemode
    p.one_mode = (C.c_int32 * 3)(*one_mode)
    p.qPLT = qPLT
    p.qPLTrescale = qPLTrescale
    p.icformat = ICFORMATS[icformat]
    p.stream_factor = stream_factor
    p.profile = profile
    p.store_mode = STORE_MODES[store_mode] if isinstance(store_mode, str) else int(store_mode)
    p.serial_z = serial_z
    p.ngpu = ngpu
    p.exchange_planes = exchange_planes
    p.pass_groups = pass_groups
    p.f_NL, p.n_s, p.Omega_M = f_NL, n_s, Omega_M
    p.q2LPT, p.lpt2_ratio, p.lpt2_f2 = q2LPT, lpt2_ratio, lpt2_f2
    p.lpt2_dealias = lpt2_dealias
    p.q3LPT, p.lpt3_terms = q3LPT, lpt3_terms
    p.lpt3_g3a, p.lpt3_g3b, p.lpt3_g3c, p.lpt3_f3 = lpt3_g3a, lpt3_g3b, lpt3_g3c, lpt3_f3
    return p


def params_from_file(path):
    """Parameters(file): returns (ZdParams, ZdParamStrings); raises on invalid input."""
    L = load_library()
    p, s = ZdParams(), ZdParamStrings()
    if L.zd_params_from_file(os.fsencode(path), C.byref(p), C.byref(s)):
        raise ValueError("Invalid Parameters given: %s" % path)
    return p, s


def param_file_string(path, key):
    """the string a parameter file assigns to `key` (zd_param_file_string); "" if it does not"""
    buf = C.create_string_buffer(1024)
    if load_library().zd_param_file_string(os.fsencode(path), key.encode(), buf, len(buf)):
        raise ValueError("parameter file %s: %s could not be read" % (path, key))
    return os.fsdecode(buf.value)


class PowerSpectrum:
    """PowerSpectrum after InitFromFile / InitFromPowerLaw + Normalize (src/power_spectrum.cpp:130-223)."""

    def __init__(self, pk, handle):
        self.pk = pk
        self._h = handle

    @classmethod
    def from_file(cls, path, boxsize, Pk_scale=1.0, Pk_norm=8.0, Pk_sigma=0.0210839935761,
                  Pk_sigma_ratio=0.0, Pk_smooth=0.0, fix_to_mean=0):
        L = load_library()
        pk, h = ZdPk(), C.c_void_p()
        if L.zd_pk_create_from_file(os.fsencode(path), Pk_scale, Pk_norm, Pk_sigma, Pk_sigma_ratio, Pk_smooth,
                                    fix_to_mean, boxsize, C.byref(h), C.byref(pk)):
            raise RuntimeError("power spectrum file %r could not be loaded" % path)
        return cls(pk, h)

    @classmethod
    def from_powerlaw(cls, index, boxsize, Pk_norm=8.0, Pk_sigma=0.02, Pk_sigma_ratio=0.0, Pk_smooth=0.0,
                      fix_to_mean=0):
        L = load_library()
        pk, h = ZdPk(), C.c_void_p()
        if L.zd_pk_create_powerlaw(index, Pk_norm, Pk_sigma, Pk_sigma_ratio, Pk_smooth, fix_to_mean, boxsize,
                                   C.byref(h), C.byref(pk)):
            raise RuntimeError("power law spectrum could not be initialised")
        return cls(pk, h)

    def power(self, k):
        return load_library().zd_pk_power(C.byref(self.pk), float(k))

    def sigmaR(self, R):
        return load_library().zd_pk_sigmaR(C.byref(self.pk), float(R))

    def tables(self):
        n = self.pk.n
        return tuple(np.ctypeslib.as_array(a, (n,)).copy() for a in (self.pk.x, self.pk.y, self.pk.y2))

    def __del__(self):
        try:
            if self._h:
                load_library().zd_pk_destroy(self._h)
                self._h = None
        except Exception:
            pass


def _fmt_name(icformat):
    return [k for k, v in ICFORMATS.items() if v == icformat][0]


def _stats_dict(st):
    return dict(max_disp=np.array(list(st.max_disp)), density_variance=st.density_variance,
                seconds_total=st.seconds_total, kernel_ms=dict(zip(KERNEL_NAMES, list(st.kernel_ms))),
                kernel_launches=dict(zip(KERNEL_NAMES, list(st.kernel_launches))),
                bytes_intermediate=st.bytes_intermediate, stream_factor=st.stream_factor,
                modes_cached=bool(st.modes_cached), bytes_sent=st.bytes_sent,
                max_disp_index=np.array(list(st.max_disp_index)))


def generate(params, ps, eig=None, collect=True, loopback=False, testing=False):
    """ZeldovichZ + ZeldovichXY on cuda:0 through zd_generate.

    collect=True gathers every delivered plane (host callback, like WriteParticlesSlab) into
    records[z, y, x] (and density[z, y, x] when qdensity); collect=False uses the NULL sink.
    loopback=True (tests; params.ngpu >= 2): zd_test_generate_loopback — the RCCL branch of the exchange on an in-process
    emulation of its calls."""
    L = load_testing_library() if (loopback or testing) else load_library()  # testing: zd_generate of the -DZD_TESTING build (zd_test_poison)
    entry = L.zd_test_generate_loopback if loopback else L.zd_generate
    eigp, eig_ppd = (None, 0)
    if eig is not None:
        eig = np.ascontiguousarray(eig, dtype=np.float64)
        eigp, eig_ppd = eig.ctypes.data, eig.shape[0]
    return _collecting_run(params, collect, lambda cb, st: entry(C.byref(params), C.byref(ps.pk), eigp, eig_ppd, cb, None, C.byref(st)),
                           "zd_generate")


def _collecting_run(params, collect, call, what):
    """call(cb, stats) -> rc with zd_generate's callback: gathers the delivered planes (collect) or runs the NULL sink"""
    n = int(params.ppd)
    st = ZdStats()
    out = {}
    if collect:
        dt = RECORD_DTYPES[_fmt_name(params.icformat)]
        rec = np.zeros((n, n * n), dtype=dt) if params.qdensity != 2 else None
        dens = np.zeros((n, n * n), dtype=np.float32) if params.qdensity else None
        seen = []

        def _cb(user, z, nrec, recp, densp):
            seen.append(int(z))
            if recp and rec is not None:
                C.memmove(rec[z].ctypes.data, recp, nrec * dt.itemsize)
            if densp and dens is not None:
                C.memmove(dens[z].ctypes.data, densp, nrec * 4)
            return 0

        cb = SLAB_CB(_cb)
        rc = call(cb, st)
        out["records"] = None if rec is None else rec.reshape(n, n, n)
        out["density"] = None if dens is None else dens.reshape(n, n, n)
        out["planes_seen"] = seen
    else:
        rc = call(SLAB_CB(), st)
    if rc:
        raise RuntimeError("%s failed (rc=%d); see stderr" % (what, rc))
    out.update(_stats_dict(st))
    return out


FIELD_KINDS = {"density": 0, "white": 1}  # ZD_FIELD_DENSITY, ZD_FIELD_WHITE


def _field_arg(field, ppd, kind, order=1):
    """(kind code, dtype code, pointer, on_device) of a field handed to generate_field / Plan.from_field: a numpy array or a torch
    tensor on the GPU, float32 or float64, of shape (ppd, ppd, ppd), C-contiguous.  Anything else raises before the library is called.
    (order != 1 at a ppd no higher-order field run takes — not a power of two in [32, 1024]: the library refuses the job by its size
    before it looks at the field, so the shape is its business.)"""
    if kind not in FIELD_KINDS:
        raise ValueError("field kind must be one of %s (got %r)" % (sorted(FIELD_KINDS), kind))
    n = int(ppd)
    if order != 1 and not (32 <= n <= 1024 and n & (n - 1) == 0):
        n = int(field.shape[0]) if getattr(field, "ndim", 0) == 3 else n
    if isinstance(field, np.ndarray):
        if field.dtype not in (np.float32, np.float64):
            raise TypeError("field: float32 or float64 expected (got %s)" % field.dtype)
        if field.shape != (n, n, n):
            raise ValueError("field: shape (%d, %d, %d) expected (got %r)" % (n, n, n, field.shape))
        if not field.flags["C_CONTIGUOUS"]:
            raise ValueError("field: a C-contiguous array [z][y][x] expected")
        return FIELD_KINDS[kind], int(field.dtype == np.float64), field.ctypes.data, 0
    if type(field).__module__.split(".")[0] == "torch" and hasattr(field, "data_ptr"):
        import torch
        if not field.is_cuda:
            raise ValueError("field: a torch tensor must live on the GPU (pass a numpy array for host data)")
        if field.dtype not in (torch.float32, torch.float64):
            raise TypeError("field: float32 or float64 expected (got %s)" % field.dtype)
        if tuple(field.shape) != (n, n, n):
            raise ValueError("field: shape (%d, %d, %d) expected (got %r)" % (n, n, n, tuple(field.shape)))
        if not field.is_contiguous():
            raise ValueError("field: a C-contiguous tensor [z][y][x] expected")
        torch.cuda.synchronize(field.device)  # the library works on its own stream
        return FIELD_KINDS[kind], int(field.dtype == torch.float64), field.data_ptr(), 1
    raise TypeError("field: a numpy array or a torch tensor on the GPU expected (got %s)" % type(field).__name__)


def generate_field(params, ps, field, kind="density", eig=None, collect=True, order=1, on_plane=None):
    """generate() with the modes taken from a caller-supplied real field instead of ZD_Seed (zd_generate_field; definition in
    csrc/zd_kernels_field.hip).  field: numpy array or torch tensor on the GPU, float32 or float64, shape (ppd, ppd, ppd) = [z][y][x],
    C-contiguous.  kind: "density" (the linear density in the run's units) or "white" (unit-variance white noise, coloured by ps).
    order: 1 the Zel'dovich run; 2 second order (2LPT) on the field (zd_generate_field_lpt; definition in csrc/zd_kernels_lpt2_field.hip):
    the parameters come WITHOUT q2LPT, lpt2_ratio and lpt2_f2 of them apply, no eigenmode table.
    on_plane: a per-plane consumer as generate_planes takes it, on_plane(z, records[y, x]); nothing is accumulated then (through
    zd_generate_field_lpt at either order: no eigenmode table)."""
    kcode, dcode, ptr, on_device = _field_arg(field, params.ppd, kind, order)
    L = load_library()
    if order != 1 or on_plane is not None:
        if eig is not None:
            raise ValueError("generate_field: order = %r%s takes no eigenmode table" % (order, "" if on_plane is None else " with on_plane"))

        def call(cb, st):
            return L.zd_generate_field_lpt(C.byref(params), C.byref(ps.pk), kcode, dcode, ptr, on_device, int(order), cb, None, C.byref(st))

        if on_plane is None:
            return _collecting_run(params, collect, call, "zd_generate_field_lpt")
        n, dt, st, count = int(params.ppd), RECORD_DTYPES[_fmt_name(params.icformat)], ZdStats(), [0]

        def _cb(user, z, nrec, recp, densp):
            count[0] += 1
            if recp:
                buf = (C.c_char * (nrec * dt.itemsize)).from_address(recp)
                return int(on_plane(int(z), np.frombuffer(buf, dtype=dt).reshape(n, n)) or 0)
            return 0

        rc = call(SLAB_CB(_cb), st)
        if rc:
            raise RuntimeError("zd_generate_field_lpt failed (rc=%d); see stderr" % rc)
        out = _stats_dict(st)
        out["planes"] = count[0]
        return out
    eigp, eig_ppd = (None, 0)
    if eig is not None:
        eig = np.ascontiguousarray(eig, dtype=np.float64)
        eigp, eig_ppd = eig.ctypes.data, eig.shape[0]
    return _collecting_run(params, collect, lambda cb, st: L.zd_generate_field(C.byref(params), C.byref(ps.pk), eigp, eig_ppd, kcode, dcode,
                                                                               ptr, on_device, cb, None, C.byref(st)), "zd_generate_field")


def _cotangent_args(named, ppd):
    """(dtype code, on_device, [pointer or None, ...], torch device or None) of the cotangents handed to field_vjp: numpy arrays or
    torch tensors on the GPU, all of one kind and dtype (float32 or float64), C-contiguous, g_q / g_v of shape (ppd, ppd, ppd, 3), g_dens
    (ppd, ppd, ppd).  Anything else raises before the library is called."""
    n = int(ppd)
    given = [(name, a) for name, a in named if a is not None]
    if not given:
        raise ValueError("field_vjp: at least one of g_q, g_v, g_dens expected")
    dtypes, devices, ptrs = set(), set(), []
    for name, a in named:
        if a is None:
            ptrs.append(None)
            continue
        shape = (n, n, n) if name == "g_dens" else (n, n, n, 3)
        if isinstance(a, np.ndarray):
            if a.dtype not in (np.float32, np.float64):
                raise TypeError("%s: float32 or float64 expected (got %s)" % (name, a.dtype))
            if a.shape != shape:
                raise ValueError("%s: shape %r expected (got %r)" % (name, shape, a.shape))
            if not a.flags["C_CONTIGUOUS"]:
                raise ValueError("%s: a C-contiguous array expected" % name)
            dtypes.add(int(a.dtype == np.float64))
            devices.add(None)
            ptrs.append(a.ctypes.data)
        elif type(a).__module__.split(".")[0] == "torch" and hasattr(a, "data_ptr"):
            import torch
            if not a.is_cuda:
                raise ValueError("%s: a torch tensor must live on the GPU (pass a numpy array for host data)" % name)
            if a.dtype not in (torch.float32, torch.float64):
                raise TypeError("%s: float32 or float64 expected (got %s)" % (name, a.dtype))
            if tuple(a.shape) != shape:
                raise ValueError("%s: shape %r expected (got %r)" % (name, shape, tuple(a.shape)))
            if not a.is_contiguous():
                raise ValueError("%s: a C-contiguous tensor expected" % name)
            dtypes.add(int(a.dtype == torch.float64))
            devices.add(a.device)
            ptrs.append(a.data_ptr())
        else:
            raise TypeError("%s: a numpy array or a torch tensor on the GPU expected (got %s)" % (name, type(a).__name__))
    if len(dtypes) != 1:
        raise TypeError("field_vjp: the cotangents must share one dtype")
    if len(devices) != 1:
        raise ValueError("field_vjp: the cotangents must all be numpy arrays or all be tensors on one GPU")
    device = devices.pop()
    return dtypes.pop(), int(device is not None), ptrs, device


def field_vjp(params, ps, g_q=None, g_v=None, g_dens=None, kind="density", eig=None, out=None):
    """The adjoint of generate_field's linear map field -> (d, v, density) (zd_field_vjp; definition in csrc/zd_kernels_field_adj.hip):
    the gradient of a scalar loss with respect to the field, float64 [z][y][x], from its gradients g_q, g_v (ppd, ppd, ppd, 3; components
    in the order of the records' d / v members) and g_dens (ppd, ppd, ppd).  Each cotangent is optional, None is an exact zero.  numpy
    arrays give a numpy array, torch tensors on the GPU a tensor there; out= (float64, C-contiguous, of either sort) is filled and
    returned instead."""
    if kind not in FIELD_KINDS:
        raise ValueError("field kind must be one of %s (got %r)" % (sorted(FIELD_KINDS), kind))
    n = int(params.ppd)
    dcode, on_device, ptrs, device = _cotangent_args((("g_q", g_q), ("g_v", g_v), ("g_dens", g_dens)), n)
    if out is None:
        if on_device:
            import torch
            out = torch.empty((n, n, n), dtype=torch.float64, device=device)
        else:
            out = np.empty((n, n, n), dtype=np.float64)
    if isinstance(out, np.ndarray):
        if out.dtype != np.float64 or out.shape != (n, n, n) or not out.flags["C_CONTIGUOUS"] or not out.flags["WRITEABLE"]:
            raise ValueError("out: a writeable C-contiguous float64 array of shape (%d, %d, %d) expected" % (n, n, n))
        outp, out_on_device = out.ctypes.data, 0
    elif type(out).__module__.split(".")[0] == "torch" and hasattr(out, "data_ptr"):
        import torch
        if not out.is_cuda or out.dtype != torch.float64 or tuple(out.shape) != (n, n, n) or not out.is_contiguous():
            raise ValueError("out: a C-contiguous float64 tensor of shape (%d, %d, %d) on the GPU expected" % (n, n, n))
        outp, out_on_device = out.data_ptr(), 1
    else:
        raise TypeError("out: a numpy array or a torch tensor on the GPU expected (got %s)" % type(out).__name__)
    if on_device or out_on_device:
        import torch
        torch.cuda.synchronize()  # the library works on its own stream
    L = load_library()
    eigp, eig_ppd = (None, 0)
    if eig is not None:
        eig = np.ascontiguousarray(eig, dtype=np.float64)
        eigp, eig_ppd = eig.ctypes.data, eig.shape[0]
    rc = L.zd_field_vjp(C.byref(params), C.byref(ps.pk), eigp, eig_ppd, FIELD_KINDS[kind], dcode, ptrs[0], ptrs[1], ptrs[2], on_device,
                        outp, out_on_device, None)
    if rc:
        raise RuntimeError("zd_field_vjp failed (rc=%d); see stderr" % rc)
    return out


PLT_MAX_PPD = 512  # ZD_PLT_MAX_PPD


def make_eigenmodes(n):
    """The PLT eigenmode table of n points per side, computed on cuda:0 (zd_make_eigenmodes; definition in csrc/zd_kernels_plt.hip):
    float64 [n][n][n/2 + 1][4] = (e_x, e_y, e_z, lambda), what generate / Plan / measure_power / direct_sum take as eig.  n: even, in
    [4, 512]."""
    n = int(n)
    if n < 4 or n > PLT_MAX_PPD or n % 2:
        raise ValueError("make_eigenmodes: n must be even and in [4, %d] (got %d)" % (PLT_MAX_PPD, n))
    out = np.empty((n, n, n // 2 + 1, 4), dtype=np.float64)
    if load_library().zd_make_eigenmodes(n, out.ctypes.data):
        raise RuntimeError("zd_make_eigenmodes failed; see stderr")
    return out


def write_eigenmodes(path, table):
    """an eigenmode table [n][n][n/2 + 1][4] as the file ZD_PLT_filename names (zd_write_eigmodes: int32 n, then the doubles)"""
    t = np.ascontiguousarray(table, dtype=np.float64)
    if t.ndim != 4 or t.shape[1] != t.shape[0] or t.shape[2] != t.shape[0] // 2 + 1 or t.shape[3] != 4:
        raise ValueError("write_eigenmodes: the table must be [n][n][n/2 + 1][4] (got %r)" % (t.shape,))
    if load_library().zd_write_eigmodes(os.fsencode(path), t.ctypes.data, t.shape[0]):
        raise RuntimeError("zd_write_eigmodes failed; see stderr")


def load_eigenmodes(path):
    """the table of an eigenmode file (zd_load_eigmodes), as an array [n][n][n/2 + 1][4]"""
    L = load_library()
    ptr, n = C.c_void_p(), C.c_int64()
    if L.zd_load_eigmodes(os.fsencode(path), C.byref(ptr), C.byref(n)):
        raise RuntimeError("zd_load_eigmodes failed; see stderr")
    try:
        shape = (n.value, n.value, n.value // 2 + 1, 4)
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_double)), shape).copy()
    finally:
        L.zd_free(ptr)


POWER_SUMS = ("sum_k", "sum_dens", "sum_input", "sum_disp", "sum_vel")


def power_nbins(ppd, bin_width=1):
    """bins of measure_power: bin b holds (b w)^2 <= kx^2 + ky^2 + kz^2 < ((b + 1) w)^2 (zd_power_nbins; no GPU needed)"""
    return int(load_library().zd_power_nbins(int(ppd), int(bin_width)))


def _power_arrays(ppd, bin_width):
    nb = power_nbins(ppd, bin_width)
    if nb <= 0:
        raise ValueError("measure_power: bin_width must be an integer >= 1")
    out = {"count": np.zeros(nb, dtype=np.int64)}
    for name in POWER_SUMS:
        out[name] = np.zeros(nb, dtype=np.float64)
    return nb, out, [out[k].ctypes.data for k in ("count",) + POWER_SUMS]


def _power_derived(out):
    """the derived columns: mean |k| of the bin, measured / input band power, modes"""
    n = out["count"]
    with np.errstate(divide="ignore", invalid="ignore"):
        out["k_mean"] = np.where(n > 0, out["sum_k"] / n, np.nan)
        out["P_measured / P_input"] = np.where(out["sum_input"] > 0, out["sum_dens"] / out["sum_input"], np.nan)
    out["nmodes"] = n.copy()
    return out


def measure_power(params, ps, eig=None, bin_width=1):
    """Band power of the modes a run with these parameters realises (zd_measure_power: one sweep on cuda:0 that bins instead of
    storing; definition in csrc/zd_kernels_pk.hip).  Returns a dict of numpy arrays over the integer |k| shells of width
    bin_width: count, sum_k, sum_dens, sum_input, sum_disp, sum_vel and the derived k_mean, "P_measured / P_input", nmodes."""
    L = load_library()
    nb, out, ptrs = _power_arrays(params.ppd, bin_width)
    eigp, eig_ppd = (None, 0)
    if eig is not None:
        eig = np.ascontiguousarray(eig, dtype=np.float64)
        eigp, eig_ppd = eig.ctypes.data, eig.shape[0]
    if L.zd_measure_power(C.byref(params), C.byref(ps.pk), eigp, eig_ppd, int(bin_width), nb, *ptrs):
        raise RuntimeError("zd_measure_power failed; see stderr")
    return _power_derived(out)


MAX_SITES = 64  # sites per direct_sum call


def _site_array(sites, ppd):
    """int64 [nsites, 3] of (z, y, x), checked before anything touches the GPU"""
    s = np.asarray(sites)
    if s.size == 0 or s.ndim != 2 or s.shape[1] != 3:
        raise ValueError("direct_sum: sites must be a non-empty [nsites, 3] array of (z, y, x)")
    if not np.issubdtype(s.dtype, np.integer):
        raise ValueError("direct_sum: sites must be integers")
    if s.shape[0] > MAX_SITES:
        raise ValueError("direct_sum: at most %d sites per call (got %d)" % (MAX_SITES, s.shape[0]))
    if s.min() < 0 or s.max() >= int(ppd):
        raise ValueError("direct_sum: every site must lie in [0, %d)^3" % int(ppd))
    return np.ascontiguousarray(s, dtype=np.int64)


def direct_sum(params, ps, sites, eig=None):
    """The fields a run with these parameters delivers at the lattice sites [(z, y, x), ...], by direct summation over the modes it
    realises (zd_direct_sum: one sweep on cuda:0 per 8 sites, no transform and no store; definition in csrc/zd_kernels_ds.hip).
    Returns float64 [nsites, 7] = qx, qy, qz, vx, vy, vz, density."""
    s = _site_array(sites, params.ppd)
    L = load_library()
    out = np.zeros((s.shape[0], 7), dtype=np.float64)
    eigp, eig_ppd = (None, 0)
    if eig is not None:
        eig = np.ascontiguousarray(eig, dtype=np.float64)
        eigp, eig_ppd = eig.ctypes.data, eig.shape[0]
    if L.zd_direct_sum(C.byref(params), C.byref(ps.pk), eigp, eig_ppd, s.shape[0], s.ctypes.data, out.ctypes.data):
        raise RuntimeError("zd_direct_sum failed; see stderr")
    return out


def lpt_direct_sum(params, ps, sites):
    """The three orders of a ZD_q2LPT / ZD_q3LPT run at the lattice sites [(z, y, x), ...], by direct summation over the first-order
    modes and the plan's resident higher-order spectra (zd_lpt_direct_sum; definition in csrc/zd_kernels_lpt_ds.hip).  Returns float64
    [nsites, 3, 6] = order 1, 2, 3 x (qx, qy, qz, vx, vy, vz); the delivered record is the sum over the orders."""
    s = _site_array(sites, params.ppd)
    out = np.zeros((s.shape[0], 3, 6), dtype=np.float64)
    if load_library().zd_lpt_direct_sum(C.byref(params), C.byref(ps.pk), s.shape[0], s.ctypes.data, out.ctypes.data):
        raise RuntimeError("zd_lpt_direct_sum failed; see stderr")
    return out


LPT_POWER_SUMS = ("sum_k", "sum_input", "sum_dens", "sum_disp1", "sum_disp2", "sum_disp3", "sum_disp", "sum_vel")


def _lpt_power_arrays(ppd, bin_width):
    nb = power_nbins(ppd, bin_width)
    if nb <= 0:
        raise ValueError("lpt_power: bin_width must be an integer >= 1")
    return nb, np.zeros(nb, dtype=np.int64), np.zeros((nb, len(LPT_POWER_SUMS)), dtype=np.float64)


def _lpt_power_dict(count, sums):
    out = {"count": count}
    for j, name in enumerate(LPT_POWER_SUMS):
        out[name] = np.ascontiguousarray(sums[:, j])
    with np.errstate(divide="ignore", invalid="ignore"):
        out["k_mean"] = np.where(count > 0, out["sum_k"] / count, np.nan)
    return out


def lpt_power(params, ps, bin_width=1):
    """Band power of a ZD_q2LPT / ZD_q3LPT run (zd_lpt_power; definition in csrc/zd_kernels_lpt_ds.hip): a dict of numpy arrays over
    the integer |k| shells of width bin_width: count, sum_k, sum_input, sum_dens, the displacement power of each order sum_disp1,
    sum_disp2, sum_disp3, of the delivered displacement sum_disp and velocity sum_vel, and the derived k_mean."""
    nb, count, sums = _lpt_power_arrays(params.ppd, bin_width)
    if load_library().zd_lpt_power(C.byref(params), C.byref(ps.pk), int(bin_width), nb, count.ctypes.data, sums.ctypes.data):
        raise RuntimeError("zd_lpt_power failed; see stderr")
    return _lpt_power_dict(count, sums)


def _position_array(positions):
    """float64 [npart, 3] of (x, y, z); the range check is the library's (one line on stderr names the particle)"""
    pos = np.ascontiguousarray(positions, dtype=np.float64)
    if pos.ndim != 2 or pos.shape[1] != 3 or pos.shape[0] < 1:
        raise ValueError("positions must be a non-empty [npart, 3] array of (x, y, z) in [0, 1)")
    return pos


def displace(params, ps, positions, order=3, tile=1, eig=None, max_particles_per_sweep=0, stats=None):
    """Displacements and velocities of a run with these parameters at the positions [npart, 3] of (x, y, z) in box units, each in
    [0, 1), replicated tile^3 times — a glass, a tiled glass, any off-lattice load (zd_displace on cuda:0; definition in
    csrc/zd_kernels_glass.hip).  order: 1 = trilinear, 3 = cubic Lagrange.  Returns float64 [npart * tile^3, 6] = qx, qy, qz, vx, vy,
    vz; particle ((a tile + b) tile + c) npart + i sits at (positions[i] + (c, b, a)) / tile.  stats (a dict): filled with the run's
    statistics and "sweeps"."""
    pos = _position_array(positions)
    total = pos.shape[0] * int(tile) ** 3 if tile >= 1 else 0
    out = np.zeros((max(total, 0), 6), dtype=np.float64)
    eigp, eig_ppd = (None, 0)
    if eig is not None:
        eig = np.ascontiguousarray(eig, dtype=np.float64)
        eigp, eig_ppd = eig.ctypes.data, eig.shape[0]
    sweeps = [0]

    def _cb(user, first, n, outp):
        sweeps[0] += 1
        C.memmove(out[first:].ctypes.data, outp, n * 48)
        return 0

    st = ZdStats()
    if load_library().zd_displace(C.byref(params), C.byref(ps.pk), eigp, eig_ppd, int(order), pos.shape[0], pos.ctypes.data, int(tile),
                                  int(max_particles_per_sweep), PARTICLE_CB(_cb), None, C.byref(st)):
        raise RuntimeError("zd_displace failed; see stderr")
    if stats is not None:
        stats.update(_stats_dict(st))
        stats["sweeps"] = sweeps[0]
    return out


class Interp:
    """The consumer object of zd_interp_*: create it for a load, add every device plane once, take the result [npart, 6]."""

    def __init__(self, ppd, icformat, positions, order=3):
        self.L = load_library()
        self.pos = _position_array(positions)
        h = C.c_void_p()
        fmt = ICFORMATS[icformat] if isinstance(icformat, str) else int(icformat)
        if self.L.zd_interp_create(int(ppd), fmt, int(order), self.pos.shape[0], self.pos.ctypes.data, C.byref(h)):
            raise RuntimeError("zd_interp_create failed; see stderr")
        self.h = h

    def add_plane(self, z, d_plane_records, stream=0):
        if self.L.zd_interp_add_plane(self.h, int(z), d_plane_records, stream):
            raise RuntimeError("zd_interp_add_plane failed; see stderr")

    def result(self):
        out = np.zeros((self.pos.shape[0], 6), dtype=np.float64)
        if self.L.zd_interp_result(self.h, out.ctypes.data):
            raise RuntimeError("zd_interp_result failed; see stderr")
        return out

    def close(self):
        if self.h:
            self.L.zd_interp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def generate_planes(params, ps, on_plane, eig=None):
    """zd_generate with a per-plane consumer: on_plane(z, records[y, x]) sees a VIEW valid only during the call (like the
    reference's single output buffer); nothing is accumulated here.  Returns the statistics + the number of planes."""
    L = load_library()
    n = int(params.ppd)
    dt = RECORD_DTYPES[_fmt_name(params.icformat)]
    st = ZdStats()
    eigp, eig_ppd = (None, 0)
    if eig is not None:
        eig = np.ascontiguousarray(eig, dtype=np.float64)
        eigp, eig_ppd = eig.ctypes.data, eig.shape[0]
    count = [0]

    def _cb(user, z, nrec, recp, densp):
        count[0] += 1
        if recp:
            buf = (C.c_char * (nrec * dt.itemsize)).from_address(recp)
            return int(on_plane(int(z), np.frombuffer(buf, dtype=dt).reshape(n, n)) or 0)  # non-zero aborts (WriteParticlesSlab failing)
        return 0

    cb = SLAB_CB(_cb)
    rc = L.zd_generate(C.byref(params), C.byref(ps.pk), eigp, eig_ppd, cb, None, C.byref(st))
    if rc:
        raise RuntimeError("zd_generate failed (rc=%d); see stderr" % rc)
    out = _stats_dict(st)
    out["planes"] = count[0]
    return out


class Plan:
    """Staged API: one rank's share of the Z and XY stages on device pointers (see the header)."""

    def __init__(self, params, ps, eig=None, rank=0, nranks=1, testing=False, _field=None, _order=1):
        self.L = load_testing_library() if testing else load_library()  # testing: the -DZD_TESTING build (zd_test_poison), tests only
        self.params = params
        self._eig = None if eig is None else np.ascontiguousarray(eig, dtype=np.float64)
        h = C.c_void_p()
        eigp, eig_ppd = (None, 0) if self._eig is None else (self._eig.ctypes.data, self._eig.shape[0])
        if _field is not None and _order != 1:  # from_field(order=2): a higher order on the field; the plan's parameters read q2LPT = 1
            if self._eig is not None:
                raise ValueError("Plan.from_field: order = %r takes no eigenmode table (ZD_qPLT has no second order)" % (_order,))
            if self.L.zd_plan_create_field_lpt(C.byref(params), C.byref(ps.pk), *_field, int(_order), C.byref(h)):
                raise RuntimeError("zd_plan_create_field_lpt failed; see stderr")
        elif _field is not None:  # from_field: (kind code, dtype code, pointer, on_device)
            if self.L.zd_plan_create_field(C.byref(params), C.byref(ps.pk), eigp, eig_ppd, *_field, C.byref(h)):
                raise RuntimeError("zd_plan_create_field failed; see stderr")
        elif self.L.zd_plan_create(C.byref(params), C.byref(ps.pk), eigp, eig_ppd, rank, nranks, C.byref(h)):
            raise RuntimeError("zd_plan_create failed")
        self.h = h
        self.rank, self.nranks = rank, nranks
        self.narray = self.L.zd_plan_narray(h)
        self.store_mode = [k for k, v in STORE_MODES.items() if v == self.L.zd_plan_store_mode(h)][0]
        self.R = self.L.zd_plan_stream_factor(h)
        self.passes = self.L.zd_plan_passes(h)          # R, or R/2 when a pass carries two z-residues
        self.plane_step = self.L.zd_plan_plane_step(h)  # stage_x plane ranges are multiples of it
        self.record_size = self.L.zd_plan_record_size(h)
        self.exchange_bytes = self.L.zd_plan_exchange_bytes(h)
        self.local_planes = self.L.zd_plan_local_planes(h)

    @classmethod
    def from_field(cls, params, ps, field, kind="density", eig=None, order=1):
        """a one-rank plan whose modes come from a caller-supplied real field (zd_plan_create_field; see generate_field): every
        method of a plan works on it.  The field is consumed here: the plan keeps its modes, not the array.  order=2: the second-order
        plan on the field (zd_plan_create_field_lpt): lpt_direct_sum and lpt_power work on it, direct_sum and measure_power refuse it."""
        return cls(params, ps, eig=eig, _field=_field_arg(field, params.ppd, kind, order), _order=order)

    def plane_z(self, residue, local_plane):
        return self.L.zd_plan_plane_z(self.h, residue, local_plane)

    def stage_z(self, residue, d_send, stream=0):
        if self.L.zd_plan_stage_z(self.h, residue, d_send, stream):
            raise RuntimeError("zd_plan_stage_z failed")

    def stage_y(self, d_recv, stream=0):
        if self.L.zd_plan_stage_y(self.h, d_recv, stream):
            raise RuntimeError("zd_plan_stage_y failed")

    def stage_x(self, residue, d_recv, plane0, nplanes, d_records, d_density=None, stream=0):
        if self.L.zd_plan_stage_x(self.h, residue, d_recv, plane0, nplanes, d_records, d_density, stream):
            raise RuntimeError("zd_plan_stage_x failed")

    def run_pass(self, residue, d_store, d_records, rec_planes, comm=None, consume=None, stream=0):
        """Z stage -> exchange (plane groups, overlapped) -> y/x stages inside the library (zd_plan_run_pass);
        consume(first_local_plane, nplanes, d_records_ptr, stream) is called per finished group of planes"""
        cb = GROUP_CB()
        if consume is not None:
            cb = GROUP_CB(lambda user, first, n, recp, st: int(consume(int(first), int(n), recp, st) or 0))
        if self.L.zd_plan_run_pass(self.h, comm.h if comm is not None else None, residue, d_store, d_records, rec_planes, cb, None, stream):
            raise RuntimeError("zd_plan_run_pass failed")

    def run_passes(self, first, step, d_store, d_store2, d_records, rec_planes, comm=None, consume=None, stream=0):
        """the passes first, first + step, ... in one call (zd_plan_run_passes); with a second store d_store2 and several ranks
        the passes are pipelined; consume(pass, first_local_plane, nplanes, d_records_ptr, stream)"""
        cb = PASS_CB()
        if consume is not None:
            cb = PASS_CB(lambda user, ps, first_, n, recp, st: int(consume(int(ps), int(first_), int(n), recp, st) or 0))
        if self.L.zd_plan_run_passes(self.h, comm.h if comm is not None else None, first, step, d_store, d_store2, d_records, rec_planes,
                                     cb, None, stream):
            raise RuntimeError("zd_plan_run_passes failed")

    def measure_power(self, bin_width=1, stream=0):
        """band power of this rank's rows (zd_plan_measure_power): the sums of the ranks add up to the whole"""
        nb, out, ptrs = _power_arrays(self.params.ppd, bin_width)
        if self.L.zd_plan_measure_power(self.h, int(bin_width), nb, *ptrs, stream):
            raise RuntimeError("zd_plan_measure_power failed; see stderr")
        return _power_derived(out)

    def direct_sum(self, sites, stream=0):
        """direct summation at the sites over this rank's rows (zd_plan_direct_sum): the arrays of the ranks add up to the whole"""
        s = _site_array(sites, self.params.ppd)
        out = np.zeros((s.shape[0], 7), dtype=np.float64)
        if self.L.zd_plan_direct_sum(self.h, s.shape[0], s.ctypes.data, out.ctypes.data, stream):
            raise RuntimeError("zd_plan_direct_sum failed; see stderr")
        return out

    def lpt_direct_sum(self, sites, stream=0):
        """the three orders of this ZD_q2LPT / ZD_q3LPT plan at the sites (zd_plan_lpt_direct_sum): [nsites, 3, 6]"""
        s = _site_array(sites, self.params.ppd)
        out = np.zeros((s.shape[0], 3, 6), dtype=np.float64)
        if self.L.zd_plan_lpt_direct_sum(self.h, s.shape[0], s.ctypes.data, out.ctypes.data, stream):
            raise RuntimeError("zd_plan_lpt_direct_sum failed; see stderr")
        return out

    def lpt_power(self, bin_width=1, stream=0):
        """band power of the three orders of this ZD_q2LPT / ZD_q3LPT plan (zd_plan_lpt_power)"""
        nb, count, sums = _lpt_power_arrays(self.params.ppd, bin_width)
        if self.L.zd_plan_lpt_power(self.h, int(bin_width), nb, count.ctypes.data, sums.ctypes.data, stream):
            raise RuntimeError("zd_plan_lpt_power failed; see stderr")
        return _lpt_power_dict(count, sums)

    def interp(self, positions, order=3, stream=0):
        """the plan's field at the positions [npart, 3] (zd_interp_create, zd_plan_interp, zd_interp_result): float64 [npart, 6]"""
        it = Interp(self.params.ppd, self.params.icformat, positions, order)
        try:
            if self.L.zd_plan_interp(self.h, it.h, stream):
                raise RuntimeError("zd_plan_interp failed; see stderr")
            return it.result()
        finally:
            it.close()

    def stats(self):
        st = ZdStats()
        if self.L.zd_plan_stats(self.h, C.byref(st)):
            raise RuntimeError("zd_plan_stats failed")
        return _stats_dict(st)

    def close(self):
        if self.h:
            self.L.zd_plan_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Comm:
    """RCCL communicator of the library (one process per GPU): `exchange_id` makes rank 0's 128-byte id known to every
    rank, e.g. lambda b: torch.distributed broadcast of a uint8 tensor"""

    def __init__(self, rank, nranks, exchange_id):
        self.L = load_library()
        buf = (C.c_ubyte * 128)()
        if rank == 0 and self.L.zd_comm_unique_id(buf):
            raise RuntimeError("zd_comm_unique_id failed")
        raw = exchange_id(bytes(buf))
        idb = (C.c_ubyte * 128).from_buffer_copy(raw)
        h = C.c_void_p()
        if self.L.zd_comm_create(rank, nranks, idb, C.byref(h)):
            raise RuntimeError("zd_comm_create failed")
        self.h = h

    def traffic(self, reset=False):
        """(bytes sent to, bytes received from) other ranks"""
        a, b = C.c_int64(), C.c_int64()
        self.L.zd_comm_traffic(self.h, C.byref(a), C.byref(b), int(reset))
        return a.value, b.value

    def probe(self, bytes_per_peer=128 << 20, reps=3):
        """GB/s one link of this rank carries per direction while every peer is sent to and received from at once (0.0 without peers)"""
        r = C.c_double()
        if self.L.zd_comm_probe(self.h, int(bytes_per_peer), int(reps), C.byref(r)):
            raise RuntimeError("zd_comm_probe failed")
        return r.value

    def abort(self):
        if self.h:
            self.L.zd_comm_abort(self.h)

    def close(self):
        if self.h:
            self.L.zd_comm_destroy(self.h)
            self.h = None


# ---- device test hooks (the -DZD_TESTING library) ---------------------------------------------------------------------------
def test_draws(seed, kxyz):
    L = load_testing_library()
    k = np.ascontiguousarray(kxyz, dtype=np.int32).reshape(-1, 3)
    out = np.zeros((k.shape[0], 2), dtype=np.uint64)
    if L.zd_test_draws(int(seed), k.shape[0], k.ctypes.data, out.ctypes.data):
        raise RuntimeError("zd_test_draws failed")
    return out


def test_modes(params, ps, kxyz):
    L = load_testing_library()
    k = np.ascontiguousarray(kxyz, dtype=np.int32).reshape(-1, 3)
    out = np.zeros((k.shape[0], 2), dtype=np.float64)
    if L.zd_test_modes(C.byref(params), C.byref(ps.pk), k.shape[0], k.ctypes.data, out.ctypes.data):
        raise RuntimeError("zd_test_modes failed")
    return out[:, 0] + 1j * out[:, 1]


def test_modes_table(params, ps, kxyz):
    """D(k) and fundamental/k^2 through k_genf's table arithmetic; returns (complex D [n], float64 [n])"""
    L = load_testing_library()
    k = np.ascontiguousarray(kxyz, dtype=np.int32).reshape(-1, 3)
    out = np.zeros((k.shape[0], 3), dtype=np.float64)
    if L.zd_test_modes_table(C.byref(params), C.byref(ps.pk), k.shape[0], k.ctypes.data, out.ctypes.data):
        raise RuntimeError("zd_test_modes_table failed")
    return out[:, 0] + 1j * out[:, 1], out[:, 2]


def test_plt_matrix(n, m_xyz, alpha=2.0, shells=4):
    """the six distinct elements xx, yy, zz, xy, xz, yz of the PLT dynamical matrix at the signed wavenumbers m_xyz [nmodes, 3] of a
    table of n points per side (zd_test_plt_matrix)"""
    L = load_testing_library()
    m = np.ascontiguousarray(m_xyz, dtype=np.int32).reshape(-1, 3)
    out = np.zeros((m.shape[0], 6), dtype=np.float64)
    if L.zd_test_plt_matrix(int(n), float(alpha), int(shells), m.shape[0], m.ctypes.data, out.ctypes.data):
        raise RuntimeError("zd_test_plt_matrix failed")
    return out


ROLES = {"main": 0, "phi": 1, "phik": 2, "lpt2_grad": 3}  # zd_route.h ROLE_*


def test_route_kernels(params, stream_factor=0, nranks=1, role="main", text=True):
    """The dispatch tables the stages of a job consult and whether each has a kernel for its key (zd_test_route_kernels; no GPU):
    {"code": the hook's return value (>= 0: accepted, that many stages without a kernel; -1 refused by the parameters alone; -2 refused
    only because a stage has no kernel), "accepted", "why", "stages": [(stage, launcher, key, present)]}.  text=False: the code alone."""
    L = load_testing_library()
    if not text:
        return L.zd_test_route_kernels(C.byref(params), stream_factor, nranks, ROLES[role], None, 0)
    buf = C.create_string_buffer(8192)
    code = L.zd_test_route_kernels(C.byref(params), stream_factor, nranks, ROLES[role], buf, len(buf))
    lines = buf.value.decode().splitlines()
    head = lines[0].split("\t", 2)
    stages = []
    for ln in lines[1:]:
        stage, launcher, key, present = ln.split("\t")
        stages.append((stage, launcher, key, present == "1"))
    return {"code": code, "accepted": head[1] == "1", "why": head[2] if len(head) > 2 else "", "stages": stages}


def test_v1_words(seed, nblocks):
    """first 624 * nblocks words of the ZD_Version = 1 stream generator (gsl_rng_mt19937) for `seed`"""
    L = load_testing_library()
    out = np.zeros(624 * nblocks, dtype=np.uint32)
    if L.zd_test_v1_words(int(seed), int(nblocks), out.ctypes.data):
        raise RuntimeError("zd_test_v1_words failed")
    return out


def test_fft(x, axis_kind):
    """x: complex128 [lines, n]; returns the unnormalised inverse DFT of every line computed on the GPU."""
    L = load_testing_library()
    x = np.ascontiguousarray(x, dtype=np.complex128)
    lines, n = x.shape
    if axis_kind == 1:  # strided situation: device layout [n][lines]
        xin = np.ascontiguousarray(x.T)
        out = np.zeros_like(xin)
        rc = L.zd_test_fft(n, lines, 1, xin.ctypes.data, out.ctypes.data)
        out = np.ascontiguousarray(out.T)
    else:
        out = np.zeros_like(x)
        rc = L.zd_test_fft(n, lines, 0, x.ctypes.data, out.ctypes.data)
    if rc:
        raise RuntimeError("zd_test_fft failed")
    return out
