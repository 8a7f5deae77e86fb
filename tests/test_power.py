"""CPU: the band-power measurement's host side — the new C ABI symbols, the bin count, the parameter key, and the definition of
the sums pinned against the oracle without a GPU."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import power_ref as pr
from conftest import ROOT, WMAP

NEW_SYMBOLS = ("zd_power_nbins", "zd_plan_measure_power", "zd_measure_power")

PAR = """BoxSize = 720
CPD = 5
ICFormat = "RVdoubleZel"
InitialConditionsDirectory = "/tmp/unused"
InitialRedshift = 49
NP = 32768
ZD_NumBlock = 2
ZD_Pk_filename = "%s"
ZD_Pk_norm = 8.0
ZD_Pk_scale = 1.0
ZD_Pk_sigma = 0.0210839935761
ZD_Pk_smooth = 0.0
ZD_Seed = 12346
ZD_Version = 2
"""


def test_new_symbols_are_declared_exported_and_listed():
    import zeldovich_plt_amd.api as api
    header = open(os.path.join(ROOT, "include", "zeldovich_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = api.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), "%s is not declared in the header" % name
        assert name in api.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    assert os.path.exists(os.path.join(ROOT, "zeldovich_plt_amd", "csrc", "zd_kernels_pk.hip"))


@pytest.mark.parametrize("ppd", [32, 100, 6912])
@pytest.mark.parametrize("w", [1, 2, 7])
def test_power_nbins_is_the_integer_shell_count(ppd, w):
    import zeldovich_plt_amd.api as api
    nb = api.power_nbins(ppd, w)
    k2max = 3 * (ppd // 2) ** 2  # the corner (N/2, N/2, N/2)
    b = nb - 1
    assert (b * w) ** 2 <= k2max < ((b + 1) * w) ** 2, "the last bin must be the corner's"
    assert nb == pr.nbins(ppd, w)
    if ppd <= 100:  # every mode of the cube has a bin, by the definition applied mode by mode
        bins = pr.bin_cube(ppd, w)
        assert bins.min() == 0 and bins.max() == nb - 1
    assert api.power_nbins(ppd, 0) == 0


def test_params_from_file_reads_the_measured_power_key(tmp_path):
    import zeldovich_plt_amd.api as api
    par = tmp_path / "a.par"
    par.write_text(PAR % WMAP)
    _p, s = api.params_from_file(str(par))
    assert s.Pk_measured_filename == b""
    par.write_text(PAR % WMAP + 'ZD_Pk_measured_filename = "/some/where/pk_measured.txt"\n')
    p, s = api.params_from_file(str(par))
    assert s.Pk_measured_filename == b"/some/where/pk_measured.txt" and p.ppd == 32


def test_binned_density_power_is_the_density_variance(oracle):
    """Parseval pins the definition: over the whole cube, Hermitian pairs twice, N^3 sum_b sum_dens = sum of delta^2 over the lattice
    (density_variance, src/output.cpp:197)"""
    n = 32
    pk = oracle.pk_from_file(WMAP, 720.0)
    p = oracle.make_params(n, qdensity=2)
    D = oracle.mode_cube(p, pk)[0]
    ref = pr.reference_sums(oracle, pk, n, 720.0, D)
    var = oracle.run(p, pk)["density_variance"]
    total = float(ref["sum_dens"].sum()) * n ** 3
    assert abs(total - var) <= 1e-12 * var, (total, var)
    # the bins partition the live modes of the cube
    assert ref["count"].sum() == np.count_nonzero(D) and ref["count"].sum() % 2 == 0
    assert ref["count"][0] == 0 and len(ref["count"]) == math.isqrt(3 * 16 * 16) + 1
