"""CPU: the host side of the direct summation at sample sites (zd_direct_sum / zd_plan_direct_sum, csrc/zd_kernels_ds.hip) — the new
C ABI symbols, the checks api.direct_sum makes before it touches the GPU, and the three parameter keys of the self-checking run
with the combinations the reader refuses."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, WMAP

NEW_SYMBOLS = ("zd_plan_direct_sum", "zd_direct_sum")

PAR = """BoxSize = 720
CPD = 5
ICFormat = "%(fmt)s"
InitialConditionsDirectory = "/tmp/unused"
InitialRedshift = 49
NP = 32768
ZD_NumBlock = 2
ZD_Pk_filename = "%(pk)s"
ZD_Pk_norm = 8.0
ZD_Pk_scale = 1.0
ZD_Pk_sigma = 0.0210839935761
ZD_Pk_smooth = 0.0
ZD_Seed = 12346
ZD_Version = %(version)d
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
    assert os.path.exists(os.path.join(ROOT, "zeldovich_plt_amd", "csrc", "zd_kernels_ds.hip"))


class _NoGpu:
    """stands in for the library: any call into it fails the test"""

    def __getattr__(self, name):
        raise AssertionError("the library was reached (%s) with a bad site array" % name)


@pytest.mark.parametrize("sites,word", [
    ([], "non-empty"),
    ([1, 2, 3], "[nsites, 3]"),
    ([[1, 2]], "[nsites, 3]"),
    ([[[1, 2, 3]]], "[nsites, 3]"),
    ([[0.5, 1.0, 2.0]], "integers"),
    ([[0, 0, 32]], "[0, 32)"),
    ([[0, 32, 0]], "[0, 32)"),
    ([[-1, 0, 0]], "[0, 32)"),
    ([[0, 0, 0]] * 65, "at most 64"),
])
def test_direct_sum_rejects_bad_site_arrays_before_the_gpu(monkeypatch, sites, word):
    import zeldovich_plt_amd.api as api
    monkeypatch.setattr(api, "load_library", lambda: _NoGpu())
    with pytest.raises(ValueError) as e:
        api.direct_sum(api.make_params(32), None, sites)
    assert word in str(e.value)
    plan = api.Plan.__new__(api.Plan)  # no plan is made: the check comes before the handle is used
    plan.params, plan.L, plan.h = api.make_params(32), _NoGpu(), None
    with pytest.raises(ValueError):
        plan.direct_sum(sites)


def test_site_arrays_are_passed_as_int64_zyx():
    import zeldovich_plt_amd.api as api
    s = api._site_array(np.array([[31, 0, 5], [0, 31, 31]], dtype=np.int32), 32)
    assert s.dtype == np.int64 and s.flags["C_CONTIGUOUS"] and s.tolist() == [[31, 0, 5], [0, 31, 31]]
    assert api._site_array([(0, 0, 0)] * 64, 32).shape == (64, 3)


def _read(tmp_path, extra, fmt="RVdoubleZel", version=2):
    import zeldovich_plt_amd.api as api
    par = tmp_path / "t.par"
    par.write_text(PAR % dict(pk=WMAP, fmt=fmt, version=version) + extra)
    return api.params_from_file(str(par))


def test_reader_parses_the_three_keys(tmp_path):
    _p, s = _read(tmp_path, "")
    assert (s.SelfCheck, s.SelfCheck_tol, s.SelfCheck_filename) == (0, 0.0, b"")
    p, s = _read(tmp_path, 'ZD_SelfCheck = 8\nZD_SelfCheck_tol = 2.5e-9\nZD_SelfCheck_filename = "/some/where/sites.txt"\n')
    assert (s.SelfCheck, s.SelfCheck_tol, s.SelfCheck_filename) == (8, 2.5e-9, b"/some/where/sites.txt") and p.ppd == 32
    assert _read(tmp_path, "ZD_SelfCheck = 64\n")[1].SelfCheck == 64
    # the default bound follows the record format: the parity bound for float64 records, the format tests' bound for float32 ones
    for fmt, tol in (("RVdoubleZel", 1e-10), ("Zeldovich", 1e-10), ("RVZel", 1e-6), ("ZelSimple", 1e-6)):
        assert _read(tmp_path, "ZD_SelfCheck = 3\n", fmt=fmt)[1].SelfCheck_tol == tol, fmt
    # the options the check runs with
    for extra in ("ZD_k_cutoff = 2\n", "ZD_CornerModes = 1\n", "ZD_qoneslab = 7\n", "ZD_qdensity = 1\n", "ZD_NumGPU = 2\n", "ZD_StreamFactor = 4\n"):
        assert _read(tmp_path, "ZD_SelfCheck = 8\n" + extra)[1].SelfCheck == 8, extra


def test_new_fields_sit_at_the_end_of_the_strings_struct():
    import zeldovich_plt_amd.api as api
    S = api.ZdParamStrings
    assert S.SelfCheck_tol.offset == S.Pk_measured_filename.offset + 1024
    assert S.SelfCheck.offset == S.SelfCheck_tol.offset + 8 and S.SelfCheck_filename.offset == S.SelfCheck.offset + 4
    assert C.sizeof(S) == (S.SelfCheck_filename.offset + 1024 + 7) // 8 * 8


REFUSED = [
    ("65 sites", "ZD_SelfCheck = 65\n", 2, "1 to 64"),
    ("negative", "ZD_SelfCheck = -1\n", 2, "1 to 64"),
    ("f_NL", "ZD_SelfCheck = 8\nZD_f_NL = 100\n", 2, "ZD_f_NL"),
    ("version 1", "ZD_SelfCheck = 8\n", 1, "ZD_Version = 1"),
    ("2LPT", "ZD_SelfCheck = 8\nZD_q2LPT = 1\n", 2, "ZD_q2LPT"),
    ("live Nyquist planes", "ZD_SelfCheck = 8\nZD_CornerModes = 1\nZD_k_cutoff = 2\n", 2, "Nyquist"),
    ("slab outside", "ZD_SelfCheck = 8\nZD_qoneslab = 32\n", 2, "ZD_qoneslab"),
    ("negative bound", "ZD_SelfCheck = 8\nZD_SelfCheck_tol = -1\n", 2, "ZD_SelfCheck_tol"),
]


@pytest.mark.parametrize("name,extra,version,word", REFUSED, ids=[r[0] for r in REFUSED])
def test_reader_refuses(tmp_path, capfd, name, extra, version, word):
    with pytest.raises(ValueError):
        _read(tmp_path, extra, version=version)
    err = capfd.readouterr().err
    line = [ln for ln in err.splitlines() if "ZD_SelfCheck" in ln]
    assert len(line) == 1 and word in line[0], err
    # ... and the same file without the key is read
    rest = "".join(ln + "\n" for ln in extra.splitlines() if not ln.startswith("ZD_SelfCheck ="))
    assert _read(tmp_path, rest, version=version)[1].SelfCheck == 0
