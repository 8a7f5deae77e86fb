"""CPU: the definition of the LPT sums (zeldovich_plt_amd/csrc/zd_kernels_lpt_ds.hip) restated in numpy (tests/lpt_sum_ref.py) and held
against tests/lpt2_ref.py and tests/lpt3_ref.py on a synthetic field, and the host side of the new entry points: symbols, argument
refusals before a plan or the GPU is touched, unchanged struct sizes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lpt2_ref
import lpt3_ref
import lpt_sum_ref as ls
from conftest import ROOT, WMAP

N, BOX = 16, 720.0
G = lpt3_ref.DEFAULTS
NEW_SYMBOLS = ("zd_plan_lpt_direct_sum", "zd_lpt_direct_sum", "zd_plan_lpt_power", "zd_lpt_power")


@pytest.fixture(scope="module")
def field():
    """a synthetic first-order field: random Hermitian D on the alive modes with a red spectrum, large enough for the higher orders
    to be some per cent of it; everything derived from it once, read-only"""
    rng = np.random.default_rng(7)
    mask = lpt2_ref.alive_mask(N, BOX)
    kv = lpt2_ref._kvec(N, BOX)
    k2 = lpt3_ref._k2(kv)
    dk = np.fft.fftn(rng.standard_normal((N, N, N))) / N ** 3 * mask / (k2 / k2.min()) * 40.0
    q = np.empty((N, N, N, 3))
    for a in range(3):
        q[..., a] = np.real(np.fft.ifftn(1j * kv[a] * dk / k2) * N ** 3)
    gamma = 3.0 / 7.0
    dk1, sk, p3k, ck = ls.spectra(q, BOX, mask, G["g3a"], G["g3b"])
    assert np.abs(dk1 - dk).max() <= 1e-13 * np.abs(dk).max()
    parts = lpt3_ref.third_order(q, BOX, mask)
    out = dict(mask=mask, q=q, psi2=lpt2_ref.second_order(q, BOX, mask), parts=parts, spectra=(dk1, sk, p3k, ck), gamma=gamma)
    for v in (q, out["psi2"]) + parts:
        v.setflags(write=False)
    return out


def _field_of(Q):
    return np.stack([ls.direct_sum_everywhere(Q[a]) for a in range(3)], axis=-1)


def test_direct_sums_equal_the_reference_fields_at_every_site(field):
    """order 1, 2, 3 summed the kernel's way — half-space rows twice the real part, the plane ky = 0 position by position — against
    the fields of lpt2_ref / lpt3_ref, to 1e-12 of each field's maximum"""
    dk, sk, p3k, ck = field["spectra"]
    q1, q2, q3 = ls.amplitudes(dk, sk, p3k, ck, BOX, field["mask"], field["gamma"], G["g3c"])
    psi3 = lpt3_ref.combine(field["parts"])
    ratios = np.abs(field["psi2"]).max() / np.abs(field["q"]).max(), np.abs(psi3).max() / np.abs(field["q"]).max()
    print("max|psi2| / max|psi1| =", ratios[0], "max|psi3| / max|psi1| =", ratios[1])
    assert ratios[0] > 1e-3 and ratios[1] > 1e-4  # (the higher orders are there)
    for name, Q, want in (("order 1", q1, field["q"]), ("order 2", q2, field["psi2"]), ("order 3", q3, psi3)):
        err = np.abs(_field_of(Q) - want).max() / np.abs(want).max()
        print(name, err)
        assert err <= 1e-12, name


def test_transverse_term_alone_pins_the_cross_product(field):
    """ZD_3LPT_terms = 4: P3 = 0, T = -g3c (s x C) alone against lpt3_ref's transverse part, to 1e-12 of ITS maximum; the wrong sign or
    the swapped index order miss by twice the field"""
    dk, sk, p3k, ck = field["spectra"]
    want = lpt3_ref.combine(field["parts"], terms=4)
    assert np.abs(want).max() > 0
    _q1, _q2, q3 = ls.amplitudes(dk, sk, 0 * p3k, ck, BOX, field["mask"], field["gamma"], G["g3c"])
    err = np.abs(_field_of(q3) - want).max() / np.abs(want).max()
    print("transverse term", err)
    assert err <= 1e-12
    _q1, _q2, q3 = ls.amplitudes(dk, sk, 0 * p3k, ck, BOX, field["mask"], field["gamma"], -G["g3c"])
    assert np.abs(_field_of(q3) - want).max() >= 1.9 * np.abs(want).max()
    _q1, _q2, q3 = ls.amplitudes(dk, sk, 0 * p3k, ck[::-1], BOX, field["mask"], field["gamma"], G["g3c"])
    assert np.abs(_field_of(q3) - want).max() >= 0.1 * np.abs(want).max()


@pytest.mark.parametrize("w", [1, 3])
def test_binned_power_of_the_orders_equals_the_binned_transform_of_the_fields(field, w):
    dk, sk, p3k, ck = field["spectra"]
    _q1, q2, q3 = ls.amplitudes(dk, sk, p3k, ck, BOX, field["mask"], field["gamma"], G["g3c"])
    for name, Q, want in (("sum_disp2", q2, field["psi2"]), ("sum_disp3", q3, lpt3_ref.combine(field["parts"]))):
        got, ref = ls.binned(Q, field["mask"], w), ls.binned_field(want, field["mask"], w)
        assert ref.max() > 0
        err = float(np.abs(got - ref).max() / ref.max())
        print(name, "w =", w, err)
        assert err <= 1e-12, name


# ---- the built library, no GPU ----------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_listed():
    import zeldovich_plt_amd.api as api
    header = open(os.path.join(ROOT, "include", "zeldovich_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = api.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), "%s is not declared in the header" % name
        assert name in api.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    assert os.path.exists(os.path.join(ROOT, "zeldovich_plt_amd", "csrc", "zd_kernels_lpt_ds.hip"))
    for method in ("lpt_direct_sum", "lpt_power"):
        assert callable(getattr(api, method)) and callable(getattr(api.Plan, method))


def test_struct_sizes_are_unchanged():
    """the feature arrives through entry points and keys read with zd_param_file_string: neither struct has a new member"""
    import zeldovich_plt_amd.api as api
    S = api.ZdParamStrings
    assert C.sizeof(S) == (S.SelfCheck_filename.offset + 1024 + 7) // 8 * 8
    assert S.PLT_compute_ppd.offset == S.SelfCheck_filename.offset + 1024
    assert [name for name, _t in S._fields_][-5:] == ["Pk_measured_filename", "SelfCheck_tol", "SelfCheck", "SelfCheck_filename", "PLT_compute_ppd"]
    # the sizes and member counts of the commit before this feature (the mirrors are held to the header by test_capi_symbols.py)
    assert (C.sizeof(api.ZdParams), len(api.ZdParams._fields_)) == (240, 40)
    assert (C.sizeof(S), len(S._fields_)) == (6312, 22)


ON = dict(q2LPT=1)
PARAM_REFUSALS = [
    ("no q2LPT", dict(), "ZD_q2LPT = 1"),
    ("PLT", dict(q2LPT=1, qPLT=1), "ZD_qPLT"),
    ("f_NL", dict(q2LPT=1, f_NL=50.0), "ZD_f_NL"),
    ("PPD 96", dict(q2LPT=1, ppd=96), "power of two"),
    ("live Nyquist planes", dict(q2LPT=1, corner_modes=1, k_cutoff=2.0), "Nyquist"),
    ("dealias with corner modes", dict(q2LPT=1, lpt2_dealias=1, corner_modes=1), "ZD_2LPT_dealias"),
    ("3LPT with dealias", dict(q2LPT=1, q3LPT=1, lpt2_dealias=1), "ZD_q3LPT"),
    ("3LPT at 2048", dict(q2LPT=1, q3LPT=1, ppd=2048), "PPD <= 1024"),
    ("3LPT terms", dict(q2LPT=1, q3LPT=1, lpt3_terms=9), "ZD_3LPT_terms"),
]


def _one_line(capfd, word):
    lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("zeldovich_hip: ") and word in lines[0], lines


@pytest.fixture(scope="module")
def lib_and_ps():
    import zeldovich_plt_amd.api as api
    return api, api.load_library(), api.PowerSpectrum.from_file(WMAP, BOX)


@pytest.mark.parametrize("name,kw,word", PARAM_REFUSALS, ids=[r[0] for r in PARAM_REFUSALS])
def test_parameters_are_refused_before_a_plan_or_the_gpu(lib_and_ps, capfd, name, kw, word):
    api, L, ps = lib_and_ps
    kw = dict(kw)
    p = api.make_params(kw.pop("ppd", 32), **kw)
    sites = np.zeros((1, 3), dtype=np.int64)
    out = np.zeros((1, 3, 6))
    capfd.readouterr()
    assert L.zd_lpt_direct_sum(C.byref(p), C.byref(ps.pk), 1, sites.ctypes.data, out.ctypes.data) != 0
    _one_line(capfd, word)
    nb = api.power_nbins(p.ppd, 1)
    count, sums = np.zeros(nb, dtype=np.int64), np.zeros((nb, 8))
    assert L.zd_lpt_power(C.byref(p), C.byref(ps.pk), 1, nb, count.ctypes.data, sums.ctypes.data) != 0
    _one_line(capfd, word)
    with pytest.raises(RuntimeError):
        api.lpt_direct_sum(p, ps, [(0, 0, 0)])
    with pytest.raises(RuntimeError):
        api.lpt_power(p, ps)
    capfd.readouterr()


def test_site_and_bin_arguments_are_refused_before_a_plan_or_the_gpu(lib_and_ps, capfd):
    api, L, ps = lib_and_ps
    p = api.make_params(32, **ON)
    out = np.zeros((65, 3, 6))
    ok = np.zeros((65, 3), dtype=np.int64)
    capfd.readouterr()

    def ds(nsites, sites, outp):
        return L.zd_lpt_direct_sum(C.byref(p), C.byref(ps.pk), nsites, sites, outp)

    for nsites, word in ((0, "1 to 64"), (-3, "1 to 64"), (65, "1 to 64")):
        assert ds(nsites, ok.ctypes.data, out.ctypes.data) != 0
        _one_line(capfd, word)
    for bad in ((0, 0, 32), (0, 32, 0), (32, 0, 0), (-1, 0, 0)):
        s = np.array([(1, 2, 3), bad], dtype=np.int64)
        assert ds(2, s.ctypes.data, out.ctypes.data) != 0
        _one_line(capfd, "outside the lattice")
    assert ds(1, None, out.ctypes.data) != 0
    _one_line(capfd, "array")
    assert ds(1, ok.ctypes.data, None) != 0
    _one_line(capfd, "array")
    assert L.zd_lpt_direct_sum(None, C.byref(ps.pk), 1, ok.ctypes.data, out.ctypes.data) != 0
    _one_line(capfd, "parameters")
    assert L.zd_plan_lpt_direct_sum(None, 1, ok.ctypes.data, out.ctypes.data, None) != 0
    _one_line(capfd, "plan")

    nb = api.power_nbins(32, 1)
    count, sums = np.zeros(nb, dtype=np.int64), np.zeros((nb, 8))

    def pw(width, nbins, cp, sp):
        return L.zd_lpt_power(C.byref(p), C.byref(ps.pk), width, nbins, cp, sp)

    for width, nbins in ((0, nb), (-2, nb), (1, nb - 1), (1, 0)):
        assert pw(width, nbins, count.ctypes.data, sums.ctypes.data) != 0
        _one_line(capfd, "zd_power_nbins")
    assert pw(1, nb, None, sums.ctypes.data) != 0
    _one_line(capfd, "array")
    assert pw(1, nb, count.ctypes.data, None) != 0
    _one_line(capfd, "array")
    assert L.zd_lpt_power(C.byref(p), None, 1, nb, count.ctypes.data, sums.ctypes.data) != 0
    _one_line(capfd, "power spectrum")
    assert L.zd_plan_lpt_power(None, 1, nb, count.ctypes.data, sums.ctypes.data, None) != 0
    _one_line(capfd, "plan")
    # the Python layer checks the site array itself, as for direct_sum
    for sites in ([], [[0, 0, 32]], [[0, 0, 0]] * 65, [[0.5, 0, 0]]):
        with pytest.raises(ValueError):
            api.lpt_direct_sum(p, ps, sites)
    with pytest.raises(ValueError):
        api.lpt_power(p, ps, bin_width=0)
