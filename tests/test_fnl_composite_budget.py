"""The stream-factor choice for ZD_f_NL on the composite grids (zd_choose_stream_factor: host code, no GPU needed) counts PhiK
beside every pass's store, and the phi round's peak before it: PhiK plus the phi planes (half-space rows on the composite
transforms, the full store on the convolution ones)."""
import ctypes as C

GB = 1 << 30
FNL = dict(f_NL=2.0e4, n_s=0.96, Omega_M=0.31)


def _R(n, budget_gb, **kw):
    import zeldovich_plt_amd.api as zd
    return zd.load_library().zd_choose_stream_factor(C.byref(zd.make_params(n, **kw)), 1, int(budget_gb * GB))


def test_fnl_2304_budget_counts_phik_and_the_phi_round():
    # PPD = 2304: PhiK 91 GiB; the phi round's half-space planes ~92 GiB; one pass of the two reference arrays ~368 GiB / R
    assert _R(2304, 270) == 2                       # ZA on its field store, nothing else resident
    assert _R(2304, 300, **FNL) == 2                # 184 GiB store + 91 GiB PhiK
    assert _R(2304, 270, **FNL) == 3                # R = 2 no longer fits beside PhiK; z lines of 768 = 256 * 3
    assert _R(2304, 190, **FNL) == 4                # the phi round (~183 GiB) still fits
    assert _R(2304, 180, **FNL) == -1               # the phi round does not: nothing runs, at any stream factor


def test_fnl_budget_on_the_convolution_path_counts_the_full_phi_store():
    # ZD_StoreMode = reference keeps the convolution transforms and the full phi store (16 N^3 bytes + PhiK 8 N^3): at PPD = 1728
    # 100 GiB holds the composite phi round (~40 + 38 GiB) but not that one (~80 + 38 GiB)
    assert _R(1728, 100, **FNL) == 3
    assert _R(1728, 100, store_mode="reference", **FNL) == -1
    assert _R(1728, 130, store_mode="reference", **FNL) == 2
    assert _R(1728, 200, **FNL) == 1
