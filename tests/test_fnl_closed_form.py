"""The closed form of a one-mode ZD_f_NL run (tests/fnl_closed_form.py) against the CPU oracle on every record: this pins the
reference that test_gpu_fnl_closed_form.py uses at sizes the oracle cannot reach to the oracle, and through it to the reference's
arithmetic, on every edge the GPU cases rely on."""
import ctypes as C

import numpy as np
import pytest

import fnl_closed_form as F
from conftest import WMAP

TOL = 1e-13  # measured <= 2e-15 with glibc's libm; the margin is for other libm builds
NS, OM = 0.96, 0.31
PLT = dict(qPLT=1, qPLTrescale=1, PLT_target_z=5.0, f_cluster=0.97)

# (PPD, k0, f_NL or the sign s of the chooser, further parameters, note)
CASES = [
    (32, (3, 5, -7), 2.0e4, {}, "generic"),
    (32, (3, 9, -7), 2.0e4, {}, "2 ky wraps into the conjugate half"),
    (32, (3, 8, -7), 2.0e4, {}, "2 ky = N/2: the second wave vanishes"),
    (32, (8, 5, 3), 2.0e4, {}, "2 kx = N/2: Nyquist plane live in the second pass"),
    (32, (3, 5, 8), 2.0e4, {}, "2 kz = N/2"),
    (32, (-8, 5, -8), "+", {}, "2 kx = 2 kz = -N/2 wrap to +N/2"),
    (32, (-3, 0, 5), 2.0e4, {}, "ky = 0 plane"),
    (64, (5, 7, -9), 2.0e4, dict(k_cutoff=2.0), "k1 outside the cutoff sphere"),
    (64, (7, 3, -6), "+", dict(k_cutoff=2.0), "k1 beyond kmax, waves of equal size"),
    (32, (3, 5, -7), -1.5e6, {}, "negative f_NL, second wave 0.6 of the first"),
    (32, (3, 5, -7), "+", {}, "f_NL from the chooser: waves of equal size"),
    (32, (3, 9, -7), "-", {}, "chooser, s = -1"),
    (32, (3, 8, -7), "+", {}, "chooser, 2 ky = N/2"),
    (48, (5, 7, -11), "+", {}, ""),
    (64, (-13, 9, 21), "-", {}, ""),
    (96, (-20, 15, 33), "+", {}, ""),
    (32, (3, 5, -7), "+", dict(PLT), "PLT + rescale: each wave its own eigenmode"),
    (48, (5, 13, -11), "-", dict(PLT), "PLT, 2 ky wraps: the eigenmode of -k1"),
    (64, (5, 7, -9), "+", dict(PLT, k_cutoff=2.0), "PLT, k_cutoff = 2"),
]


def setup_case(oracle, n, k0, f, kw):
    """(opk, op, eig) of a case; f: a number, or '+' / '-' for choose_f_nl with s = +1 / -1"""
    opk = oracle.pk_from_file(WMAP, 720.0)
    oracle.lib().zdo_pk_set_primordial(C.byref(opk), NS)
    eig = oracle.synthetic_eigenmodes(24) if kw.get("qPLT") else None
    mk = lambda f_: oracle.make_params(n, numblock=2, icformat="RVdoubleZel", qonemode=1, one_mode=k0, f_NL=f_, n_s=NS, Omega_M=OM, **kw)
    if isinstance(f, str):
        f = F.choose_f_nl(oracle, opk, mk(1.0), k0, s=1 if f == "+" else -1)
    return opk, mk(f), eig


@pytest.mark.parametrize("n,k0,f,kw,note", CASES, ids=["%d-%s-%s%s" % (n, "_".join(map(str, k0)), f, "".join("-%s=%s" % i for i in kw.items()))
                                                      for n, k0, f, kw, _ in CASES])
def test_closed_form_equals_the_oracle(oracle, n, k0, f, kw, note):
    """every record of the oracle's run against two_waves, per component of d and v to 1e-13 of the largest component; max_disp
    (magnitudes: a plane wave ties) and density_variance too"""
    opk, op, eig = setup_case(oracle, n, k0, f, kw)
    ref = oracle.run(op, opk, eig=eig, eig_ppd=0 if eig is None else eig.shape[0])
    idx = np.arange(n)
    want = F.two_waves(oracle, opk, op, k0, (idx[:, None, None], idx[None, :, None], idx[None, None, :]), eig=eig)
    ratio = abs(want["D1"]) / abs(want["D0"])
    if isinstance(f, str):
        assert want["D1"] == 0 or abs(ratio - 1) < 1e-12
    if "N/2: the second wave" in note or "chooser, 2 ky" in note:
        assert want["D1"] == 0
    else:
        assert ratio > 1e-3, ratio
    errs = {}
    for fld in ("d", "v"):
        scale = np.abs(want[fld]).max()
        assert scale > 0
        errs[fld] = max(np.abs(ref["records"][fld][..., c] - want[fld][..., c]).max() / scale for c in range(3))
    errs["max_disp"] = np.abs(np.abs(ref["max_disp"]) - want["max_disp"]).max() / want["max_disp"].max()
    errs["variance"] = abs(ref["density_variance"] - want["density_variance"]) / want["density_variance"]
    print("PPD %3d k0 %-14s k1 %-14s f_NL %+.4e |D1/D0| %.3g  d %.1e v %.1e max_disp %.1e variance %.1e  %s"
          % (n, k0, want["k1"], op.f_NL, ratio, errs["d"], errs["v"], errs["max_disp"], errs["variance"], note))
    assert all(e <= TOL for e in errs.values()), errs


@pytest.mark.parametrize("k0", [(3, 0, -7), (3, 0, 7), (-3, 0, -7), (-3, 0, 0), (3, -5, 7), (16, 5, 3), (0, 0, 0), (12, 12, 12)])
def test_modes_outside_the_form_are_refused(k0):
    """ky = 0 on the half of the plane the reference's Hermitian fix overwrites, ky < 0 (never drawn), modes the zero rule removes"""
    with pytest.raises(ValueError):
        F.check_mode(32, k0)
