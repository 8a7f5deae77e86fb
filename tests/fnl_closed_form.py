"""The closed form of a one-mode ZD_f_NL run (a helper of test_fnl_closed_form.py and test_gpu_fnl_closed_form.py, not a test).

ZD_qonemode = 1, ZD_one_mode = k0, ZD_f_NL = f: the phi pass holds one mode and its conjugate, phi(x) = 2 Re[phi0 e^{i k0.x}] with
phi0 = D0 / M(k0), so phi^2 = 2 |phi0|^2 + 2 Re[phi0^2 e^{2 i k0.x}].  The second pass takes D = PhiK * M on every mode but k = 0
(the zero rule and qonemode are bypassed there, src/zeldovich.cpp:393-400), so the run is exactly two plane waves:

    D(k0) = D0                                  the draw (zdo_mode_draw)
    D(k1) = f (D0 / M(k0))^2 M(k1)              k1 = 2 k0 wrapped into (-N/2, N/2] per axis; zero when |k1_y| = N/2 (the phi round
                                                zeroes that row, src/zeldovich.cpp:726-736); the k = 0 term is dropped
    M(k)  = 2 / (1 + z_initial) c^2 T(|k|) k^2 / (3 Omega_M H0^2),  T = zdo_infer_Tk after zdo_pk_set_primordial(n_s)

and each wave contributes d_j(x) = rescale e_j fund / k^2 (-2) (Re D sin t + Im D cos t), t = 2 pi (k.x mod N) / N, with e_j = k_j,
rescale = 1 and v = d (sqrt(1 + 24 f_cluster) - 1) / 4 without PLT; with PLT each wave takes the eigenmode and growth factor of
its own wavevector (zdo_get_eigenmode) and v = f(k) d per wave.

Everything here is float64 numpy on the oracle's per-mode pieces (the draw, T(k), the eigenmode table look-up); the phases are exact:
k.x mod N in integers, sin / cos from a table of N entries evaluated in long double.  Because k1 = 2 k0 (mod N), the field at a site
depends only on m = k0.x mod N, which is what makes max_disp and density_variance closed forms too."""
import ctypes as C
from math import gcd

import numpy as np

C_LIGHT, H0 = 299792.458, 100.0


def wrap(k, n):
    """k modulo n in (-n/2, n/2]"""
    k = int(k) % n
    return k - n if k > n // 2 else k


def check_mode(n, k0, k_cutoff=1.0):
    """refuse the one-mode wavevectors the form does not describe"""
    kx, ky, kz = (int(v) for v in k0)
    if ky < 0:
        raise ValueError("ky < 0 is never drawn (the generator walks the half space ky >= 0)")
    if ky == 0 and not (kx < 0 and kz > 0):
        # measured against the oracle: the reference's ky = 0 Hermitian fix keeps the draws of kz > 0 (kz = 0: kx > 0) and overwrites the
        # other half with conjugates, so a mode there vanishes, e.g. (3, 0, -7), (-3, 0, -7), (-3, 0, 0).  Only kx < 0, kz > 0 is taken.
        raise ValueError("ky = 0: the reference's Hermitian fix overwrites half of that plane; use kx < 0 and kz > 0")
    kmax = int(n // 2 / k_cutoff + .5)
    if max(abs(kx), abs(ky), abs(kz)) >= kmax or (kx * kx + ky * ky + kz * kz) >= (n / 2 / k_cutoff) ** 2:
        raise ValueError("k0 is removed by the zero rule")


def transfer_multiplier(oracle, opk, op, k):
    """M(k): phi = D / M (src/zeldovich.cpp:377-400)"""
    k2 = sum(int(c) * int(c) for c in k) * op.fundamental ** 2
    T = oracle.lib().zdo_infer_Tk(C.byref(opk), float(np.sqrt(k2)))
    return 2.0 * (1.0 / (1.0 + op.z_initial)) * C_LIGHT * C_LIGHT * T * k2 / (3.0 * op.Omega_M * H0 * H0)


def draw(oracle, opk, op, k0):
    r, D = (C.c_uint64 * 2)(), (C.c_double * 2)()
    oracle.lib().zdo_mode_draw(C.byref(op), C.byref(opk), int(k0[0]), int(k0[1]), int(k0[2]), r, D)
    return complex(D[0], D[1])


def choose_f_nl(oracle, opk, op, k0, s=1):
    """the f_NL that makes the second wave as large as the first: |D(k1)| = |D0|  <=>  f = s M(k0)^2 / (|D0| M(k1)), s = +-1.
    Built from the form alone; the code under test has no part in the number."""
    assert s in (1, -1)
    n = int(op.ppd)
    check_mode(n, k0, op.k_cutoff)
    k1 = tuple(wrap(2 * int(c), n) for c in k0)
    assert any(k1)
    M0, M1 = transfer_multiplier(oracle, opk, op, k0), transfer_multiplier(oracle, opk, op, k1)
    return s * M0 * M0 / (abs(draw(oracle, opk, op, k0)) * M1)


def _trig(n):
    """sin / cos of 2 pi m / N, m = 0 ... N - 1, evaluated in long double"""
    t = 2 * np.pi * np.arange(n, dtype=np.longdouble) / np.longdouble(n)
    return np.sin(t).astype(np.float64), np.cos(t).astype(np.float64)


class _Wave:
    """one plane wave: wavevector k (ky >= 0 half where an eigenmode is looked up), amplitude D, and its per-component factors"""

    def __init__(self, oracle, op, k, D, eig):
        n = int(op.ppd)
        self.k, self.D = tuple(int(c) for c in k), complex(D)
        k2 = sum(c * c for c in self.k) * op.fundamental ** 2
        if not op.qPLT:
            e = [float(c) for c in self.k]
            self.amp = [e[j] * op.fundamental / k2 for j in range(3)]  # j = x, y, z
            self.vfac = (np.sqrt(1 + 24 * op.f_cluster) - 1) / 4
            return
        kk, DD = self.k, self.D
        if kk[1] < 0:  # the generator looks the eigenmode up on the half space ky >= 0 and reflects: the same wave from -k, conj(D)
            kk, DD = tuple(-c for c in kk), DD.conjugate()
        self.k, self.D = kk, DD
        e = (C.c_double * 4)()
        oracle.lib().zdo_get_eigenmode(eig.ctypes.data, eig.shape[0], kk[0], kk[1], kk[2], n, 1, e)
        f = (np.sqrt(1 + 24 * e[3] * op.f_cluster) - 1) / 4
        rescale = 1.0
        if op.qPLTrescale:
            target_f = (np.sqrt(1 + 24 * op.f_cluster) - 1) / 4
            rescale = ((1 / (1 + op.PLT_target_z)) / (1 / (1 + op.z_initial))) ** (target_f - f)
        self.amp = [rescale * e[j] * op.fundamental / k2 for j in range(3)]
        self.vfac = f

    def at_residue(self, m, sin, cos):
        """-2 (Re D sin t + Im D cos t) at t = 2 pi m / N"""
        return -2.0 * (self.D.real * sin[m] + self.D.imag * cos[m])


def two_waves(oracle, opk, op, k0, sites, eig=None):
    """the run ZD_qonemode = 1, ZD_one_mode = k0 of `op` (oracle parameters: ppd, f_NL, n_s through opk, Omega_M, z_initial,
    f_cluster, k_cutoff, PLT settings) at the lattice sites (z, y, x) — integer arrays that broadcast against each other.
    Returns k1, D0, D1, d and v as float64 [..., 3] in the records' component order (qz, qy, qx), and max_disp (magnitudes, in
    (x, y, z) order like the library's) and density_variance over the whole lattice."""
    n = int(op.ppd)
    check_mode(n, k0, op.k_cutoff)
    k0 = tuple(int(c) for c in k0)
    k1 = tuple(wrap(2 * c, n) for c in k0)
    D0 = draw(oracle, opk, op, k0)
    M0, M1 = transfer_multiplier(oracle, opk, op, k0), transfer_multiplier(oracle, opk, op, k1)
    D1 = op.f_NL * (D0 / M0) ** 2 * M1
    if abs(k1[1]) == n // 2:
        D1 = 0j
    if op.qPLT and (k1[1] == 0 or n // 2 in (abs(k1[0]), abs(k1[2]))):
        raise ValueError("PLT: k1 on the ky = 0 or a Nyquist plane has no unique eigenmode look-up; not covered by the form")
    sin, cos = _trig(n)
    waves = [_Wave(oracle, op, k0, D0, eig), _Wave(oracle, op, k1, D1, eig)]
    z, y, x = (np.asarray(a, dtype=np.int64) for a in sites)
    shape = np.broadcast(z, y, x).shape
    d, v = np.zeros(shape + (3,)), np.zeros(shape + (3,))
    for w in waves:
        m = (w.k[0] * x + w.k[1] * y + w.k[2] * z) % n  # exact: |k.x| < 3 N^2 / 2
        s = w.at_residue(m, sin, cos)
        for j in range(3):
            d[..., 2 - j] += w.amp[j] * s
            v[..., 2 - j] += w.vfac * w.amp[j] * s
    # over the whole lattice: every wave's phase is a multiple of m0 = k0.x mod N (k1 = 2 k0 mod N; a reflected wave: -2 k0), and m0 takes
    # the multiples of g = gcd(k0, N), each the same number of times
    g = gcd(gcd(gcd(abs(k0[0]), abs(k0[1])), abs(k0[2])), n)
    m0 = np.arange(0, n, g, dtype=np.int64)
    mult = [1, 2 if waves[1].k == k1 else -2]
    res = [w.at_residue((c * m0) % n, sin, cos) for w, c in zip(waves, mult)]
    max_disp = np.array([np.abs(sum(w.amp[j] * r for w, r in zip(waves, res))).max() for j in range(3)])
    dens = sum(w.D.real * cos[(c * m0) % n] - w.D.imag * sin[(c * m0) % n] for w, c in zip(waves, mult)) * 2.0
    density_variance = float((dens * dens).sum()) * (float(n) ** 3 / len(m0))
    return dict(k1=k1, D0=D0, D1=D1, d=d, v=v, max_disp=max_disp, density_variance=density_variance)
