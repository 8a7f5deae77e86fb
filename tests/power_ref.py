"""numpy restatement of the band-power measurement (csrc/zd_kernels_pk.hip, zd_measure_power), applied to the oracle's mode
cubes: integer |k| shells, sums over the whole cube (Hermitian pairs twice) restricted to the modes the zero rule leaves alive.
Sums are accumulated in long double so that the check's own rounding stays below the bounds it is used with."""
import ctypes as C
import math

import numpy as np


def ksigned(n):
    idx = np.arange(n)
    return np.where(idx > n // 2, idx - n, idx).astype(np.int64)


def k2_cube(n):
    """integer kx^2 + ky^2 + kz^2 in the oracle's cube order [ky][kz][kx]"""
    k = ksigned(n)
    return (k[:, None, None] ** 2 + k[None, :, None] ** 2 + k[None, None, :] ** 2).astype(np.int64)


def nbins(n, w):
    """bins (b w)^2 <= k2 < ((b + 1) w)^2 that hold every mode of the cube"""
    return math.isqrt(3 * (n // 2) ** 2) // w + 1


def bin_cube(n, w):
    k2 = k2_cube(n)
    s = np.floor(np.sqrt(k2.astype(np.float64))).astype(np.int64)
    s = np.where(s * s > k2, s - 1, s)
    s = np.where((s + 1) * (s + 1) <= k2, s + 1, s)
    b = s // w
    assert np.all((b * w) ** 2 <= k2) and np.all(k2 < ((b + 1) * w) ** 2)
    return b


def alive_mask(D):
    """modes the zero rule leaves alive = modes of the oracle's cube that carry a draw; the origin is excluded"""
    m = D != 0
    m[0, 0, 0] = False
    return m


def binsum(vals, bins, mask, nb):
    """per-bin sums of vals over mask, in long double"""
    v = np.asarray(vals)[mask].astype(np.longdouble)
    b = bins[mask]
    order = np.argsort(b, kind="stable")
    v, b = v[order], b[order]
    out = np.zeros(nb, dtype=np.longdouble)
    if b.size:
        ub, start = np.unique(b, return_index=True)
        out[ub] = np.add.reduceat(v, start)
    return out


def hermitian_parts(A):
    """A = f + i g with f, g Hermitian cubes: f = (A(k) + conj A(-k)) / 2, g = (A(k) - conj A(-k)) / 2i"""
    n = A.shape[0]
    neg = (-np.arange(n)) % n
    Am = np.conj(A[neg][:, neg][:, :, neg])
    return (A + Am) / 2, (A - Am) / 2j


def input_power_cube(oracle, pk, n, boxsize):
    """PowerSpectrum::power at |k| = sqrt(k2 fundamental^2) of every mode (0 at the origin)"""
    fund = 2.0 * np.pi / boxsize
    k2 = k2_cube(n)
    uniq, inv = np.unique(k2, return_inverse=True)
    L = oracle.lib()
    P = np.array([0.0 if u == 0 else L.zdo_power(C.byref(pk), float(np.sqrt(float(u) * (fund * fund)))) for u in uniq])
    return P[inv].reshape(k2.shape)


def reference_sums(oracle, pk, n, boxsize, D, w=1, mask=None):
    """count, sum_k, sum_dens, sum_input of the density cube D [ky][kz][kx]"""
    nb = nbins(n, w)
    bins = bin_cube(n, w)
    m = alive_mask(D) if mask is None else mask
    fund = 2.0 * np.pi / boxsize
    return dict(count=np.bincount(bins[m], minlength=nb).astype(np.int64),
                sum_k=binsum(np.sqrt(k2_cube(n).astype(np.longdouble)) * np.longdouble(fund), bins, m, nb),
                sum_dens=binsum(D.real.astype(np.longdouble) ** 2 + D.imag.astype(np.longdouble) ** 2, bins, m, nb),
                sum_input=binsum(input_power_cube(oracle, pk, n, boxsize), bins, m, nb))


def close(got, want, tol):
    """|got - want| <= tol * want per bin (want >= 0)"""
    got = np.asarray(got, dtype=np.longdouble)
    return bool(np.all(np.abs(got - want) <= tol * np.abs(want)))


def worst(got, want):
    got = np.asarray(got, dtype=np.longdouble)
    nz = want != 0
    return float(np.max(np.abs(got[nz] - want[nz]) / np.abs(want[nz]))) if nz.any() else 0.0
