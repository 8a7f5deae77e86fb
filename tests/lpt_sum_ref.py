"""The per-order amplitudes and sums of zeldovich_plt_amd/csrc/zd_kernels_lpt_ds.hip restated in numpy.

Conventions of tests/lpt2_ref.py and tests/lpt3_ref.py: cubes are indexed [z, y, x], component a of a vector goes with the wavenumber
of array axis a (0 = z, 1 = y, 2 = x: the order of the `d` and `v` fields of a record), and eps_ijk is taken in that order of the
axes.  The library labels the components (x, y, z); psi3 holds two cross products, so it is the same vector either way.
"""
import numpy as np

import lpt2_ref
import lpt3_ref
import power_ref


def s_vectors(n, boxsize):
    """s_a = k_a / k^2 in physical units (= k_a fundamental / k^2 of the kernels with k^2 in physical units), 0 at k = 0: three cubes"""
    kv = lpt2_ref._kvec(n, boxsize)
    k2 = lpt3_ref._k2(kv)
    s = [np.broadcast_to(kv[a] / k2, (n, n, n)).copy() for a in range(3)]
    for a in range(3):
        s[a][0, 0, 0] = 0.0
    return s


def spectra(q, boxsize, mask, g3a, g3b):
    """what an LPT plan keeps resident, from the first-order field q[z, y, x, 3]: D(k), S(k), P3(k), [C_0, C_1, C_2](k) — the masked
    forward transforms (N^-3) of the sources lpt3_ref.sources forms"""
    n = q.shape[0]
    s3a, s3b, c, sk = lpt3_ref.sources(q, boxsize, mask)

    def spectrum(f):
        fk = np.fft.fftn(f) / n ** 3 * mask
        fk[0, 0, 0] = 0.0
        return fk

    return lpt3_ref.first_order_modes(q, boxsize) * mask, sk, spectrum(g3a * s3a + g3b * s3b), [spectrum(ci) for ci in c]


def amplitudes(dk, sk, p3k, ck, boxsize, mask, gamma, g3c):
    """Q1, Q2, Q3: per order the three cubes Q_a(k) of the definition; orders 2 and 3 restricted to the alive mask"""
    n = dk.shape[0]
    s = s_vectors(n, boxsize)
    q1 = [s[a] * dk for a in range(3)]
    q2 = [s[a] * gamma * sk * mask for a in range(3)]
    q3 = []
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        q3.append((s[i] * p3k - g3c * (s[j] * ck[k] - s[k] * ck[j])) * mask)  # s_i P3 + T_i, T = -g3c (s x C)
    return q1, q2, q3


def direct_sum_everywhere(Q):
    """field(x) = sum_k i Q(k) e^{+2 pi i k.x / N} at every lattice site, summed the way the kernel does: the half-space rows
    1 <= ky < N/2 stand for themselves and their Hermitian twins (2 Re), the plane ky = 0 is summed position by position (Re); the row
    ky = N/2 is not read.  Plain matrix products with the N x N phase table, no FFT."""
    n = Q.shape[0]
    idx = np.arange(n)
    W = np.exp(2j * np.pi * np.outer(idx, idx) / n)  # W[x, k] (indices stand for wavenumbers: they agree mod N)
    half = Q[:, :n // 2, :].copy()
    half[:, 1:, :] *= 2.0
    t = np.einsum("zk,kyx->zyx", W, 1j * half)           # z
    t = np.einsum("xk,zyk->zyx", W, t)                   # x
    return np.real(np.einsum("yk,zkx->zyx", W[:, :n // 2], t))  # y over the half space


def binned(cubes, mask, w=1):
    """sum over the alive modes of a bin of sum_a |cube_a|^2, in long double"""
    n = cubes[0].shape[0]
    p = sum(np.abs(c.astype(np.complex128)) ** 2 for c in cubes)
    return power_ref.binsum(p, power_ref.bin_cube(n, w), mask, power_ref.nbins(n, w))


def binned_field(field, mask, w=1):
    """the same of the transform of a real vector field[z, y, x, 3] (N^-3: the amplitudes of its unnormalised inverse transform)"""
    n = field.shape[0]
    return binned([np.fft.fftn(field[..., a]) / n ** 3 for a in range(3)], mask, w)
