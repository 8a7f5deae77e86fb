"""The de-aliased second-order source (ZD_2LPT_dealias, step 2' of the definition in zeldovich_plt_amd/csrc/zd_kernels_lpt2.hip) in
numpy, in the style of tests/lpt2_ref.py: it starts from a delivered displacement field and uses nothing of the library.

Steps 1-3 run on the lattice of M = 3 N / 2 points per side: the modes of the N run (Nyquist planes dead) sit at their signed
wavenumbers in an M^3 cube, the gradients are inverse-transformed to M^3, S(x) is formed there, and of S(k) = fftn(S) / M^3 only
|k_i| < N/2 is kept.  A product of two modes with |k_i| < N/2 has |k_i| < N, which on 3 N / 2 points folds to |k_i| > N/2 only: what is
kept is exact.  Step 4 is lpt2_ref's, at N."""
import numpy as np

import lpt2_ref


def _embed_index(n, m):
    """index on the m lattice of every index of the n lattice with the same signed wavenumber (index n/2 maps to +n/2)"""
    return np.where(np.arange(n) > n // 2, np.arange(n) + (m - n), np.arange(n))


def source_k(q, boxsize):
    """S(k) on the N cube, scaled by M^-3, Nyquist planes of N zero: complex [n, n, n] from q[z, y, x, 3]"""
    n = q.shape[0]
    assert q.shape == (n, n, n, 3) and n % 2 == 0
    m = 3 * n // 2
    idx = _embed_index(n, m)
    sel = np.ix_(idx, idx, idx)
    nyq = np.ones((n, n, n), dtype=bool)
    for a in range(3):
        cut = [slice(None)] * 3
        cut[a] = n // 2
        nyq[tuple(cut)] = False
    km = lpt2_ref.wavenumbers(m).astype(np.float64) * (2.0 * np.pi / boxsize)
    kv = [km[:, None, None], km[None, :, None], km[None, None, :]]
    F = []
    for b in range(3):
        big = np.zeros((m, m, m), dtype=np.complex128)
        big[sel] = np.fft.fftn(q[..., b]) / n ** 3 * nyq
        F.append(big)

    def grad(a, b):  # unnormalised inverse transform to M^3
        return np.real(np.fft.ifftn(1j * kv[a] * F[b]) * m ** 3)

    d = [grad(a, a) for a in range(3)]
    s = d[0] * d[1] + d[0] * d[2] + d[1] * d[2]
    for a in range(3):
        for b in range(a + 1, 3):
            s -= grad(a, b) ** 2
    return (np.fft.fftn(s) / m ** 3)[sel] * nyq


def second_order(q, boxsize, mask, lpt2_ratio=-3.0 / 7.0):
    """steps 1, 2', 3, 4: psi2[z, y, x, 3] of the displacement field q (a ZA run's records); mask = lpt2_ref.alive_mask(...)"""
    n = q.shape[0]
    kv = lpt2_ref._kvec(n, boxsize)
    sk = source_k(q, boxsize) * mask
    sk[0, 0, 0] = 0.0
    k2 = kv[0] ** 2 + kv[1] ** 2 + kv[2] ** 2
    k2[0, 0, 0] = 1.0
    gamma = -lpt2_ratio
    out = np.empty(q.shape, dtype=np.float64)
    for j in range(3):
        out[..., j] = np.real(np.fft.ifftn(1j * kv[j] * gamma * sk / k2) * n ** 3)
    return out
