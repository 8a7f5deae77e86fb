"""Second-order (2LPT) displacements in numpy: a restatement of steps 1-4 of the definition in
zeldovich_plt_amd/csrc/zd_kernels_lpt2.hip that starts from a delivered displacement field and uses nothing of the library.

Arrays are indexed [z, y, x] as the records are, and component a of a vector field is its component along array axis a — the order
of the `d` and `v` fields of a record (src/output.cpp:128-141: displ = (qz, qy, qx)).  The construction is isotropic, so all that
matters is that component a goes with the wavenumber of axis a.
"""
import numpy as np


def wavenumbers(n):
    """signed integer wavenumbers of an axis, -n/2 < k <= n/2 (the generator's convention: index n/2 is +n/2)"""
    k = np.arange(n)
    return np.where(k > n // 2, k - n, k)


def alive_mask(n, boxsize, k_cutoff=1.0, corner_modes=0):
    """the modes the zero rule of src/zeldovich.cpp:350-353 leaves alive, k = 0 excluded: bool [n, n, n]"""
    k = wavenumbers(n)
    kz, ky, kx = np.meshgrid(k, k, k, indexing="ij")
    kmax = int((n // 2) * (1.0 / k_cutoff) + .5)
    fundamental = 2.0 * np.pi / boxsize
    nyquist = np.pi / (boxsize / n)
    dead = (np.abs(kx) == kmax) | (np.abs(ky) == kmax) | (np.abs(kz) == kmax)
    k2i = kx * kx + ky * ky + kz * kz
    if not corner_modes:
        dead |= k2i.astype(np.float64) * (fundamental * fundamental) >= nyquist * nyquist / (k_cutoff * k_cutoff)
    dead |= k2i == 0
    return ~dead


def _kvec(n, boxsize):
    k = wavenumbers(n).astype(np.float64) * (2.0 * np.pi / boxsize)
    return [k[:, None, None], k[None, :, None], k[None, None, :]]


def source(q, boxsize):
    """steps 1, 2: S(x) = sum_{a<b} [psi_aa psi_bb - psi_ab^2] from q[z, y, x, 3], psi_ab(k) = i k_a F_b(k) with the Nyquist planes dead"""
    n = q.shape[0]
    assert q.shape == (n, n, n, 3)
    kv = _kvec(n, boxsize)
    nyq = np.ones((n, n, n), dtype=bool)
    for a in range(3):
        idx = [slice(None)] * 3
        idx[a] = n // 2
        nyq[tuple(idx)] = False
    F = [np.fft.fftn(q[..., b]) / n ** 3 * nyq for b in range(3)]  # q_b(x) = sum_k F_b(k) e^{+2 pi i k.x / N}

    def grad(a, b):  # unnormalised inverse transform, like q
        return np.real(np.fft.ifftn(1j * kv[a] * F[b]) * n ** 3)

    d = [grad(a, a) for a in range(3)]
    s = d[0] * d[1] + d[0] * d[2] + d[1] * d[2]
    for a in range(3):
        for b in range(a + 1, 3):
            s -= grad(a, b) ** 2
    return s


def second_order(q, boxsize, mask, lpt2_ratio=-3.0 / 7.0):
    """steps 1-4: psi2[z, y, x, 3] of the displacement field q[z, y, x, 3] (a ZA run's records); mask = alive_mask(...);
    gamma = -lpt2_ratio"""
    n = q.shape[0]
    kv = _kvec(n, boxsize)
    sk = np.fft.fftn(source(q, boxsize)) / n ** 3 * mask  # step 3
    sk[0, 0, 0] = 0.0
    k2 = kv[0] ** 2 + kv[1] ** 2 + kv[2] ** 2
    k2[0, 0, 0] = 1.0
    gamma = -lpt2_ratio
    out = np.empty(q.shape, dtype=np.float64)
    for j in range(3):
        out[..., j] = np.real(np.fft.ifftn(1j * kv[j] * gamma * sk / k2) * n ** 3)  # step 4
    return out


def default_coefficients(f_cluster):
    """(alpha, lpt2_ratio, f2) of the f_cluster-EdS background: alpha = (sqrt(1 + 24 f_cluster) - 1) / 4, D2 / D1^2 =
    -(2 alpha + 1) / (6 alpha + 1), f2 = 2 alpha"""
    alpha = (np.sqrt(1.0 + 24.0 * f_cluster) - 1.0) / 4.0
    return alpha, -(2 * alpha + 1) / (6 * alpha + 1), 2 * alpha
