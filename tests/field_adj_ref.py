"""numpy restatement of the adjoint of a field run (definition: zeldovich_plt_amd/csrc/zd_kernels_field_adj.hip), for the tests of
field_vjp.  tests/test_field_adj.py pins it to field_ref.displace through the dot-product identity.

Conventions are field_ref's: arrays [z][y][x], fftn the forward sum, components in the records' order (q_z, q_y, q_x).  With
D = alive A fftn(a), q_j = N^3 ifftn(i s_j D).real, v_j = N^3 ifftn(i f s_j D).real, dens = N^3 ifftn(D).real, the adjoint of the
cotangents (g_q, g_v, g_dens) is
    H = alive A [ sum_j conj(i s_j) (fftn(g_q,j) + f fftn(g_v,j)) + fftn(g_dens) ],     abar = N^3 ifftn(H).real
The mask, the winners, the mirror and the oracle's eigenmode lookup are the ones field_ref.displace uses."""
import ctypes as C

import numpy as np

import field_ref


def coefficients(params, eig=None, oracle=None):
    """(alive, [s_z, s_y, s_x], f) on the whole FFT grid, exactly as field_ref.displace forms them (f a number for ZA)"""
    n = int(params.ppd)
    alive = field_ref.alive_mask(params)
    kz, ky, kx = field_ref._grid(n)
    k2i = kx * kx + ky * ky + kz * kz
    ik2 = 1.0 / (np.where(k2i > 0, k2i, 1) * params.fundamental ** 2)
    if not params.qPLT:
        s = [k * params.fundamental * ik2 for k in (kz, ky, kx)]
        return alive, s, (np.sqrt(1.0 + 24 * params.f_cluster) - 1) * .25
    L = oracle.lib()
    eig = np.ascontiguousarray(eig, dtype=np.float64)
    win = field_ref.winners(n) & alive
    e4 = np.zeros((n, n, n, 4))
    out = (C.c_double * 4)()
    for z, y, x in zip(*np.nonzero(win)):
        L.zdo_get_eigenmode(eig.ctypes.data, eig.shape[0], int(kx[z, y, x]), int(ky[z, y, x]), int(kz[z, y, x]), n, 1, out)
        e4[z, y, x] = out[:]
    f = (np.sqrt(1.0 + 24 * e4[..., 3] * params.f_cluster) - 1) * .25
    rescale = np.ones_like(f)
    if params.qPLTrescale:
        target_f = (np.sqrt(1.0 + 24 * params.f_cluster) - 1) / 4.
        rescale = ((1. / (1 + params.PLT_target_z)) / (1. / (1 + params.z_initial))) ** (target_f - f)
    s = [np.where(win, rescale * e4[..., j] * params.fundamental * ik2, 0.0) for j in (2, 1, 0)]
    s = [sj - field_ref._mirror(sj) for sj in s]
    f = np.where(win, f, 0.0)
    return alive, s, f + field_ref._mirror(f)


def amplitude(params, kind="density", ps=None):
    """A(|k|^2) on the FFT grid: 1 / N^3, or sqrt(power(|k|) / N^3) for white noise (field_ref.white_to_density's table)"""
    n = int(params.ppd)
    if kind == "density":
        return np.full((n, n, n), 1.0 / n ** 3)
    kz, ky, kx = field_ref._grid(n)
    k2i = kx * kx + ky * ky + kz * kz
    vals, inv = np.unique(k2i, return_inverse=True)
    amp = np.array([np.sqrt(ps.power(np.sqrt(float(v) * params.fundamental ** 2)) / n ** 3) if v > 0 else 0.0 for v in vals])
    return amp[inv.reshape(k2i.shape)]


def vjp(params, g_q=None, g_v=None, g_dens=None, kind="density", ps=None, eig=None, oracle=None, with_residue=False):
    """abar, float64 [z][y][x]; with_residue: also max|Im N^3 ifftn(H)|, which the Hermitian symmetry of H makes round-off"""
    n = int(params.ppd)
    alive, s, f = coefficients(params, eig=eig, oracle=oracle)
    H = np.zeros((n, n, n), dtype=np.complex128)
    for j in range(3):
        G = np.zeros((n, n, n), dtype=np.complex128)
        if g_q is not None:
            G += np.fft.fftn(np.asarray(g_q, dtype=np.float64)[..., j])
        if g_v is not None:
            G += f * np.fft.fftn(np.asarray(g_v, dtype=np.float64)[..., j])
        H += np.conj(1j * s[j]) * G
    if g_dens is not None:
        H += np.fft.fftn(np.asarray(g_dens, dtype=np.float64))
    H *= alive * amplitude(params, kind, ps)
    full = np.fft.ifftn(H) * float(n) ** 3
    abar = np.ascontiguousarray(full.real)
    return (abar, np.abs(full.imag).max()) if with_residue else abar


def plane_wave_cotangent(n, m, phi, c, B, cv=None, Bv=0.0, xp=np, device=None, dtype=None):
    """g_q = B cos(theta) in component c (+ g_v = Bv cos(theta) in component cv), theta(x) = 2 pi m.x / n + phi with m = (m_x, m_y, m_z):
    (g_q, g_v or None), [z][y][x][3].  The phases go through integer arithmetic mod n; xp = torch (+ device) builds the arrays there,
    plane by plane, as field_ref.plane_waves builds its field."""
    mx, my, mz = m
    if xp is np:
        idx = np.arange(n, dtype=np.int64)
        r = (mz * idx[:, None, None] + my * idx[None, :, None] + mx * idx[None, None, :]) % n
        cos = np.cos(2.0 * np.pi * r / n + phi)
        g_q = np.zeros((n, n, n, 3), dtype=dtype or np.float64)
        g_q[..., c] = B * cos
        g_v = None
        if cv is not None:
            g_v = np.zeros((n, n, n, 3), dtype=dtype or np.float64)
            g_v[..., cv] = Bv * cos
        return g_q, g_v
    dtype = dtype or xp.float64
    idx = xp.arange(n, dtype=xp.int64, device=device)
    table = xp.cos(2.0 * np.pi * idx.to(xp.float64) / n + phi)  # the cosine of every phase residue
    mxy = (my * idx[:, None] + mx * idx[None, :]) % n
    g_q = xp.zeros((n, n, n, 3), dtype=dtype, device=device)
    g_v = xp.zeros((n, n, n, 3), dtype=dtype, device=device) if cv is not None else None
    for z in range(n):
        cos = table[(mxy + (mz * z) % n) % n]
        g_q[z, :, :, c] = (B * cos).to(dtype)
        if cv is not None:
            g_v[z, :, :, cv] = (Bv * cos).to(dtype)
    return g_q, g_v


def plane_wave_adjoint(n, m, phi, c, B, boxsize, sites, cv=None, Bv=0.0, f_cluster=1.0):
    """the ZA adjoint of plane_wave_cotangent on a density field, in closed form at the lattice sites [(z, y, x), ...]:
    abar = (B m_c + f Bv m_cv) sin(theta) / (|m|^2 fundamental), the components of m in the records' order (m_z, m_y, m_x)"""
    mx, my, mz = m
    rec = (mz, my, mx)
    fund = 2.0 * np.pi / boxsize
    f = (np.sqrt(1.0 + 24 * f_cluster) - 1) * .25
    s = np.asarray(sites, dtype=np.int64).reshape(-1, 3)
    theta = 2.0 * np.pi * ((mz * s[:, 0] + my * s[:, 1] + mx * s[:, 2]) % n) / n + phi
    amp = B * rec[c] + (f * Bv * rec[cv] if cv is not None else 0.0)
    return amp * np.sin(theta) / (float(mx * mx + my * my + mz * mz) * fund)
