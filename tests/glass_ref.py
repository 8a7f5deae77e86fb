"""The definition of zeldovich_plt_amd/csrc/zd_kernels_glass.hip in numpy: the delivered records of a run interpolated at arbitrary
positions (trilinear, or cubic Lagrange through four points per axis).  The reference of tests/test_glass.py and
tests/test_gpu_glass.py; test infrastructure only."""
import numpy as np


def weights(tau, order):
    """[order + 1, n] weights of the offsets 0, 1 (order 1) or -1, 0, 1, 2 (order 3) at tau [n]"""
    t = np.asarray(tau, dtype=np.float64)
    if order == 1:
        return np.stack([1.0 - t, t])
    if order == 3:
        return np.stack([-t * (t - 1.0) * (t - 2.0) / 6.0, (t + 1.0) * (t - 1.0) * (t - 2.0) / 2.0,
                         -(t + 1.0) * t * (t - 2.0) / 2.0, (t + 1.0) * t * (t - 1.0) / 6.0])
    raise ValueError("order must be 1 or 3")


def offsets(order):
    return np.arange(2) if order == 1 else np.arange(-1, 3)


def tiled(positions, tile):
    """the load replicated tile^3 times: particle ((a t + b) t + c) npart + i sits at (p_i + (c, b, a)) / t"""
    p = np.asarray(positions, dtype=np.float64)
    t = int(tile)
    a, b, c = np.meshgrid(np.arange(t), np.arange(t), np.arange(t), indexing="ij")
    off = np.stack([c.ravel(), b.ravel(), a.ravel()], axis=1).astype(np.float64)  # (x, y, z) offsets in index order
    return ((p[None, :, :] + off[:, None, :]) / float(t)).reshape(-1, 3)


def lattice(positions, n):
    """per axis: cell index mod n and tau of u = p n"""
    u = np.asarray(positions, dtype=np.float64) * float(n)
    i0 = np.floor(u)
    return i0.astype(np.int64) % n, u - i0


def fields_of_records(records):
    """float64 [n, n, n, 6] = qx, qy, qz, vx, vy, vz of records[z, y, x] (which hold (z, y, x) components); no velocity: zeros"""
    n = records.shape[0]
    out = np.zeros((n, n, n, 6), dtype=np.float64)
    out[..., :3] = records["d"][..., ::-1]
    if "v" in records.dtype.names:
        out[..., 3:] = records["v"][..., ::-1]
    return out


def interpolate(field, positions, order):
    """psi(p) = sum_z sum_y sum_x w_z w_y w_x field[z][y][x] for field [n, n, n, nq] at positions [npart, 3] of (x, y, z) in [0, 1)"""
    f = np.asarray(field, dtype=np.float64)
    n = f.shape[0]
    cell, tau = lattice(positions, n)
    wx, wy, wz = (weights(tau[:, a], order) for a in range(3))
    out = np.zeros((cell.shape[0], f.shape[-1]), dtype=np.float64)
    for kz, oz in enumerate(offsets(order)):
        z = (cell[:, 2] + oz) % n
        for ky, oy in enumerate(offsets(order)):
            y = (cell[:, 1] + oy) % n
            for kx, ox in enumerate(offsets(order)):
                x = (cell[:, 0] + ox) % n
                out += (wz[kz] * wy[ky] * wx[kx])[:, None] * f[z, y, x]
    return out
