"""The PLT eigenmode table in numpy / scipy: the definition in the header of csrc/zd_kernels_plt.hip, restated independently
(test yardstick only; tests/test_plt_eigen.py pins it, tests/test_gpu_plt_eigen.py measures the GPU against it).

Simple cubic lattice of spacing 1 under periodic gravity (Marcos et al. 2006), wavevector k = 2 pi m / n for signed integers m:

    D_ab(k) = delta_ab / 3 - S_ab(k) / (4 pi),      S_ab(k) = sum_{R != 0} cos(k.R) d_a d_b (1/r) at R

with S in its Ewald form, splitting parameter alpha, shells R, m' in [-s, s]^3:

    S_ab = sum_{R != 0} cos(k.R) [A(R) R_a R_b - B(R) delta_ab] + 4 alpha^3 / (3 sqrt pi) delta_ab
           - 4 pi sum_m' q_a q_b exp(-q^2 / 4 alpha^2) / q^2,     q = 2 pi m' + k
    A(R) = [3 erfc(alpha R) / R^3 + (2 alpha / sqrt pi) exp(-alpha^2 R^2) (3 / R^2 + 2 alpha^2)] / R^2
    B(R) = erfc(alpha R) / R^3 + (2 alpha / sqrt pi) exp(-alpha^2 R^2) / R^2

The mode of a wavevector: eigenvalues within 1e-9 of each other (chained) form one eigenspace; the eigenspace that carries the
largest projection of khat = m / |m| gives lambda (the mean of its eigenvalues) and e = that projection, normalised.  Entry
m = 0 is (0, 0, 0, 1).  Table layout: float64 [n][n][n/2 + 1][4] = (e_x, e_y, e_z, lambda), index i <-> m = i for i <= n/2
(index n/2 is +n/2), else i - n.
"""
import numpy as np
from scipy.special import erfc

ALPHA, SHELLS = 2.0, 4
GROUP_TOL = 1e-9

_shell_cache = {}


def _shells(alpha, s):
    """R != 0 in [-s, s]^3 with A(R), B(R); the reciprocal m' in [-s, s]^3"""
    key = (float(alpha), int(s))
    if key not in _shell_cache:
        r = np.arange(-s, s + 1)
        R = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
        M = R.copy()
        R = R[np.any(R != 0, axis=1)]
        d = np.sqrt((R * R).sum(1))
        g = 2.0 * alpha / np.sqrt(np.pi) * np.exp(-alpha * alpha * d * d)
        A = (3.0 * erfc(alpha * d) / d ** 3 + g * (3.0 / d ** 2 + 2.0 * alpha * alpha)) / d ** 2
        B = erfc(alpha * d) / d ** 3 + g / d ** 2
        _shell_cache[key] = (R, A, B, M)
    return _shell_cache[key]


def signed(i, n):
    """table index -> signed wavenumber: index n/2 is +n/2"""
    i = np.asarray(i)
    return np.where(i <= n // 2, i, i - n)


def matrix(m, n, alpha=ALPHA, shells=SHELLS):
    """D(k) (3 x 3) at k = 2 pi m / n; m need not be an integer vector (the fluid-limit test uses fractions through n)"""
    R, A, B, M = _shells(alpha, shells)
    k = 2.0 * np.pi * np.asarray(m, dtype=np.float64) / n
    c = np.cos(R @ k)
    S = np.einsum("i,ia,ib->ab", c * A, R, R) - np.eye(3) * np.sum(c * B)
    S += np.eye(3) * (4.0 * alpha ** 3 / (3.0 * np.sqrt(np.pi)))
    q = 2.0 * np.pi * M + k
    q2 = (q * q).sum(1)
    ok = q2 > 0
    w = np.exp(-q2[ok] / (4.0 * alpha * alpha)) / q2[ok]
    S -= 4.0 * np.pi * np.einsum("i,ia,ib->ab", w, q[ok], q[ok])
    return np.eye(3) / 3.0 - S / (4.0 * np.pi)


def six(D):
    """the six distinct elements in the order of zd_test_plt_matrix: xx, yy, zz, xy, xz, yz"""
    return np.array([D[0, 0], D[1, 1], D[2, 2], D[0, 1], D[0, 2], D[1, 2]])


def select(D, m):
    """(e[3], lambda, gap, margin, all eigenvalues): the selection rule; gap = distance from the chosen eigenspace to the nearest
    eigenvalue outside it (inf if there is none), margin = best minus second-best projection weight (the best one if alone)"""
    m = np.asarray(m, dtype=np.float64)
    khat = m / np.sqrt((m * m).sum())
    w, V = np.linalg.eigh(D)  # ascending
    groups, cur = [], [0]
    for i in (1, 2):
        if w[i] - w[i - 1] < GROUP_TOL:
            cur.append(i)
        else:
            groups.append(cur)
            cur = [i]
    groups.append(cur)
    p = V.T @ khat
    weight = [float((p[g] ** 2).sum()) for g in groups]
    best = int(np.argmax(weight))
    g = groups[best]
    e = V[:, g] @ p[g]
    e /= np.sqrt((e * e).sum())
    lam = float(np.mean(w[g]))
    others = [w[i] for i in range(3) if i not in g]
    gap = min(abs(lam - o) for o in others) if others else np.inf
    rest = sorted(weight[:best] + weight[best + 1:])
    margin = weight[best] - (rest[-1] if rest else 0.0)
    return e, lam, gap, margin, w


def mode(m, n, alpha=ALPHA, shells=SHELLS):
    return select(matrix(m, n, alpha, shells), m)


def table(n, alpha=ALPHA, shells=SHELLS, with_matrix=False):
    """the whole table [n][n][n/2+1][4], plus per mode the eigenvalue gap and the projection margin (and D's six elements)"""
    h = n // 2 + 1
    T = np.zeros((n, n, h, 4))
    gap = np.full((n, n, h), np.inf)
    margin = np.ones((n, n, h))
    D6 = np.zeros((n, n, h, 6)) if with_matrix else None
    for ix in range(n):
        for iy in range(n):
            for iz in range(h):
                m = (int(signed(ix, n)), int(signed(iy, n)), iz)
                if m == (0, 0, 0):
                    T[ix, iy, iz] = (0, 0, 0, 1)
                    if with_matrix:
                        D6[ix, iy, iz] = six(matrix(m, n, alpha, shells))
                    continue
                D = matrix(m, n, alpha, shells)
                e, lam, g, mg, _w = select(D, m)
                T[ix, iy, iz, :3] = e
                T[ix, iy, iz, 3] = lam
                gap[ix, iy, iz], margin[ix, iy, iz] = g, mg
                if with_matrix:
                    D6[ix, iy, iz] = six(D)
    return (T, gap, margin, D6) if with_matrix else (T, gap, margin)
