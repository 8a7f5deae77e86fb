"""numpy restatement of a run on a caller-supplied field (definition: zeldovich_plt_amd/csrc/zd_kernels_field.hip), for the tests of
generate_field / Plan.from_field.  tests/test_field.py pins it to the oracle's records.

Conventions.  Fields are [z][y][x]; numpy's fftn is the forward sum (exp(-i)), the path's transforms are the unnormalised exp(+i) sums,
so D(k) = fftn(a) / N^3 and a field is N^3 ifftn(F).real.  Signed integer wavenumbers with N/2 kept as +N/2.  Displacements and
velocities come back as float64 [z][y][x][3] in the component order of the records' "d" and "v" members: (q_z, q_y, q_x).
`params` is any parameter object with the reference's members (api.make_params or the oracle's make_params)."""
import ctypes as C

import numpy as np


def wavenumbers(n):
    idx = np.arange(n)
    return np.where(idx > n // 2, idx - n, idx)


def _grid(n):
    k = wavenumbers(n)
    return np.meshgrid(k, k, k, indexing="ij")  # kz, ky, kx of [z][y][x]


def _corner_modes(params):
    return int(getattr(params, "corner_modes", getattr(params, "CornerModes", 0)))


def _mirror(a):
    """a(-k) on the FFT grid"""
    return np.roll(a[::-1, ::-1, ::-1], 1, axis=(0, 1, 2))


def winners(n):
    """the half space whose modes the path reads (ky > 0; on ky = 0: kz > 0; on ky = kz = 0: kx > 0); every other mode is the
    conjugate of its mirror image (src/zeldovich.cpp:485-503)"""
    kz, ky, kx = _grid(n)
    return (ky > 0) | ((ky == 0) & ((kz > 0) | ((kz == 0) & (kx > 0))))


def alive_mask(params):
    """The zero rule (src/zeldovich.cpp:350-356) on the whole FFT grid, bool [kz][ky][kx]: dead are the |k_i| = kmax planes,
    k^2 >= k^2_cutoff without CornerModes, every mode but ZD_one_mode with ZD_qonemode, k = 0, and the planes |k_i| = N/2 (which the
    rule clears by itself unless CornerModes meets k_cutoff != 1).  The rule is asked on the half space the path reads; the other
    half mirrors it."""
    n = int(params.ppd)
    half = n // 2
    kmax = int(float(half) * (1.0 / params.k_cutoff) + .5)
    kz, ky, kx = _grid(n)
    k2i = kx * kx + ky * ky + kz * kz
    dead = (np.abs(kx) == kmax) | (np.abs(ky) == kmax) | (np.abs(kz) == kmax) | (k2i == 0)
    dead |= (np.abs(kx) == half) | (np.abs(ky) == half) | (np.abs(kz) == half)
    if not _corner_modes(params):
        k2_cutoff = params.nyquist * params.nyquist / (params.k_cutoff * params.k_cutoff)
        dead |= k2i.astype(np.float64) * (params.fundamental * params.fundamental) >= k2_cutoff
    if params.qonemode:
        om = [int(c) for c in params.one_mode]
        dead |= ~((kx == om[0]) & (ky == om[1]) & (kz == om[2]))
    alive = ~dead
    return np.where(winners(n), alive, _mirror(alive))


def _fields(F):
    """real field of the spectrum F (the path's unnormalised exp(+i) sum)"""
    return np.ascontiguousarray(np.fft.ifftn(F).real) * F.size


def displace(delta, params, eig=None, oracle=None):
    """What a field run makes of the density field delta [z][y][x]: (q, v, masked density), float64; q and v [z][y][x][3] in the
    records' order (q_z, q_y, q_x).  ZA: q_j(k) = i k_j D / k^2, v = vnorm q with the vnorm of src/output.cpp:78-82.  PLT (params.qPLT,
    eig = the eigenmode table, oracle = the oracle module): q_j(k) = i rescale e_j D / (k^2 / fundamental ...) as src/zeldovich.cpp:
    403-434 forms it, the eigenmode of a half-space mode from the oracle's lookup, v_j = f q_j mode by mode."""
    n = int(params.ppd)
    delta = np.asarray(delta, dtype=np.float64)
    assert delta.shape == (n, n, n)
    alive = alive_mask(params)
    D = np.fft.fftn(delta) / delta.size * alive
    kz, ky, kx = _grid(n)
    k2i = kx * kx + ky * ky + kz * kz
    ik2 = 1.0 / (np.where(k2i > 0, k2i, 1) * params.fundamental ** 2)
    if not params.qPLT:
        s = [k * params.fundamental * ik2 for k in (kz, ky, kx)]  # records' order
        f = (np.sqrt(1.0 + 24 * params.f_cluster) - 1) * .25
    else:
        L = oracle.lib()
        eig = np.ascontiguousarray(eig, dtype=np.float64)
        win = winners(n) & alive
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
        s = [np.where(win, rescale * e4[..., j] * params.fundamental * ik2, 0.0) for j in (2, 1, 0)]  # e = (e_x, e_y, e_z)
        s = [sj - _mirror(sj) for sj in s]  # the mirrored mode is the conjugate copy: s(-k) = -s(k), f(-k) = f(k)
        f = np.where(win, f, 0.0)
        f = f + _mirror(f)
    q = np.stack([_fields(1j * sj * D) for sj in s], axis=-1)
    v = np.stack([_fields(1j * f * sj * D) for sj in s], axis=-1)
    return q, v, _fields(D)


def white_to_density(w, ps, params):
    """the density field whose modes are W(k) sqrt(power(|k|) / N^3), W the unnormalised forward sum of the white-noise field w
    (ps: anything with .power(k))"""
    n = int(params.ppd)
    w = np.asarray(w, dtype=np.float64)
    kz, ky, kx = _grid(n)
    k2i = kx * kx + ky * ky + kz * kz
    vals, inv = np.unique(k2i, return_inverse=True)
    amp = np.array([np.sqrt(ps.power(np.sqrt(float(v) * params.fundamental ** 2)) / w.size) if v > 0 else 0.0 for v in vals])
    return _fields(np.fft.fftn(w) * amp[inv.reshape(k2i.shape)])


def delta_from_za(records, boxsize):
    """the density whose Zel'dovich displacement the records are: -div q, spectrally (Nyquist planes, which carry nothing, zeroed)"""
    q = np.asarray(records["d"], dtype=np.float64)
    n = q.shape[0]
    fund = 2.0 * np.pi / boxsize
    ks = list(_grid(n))  # kz, ky, kx = the records' component order
    Dk = np.zeros((n, n, n), dtype=np.complex128)
    for j in range(3):
        Dk -= 1j * ks[j] * fund * np.fft.fftn(q[..., j])
    for k in ks:
        Dk[np.abs(k) == n // 2] = 0.0
    return np.ascontiguousarray(np.fft.ifftn(Dk).real)


def plane_waves(n, waves, boxsize, sites, f_cluster=1.0, xp=np, device=None):
    """A field of a few cosine waves, a(x) = sum_w A_w cos(2 pi k_w.x / n + phi_w) with waves = [((kx, ky, kz), A, phi), ...], and its
    Zel'dovich displacement in closed form at the lattice sites [(z, y, x), ...]: q_j = -sum_w A_w k_j sin(theta_w) / (k_w^2
    fundamental).  Returns (field [z][y][x] float64, q [nsites][3], v [nsites][3]) — q, v in the records' order (q_z, q_y, q_x).
    xp = torch (+ device) builds the field there, plane by plane; the phases go through integer arithmetic mod n either way."""
    fund = 2.0 * np.pi / boxsize
    s = np.asarray(sites, dtype=np.int64).reshape(-1, 3)
    q = np.zeros((s.shape[0], 3))
    for (kx, ky, kz), A, phi in waves:
        m = (kz * s[:, 0] + ky * s[:, 1] + kx * s[:, 2]) % n
        theta = 2.0 * np.pi * m / n + phi
        k2 = float(kx * kx + ky * ky + kz * kz)
        for j, kj in enumerate((kz, ky, kx)):
            q[:, j] -= A * kj * np.sin(theta) / (k2 * fund)
    v = (np.sqrt(1.0 + 24 * f_cluster) - 1) * .25 * q
    if xp is None:  # the closed form alone
        return None, q, v
    if xp is np:
        idx = np.arange(n, dtype=np.int64)
        field = np.zeros((n, n, n))
        for (kx, ky, kz), A, phi in waves:
            m = (kz * idx[:, None, None] + ky * idx[None, :, None] + kx * idx[None, None, :]) % n
            field += A * np.cos(2.0 * np.pi * m / n + phi)
        return field, q, v
    idx = xp.arange(n, dtype=xp.int64, device=device)
    field = xp.zeros((n, n, n), dtype=xp.float64, device=device)
    for (kx, ky, kz), A, phi in waves:
        table = A * xp.cos(2.0 * np.pi * idx.to(xp.float64) / n + phi)  # the cosine of every phase residue
        mxy = (ky * idx[:, None] + kx * idx[None, :]) % n
        for z in range(n):
            field[z] += table[(mxy + (kz * z) % n) % n]
    return field, q, v
