"""Separable dense fields and the direct sums of a field run and of its adjoint: a yardstick for generate_field / Plan.from_field /
field_vjp that is dense in x and in k, uses no N^3 transform and is cheap at 2048.  tests/test_field_sum.py pins it to
field_ref.displace, field_adj_ref.vjp and the oracle's eigenmode lookup.

Fields.  a[z][y][x] = sum_r u_r(z) v_r(y) w_r(x), rank 2, factors drawn from {-8 ... 8} / 8: every value, product and sum is a multiple
of 1/512 below 2 in magnitude, exact in float32 as in float64, so one field serves both dtypes bit for bit.  `factors` are float64
[3][rank][N] = (u, v, w).  The unnormalised forward sum (numpy's fftn) of such a field is the outer product of three length-N
numpy.fft.fft results, F(k) = sum_r U_r(kz) V_r(ky) W_r(kx) — dense: a random factor has no zero bin.

Sums.  With the conventions of field_ref (arrays [z][y][x], signed wavenumbers with N/2 kept as +N/2, components in the records'
order (q_z, q_y, q_x)) every real output of a field run or of its adjoint is
    out(x) = sum_k C(k) e^{2 pi i k.x / N} = 2 Re sum_{k in the half space} C(k) e^{2 pi i k.x / N},
the half space being field_ref.winners (ky > 0; on ky = 0: kz > 0; on ky = kz = 0: kx > 0) and C(-k) = conj C(k) there because s_j is
odd, f even and the field real.  Forward: C = i s_j D (q_j), i f s_j D (v_j), D (density), D = alive A F, A = 1 / N^3 or the
white-noise amplitude amp[|k|^2].  Adjoint: C = H = alive A [sum_j conj(i s_j) (G_q,j + f G_v,j) + G_dens], G the forward sums of the
cotangents.  `sweep` goes over the ky rows once: the mode factors of a row (alive, s_j, f with the eigenmode lookup and the rescale)
are formed once and shared by all sites and outputs; the row is contracted over kz against the phase factors of the distinct z among
the sites (a matrix product), and what is left, [output][z][ky][kx], is summed over kx and ky site by site at the end.  It also
returns sum_k |C(k)|^2, the mean square of the output over the lattice (Parseval): a scale without the output itself.  Phases are
looked up in a table of the N-th roots of unity by the integer k.x mod N.  torch float64 / complex128 on the device it is given; the
CPU will do."""
import numpy as np
import torch

import field_ref

RANK = 2


# ---- separable fields ----------------------------------------------------------------------------------------------------------
def factors(n, seed, rank=RANK):
    """float64 [3][rank][n] = (u, v, w) of a[z][y][x] = sum_r u_r(z) v_r(y) w_r(x), values in {-8 ... 8} / 8"""
    f = np.random.default_rng(seed).integers(-8, 9, (3, rank, n)).astype(np.float64) / 8.0
    f.setflags(write=False)
    return f


def cotangent_factors(n, seed, rank=RANK):
    """float64 [3][3][rank][n]: the factors of the three components of a cotangent [z][y][x][3], independent fields"""
    f = np.stack([factors(n, 1000 * seed + 17 * c + 1, rank) for c in range(3)])
    f.setflags(write=False)
    return f


def field_numpy(fac):
    u, v, w = np.asarray(fac)
    return np.einsum("rz,ry,rx->zyx", u, v, w)


def field_values(fac, sites):
    """the field at the lattice sites [(z, y, x), ...], float64"""
    u, v, w = np.asarray(fac)
    s = np.asarray(sites, dtype=np.int64).reshape(-1, 3)
    return (u[:, s[:, 0]] * v[:, s[:, 1]] * w[:, s[:, 2]]).sum(0)


def build_field(fac, dtype, device):
    """the field [z][y][x] as a torch tensor on `device`, plane by plane (exact in float32 and float64)"""
    u, v, w = (torch.from_numpy(np.array(f, dtype=np.float64)).to(device) for f in np.asarray(fac))
    n = u.shape[1]
    out = torch.empty((n, n, n), dtype=dtype, device=device)
    vw = v[:, :, None] * w[:, None, :]  # [rank][y][x]
    for z in range(n):
        out[z] = (u[:, z, None, None] * vw).sum(0).to(dtype)
    return out


def build_cotangent(fac3, dtype, device):
    """three separable fields interleaved, [z][y][x][3]"""
    n = np.asarray(fac3).shape[-1]
    out = torch.empty((n, n, n, 3), dtype=dtype, device=device)
    for c in range(3):
        u, v, w = (torch.from_numpy(np.array(f, dtype=np.float64)).to(device) for f in np.asarray(fac3)[c])
        vw = v[:, :, None] * w[:, None, :]
        for z in range(n):
            out[z, :, :, c] = (u[:, z, None, None] * vw).sum(0).to(dtype)
    return out


def spectrum_numpy(fac):
    """fftn(a), the unnormalised forward sum, complex128 [kz][ky][kx] in FFT index order (small N only)"""
    U, V, W = np.fft.fft(np.asarray(fac), axis=-1)
    return np.einsum("rz,ry,rx->zyx", U, V, W)


class _Spectra:
    """U, V, W of a separable field on the device: row(ky) = F[kz][kx] of that ky"""

    def __init__(self, fac, device):
        hat = np.fft.fft(np.asarray(fac, dtype=np.float64), axis=-1)  # three sets of `rank` length-N transforms
        self.U, self.V, self.W = (torch.from_numpy(np.ascontiguousarray(h)).to(device) for h in hat)

    def row(self, ky):
        return torch.matmul((self.U * self.V[:, ky, None]).transpose(0, 1), self.W)


# ---- the eigenmode lookup, vectorised --------------------------------------------------------------------------------------------
def eigenmode_lookup(eig, n, kx, ky, kz):
    """get_eigenmode of the reference (src/zeldovich.cpp:149-276) for tensors of signed integer wavenumbers (broadcast against each
    other): float64 [..., 4] = (k^2 / (k.e) e_x, e_y, e_z; lambda).  eig: torch float64 [E][E][E/2 + 1][4] indexed [ikx][iky][ikz].
    E % n == 0: the table entry at the exact stride.  Otherwise trilinear in table coordinates E/n * index, a coordinate strictly
    between E/2 and E/2 + 1 (the +-Nyquist seam) mapped up to E/2 + 1, the upper neighbour of E - 1 wrapping to 0, corners of zero
    weight not read.  Then e_z takes the sign of kz, e is normalised, and k^2 / (k.e) is 0 where k = 0 or it is not finite."""
    E = int(eig.shape[0])
    hp, ph = E // 2 + 1, E // 2
    kx, ky, kz = torch.broadcast_tensors(torch.as_tensor(kx), torch.as_tensor(ky), torch.as_tensor(kz))
    kx, ky, kz = kx.to(eig.device, torch.int64), ky.to(eig.device, torch.int64), kz.to(eig.device, torch.int64)
    ikx = torch.where(kx < 0, n + kx, kx)
    iky = torch.where(ky < 0, n + ky, ky)
    ikz = torch.where(kz < 0, n + kz, kz)
    ikz = torch.where(ikz > n // 2, n - ikz, ikz)
    if E % n == 0:
        st = E // n
        e = eig[ikx * st, iky * st, ikz * st]
    else:
        ratio = float(E) / n

        def axis(i):
            f = ratio * i.to(torch.float64)
            f = torch.where((f > ph) & (f < hp), torch.floor(f + 1), f)
            lo = f.to(torch.int64)
            hi = torch.where(lo + 1 == E, torch.zeros_like(lo), lo + 1)
            return lo, hi, f - lo.to(torch.float64)

        (xl, xh, fx), (yl, yh, fy), (zl, zh, fz) = axis(ikx), axis(iky), axis(ikz)
        e = torch.zeros(kx.shape + (4,), dtype=torch.float64, device=eig.device)
        for ix, wx in ((xl, 1 - fx), (xh, fx)):  # the order of the reference's eight terms: z fastest
            for iy, wy in ((yl, 1 - fy), (yh, fy)):
                for iz, wz in ((zl, 1 - fz), (zh, fz)):
                    w = wx * wy * wz
                    val = eig[ix, iy, iz.clamp(max=hp - 1)]  # (an index past the kz half space only ever carries weight 0)
                    e = e + torch.where((w != 0)[..., None], w[..., None] * val, torch.zeros_like(val))
    e0, e1, e3 = e[..., 0], e[..., 1], e[..., 3]
    e2 = torch.where(kz < 0, -e[..., 2], e[..., 2])
    mag = torch.sqrt(e0 * e0 + e1 * e1 + e2 * e2)
    e0, e1, e2 = e0 / mag, e1 / mag, e2 / mag
    k2 = (kx * kx + ky * ky + kz * kz).to(torch.float64)
    norm = k2 / (kx.to(torch.float64) * e0 + ky.to(torch.float64) * e1 + kz.to(torch.float64) * e2)
    norm = torch.where((k2 == 0) | ~torch.isfinite(norm), torch.zeros_like(norm), norm)
    return torch.stack([norm * e0, norm * e1, norm * e2, e3], dim=-1)


# ---- the mode factors of one ky row ----------------------------------------------------------------------------------------------
def _axis_weights(i, n, E, width):
    """the lookup along one axis as a matrix, float64 [len(i)][width]: row = the weights eigenmode_lookup gives the table entries for
    the table-space index i (one entry at the exact stride; else two neighbours, the seam rule and the wrap as there)"""
    i = np.asarray(i, dtype=np.int64)
    if E % n == 0:
        lo, frac = i * (E // n), np.zeros(len(i))
    else:
        f = float(E) / n * i.astype(np.float64)
        f = np.where((f > E // 2) & (f < E // 2 + 1), np.floor(f + 1), f)
        lo = f.astype(np.int64)
        frac = f - lo
    hi = np.where(lo + 1 == E, 0, lo + 1)
    W = np.zeros((len(i), width))
    rows = np.arange(len(i))
    W[rows, lo] += 1 - frac
    two = frac != 0  # (a neighbour of zero weight is not read: it may lie past the kz half space)
    W[rows[two], hi[two]] += frac[two]
    return W


class Modes:
    """alive, s_j and f of field_ref.displace, row by row on the half space.  params: api.make_params or the oracle's.  What does not
    depend on the row is formed once: the dead planes of kx and kz, kx^2 + kz^2, the first integer |k|^2 the cut-off removes (the
    float comparison of the zero rule, asked for every integer once), the lookup's weights along x and z (the trilinear lookup of a
    row is then two matrix products; eigenmode_lookup is the mode-by-mode form, and test_field_sum.py holds both to the oracle)."""

    def __init__(self, params, device, eig=None):
        self.p, self.device = params, device
        n = self.n = int(params.ppd)
        half = self.half = n // 2
        kmax = self.kmax = int(float(half) * (1.0 / params.k_cutoff) + .5)
        idx = torch.arange(n, device=device)
        k = self.k = torch.where(idx > half, idx - n, idx)
        kz, kx = k[:, None], k[None, :]
        self.kzf, self.kxf = kz.to(torch.float64), kx.to(torch.float64)
        self.fund = float(params.fundamental)
        self.kxz2 = kx * kx + kz * kz
        dead = (kx.abs() == kmax) | (kz.abs() == kmax) | (kx.abs() == half) | (kz.abs() == half)
        if params.qonemode:
            dead = dead | ~((kx == int(params.one_mode[0])) & (kz == int(params.one_mode[2])))
        self.base_live = ~dead
        self.row0 = (kz > 0) | ((kz == 0) & (kx > 0))
        self.k2i_cut = None
        if not field_ref._corner_modes(params):
            k2_cutoff = params.nyquist * params.nyquist / (params.k_cutoff * params.k_cutoff)
            gone = np.arange(3 * half * half + 2, dtype=np.float64) * (self.fund * self.fund) >= k2_cutoff
            self.k2i_cut = int(np.argmax(gone)) if gone.any() else len(gone)
        self.plt = bool(params.qPLT)
        self.f_za = (np.sqrt(1.0 + 24 * params.f_cluster) - 1) * .25
        if self.plt:
            self.eig = torch.from_numpy(np.ascontiguousarray(eig, dtype=np.float64)).to(device)
            self.E = E = int(self.eig.shape[0])
            kn = field_ref.wavenumbers(n)
            ik = np.where(kn < 0, n + kn, kn)
            self.Xw = torch.from_numpy(_axis_weights(ik, n, E, E)).to(device)  # [kx][table x]
            self.Zw = torch.from_numpy(_axis_weights(np.where(ik > half, n - ik, ik), n, E, E // 2 + 1)).to(device)  # [kz][table z]
            self.sgnz = torch.where(kz < 0, -1.0, 1.0).to(torch.float64)

    def eig_row(self, ky):
        """eigenmode_lookup for the whole row ky >= 0: float64 [4][kz][kx]"""
        wy = _axis_weights([ky], self.n, self.E, self.E)[0]
        T = sum(float(wy[b]) * self.eig[:, b] for b in np.nonzero(wy)[0])  # [table x][table z][4]
        e = torch.matmul(torch.matmul(self.Zw, T.permute(2, 1, 0)), self.Xw.T)  # [4][kz][kx]
        e0, e1, e2 = e[0], e[1], e[2] * self.sgnz
        mag = torch.sqrt(e0 * e0 + e1 * e1 + e2 * e2)
        e0, e1, e2 = e0 / mag, e1 / mag, e2 / mag
        k2 = (self.kxz2 + ky * ky).to(torch.float64)
        norm = k2 / (self.kxf * e0 + ky * e1 + self.kzf * e2)
        norm = torch.where((k2 == 0) | ~torch.isfinite(norm), torch.zeros_like(norm), norm)
        return torch.stack([norm * e0, norm * e1, norm * e2, e[3]])

    def row(self, ky):
        """ky in 0 ... N/2: None if the whole row is dead, else (live bool [kz][kx], k2i int64 [kz][kx], s float64 [3][kz][kx] in the
        records' order, f: a number (ZA) or [kz][kx]); s and f are zero where live is not"""
        p = self.p
        if ky == self.half or ky == self.kmax or (p.qonemode and int(p.one_mode[1]) != ky):
            return None
        k2i = self.kxz2 + ky * ky
        live = self.base_live if self.k2i_cut is None else self.base_live & (k2i < self.k2i_cut)
        if ky == 0:
            live = live & self.row0  # (k = 0 goes here as well)
        if not bool(live.any()):
            return None
        zero = torch.zeros((), dtype=torch.float64, device=self.device)
        w = torch.where(live, self.fund / (k2i.to(torch.float64) * self.fund ** 2), zero)  # fundamental / k^2 on the live modes
        if not self.plt:
            return live, k2i, torch.stack([self.kzf * w, ky * w, self.kxf * w]), self.f_za
        e4 = self.eig_row(ky)
        f = torch.where(live, (torch.sqrt(1.0 + 24 * e4[3] * p.f_cluster) - 1) * .25, zero)
        if p.qPLTrescale:
            w = w * ((1. / (1 + p.PLT_target_z)) / (1. / (1 + p.z_initial))) ** (self.f_za - f)
        return live, k2i, torch.where(live, e4[[2, 1, 0]] * w, zero), f


def _amplitude(n, kind, amp, live, k2i):
    """alive A(|k|^2) on a row, float64 [kz][kx]: A = 1 / N^3, or amp[k2i] (every live mode must have an entry)"""
    if kind == "density":
        return live.to(torch.float64) * (1.0 / float(n) ** 3)
    assert kind == "white" and amp is not None
    assert int(k2i[live].max()) < amp.shape[0], "the amplitude table ends below a live mode"
    return torch.where(live, amp[k2i.clamp(max=amp.shape[0] - 1)], torch.zeros((), dtype=torch.float64, device=amp.device))


def amp_table(ps, params, count):
    """the white-noise amplitude by integer |k|^2 < count: sqrt(power(|k|) / N^3), amp[0] = 0; one ps.power call per entry"""
    n3 = float(params.ppd) ** 3
    return np.array([0.0] + [np.sqrt(ps.power(np.sqrt(float(i) * params.fundamental ** 2)) / n3) for i in range(1, count)])


def amp_powerlaw(ps, params, index, count):
    """amp_table for a pure power law power(k) = power(k1) (k / k1)^index (no smoothing), vectorised from ps.power at k1 = the
    fundamental; the caller checks a few entries against amp_table"""
    k2 = np.arange(count, dtype=np.float64)
    k2[0] = 1.0
    a = np.sqrt(ps.power(params.fundamental) * k2 ** (index / 2.0) / float(params.ppd) ** 3)
    a[0] = 0.0
    return a


# ---- the sweep -----------------------------------------------------------------------------------------------------------------
def sweep(n, sites, row_fn, nout, device, phase=None):
    """out[j][s] = 2 Re sum over the half space of C_j(k) e^{2 pi i k.x_s / N} at the lattice sites x_s = (z, y, x), and
    power[j] = sum over ALL k of |C_j(k)|^2 = the mean of out_j^2 over the lattice.  row_fn(ky), ky = 0 ... N/2, gives complex128
    [nout][kz][kx] in FFT index order, zero outside the half space, or None for a dead row; phase: a complex constant per output that
    C_j is still to be multiplied by (i or -i: applied after the kz contraction).  Returns (float64 [nout][S], [nout])."""
    s = torch.from_numpy(np.ascontiguousarray(np.asarray(sites, dtype=np.int64).reshape(-1, 3))).to(device)
    idx = torch.arange(n, device=device)
    k = torch.where(idx > n // 2, idx - n, idx)
    ang = 2.0 * np.pi * idx.to(torch.float64) / n
    roots = torch.complex(torch.cos(ang), torch.sin(ang))  # e^{2 pi i m / N}, m = 0 ... N-1
    uz, zinv = torch.unique(s[:, 0], return_inverse=True)
    Ez = roots[torch.remainder(uz[:, None] * k[None, :], n)]  # [Z][kz]
    nz, Ezr = uz.shape[0], torch.cat([Ez.real, Ez.imag]).contiguous()  # [2 Z][kz]
    nrow = n // 2 + 1
    P = torch.zeros((nout, uz.shape[0], nrow, n), dtype=torch.complex128, device=device)
    power = torch.zeros(nout, dtype=torch.float64, device=device)
    for ky in range(nrow):
        C = row_fn(ky)
        if C is None:
            continue
        power += 2.0 * torch.linalg.vector_norm(C, dim=(1, 2)) ** 2
        # [Z][kz] x [nout][kz][kx] as one real product, (Re Ez; Im Ez) x (Re C, Im C interleaved along kx)
        R = torch.matmul(Ezr, torch.view_as_real(C.contiguous()).reshape(nout, n, 2 * n)).view(nout, 2, nz, n, 2)
        P[:, :, ky, :] = torch.complex(R[:, 0, :, :, 0] - R[:, 1, :, :, 1], R[:, 0, :, :, 1] + R[:, 1, :, :, 0])
    if phase is not None:
        P *= torch.as_tensor(phase, dtype=torch.complex128, device=device)[:, None, None, None]
    out = torch.zeros((nout, s.shape[0]), dtype=torch.float64, device=device)
    kyv = torch.arange(nrow, device=device)
    batch = max(64, (1 << 25) // (max(nout, 2) * n))
    for zi in range(uz.shape[0]):
        sel = torch.nonzero(zinv == zi).reshape(-1)
        for b0 in range(0, sel.shape[0], batch):
            b = sel[b0:b0 + batch]
            Ex = roots[torch.remainder(k[:, None] * s[b, 2][None, :], n)]  # [kx][B]
            Ey = roots[torch.remainder(kyv[:, None] * s[b, 1][None, :], n)]  # [ky][B]
            out[:, b] = 2.0 * (torch.matmul(P[:, zi], Ex) * Ey).sum(dim=1).real
    return out, power


def forward(fac, params, sites, kind="density", amp=None, eig=None, device="cpu"):
    """What a field run makes of the separable field `fac` at the lattice sites [(z, y, x), ...], by field_ref.displace's definition:
    dict(q [S][3], v [S][3] (records' order), dens [S], rms_q, rms_v, rms_dens) — numpy float64; rms_q and rms_v are over the lattice
    and the three components.  kind = "white": amp = the amplitude by integer |k|^2 (amp_table / amp_powerlaw)."""
    n = int(params.ppd)
    modes, spec = Modes(params, device, eig=eig), _Spectra(fac, device)
    if amp is not None:
        amp = torch.from_numpy(np.ascontiguousarray(amp, dtype=np.float64)).to(device)

    def row(ky):
        m = modes.row(ky)
        if m is None:
            return None
        live, k2i, s, f = m
        D = spec.row(ky) * _amplitude(n, kind, amp, live, k2i)
        C = torch.empty((7, n, n), dtype=torch.complex128, device=device)
        torch.mul(s, D, out=C[0:3])  # (times i: the phase)
        torch.mul(C[0:3], f, out=C[3:6])
        C[6] = D
        return C

    out, power = sweep(n, sites, row, 7, device, phase=[1j] * 6 + [1.0])
    out, power = out.cpu().numpy(), power.cpu().numpy()
    return dict(q=out[0:3].T.copy(), v=out[3:6].T.copy(), dens=out[6].copy(), rms_q=float(np.sqrt(power[0:3].mean())),
                rms_v=float(np.sqrt(power[3:6].mean())), rms_dens=float(np.sqrt(power[6])))


def adjoint(params, sites, fac_q=None, fac_v=None, fac_dens=None, kind="density", amp=None, eig=None, device="cpu"):
    """abar of field_adj_ref.vjp for separable cotangents (fac_q, fac_v: cotangent_factors; fac_dens: factors; None = an exact zero)
    at the lattice sites: (abar float64 [S], rms of abar over the lattice)"""
    n = int(params.ppd)
    modes = Modes(params, device, eig=eig)
    sq = [_Spectra(fac_q[c], device) for c in range(3)] if fac_q is not None else None
    sv = [_Spectra(fac_v[c], device) for c in range(3)] if fac_v is not None else None
    sd = _Spectra(fac_dens, device) if fac_dens is not None else None
    if amp is not None:
        amp = torch.from_numpy(np.ascontiguousarray(amp, dtype=np.float64)).to(device)

    def row(ky):
        m = modes.row(ky)
        if m is None:
            return None
        live, k2i, s, f = m
        H = torch.zeros((n, n), dtype=torch.complex128, device=device)
        for j in range(3):  # sum_j s_j (G_q,j + f G_v,j), then times conj(i) = -i
            if sq is not None:
                H += s[j] * sq[j].row(ky)
            if sv is not None:
                H += (f * s[j]) * sv[j].row(ky)
        A = _amplitude(n, kind, amp, live, k2i)
        H *= -1j * A
        if sd is not None:
            H += sd.row(ky) * A
        return H[None]

    out, power = sweep(n, sites, row, 1, device)
    return out[0].cpu().numpy(), float(np.sqrt(power[0].item()))
