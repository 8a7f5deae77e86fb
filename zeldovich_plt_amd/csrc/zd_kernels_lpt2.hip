// zd_kernels_lpt2.hip — second-order Lagrangian displacements (2LPT) for ZA runs in Fourier space: the generator of the
// second-order round's gradient pairs and of the final pass, and the x-line kernel that forms the source on the lattice
// (zd_params.q2LPT, include/zeldovich_hip.h).  The reference has no second order; this definition is the contract.
//
// DEFINITION
//   Let psi1(x) be the displacement field a ZA run delivers: q_j(x) = sum_k F_j(k) e^{+2 pi i k.x / N}, F_j = i k_j D(k) / k^2, k in
//   physical units (`fundamental`), over the modes the zero rule leaves alive.
//   1. Gradients.  psi1_{a,b}(k) = i k_a F_b(k) = -k_a k_b D(k) / k^2: six distinct fields, symmetric.  Signed integer wavenumbers;
//      the Nyquist planes are dead as in the first order.  Inverse-transformed to the lattice, unnormalised, like q.
//   2. Source.  S(x) = sum_{a<b} [ psi1_{a,a} psi1_{b,b} - (psi1_{a,b})^2 ], pointwise on the N^3 lattice.  No de-aliasing
//      (2LPTic's convention).
//   2'. De-aliased source (zd_params.lpt2_dealias = 1, ZD_2LPT_dealias; Orszag's 3/2 rule).  Steps 1 - 3 run on the lattice of M = 3 N / 2
//      points per side.  The six gradient fields carry the same modes as before — the alive modes of the PPD = N run, Nyquist planes
//      of N dead — at their signed wavenumbers in an M^3 cube, zero elsewhere, inverse-transformed unnormalised to M^3.  S(x) is formed
//      pointwise on M^3.  S(k) = M^-3 sum_x S(x) e^{-2 pi i k.x / M} is kept only for |k_i| < N/2 and multiplied by the alive mask of
//      the N run, with S(0) = 0.  Steps 4 and 5 are unchanged and run at N.  A product of two modes with |k_i| < N/2 has |k_i| < N;
//      on M = 3 N / 2 points it folds only to |k_i| > N/2, which is dropped: the S(k) kept is exact.  (At ZD_k_cutoff >= 1.5 nothing
//      aliases in step 2 either, and the two agree to rounding.)
//   3. Forward transform.  S(k) = N^-3 sum_x S(x) e^{-2 pi i k.x / N}, multiplied by the same alive mask as D(k): the zero rule
//      (Nyquist planes, ZD_k_cutoff, the corner rule), with S(0) = 0.  (The one-mode filter is not part of the mask.)
//   4. Second-order displacement.  psi2_j(k) = i k_j gamma S(k) / k^2, gamma = -lpt2_ratio: div psi2 = -gamma S.
//   5. Records.  displacement = psi1 + psi2, velocity = alpha psi1 + f2 psi2, alpha = vnorm = (sqrt(1 + 24 f_cluster) - 1) / 4.
//   Defaults, from D'' + D'/2 - (3/2) f_cl D = source (in ln a) of the f_cluster-EdS background vnorm encodes:
//      lpt2_ratio = D2 / D1^2 = -(2 alpha + 1) / (6 alpha + 1)  (-3/7 at f_cluster = 1),  f2 = 2 alpha.
//   In terms of modes: the position fields are the ZA fields of D + gamma S, the velocity fields the ZA fields of
//   alpha D + f2 gamma S.
//
// AS BUILT
//   Second-order round (zd_capi_rounds.cpp make_lpt2_source; once per plan, the whole field resident, stream factor 1): four passes over
//   ONE complex array that packs two Hermitian gradient fields as A + iB,
//        pass 1: (psi_xx, psi_yy + psi_zz)   pass 2: (psi_yy, psi_zz)   pass 3: (psi_xy, psi_xz)   pass 4: (psi_yz, 0),
//   each one k_gen_lpt2<2> -> k_zfft -> k_yfft (the one-array store of the f_NL phi round) -> k_xlpt2, which transforms an x line
//   in registers and adds Re Im (passes 1, 2) or subtracts Re^2 + Im^2 (passes 3, 4) into a real N^3 accumulator:
//        S = psi_xx (psi_yy + psi_zz) + psi_yy psi_zz - psi_xy^2 - psi_xz^2 - psi_yz^2.
//   On pass 4 the same kernel scales by N^-3 and transforms the row forward in place; k_yfwd and k_zfwd of the f_NL round then give
//   the half-space S(k)[ky][kz][x].  D is REGENERATED in every pass (counter-addressed draws; modes_cached stays 0): keeping
//   D would cost 8 N^3 bytes beside the 24 N^3 of the round for a generator that is a small part of a pass.
//   De-aliased round (make_lpt2_source_dealiased; kernels: zd_kernels_lpt2q.hip): the same four passes with a plan AT the lattice M
//   (ZD_k_cutoff x 1.5, same box and seed: the counter-addressed draws and the zero rule give exactly the modes of the N run), on a
//   one-array store [z][y][x] of the reference-array family: k_gen_lpt2<2> -> k_refq_cols (z) -> k_any_scatter -> k_refq_cols (y) ->
//   k_xlpt2q into a real M^3 accumulator; then the y columns |kx| < N/2 and k_lpt2q_zsrc, which truncates to the N cube and writes
//   S(k)[ky][kz][x] in the N layout.  Peak (16 + 8) M^3 = 81 N^3 bytes.
//   Final pass: k_gen_lpt2<7> forms the seven jobs of the reference's four arrays (density + i qx | qy + i qz | i vx | vy + i vz,
//   the PLT shape) from its own draws and S(k): the density from D, positions from D + gamma S, velocities from
//   alpha D + f2 gamma S with the ZA coefficients s_j = k_j fundamental / k^2.  The z, y and x stages and the PLT epilogue (velocity
//   scale 1) are the existing kernels.  A mode the mask kills contributes nothing, whatever S(k) holds there.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "zd_device.h"
#include "zd_launch.h"
#include "zd_genmath.h"

using namespace zd;
using zdfft::cplx;
using zdpcg::u128;
using namespace zdgen;

__constant__ zdpcg::BitTable c_bits_l2;

extern "C" int zdk_upload_bit_table_lpt2(const zdpcg::BitTable *host) {
    return (int) hipMemcpyToSymbol(HIP_SYMBOL(c_bits_l2), host, sizeof(zdpcg::BitTable));
}

namespace {

__device__ __forceinline__ u128 advance_bits_l2(u128 s, uint64_t delta) {
    for (int i = 0; i < zdpcg::NBITS; i++) {
        if ((delta >> i) == 0) break;
        if ((delta >> i) & 1ULL) s = zdpcg::apply(c_bits_l2.m[i], s);
    }
    return s;
}

// the alive mask of the definition: the zero rule of LoadPlane (src/zeldovich.cpp:350-353) without the one-mode filter, and k = 0
__device__ __forceinline__ bool lpt2_masked(const GenConst &g, int kx, int ky, int kz, int k2i, double k2v) {
    const int ax = kx < 0 ? -kx : kx, az = kz < 0 ? -kz : kz;
    if (k2i == 0 || ax == g.kmax || az == g.kmax || ky == g.kmax) return true;
    return !g.corner_modes && k2v >= g.k2_cutoff;
}

// k_gen_lpt2: the general generator (k_gen, zd_kernels.hip: one thread owns one x and GEN_ZR consecutive k2, walks the R fold terms
// of each with the z-major RNG walk, folds for the residue, writes Y[((j nky + kyl) L + k2) N + x]) with the amplitudes and
// coefficients of the second order.
//   NJ = 2, g.lpt2 = 1 .. 4: the gradient pair of that pass, jobs (cA + i cB) D and (cA - i cB) D (JOB_G2_SELF / _TWIN; cA, cB real
//           and even in k, so the conjugated ky = 0 copies keep their sign)
//   NJ = 7, g.lpt2 = 5: the final pass, the reference's seven jobs (JOB_A_SELF .. JOB_D_TWIN) with D, P = D + gamma S and
//           V = alpha D + f2 gamma S in the places of D, D and f D
// grid: (ceil(N / GEN_BX), L / GEN_ZR, nky)  block: GEN_BX
template <int NJ, bool PLAW>
__global__ __launch_bounds__(GEN_BX) void k_gen_lpt2(GenConst g, GenJumps J, StoreLayout S, int zW, int ky0, int nky, int L, int residue,
                                                     const cplx *__restrict__ twN, cplx *__restrict__ Y) {
    const int N = g.N, half = g.half, R = N / L;
    const int x   = blockIdx.x * GEN_BX + threadIdx.x;
    const int k20 = blockIdx.y * GEN_ZR;
    const int kyl = blockIdx.z;
    const int ky  = ky0 + kyl * S.ky_stride;
    if (x >= N) return;
    const int kx = x > half ? x - N : x;
    if (S.prune & 1) {  // the z-FFT tiles this column belongs to (self, and twin shifted by one column) are identically zero
        bool all_zero = true;
        const int xt0 = x - x % zW;
        for (int i = -1; i <= zW; i++) {
            const int xi = modn(N, xt0 + i + N);
            all_zero = all_zero && column_is_zero(S, xi > half ? xi - N : xi, ky);
        }
        if (all_zero) return;
    }
    u128 s = 0;
    if (ky != 0) {  // state one step ahead of the first mode's counter
        const int kz0 = k20 > half ? k20 - N : k20;  // k20 > N/2 only happens when R = 1
        s = advance_bits_l2(g.row_state[ky], 2ULL * ((uint64_t) (kz0 & 65535) * 65536ULL + (uint64_t) (kx & 65535)) + 1ULL);
    }
#pragma unroll 1
    for (int zi = 0; zi < GEN_ZR; zi++) {
        const int k2 = k20 + zi;
        double accr[NJ], acci[NJ];
#pragma unroll
        for (int j = 0; j < NJ; j++) accr[j] = acci[j] = 0.0;
#pragma unroll 1
        for (int k1 = 0; k1 < R; k1++) {
            const int z = k2 + L * k1;
            // ---- which mode feeds (ky, z, x), and its two raw draws (k_gen) ----
            int zs = z, xs = x;
            bool cj = false;
            uint64_t r1, r2;
            if (ky != 0) {
                r1 = zdpcg::output(s);
                const u128 s2 = zdpcg::step(s);
                r2 = zdpcg::output(s2);
                int zb;
                const zdpcg::Affine *m;
                if (k1 + 1 < R) {
                    zb = z + L;
                    m  = &J.fwd[(z > half) != (zb > half)];
                } else {
                    zb = k2 + 1;
                    m  = &J.back[(z > half) != (zb > half)];
                }
                s = zdpcg::apply(*m, s2);
            } else {  // ky = 0: "loser" positions take the conjugate of the winner's mode (zeldovich.cpp:485-503)
                if (z > half) {
                    zs = N - z;
                    xs = x ? N - x : 0;
                    cj = true;
                } else if (z == 0 && x > half) {
                    xs = N - x;
                    cj = true;
                }
                const int kxs = xs > half ? xs - N : xs, kzs = zs > half ? zs - N : zs;
                const u128 t = advance_bits_l2(g.row_state[0], 2ULL * ((uint64_t) (kzs & 65535) * 65536ULL + (uint64_t) (kxs & 65535)) + 1ULL);
                r1 = zdpcg::output(t);
                r2 = zdpcg::output(zdpcg::step(t));
            }
            const int kxm = xs > half ? xs - N : xs, kzm = zs > half ? zs - N : zs;  // generated mode
            const int k2i = kxm * kxm + ky * ky + kzm * kzm;
            const double k2v = (double) k2i * g.fundamental2;
            if (lpt2_masked(g, kxm, ky, kzm, k2i, k2v)) continue;
            double dr = 0.0, di = 0.0, ik2;
            const bool drawn = !g.qonemode || (kxm == g.one_mode[0] && ky == g.one_mode[1] && kzm == g.one_mode[2]);
            if (g.pk_tab) {  // {P(k), 1/k^2} by integer k^2
                const double2 pv = g.pk_tab[k2i];
                ik2 = pv.y;
                if (drawn) gauss_from_pk(g, pv.x, r1, r2, dr, di);
            } else {
                ik2 = 1.0 / k2v;
                if (drawn) gauss_mode<PLAW>(g, k2v, r1, r2, dr, di);
            }
            if constexpr (NJ == 2) {
                if (dr == 0.0 && di == 0.0) continue;
                if (cj) di = -di;  // conjugated copy of the mode at -k; the coefficients are even
                if (R > 1) {  // W_R^{k1 r}
                    const cplx w = twN[modn(N, k1 * residue * L)];
                    const double a = dr * w.x - di * w.y, b = dr * w.y + di * w.x;
                    dr = a;
                    di = b;
                }
                // -k_a k_b / k^2 in integer wavenumbers (the fundamentals cancel)
                const double ikk = 1.0 / (double) k2i;
                const double fx = (double) kxm, fy = (double) ky, fz = (double) kzm;
                double cA, cB;
                switch (g.lpt2) {
                    case 1: cA = -fx * fx * ikk; cB = -(fy * fy + fz * fz) * ikk; break;
                    case 2: cA = -fy * fy * ikk; cB = -fz * fz * ikk; break;
                    case 3: cA = -fx * fy * ikk; cB = -fx * fz * ikk; break;
                    default: cA = -fy * fz * ikk; cB = 0.0; break;
                }
                accr[0] += cA * dr - cB * di;
                acci[0] += cA * di + cB * dr;
                accr[1] += cA * dr + cB * di;
                acci[1] += cA * di - cB * dr;
            } else {
                // S(k) of the source mode (half-space rows [ky][kz][x], one rank), P = D + gamma S, V = alpha D + f2 gamma S
                const cplx sk = g.lpt2_sk[((long long) ky * N + zs) * N + xs];
                double pr = dr + g.lpt2_gamma * sk.x, pi = di + g.lpt2_gamma * sk.y;
                double vr = g.lpt2_alpha * dr + g.lpt2_f2g * sk.x, vi = g.lpt2_alpha * di + g.lpt2_f2g * sk.y;
                double sx = (double) kxm * g.fundamental * ik2, sy = (double) ky * g.fundamental * ik2, sz = (double) kzm * g.fundamental * ik2;
                if (cj) {  // conjugated copy of the mode at -k: amplitudes -> conj, s -> -s(-k)
                    di = -di;
                    pi = -pi;
                    vi = -vi;
                    sx = -sx;
                    sy = -sy;
                    sz = -sz;
                }
                if (R > 1) {  // W_R^{k1 r}
                    const cplx w = twN[modn(N, k1 * residue * L)];
                    double a = dr * w.x - di * w.y, b = dr * w.y + di * w.x;
                    dr = a;
                    di = b;
                    a  = pr * w.x - pi * w.y;
                    b  = pr * w.y + pi * w.x;
                    pr = a;
                    pi = b;
                    a  = vr * w.x - vi * w.y;
                    b  = vr * w.y + vi * w.x;
                    vr = a;
                    vi = b;
                }
                // JOB_A_SELF (1 - sx) | JOB_A_TWIN (1 + sx): the density from D, qx from P
                accr[0] += dr - sx * pr;
                acci[0] += di - sx * pi;
                accr[1] += dr + sx * pr;
                acci[1] += di + sx * pi;
                // JOB_B_SELF (-sz + i sy) P | JOB_B_TWIN (sz + i sy) P
                const double yr = -sy * pi, yi = sy * pr;  // i sy P
                accr[2] += yr - sz * pr;
                acci[2] += yi - sz * pi;
                accr[3] += yr + sz * pr;
                acci[3] += yi + sz * pi;
                // JOB_C_BOTH (-sx) V | JOB_D_SELF (-sz + i sy) V | JOB_D_TWIN (sz + i sy) V
                accr[4] -= sx * vr;
                acci[4] -= sx * vi;
                const double wr = -sy * vi, wi = sy * vr;  // i sy V
                accr[5] += wr - sz * vr;
                acci[5] += wi - sz * vi;
                accr[6] += wr + sz * vr;
                acci[6] += wi + sz * vi;
            }
        }
        double tr = 1.0, ti = 0.0;  // W_N^{k2 r}
        if (R > 1) {
            const cplx w = twN[modn(N, k2 * residue)];
            tr = w.x;
            ti = w.y;
        }
#pragma unroll
        for (int j = 0; j < NJ; j++) {
            // a slab holds < 2^31 elements (1.5 GB / 16 B): 32-bit index arithmetic
            const unsigned idx = (unsigned) (((j * nky + kyl) * L + k2) * N + x);
            Y[idx] = cplx{accr[j] * tr - acci[j] * ti, accr[j] * ti + acci[j] * tr};
        }
    }
}

// k_xlpt2: rows of the one-array store in gradient pass `pass` (k_xphi's shape, zd_kernels.hip): inverse x transform in registers;
// the line now holds A(x) + i B(x) of the pass's two gradient fields.  acc[(z N + y) N + x] = (pass 1) A B, += A B (pass 2),
// -= A^2 + B^2 (passes 3, 4).  Pass 4 goes on: the row takes S(x) / N^3 and is transformed forward in place (a forward transform is
// conj o inverse o conj; the input is real).
//   grid: (N / ROWS, nplanes)   block: ROWS * N / E
template <int N, int E, int ROWS>
__global__ __launch_bounds__(ROWS *N / E) void k_xlpt2(StoreLayout S, int pass, double inv_ppd3, const cplx *__restrict__ tw,
                                                      cplx *__restrict__ data, double *__restrict__ acc) {
    using PL  = zdfft::Plan<N, E>;
    using LDS = zdfft::LineInner<N, ROWS>;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr int T = PL::T;
    const int t = threadIdx.x % T, row = threadIdx.x / T;
    const int y = blockIdx.x * ROWS + row, pl = blockIdx.y;
    cplx *p = data + row_offset(S, pl, 0, y);
    double re[E], im[E];
#pragma unroll
    for (int e = 0; e < E; e++) {
        const cplx v = p[t + T * e];
        re[e] = v.x;
        im[e] = v.y;
    }
    zdfft::fft_line<PL, LDS>(re, im, t, row, lds, tw);
    double *a = acc + ((long long) pl * N + y) * N;
    int t2 = t;
    asm volatile("" : "+v"(t2));  // keep the address arithmetic behind the transform (register pressure, as in k_xphi)
#pragma unroll
    for (int e = 0; e < E; e++) {
        const int xx = t2 + T * e;
        double s = pass == 1 ? 0.0 : a[xx];
        s = pass <= 2 ? fma(re[e], im[e], s) : s - fma(re[e], re[e], im[e] * im[e]);
        if (pass < 4) a[xx] = s;
        re[e] = s * inv_ppd3;
        im[e] = 0.0;
    }
    if (pass < 4) return;  // (uniform over the launch)
    __syncthreads();
    zdfft::fft_line<PL, LDS>(re, im, t, row, lds, tw);
    int t3 = t;
    asm volatile("" : "+v"(t3));
#pragma unroll
    for (int e = 0; e < E; e++) p[t3 + T * e] = cplx{re[e], -im[e]};
}

template <int NJ, bool PLAW>
int launch_gen_lpt2_t(const GenConst &g, const GenJumps &J, const StoreLayout &S, int ky0, int nky, int L, int residue, const void *twN,
                      void *Y, hipStream_t st) {
    const int N = g.N;
    dim3 grid((N + GEN_BX - 1) / GEN_BX, L / GEN_ZR, nky), block(GEN_BX);
    const int zw = zfft_tile_width(L) > 0 ? zfft_tile_width(L) : 16;
    hipLaunchKernelGGL((k_gen_lpt2<NJ, PLAW>), grid, block, 0, st, g, J, S, zw, ky0, nky, L, residue, (const cplx *) twN, (cplx *) Y);
    ZD_LAUNCH_CHECK();
    return 0;
}

template <int N, int E, int ROWS>
int launch_lpt2_xsrc_t(const StoreLayout &S, int pass, const void *tw, void *data, double *acc, int nplanes, hipStream_t st) {
    constexpr int threads = ROWS * N / E;
    const size_t shmem = sizeof(double) * zdfft::LineInner<N, ROWS>::SIZE;
    ZD_PROBE_RETURN();
    set_dyn_lds<k_xlpt2<N, E, ROWS>>(shmem);
    const double inv = 1. / N / N / N;
    hipLaunchKernelGGL((k_xlpt2<N, E, ROWS>), dim3(N / ROWS, nplanes), dim3(threads), shmem, st, S, pass, inv, (const cplx *) tw, (cplx *) data,
                       acc);
    ZD_LAUNCH_CHECK();
    return 0;
}

}  // namespace

namespace zd {

int launch_gen_lpt2(const GenConst &g, const GenJumps &J, const JobList &jobs, const StoreLayout &S, int ky0, int nky, int L, int residue,
                    const void *twN, void *Y, hipStream_t st) {
    if (L % GEN_ZR || g.N % L) return 2;
#define GCASE(nj)                                                                                                 \
    return g.is_powerlaw ? launch_gen_lpt2_t<nj, true>(g, J, S, ky0, nky, L, residue, twN, Y, st)                 \
                         : launch_gen_lpt2_t<nj, false>(g, J, S, ky0, nky, L, residue, twN, Y, st);
    if (g.lpt2 >= 1 && g.lpt2 <= 4 && jobs.n == 2) GCASE(2)
    if (g.lpt2 == 5 && jobs.n == 7 && g.lpt2_sk) GCASE(7)
#undef GCASE
    ZD_TABLE_MISS("zeldovich_hip: no second-order generator for pass %d with %d jobs\n", g.lpt2, jobs.n);
    return 2;
}

// (the row counts of the f_NL round's x kernel, launch_fnl_stage)
int launch_lpt2_xsrc(const StoreLayout &S, int pass, const void *tw, void *data, double *acc, int nplanes, hipStream_t st) {
    if (pass < 1 || pass > 4 || S.narray != 1) return 2;
#define LCASE(n, e, rows) \
    case n: return launch_lpt2_xsrc_t<n, e, rows>(S, pass, tw, data, acc, nplanes, st);
    switch (S.N) {
        LCASE(32, 16, 32)
        LCASE(64, 16, 32)
        LCASE(128, 16, 32)
        LCASE(256, 16, 16)
        LCASE(512, 16, 8)
        LCASE(1024, 16, 4)
        LCASE(2048, 16, 2)
    }
#undef LCASE
    ZD_TABLE_MISS("zeldovich_hip: the second-order round supports PPD = 32..2048 (power of two), got %d\n", S.N);
    return 2;
}

}  // namespace zd
