// zd_kernels_lpt2_field.hip — second-order Lagrangian displacements (2LPT) on a caller-supplied field: the generator of the second-order
// round's gradient pairs and of the final pass when the first-order modes are READ from the field's PhiK instead of drawn.  gfx950.
//
// DEFINITION
//   Start from D(k), the modes of the supplied field exactly as a first-order field run holds them in PhiK: the intake of
//   zd_kernels_field.hip — D(k) = N^-3 x the forward sum of a density, or W(k) sqrt(power / N^3) of white noise; cleared by the zero rule
//   (mode_is_zero: the |k_i| = kmax planes, k^2 >= k^2_cutoff, ZD_qonemode, k = 0) and on the |k_i| = N/2 planes.  Then steps 1 - 5 of the
//   DEFINITION in zd_kernels_lpt2.hip apply unchanged:
//   1. gradients psi1_{a,b}(k) = -k_a k_b D(k) / k^2, signed integer wavenumbers, inverse-transformed unnormalised;
//   2. S(x) = sum_{a<b} [ psi1_{a,a} psi1_{b,b} - (psi1_{a,b})^2 ] pointwise on the N^3 lattice, no de-aliasing;
//   3. S(k) = N^-3 sum_x S(x) e^{-2 pi i k.x / N} times the alive mask lpt2_masked (the zero rule without the one-mode filter), S(0) = 0;
//   4. psi2_j(k) = i k_j gamma S(k) / k^2, gamma = -lpt2_ratio;
//   5. displacement = psi1 + psi2, velocity = alpha psi1 + f2 psi2: the position fields are the ZA fields of D + gamma S, the velocity
//      fields those of alpha D + f2 gamma S, with alpha, lpt2_ratio and f2 as zd_route.h resolves them from ZD_2LPT_D2, ZD_2LPT_f2 and
//      ZD_f_cluster.
//   It is the seeded ZD_q2LPT run with "D drawn from its counter" replaced by "D read from the field's PhiK".  ZD_Seed is ignored; no draw
//   is made.  The order is an argument of the field call (zd_generate_field_lpt, zd_plan_create_field_lpt), not ZD_q2LPT in the
//   parameters; third order, the de-aliased round, composite sizes and several GPUs are not built for a field.
//
// AS BUILT
//   k_gen_lpt2_field<NJ> is the field form of k_gen_lpt2<NJ> (zd_kernels_lpt2.hip) and writes the same folded inputs
//   Y[((j nky + kyl) L + k2) N + x] for the same jobs: NJ = 2 the gradient pair of pass g.lpt2 = 1 .. 4, NJ = 7 the final pass
//   (g.lpt2 = 5).  Grid, store indexing, the fold over the R terms of a residue with the W_R / W_N twiddles, the S.prune column skip, the
//   ky = 0 "loser takes the conjugate of the winner" rule with its sign flips of s_j, and the job arithmetic are k_gen_lpt2's.  The RNG
//   walk is gone: a live mode is ONE 16-byte load of D at PhiK[(ky N + zs) N + xs] — the final form also loads S(k) at the same
//   index — coalesced along x (on the ky = 0 row the mirrored reads run backwards); a masked mode loads nothing.  D is PhiK itself
//   (no multiplication by fnl_M).  The z, y and x stages, k_xlpt2 and the forward chain of the round are the existing kernels.
//   Memory: PhiK (8 N^3 bytes) stays resident through the round (peak 32 N^3 bytes + the row pad) and, with S(k), beside every pass's
//   store afterwards (16 N^3 bytes).  Bytes by count: a gradient pass reads 8 N^3 bytes of PhiK and writes 16 N^3 of folded inputs;
//   the final pass reads 16 N^3 (D and S) and writes the inputs of the four arrays.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "zd_device.h"
#include "zd_launch.h"
#include "zd_genmath.h"

using namespace zd;
using zdfft::cplx;
using zdgen::modn;

namespace {

// the alive mask of the definition (lpt2_masked, zd_kernels_lpt2.hip)
__device__ __forceinline__ bool lpt2f_masked(const GenConst &g, int kx, int ky, int kz, int k2i, double k2v) {
    const int ax = kx < 0 ? -kx : kx, az = kz < 0 ? -kz : kz;
    if (k2i == 0 || ax == g.kmax || az == g.kmax || ky == g.kmax) return true;
    return !g.corner_modes && k2v >= g.k2_cutoff;
}

// k_gen_lpt2_field: one thread owns one x and GEN_ZR consecutive k2, folds the R terms of each for the residue and writes
// Y[((j nky + kyl) L + k2) N + x]; g.phik = D(k)[ky][kz][x] (half-space rows ky < N/2, one rank), NJ = 7: g.lpt2_sk = S(k) likewise
// grid: (ceil(N / GEN_BX), L / GEN_ZR, nky)  block: GEN_BX
template <int NJ>
__global__ __launch_bounds__(GEN_BX) void k_gen_lpt2_field(GenConst g, StoreLayout S, int zW, int ky0, int nky, int L, int residue,
                                                           const cplx *__restrict__ twN, cplx *__restrict__ Y) {
    const int N = g.N, half = g.half, R = N / L;
    const int x   = blockIdx.x * GEN_BX + threadIdx.x;
    const int k20 = blockIdx.y * GEN_ZR;
    const int kyl = blockIdx.z;
    const int ky  = ky0 + kyl * S.ky_stride;
    if (x >= N) return;
    if (S.prune & 1) {  // the z-FFT tiles this column belongs to (self, and twin shifted by one column) are identically zero
        bool all_zero = true;
        const int xt0 = x - x % zW;
        for (int i = -1; i <= zW; i++) {
            const int xi = modn(N, xt0 + i + N);
            all_zero = all_zero && column_is_zero(S, xi > half ? xi - N : xi, ky);
        }
        if (all_zero) return;
    }
    const cplx *__restrict__ D = g.phik + (long long) ky * N * N;
    const cplx *__restrict__ SK = NJ == 7 ? g.lpt2_sk + (long long) ky * N * N : nullptr;
#pragma unroll 1
    for (int zi = 0; zi < GEN_ZR; zi++) {
        const int k2 = k20 + zi;
        double accr[NJ], acci[NJ];
#pragma unroll
        for (int j = 0; j < NJ; j++) accr[j] = acci[j] = 0.0;
#pragma unroll 1
        for (int k1 = 0; k1 < R; k1++) {
            const int z = k2 + L * k1;
            // ---- which mode feeds (ky, z, x) ----
            int zs = z, xs = x;
            bool cj = false;
            if (ky == 0) {  // "loser" positions take the conjugate of the winner's mode (zeldovich.cpp:485-503)
                if (z > half) {
                    zs = N - z;
                    xs = x ? N - x : 0;
                    cj = true;
                } else if (z == 0 && x > half) {
                    xs = N - x;
                    cj = true;
                }
            }
            const int kxm = xs > half ? xs - N : xs, kzm = zs > half ? zs - N : zs;  // the mode that is read
            const int k2i = kxm * kxm + ky * ky + kzm * kzm;
            const double k2v = (double) k2i * g.fundamental2;
            if (lpt2f_masked(g, kxm, ky, kzm, k2i, k2v)) continue;  // (nothing is loaded)
            const int at = zs * N + xs;  // (inside the row: < N^2)
            const cplx dk = D[at];
            double dr = dk.x, di = dk.y;
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
                // S(k) of the same mode, P = D + gamma S, V = alpha D + f2 gamma S
                const cplx sk = SK[at];
                // 1 / k^2 in physical units as the seeded generator has it: its table entry where the plan has one, else 1 / k2v
                const double ik2 = g.pk_tab ? g.pk_tab[k2i].y : 1.0 / k2v;
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

template <int NJ>
int launch_gen_lpt2_field_t(const GenConst &g, const StoreLayout &S, int ky0, int nky, int L, int residue, const void *twN, void *Y,
                            hipStream_t st) {
    const int N = g.N;
    dim3 grid((N + GEN_BX - 1) / GEN_BX, L / GEN_ZR, nky), block(GEN_BX);
    const int zw = zfft_tile_width(L) > 0 ? zfft_tile_width(L) : 16;
    ZD_PROBE_RETURN();
    hipLaunchKernelGGL((k_gen_lpt2_field<NJ>), grid, block, 0, st, g, S, zw, ky0, nky, L, residue, (const cplx *) twN, (cplx *) Y);
    ZD_LAUNCH_CHECK();
    return 0;
}

}  // namespace

namespace zd {

// PhiK and S(k) hold the half-space rows of ONE rank ([ky][kz][x], ky < N/2): the rows of the launch must be those
int launch_gen_lpt2_field(const GenConst &g, const JobList &jobs, const StoreLayout &S, int ky0, int nky, int L, int residue, const void *twN,
                          void *Y, hipStream_t st) {
    if (L % GEN_ZR || g.N % L) return 2;
    const bool rows_ok = g.phik && S.ky_stride == 1 && ky0 >= 0 && ky0 + nky <= g.half;
    if (rows_ok && g.lpt2 >= 1 && g.lpt2 <= 4 && jobs.n == 2) return launch_gen_lpt2_field_t<2>(g, S, ky0, nky, L, residue, twN, Y, st);
    if (rows_ok && g.lpt2 == 5 && jobs.n == 7 && g.lpt2_sk) return launch_gen_lpt2_field_t<7>(g, S, ky0, nky, L, residue, twN, Y, st);
    ZD_TABLE_MISS("zeldovich_hip: ZD_Field: no second-order generator on a field for pass %d with %d jobs (rows %d .. %d, stride %d)\n", g.lpt2,
                  jobs.n, ky0, ky0 + nky - 1, S.ky_stride);
    return 2;
}

}  // namespace zd
