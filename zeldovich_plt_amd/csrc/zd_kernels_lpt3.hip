// zd_kernels_lpt3.hip — third-order Lagrangian displacements (3LPT) on top of the second order (zd_params.q3LPT,
// include/zeldovich_hip.h): the generator of the third-order round's Hessian pairs and of the final pass, the x-line kernels that carry
// the Hessians to the lattice and the sources back, and the pointwise kernel that forms the sources.  The reference has no third
// order; this definition is the contract.
//
// DEFINITION
//   Notation of zd_kernels_lpt2.hip: F_j = i k_j D(k) / k^2 are the first-order modes, k in physical units (`fundamental`), signed
//   integer wavenumbers, the Nyquist planes dead; the inverse transform is unnormalised, the forward transform carries N^-3.  S(k) is
//   the masked second-order source of steps 2 - 3 there.
//   1. Hessians.  For a spectrum X, T_ab[X](k) = k_a k_b X(k) / k^2, T(0) = 0, inverse-transformed to the lattice.  Twelve real fields:
//      T_ab[D] and T_ab[S] for the six pairs ab.  T_ab[D] = -psi1_{a,b}; tr T[D] and tr T[S] are the inverse transforms of D and S(k).
//   2. Sources, pointwise on the N^3 lattice, no de-aliasing:
//        S3a = det T[D]
//        S3b = 1/2 (tr T[S] tr T[D] - sum_ab T_ab[S] T_ab[D])
//        C_i = eps_ijk sum_l T_jl[S] T_kl[D],  i = x, y, z.
//   3. Forward transform.  P3(k) = N^-3 sum_x (g3a S3a + g3b S3b) e^{-2 pi i k.x / N}, and C_i(k) the same way; each multiplied by the
//      alive mask of step 3 of the 2LPT definition and 0 at k = 0.
//   4. Third-order displacement.  psi3_j(k) = i k_j P3(k) / k^2 - g3c i (k x C(k))_j / k^2.
//   5. Records.  displacement = psi1 + psi2 + psi3, velocity = alpha psi1 + f2 psi2 + f3 psi3.
//   6. Defaults, given at f_cluster = 1 only: g3a = -1/3, g3b = +10/21, g3c = +1/7, f3 = 3 (= 3 alpha).  In the usual notation
//        x = q - D grad phi1 - (3/7) D^2 grad phi2 + (1/3) D^3 grad phi3a - (10/21) D^3 grad phi3b + (1/7) D^3 curl A3c,
//      lap phi2 = S, lap A3c = grad phi2_{,l} x grad phi1_{,l}; phi2_{,ab} = T_ab[S], phi1_{,ab} = T_ab[D].  zd_params.lpt3_terms leaves
//      terms out (bit 1 = 3a, 2 = 3b, 4 = 3c): a term that is out has coefficient 0.
//
// AS BUILT
//   Third-order round (zd_capi_rounds.cpp make_lpt3_sources; once per plan, after the second-order round, S(k) resident, stream factor 1).
//   Six pair passes ab = xx, yy, zz, xy, xz, yz over the ONE complex array of the second-order round's plan: k_gen_lpt3<2> packs
//   T_ab[D] + i T_ab[S] (the real, even coefficient k_a k_b / k^2 applied to the regenerated D and to S(k) read at the mode) ->
//   k_zfft -> k_yfft -> k_xlpt3, which transforms an x line in registers and writes Re and Im to two real N^3 arrays.  The twelve
//   fields take 96 N^3 bytes; with the 16 N^3 store and S(k) the round peaks at 120 N^3 bytes (129 GB at 1024: the size limit).
//   k_lpt3_point reads the twelve fields at a site and writes g3a S3a + g3b S3b, C_x, C_y, C_z over T_xx, T_yy, T_zz, T_xy of D
//   (96 B read, 32 B written per site; 16-byte accesses, no LDS).  The other eight fields are freed, the four results go one after the
//   other through k_xfwd3 (row / N^3, forward x transform into the store) and k_yfwd, k_zfwd of the f_NL round into four half-space
//   arrays [ky][kz][x] laid out like S(k).  Resident afterwards: S(k), P3(k), C_x,y,z(k) = 40 N^3 bytes.
//   Final pass: k_gen_lpt3<7> forms the seven jobs of the reference's four arrays as k_gen_lpt2<7> does, with the vector amplitudes
//        Q_j = s_j (D + gamma S + P3) + T_j,   V_j = s_j (alpha D + f2 gamma S + f3 P3) + f3 T_j,   T = -g3c (s x C),
//   s_j = k_j fundamental / k^2, in the places of s_j P and s_j V (q_j = i Q_j, v_j = i V_j).  A mode the mask kills contributes nothing.
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

__constant__ zdpcg::BitTable c_bits_l3;

extern "C" int zdk_upload_bit_table_lpt3(const zdpcg::BitTable *host) {
    return (int) hipMemcpyToSymbol(HIP_SYMBOL(c_bits_l3), host, sizeof(zdpcg::BitTable));
}

namespace {

__device__ __forceinline__ u128 advance_bits_l3(u128 s, uint64_t delta) {
    for (int i = 0; i < zdpcg::NBITS; i++) {
        if ((delta >> i) == 0) break;
        if ((delta >> i) & 1ULL) s = zdpcg::apply(c_bits_l3.m[i], s);
    }
    return s;
}

// the alive mask of the definition (lpt2_masked, zd_kernels_lpt2.hip)
__device__ __forceinline__ bool lpt3_masked(const GenConst &g, int kx, int ky, int kz, int k2i, double k2v) {
    const int ax = kx < 0 ? -kx : kx, az = kz < 0 ? -kz : kz;
    if (k2i == 0 || ax == g.kmax || az == g.kmax || ky == g.kmax) return true;
    return !g.corner_modes && k2v >= g.k2_cutoff;
}

__device__ __forceinline__ void rotate(double &r, double &i, const cplx w) {
    const double a = r * w.x - i * w.y, b = r * w.y + i * w.x;
    r = a;
    i = b;
}

// k_gen_lpt3: the mode walk of k_gen_lpt2 (zd_kernels_lpt2.hip) with the amplitudes and coefficients of the third order.
//   NJ = 2, g.lpt3 = 1 .. 6: the Hessian pair of that pass (xx, yy, zz, xy, xz, yz), jobs c (D + i S) and c (D - i S) with
//           c = k_a k_b / k^2 (JOB_G2_SELF / _TWIN; c real and even in k)
//   NJ = 7, g.lpt3 = 7: the final pass, the reference's seven jobs (JOB_A_SELF .. JOB_D_TWIN) with D and the vector amplitudes Q_j, V_j
//           of the header in the places of D, s_j D and f s_j D
// grid: (ceil(N / GEN_BX), L / GEN_ZR, nky)  block: GEN_BX
template <int NJ, bool PLAW>
__global__ __launch_bounds__(GEN_BX) void k_gen_lpt3(GenConst g, GenJumps J, StoreLayout S, int zW, int ky0, int nky, int L, int residue,
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
        s = advance_bits_l3(g.row_state[ky], 2ULL * ((uint64_t) (kz0 & 65535) * 65536ULL + (uint64_t) (kx & 65535)) + 1ULL);
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
                const u128 t = advance_bits_l3(g.row_state[0], 2ULL * ((uint64_t) (kzs & 65535) * 65536ULL + (uint64_t) (kxs & 65535)) + 1ULL);
                r1 = zdpcg::output(t);
                r2 = zdpcg::output(zdpcg::step(t));
            }
            const int kxm = xs > half ? xs - N : xs, kzm = zs > half ? zs - N : zs;  // generated mode
            const int k2i = kxm * kxm + ky * ky + kzm * kzm;
            const double k2v = (double) k2i * g.fundamental2;
            if (lpt3_masked(g, kxm, ky, kzm, k2i, k2v)) continue;
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
            // the resident spectra of the source mode (half-space rows [ky][kz][x], one rank)
            const long long at = ((long long) ky * N + zs) * N + xs;
            const cplx sk = g.lpt2_sk[at];
            const cplx w  = R > 1 ? twN[modn(N, k1 * residue * L)] : cplx{1.0, 0.0};  // W_R^{k1 r}
            if constexpr (NJ == 2) {
                double sr = sk.x, si = sk.y;
                if (cj) {  // conjugated copy of the mode at -k; the coefficient is even
                    di = -di;
                    si = -si;
                }
                if (R > 1) {
                    rotate(dr, di, w);
                    rotate(sr, si, w);
                }
                // k_a k_b / k^2 in integer wavenumbers (the fundamentals cancel)
                const double fx = (double) kxm, fy = (double) ky, fz = (double) kzm;
                double c;
                switch (g.lpt3) {
                    case 1: c = fx * fx; break;
                    case 2: c = fy * fy; break;
                    case 3: c = fz * fz; break;
                    case 4: c = fx * fy; break;
                    case 5: c = fx * fz; break;
                    default: c = fy * fz; break;
                }
                c /= (double) k2i;
                accr[0] += c * (dr - si);  // c (D + i S)
                acci[0] += c * (di + sr);
                accr[1] += c * (dr + si);  // c (D - i S)
                acci[1] += c * (di - sr);
            } else {
                const cplx p3 = g.lpt3_p3[at], cx = g.lpt3_c[0][at], cy = g.lpt3_c[1][at], cz = g.lpt3_c[2][at];
                // longitudinal amplitudes: P = D + gamma S + P3, W = alpha D + f2 gamma S + f3 P3
                const double pr = dr + g.lpt2_gamma * sk.x + p3.x, pi = di + g.lpt2_gamma * sk.y + p3.y;
                const double wr = g.lpt2_alpha * dr + g.lpt2_f2g * sk.x + g.lpt3_f3 * p3.x;
                const double wi = g.lpt2_alpha * di + g.lpt2_f2g * sk.y + g.lpt3_f3 * p3.y;
                const double sx = (double) kxm * g.fundamental * ik2, sy = (double) ky * g.fundamental * ik2, sz = (double) kzm * g.fundamental * ik2;
                // transverse vector T = -g3c (s x C)
                const double txr = -g.lpt3_g3c * (sy * cz.x - sz * cy.x), txi = -g.lpt3_g3c * (sy * cz.y - sz * cy.y);
                const double tyr = -g.lpt3_g3c * (sz * cx.x - sx * cz.x), tyi = -g.lpt3_g3c * (sz * cx.y - sx * cz.y);
                const double tzr = -g.lpt3_g3c * (sx * cy.x - sy * cx.x), tzi = -g.lpt3_g3c * (sx * cy.y - sy * cx.y);
                double qr[3] = {sx * pr + txr, sy * pr + tyr, sz * pr + tzr}, qi[3] = {sx * pi + txi, sy * pi + tyi, sz * pi + tzi};
                double vr[3] = {sx * wr + g.lpt3_f3 * txr, sy * wr + g.lpt3_f3 * tyr, sz * wr + g.lpt3_f3 * tzr};
                double vi[3] = {sx * wi + g.lpt3_f3 * txi, sy * wi + g.lpt3_f3 * tyi, sz * wi + g.lpt3_f3 * tzi};
                if (cj) {  // conjugated copy of the mode at -k: D -> conj D, Q(-k) = -conj Q(k), V likewise
                    di = -di;
#pragma unroll
                    for (int j = 0; j < 3; j++) {
                        qr[j] = -qr[j];
                        vr[j] = -vr[j];
                    }
                }
                if (R > 1) {
                    rotate(dr, di, w);
#pragma unroll
                    for (int j = 0; j < 3; j++) {
                        rotate(qr[j], qi[j], w);
                        rotate(vr[j], vi[j], w);
                    }
                }
                // JOB_A_SELF D - Q_x | JOB_A_TWIN D + Q_x: the density from D, qx = i Q_x
                accr[0] += dr - qr[0];
                acci[0] += di - qi[0];
                accr[1] += dr + qr[0];
                acci[1] += di + qi[0];
                // JOB_B_SELF -Q_z + i Q_y | JOB_B_TWIN Q_z + i Q_y
                accr[2] += -qi[1] - qr[2];
                acci[2] += qr[1] - qi[2];
                accr[3] += -qi[1] + qr[2];
                acci[3] += qr[1] + qi[2];
                // JOB_C_BOTH -V_x | JOB_D_SELF -V_z + i V_y | JOB_D_TWIN V_z + i V_y
                accr[4] -= vr[0];
                acci[4] -= vi[0];
                accr[5] += -vi[1] - vr[2];
                acci[5] += vr[1] - vi[2];
                accr[6] += -vi[1] + vr[2];
                acci[6] += vr[1] + vi[2];
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

// k_xlpt3: rows of the one-array store in a pair pass (k_xlpt2's shape): inverse x transform in registers; the line then holds
// T_ab[D](x) + i T_ab[S](x).  td[(z N + y) N + x] = Re, ts[(z N + y) N + x] = Im.
//   grid: (N / ROWS, nplanes)   block: ROWS * N / E
template <int N, int E, int ROWS>
__global__ __launch_bounds__(ROWS *N / E) void k_xlpt3(StoreLayout S, const cplx *__restrict__ tw, const cplx *__restrict__ data,
                                                      double *__restrict__ td, double *__restrict__ ts) {
    using PL  = zdfft::Plan<N, E>;
    using LDS = zdfft::LineInner<N, ROWS>;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr int T = PL::T;
    const int t = threadIdx.x % T, row = threadIdx.x / T;
    const int y = blockIdx.x * ROWS + row, pl = blockIdx.y;
    const cplx *p = data + row_offset(S, pl, 0, y);
    double re[E], im[E];
#pragma unroll
    for (int e = 0; e < E; e++) {
        const cplx v = p[t + T * e];
        re[e] = v.x;
        im[e] = v.y;
    }
    zdfft::fft_line<PL, LDS>(re, im, t, row, lds, tw);
    const long long line = ((long long) pl * N + y) * N;
    int t2 = t;
    asm volatile("" : "+v"(t2));  // keep the address arithmetic behind the transform (register pressure, as in k_xphi)
#pragma unroll
    for (int e = 0; e < E; e++) {
        td[line + t2 + T * e] = re[e];
        ts[line + t2 + T * e] = im[e];
    }
}

// k_xfwd3: the way back: row (z, y) of the real field src, scaled by N^-3, transformed forward (conj o inverse o conj; the input is
// real) into the row of the one-array store, where k_yfwd and k_zfwd (zd_kernels.hip) take over.
//   grid: (N / ROWS, nplanes)   block: ROWS * N / E
template <int N, int E, int ROWS>
__global__ __launch_bounds__(ROWS *N / E) void k_xfwd3(StoreLayout S, double inv_ppd3, const cplx *__restrict__ tw, const double *__restrict__ src,
                                                      cplx *__restrict__ data) {
    using PL  = zdfft::Plan<N, E>;
    using LDS = zdfft::LineInner<N, ROWS>;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr int T = PL::T;
    const int t = threadIdx.x % T, row = threadIdx.x / T;
    const int y = blockIdx.x * ROWS + row, pl = blockIdx.y;
    const double *a = src + ((long long) pl * N + y) * N;
    double re[E], im[E];
#pragma unroll
    for (int e = 0; e < E; e++) {
        re[e] = a[t + T * e] * inv_ppd3;
        im[e] = 0.0;
    }
    zdfft::fft_line<PL, LDS>(re, im, t, row, lds, tw);
    cplx *p = data + row_offset(S, pl, 0, y);
    int t2 = t;
    asm volatile("" : "+v"(t2));
#pragma unroll
    for (int e = 0; e < E; e++) p[t2 + T * e] = cplx{re[e], -im[e]};
}

// k_lpt3_point: step 2 at two neighbouring sites per thread.  Reads the twelve Hessian fields (order xx, yy, zz, xy, xz, yz), writes
// g3a S3a + g3b S3b over d[0] and C_x, C_y, C_z over d[1], d[2], d[3]: every site is read in full before it is written, by the one
// thread that owns it.  n2 = N^3 / 2.
//   grid: ceil(n2 / 256)   block: 256
__global__ __launch_bounds__(256) void k_lpt3_point(Lpt3Fields F, double g3a, double g3b, long long n2) {
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    if (i >= n2) return;
    double2 d[6], s[6];
#pragma unroll
    for (int f = 0; f < 6; f++) {
        d[f] = reinterpret_cast<const double2 *>(F.d[f])[i];
        s[f] = reinterpret_cast<const double2 *>(F.s[f])[i];
    }
    double2 out[4];
#pragma unroll
    for (int h = 0; h < 2; h++) {
        double D[6], Sg[6];
#pragma unroll
        for (int f = 0; f < 6; f++) {
            D[f]  = h ? d[f].y : d[f].x;
            Sg[f] = h ? s[f].y : s[f].x;
        }
        const double dxx = D[0], dyy = D[1], dzz = D[2], dxy = D[3], dxz = D[4], dyz = D[5];
        const double sxx = Sg[0], syy = Sg[1], szz = Sg[2], sxy = Sg[3], sxz = Sg[4], syz = Sg[5];
        const double det = dxx * (dyy * dzz - dyz * dyz) - dxy * (dxy * dzz - dyz * dxz) + dxz * (dxy * dyz - dyy * dxz);
        const double s3b = 0.5 * ((sxx + syy + szz) * (dxx + dyy + dzz) - (sxx * dxx + syy * dyy + szz * dzz)) - (sxy * dxy + sxz * dxz + syz * dyz);
        const double p   = g3a * det + g3b * s3b;
        // C_i = eps_ijk sum_l T_jl[S] T_kl[D]
        const double cx = (sxy * dxz + syy * dyz + syz * dzz) - (sxz * dxy + syz * dyy + szz * dyz);
        const double cy = (sxz * dxx + syz * dxy + szz * dxz) - (sxx * dxz + sxy * dyz + sxz * dzz);
        const double cz = (sxx * dxy + sxy * dyy + sxz * dyz) - (sxy * dxx + syy * dxy + syz * dxz);
        if (h) {
            out[0].y = p;
            out[1].y = cx;
            out[2].y = cy;
            out[3].y = cz;
        } else {
            out[0].x = p;
            out[1].x = cx;
            out[2].x = cy;
            out[3].x = cz;
        }
    }
#pragma unroll
    for (int f = 0; f < 4; f++) reinterpret_cast<double2 *>(F.d[f])[i] = out[f];
}

template <int NJ, bool PLAW>
int launch_gen_lpt3_t(const GenConst &g, const GenJumps &J, const StoreLayout &S, int ky0, int nky, int L, int residue, const void *twN,
                      void *Y, hipStream_t st) {
    const int N = g.N;
    dim3 grid((N + GEN_BX - 1) / GEN_BX, L / GEN_ZR, nky), block(GEN_BX);
    const int zw = zfft_tile_width(L) > 0 ? zfft_tile_width(L) : 16;
    hipLaunchKernelGGL((k_gen_lpt3<NJ, PLAW>), grid, block, 0, st, g, J, S, zw, ky0, nky, L, residue, (const cplx *) twN, (cplx *) Y);
    ZD_LAUNCH_CHECK();
    return 0;
}

template <int N, int E, int ROWS>
int launch_lpt3_xpair_t(const StoreLayout &S, const void *tw, const void *data, double *td, double *ts, int nplanes, hipStream_t st) {
    constexpr int threads = ROWS * N / E;
    const size_t shmem = sizeof(double) * zdfft::LineInner<N, ROWS>::SIZE;
    ZD_PROBE_RETURN();
    set_dyn_lds<k_xlpt3<N, E, ROWS>>(shmem);
    hipLaunchKernelGGL((k_xlpt3<N, E, ROWS>), dim3(N / ROWS, nplanes), dim3(threads), shmem, st, S, (const cplx *) tw, (const cplx *) data, td, ts);
    ZD_LAUNCH_CHECK();
    return 0;
}

template <int N, int E, int ROWS>
int launch_lpt3_xfwd_t(const StoreLayout &S, const void *tw, const double *src, void *data, int nplanes, hipStream_t st) {
    constexpr int threads = ROWS * N / E;
    const size_t shmem = sizeof(double) * zdfft::LineInner<N, ROWS>::SIZE;
    ZD_PROBE_RETURN();
    set_dyn_lds<k_xfwd3<N, E, ROWS>>(shmem);
    const double inv = 1. / N / N / N;
    hipLaunchKernelGGL((k_xfwd3<N, E, ROWS>), dim3(N / ROWS, nplanes), dim3(threads), shmem, st, S, inv, (const cplx *) tw, src, (cplx *) data);
    ZD_LAUNCH_CHECK();
    return 0;
}

}  // namespace

namespace zd {

int launch_gen_lpt3(const GenConst &g, const GenJumps &J, const JobList &jobs, const StoreLayout &S, int ky0, int nky, int L, int residue,
                    const void *twN, void *Y, hipStream_t st) {
    if (L % GEN_ZR || g.N % L || !g.lpt2_sk) return 2;
#define GCASE(nj)                                                                                                 \
    return g.is_powerlaw ? launch_gen_lpt3_t<nj, true>(g, J, S, ky0, nky, L, residue, twN, Y, st)                 \
                         : launch_gen_lpt3_t<nj, false>(g, J, S, ky0, nky, L, residue, twN, Y, st);
    if (g.lpt3 >= 1 && g.lpt3 <= 6 && jobs.n == 2) GCASE(2)
    if (g.lpt3 == 7 && jobs.n == 7 && g.lpt3_p3 && g.lpt3_c[0] && g.lpt3_c[1] && g.lpt3_c[2]) GCASE(7)
#undef GCASE
    ZD_TABLE_MISS("zeldovich_hip: no third-order generator for pass %d with %d jobs\n", g.lpt3, jobs.n);
    return 2;
}

// (the row counts of launch_lpt2_xsrc; the round's memory stops it at 1024)
int launch_lpt3_xpair(const StoreLayout &S, const void *tw, const void *data, double *td, double *ts, int nplanes, hipStream_t st) {
    if (S.narray != 1) return 2;
#define LCASE(n, e, rows) \
    case n: return launch_lpt3_xpair_t<n, e, rows>(S, tw, data, td, ts, nplanes, st);
    switch (S.N) {
        LCASE(32, 16, 32)
        LCASE(64, 16, 32)
        LCASE(128, 16, 32)
        LCASE(256, 16, 16)
        LCASE(512, 16, 8)
        LCASE(1024, 16, 4)
    }
#undef LCASE
    ZD_TABLE_MISS("zeldovich_hip: the third-order round supports PPD = 32..1024 (power of two), got %d\n", S.N);
    return 2;
}

int launch_lpt3_xfwd(const StoreLayout &S, const void *tw, const double *src, void *data, int nplanes, hipStream_t st) {
    if (S.narray != 1) return 2;
#define LCASE(n, e, rows) \
    case n: return launch_lpt3_xfwd_t<n, e, rows>(S, tw, src, data, nplanes, st);
    switch (S.N) {
        LCASE(32, 16, 32)
        LCASE(64, 16, 32)
        LCASE(128, 16, 32)
        LCASE(256, 16, 16)
        LCASE(512, 16, 8)
        LCASE(1024, 16, 4)
    }
#undef LCASE
    ZD_TABLE_MISS("zeldovich_hip: the third-order round supports PPD = 32..1024 (power of two), got %d\n", S.N);
    return 2;
}

int launch_lpt3_point(const Lpt3Fields &F, double g3a, double g3b, long long nsites, hipStream_t st) {
    const long long n2 = nsites / 2;  // (N^3 is even)
    hipLaunchKernelGGL(k_lpt3_point, dim3((unsigned) ((n2 + 255) / 256)), dim3(256), 0, st, F, g3a, g3b, n2);
    ZD_LAUNCH_CHECK();
    return 0;
}

}  // namespace zd
