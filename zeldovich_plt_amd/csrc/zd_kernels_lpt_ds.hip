// zd_kernels_lpt_ds.hip — ZD_q2LPT / ZD_q3LPT plans check themselves and report their power: direct summation of the first, second
// and third order at sample sites, and the band power of the same amplitudes (zd_plan_lpt_direct_sum / zd_lpt_direct_sum,
// zd_plan_lpt_power / zd_lpt_power, include/zeldovich_hip.h).  No FFT, no block store, no scatter: after plan creation an LPT plan
// keeps S(k) — with the third order also P3(k) and C_x,y,z(k) — resident as half-space rows [ky][kz][x] (GenConst::lpt2_sk, lpt3_p3,
// lpt3_c), and a delivered record is the unnormalised inverse transform of amplitudes that are linear in them.
//
// DEFINITION
//   Notation of zd_kernels_lpt2.hip and zd_kernels_lpt3.hip: s_j = k_j fundamental / k^2 with signed integer wavenumbers
//   (-N/2 < k_i <= N/2), the alive mask lpt2_masked (the zero rule without the one-mode filter), k = 0 excluded.  Per mode
//        order 1   Q1_j = s_j D               V1_j = alpha Q1_j     D regenerated from its counter under the zero rule, the one-mode
//                                                                   filter included (k_ds_sweep / sweep_modes)
//        order 2   Q2_j = s_j gamma S(k)      V2_j = f2 Q2_j
//        order 3   Q3_j = s_j P3(k) + T_j     V3_j = f3 Q3_j        T = -g3c (s x C(k))
//   gamma = -lpt2_ratio, alpha = lpt2_alpha, f2, g3c, f3 as zd_route.h resolves them.  Orders 2 and 3 are restricted to the alive mask;
//   order 3 is zero on a plan without ZD_q3LPT.  One-mode plans (ZD_qonemode): a single plane wave has no higher order — psi1_{a,b} is
//   proportional to k_a k_b, so S = sum_{a<b} [psi1_{a,a} psi1_{b,b} - (psi1_{a,b})^2], det T[D] and, with S, S3b and C vanish
//   identically — and orders 2 and 3 ARE zero there: what the rounds leave in the arrays of such a plan is their rounding residue (1e-26
//   of the first order at PPD 64), which the sums do not report; the spectral kernel is not launched and the power sweep reads nothing.
//   Everywhere else S, P3 and C enter AS THE PLAN HOLDS THEM: the sums pin the final pass of a run
//   (k_gen_lpt2<7> / k_gen_lpt3<7>, the z, y, x stages, the four-array epilogue, any stream factor), not the rounds that made the spectra.
//   Sites.  field(x) = sum_k i Q_j(k) e^{+2 pi i k.x / N} over all N^3 signed wavevectors.  A half-space row ky >= 1 stands for itself
//          and its Hermitian twin and contributes 2 Re; the plane ky = 0 is summed position by position, each position with its own
//          entry of the resident arrays, taking the real part.  out18[site][order 1, 2, 3][qx, qy, qz, vx, vy, vz]; the delivered
//          record is the sum over the orders.
//   Power. Bins, Hermitian counting and the count of zd_kernels_pk.hip (the modes the zero rule leaves alive, the one-mode filter
//          included).  Per bin: count, sum_k, sum_input = sum P(|k|), sum_dens = sum |D|^2, sum_disp1 = sum_j |Q1_j|^2, sum_disp2,
//          sum_disp3, sum_disp = sum_j |Q1_j + Q2_j + Q3_j|^2, sum_vel = sum_j |V1_j + V2_j + V3_j|^2.
//   Refusals.  A plan or parameters without ZD_q2LPT = 1; whatever lpt2_refusal, lpt2_dealias_refusal and lpt3_refusal refuse; fewer
//          than 1 or more than 64 sites, a site outside [0, N)^3, NULL arrays; bin_width < 1 or fewer bins than zd_power_nbins.
//
// k_ds_lpt<O3, NS>: the higher orders at NS sites, a pure spectral sum (no RNG, no transform).  One thread per x walks every z of a
//   half-space row ky < N/2 (the row ky = N/2 does not exist in the arrays) and reads S — with O3 also P3, C_x, C_y, C_z — with 16-byte
//   loads coalesced along x: 8 N^3 bytes (2LPT) or 40 N^3 bytes (3LPT) per launch group.  V = f Q within an order, so three sums per
//   order and site are kept (the host scales by f2 / f3).  Phases as in the FAST rows of k_ds_sweep: (kx x + ky y + kz z) mod N in
//   integers, looked up in the plan's length-N table, re-seeded every DS_RESEED z steps and rotated by the site's e^{2 pi i z_s / N}
//   in between; no sincos of an unreduced argument.  Lanes with x >= N and masked modes load nothing.  thread -> wave (shuffles) ->
//   workgroup (LDS) -> one partial per workgroup -> k_ds_reduce (zd_kernels_ds.hip), every step in a fixed order, no floating-point
//   atomics: two calls on one plan return the same bits.  The first order comes from k_ds_sweep on the plan's GenConst with
//   vnorm = lpt2_alpha (ds_sweep_sites).
// k_pk_lpt<O3, PLAW, FAST>: the walk of k_pk_sweep (sweep_modes, draws included: the total needs D at the mode); the resident spectra
//   are read at the generated mode's own indices, as the sweep reads PhiK on a ZD_f_NL plan.  Binning as in k_pk_sweep: runs in
//   registers, an LDS window of PK_WIN bins per workgroup, global double atomics for the flush; counts are integer atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "zd_plan.h"
#include "zd_launch.h"
#include "zd_genmath.h"
#include "zd_sweep.h"
#include "zd_route.h"

using namespace zd;
using zdfft::cplx;
using namespace zdgen;
using zdsweep::DsSites;
using zdsweep::DS_BX;
using zdsweep::DS_NS;
using zdsweep::DS_RESEED;
using zdsweep::DS_MAX_SITES;
using zdsweep::SweepJumps;
using zdsweep::SweepMode;

namespace {

// the alive mask of the definition (lpt2_masked, zd_kernels_lpt2.hip)
__device__ __forceinline__ bool lptds_masked(const GenConst &g, int kx, int ky, int kz, int k2i, double k2v) {
    const int ax = kx < 0 ? -kx : kx, az = kz < 0 ? -kz : kz;
    if (k2i == 0 || ax == g.kmax || az == g.kmax || ky == g.kmax) return true;
    return !g.corner_modes && k2v >= g.k2_cutoff;
}

// the higher-order vector amplitudes of a mode from the resident spectra at element `at`: q2_j = s_j gamma S, and with O3
// q3_j = s_j P3 + T_j, T = -g3c (s x C) (the arithmetic of k_gen_lpt3<7>)
template <bool O3>
__device__ __forceinline__ void lpt_amplitudes(const GenConst &g, long long at, const double (&s)[3], double (&q2r)[3], double (&q2i)[3],
                                               double (&q3r)[3], double (&q3i)[3]) {
    const cplx sk = g.lpt2_sk[at];
    const double ar = g.lpt2_gamma * sk.x, ai = g.lpt2_gamma * sk.y;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        q2r[j] = s[j] * ar;
        q2i[j] = s[j] * ai;
    }
    if constexpr (O3) {
        const cplx p3 = g.lpt3_p3[at], cx = g.lpt3_c[0][at], cy = g.lpt3_c[1][at], cz = g.lpt3_c[2][at];
        const double c3 = -g.lpt3_g3c;
        q3r[0] = s[0] * p3.x + c3 * (s[1] * cz.x - s[2] * cy.x), q3i[0] = s[0] * p3.y + c3 * (s[1] * cz.y - s[2] * cy.y);
        q3r[1] = s[1] * p3.x + c3 * (s[2] * cx.x - s[0] * cz.x), q3i[1] = s[1] * p3.y + c3 * (s[2] * cx.y - s[0] * cz.y);
        q3r[2] = s[2] * p3.x + c3 * (s[0] * cy.x - s[1] * cx.x), q3i[2] = s[2] * p3.y + c3 * (s[0] * cy.y - s[1] * cx.y);
    } else {
#pragma unroll
        for (int j = 0; j < 3; j++) q3r[j] = q3i[j] = 0.0;
    }
}

// ---- the higher orders at sample sites ----
// grid: (ceil(N / DS_BX), nrows)  block: DS_BX;  partial[(row * gridDim.x + blockIdx.x) * NS * NQ + site * NQ + q], NQ = 3 (6 with O3):
// order 2 x, y, z (then order 3 x, y, z)
template <bool O3, int NS>
__global__ __launch_bounds__(DS_BX) void k_ds_lpt(GenConst g, DsSites<NS> S, int ky_first, const cplx *__restrict__ twN, double *__restrict__ partial) {
    constexpr int NQ = O3 ? 6 : 3, NV = NS * NQ;
    __shared__ double stage[(DS_BX / 64) * NV];
    const int N = g.N, half = g.half;
    const int ky = ky_first + (int) blockIdx.y;
    const int x0 = (int) blockIdx.x * DS_BX;
    const bool act = x0 + (int) threadIdx.x < N;
    const int x  = act ? x0 + (int) threadIdx.x : 0;
    const int kx = x > half ? x - N : x;
    const double weight = ky != 0 ? 2.0 : 1.0;  // a half-space row ky >= 1 stands for itself and its Hermitian twin
    double acc[NS][NQ];
#pragma unroll
    for (int s = 0; s < NS; s++)
#pragma unroll
        for (int q = 0; q < NQ; q++) acc[s][q] = 0.0;
    cplx ph[NS];  // the sites' phases at position (x, zlast)
    int zlast = -2, zseed = 0;
    const int kxy2 = kx * kx + ky * ky;
    const long long row = (long long) ky * N * N + x;
#pragma unroll 1
    for (int z = 0; z < N; z++) {
        const int kz  = z > half ? z - N : z;
        const int k2i = kxy2 + kz * kz;
        const double k2v = (double) k2i * g.fundamental2;
        const bool live = act && !lptds_masked(g, kx, ky, kz, k2i, k2v);
        if (!__any(live)) continue;  // (wave-uniform: whole waves skip, never single lanes)
        if (z != zlast + 1 || z - zseed >= DS_RESEED) {
#pragma unroll
            for (int s = 0; s < NS; s++) ph[s] = twN[modn(N, x * S.x[s] + ky * S.y[s] + z * S.z[s])];
            zseed = z;
        } else {
#pragma unroll
            for (int s = 0; s < NS; s++) {
                const double c = ph[s].x, sn = ph[s].y;
                ph[s].x = fma(c, S.wr[s], -sn * S.wi[s]);
                ph[s].y = fma(c, S.wi[s], sn * S.wr[s]);
            }
        }
        zlast = z;
        if (!live) continue;  // a masked mode or a lane beyond the row: nothing is read, nothing is added
        const double q = weight * g.fundamental / k2v;
        const double sj[3] = {(double) kx * q, (double) ky * q, (double) kz * q};
        double q2r[3], q2i[3], q3r[3], q3i[3];
        lpt_amplitudes<O3>(g, row + (long long) z * N, sj, q2r, q2i, q3r, q3i);
#pragma unroll
        for (int s = 0; s < NS; s++) {  // Re(i Q e^{i t}) = -(Q_r sin t + Q_i cos t)
            const double c = ph[s].x, sn = ph[s].y;
#pragma unroll
            for (int j = 0; j < 3; j++) {
                acc[s][j] -= fma(q2r[j], sn, q2i[j] * c);
                if constexpr (O3) acc[s][3 + j] -= fma(q3r[j], sn, q3i[j] * c);
            }
        }
    }
    // thread -> wave -> workgroup, every step in a fixed order
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int s = 0; s < NS; s++)
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            double v = acc[s][q];
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
            if (lane == 0) stage[wave * NV + s * NQ + q] = v;
        }
    __syncthreads();
    if (threadIdx.x < NV) {
        double v = stage[threadIdx.x];
        for (int w = 1; w < DS_BX / 64; w++) v += stage[w * NV + threadIdx.x];
        partial[((size_t) blockIdx.y * gridDim.x + blockIdx.x) * NV + threadIdx.x] = v;
    }
}

template <bool O3>
int launch_ds_lpt_t(const GenConst &g, const DsSites<DS_NS> &S, int nrows, const cplx *twN, double *partial, hipStream_t st) {
    hipLaunchKernelGGL((k_ds_lpt<O3, DS_NS>), dim3((g.N + DS_BX - 1) / DS_BX, nrows), dim3(DS_BX), 0, st, g, S, 0, twN, partial);
    ZD_LAUNCH_CHECK();
    return 0;
}

// ---- band power ----
constexpr int PK_BX  = 256;  // threads (consecutive x) per workgroup
constexpr int PK_ZC  = 256;  // z indices one thread walks
constexpr int PK_WIN = 384;  // bins of the LDS window (zd_kernels_pk.hip)
constexpr int PL_NV  = 8;    // sum_k, sum_input, sum_dens, sum_disp1, sum_disp2, sum_disp3, sum_disp, sum_vel

// floor(sqrt(k2i)) from an approximate root
__device__ __forceinline__ int lpt_isqrt_fix(int k2i, double root) {
    int s = (int) root;
    if (s * s > k2i) s--;
    else if ((s + 1) * (s + 1) <= k2i) s++;
    return s;
}

// grid: (ceil(N / PK_BX), ceil(N / zc), nrows)  block: PK_BX;  gsum[column][nbins]
template <bool O3, bool PLAW, bool FAST>
__global__ __launch_bounds__(PK_BX) void k_pk_lpt(GenConst g, SweepJumps J, int ky_first, int lG, int zc, int w, int nbins, double f2, double f3,
                                                   unsigned long long *__restrict__ gcount, double *__restrict__ gsum) {
    extern __shared__ double pl_lds[];
    const int ntab = FAST ? g.genf_n : 0;
    double *T      = pl_lds;         // LDS image of k_genf (FAST)
    double *wsum   = pl_lds + ntab;  // [PL_NV][PK_WIN]
    unsigned *wcnt = reinterpret_cast<unsigned *>(wsum + PL_NV * PK_WIN);
    const int N = g.N, half = g.half;
    for (int i = threadIdx.x; i < ntab; i += PK_BX) T[i] = g.genf_tab[i];
    for (int i = threadIdx.x; i < PL_NV * PK_WIN; i += PK_BX) wsum[i] = 0.0;
    for (int i = threadIdx.x; i < PK_WIN; i += PK_BX) wcnt[i] = 0u;
    const int ky  = ky_first + (int) blockIdx.z;
    const int x0  = (int) blockIdx.x * PK_BX, xl = min(N - 1, x0 + PK_BX - 1);
    const int z0  = (int) blockIdx.y * zc, z1 = min(N, z0 + zc);
    const bool act = x0 + (int) threadIdx.x < N;
    const int x   = act ? x0 + (int) threadIdx.x : 0;
    int bmin;  // first bin of the window: |k_i| of an index is a tent, so its minimum over a range sits at an end
    {
        auto tent = [&](int i) { return i > half ? N - i : i; };
        const int ax = min(tent(x0), tent(xl)), az = min(tent(z0), tent(z1 - 1));
        const int k2 = ax * ax + ky * ky + az * az;
        const int s  = lpt_isqrt_fix(k2, sqrt((double) k2));
        bmin = w == 1 ? s : s / w;
    }
    __syncthreads();
    const unsigned weight = ky != 0 ? 2u : 1u;  // a half-space row ky >= 1 stands for itself and its Hermitian twin
    int run_b = -1;
    unsigned run_n = 0;
    double run_v[PL_NV];
#pragma unroll
    for (int j = 0; j < PL_NV; j++) run_v[j] = 0.0;
    auto flush = [&]() {
        if (run_n == 0) return;
        const int i = run_b - bmin;
        if (i >= 0 && i < PK_WIN) {
            atomicAdd(&wcnt[i], run_n);
#pragma unroll
            for (int j = 0; j < PL_NV; j++) unsafeAtomicAdd(&wsum[j * PK_WIN + i], run_v[j]);
        } else if (run_b < nbins) {
            atomicAdd(&gcount[run_b], (unsigned long long) run_n * weight);
#pragma unroll
            for (int j = 0; j < PL_NV; j++) unsafeAtomicAdd(&gsum[(size_t) j * nbins + run_b], run_v[j] * (double) weight);
        }
        run_n = 0;
#pragma unroll
        for (int j = 0; j < PL_NV; j++) run_v[j] = 0.0;
    };
    zdsweep::sweep_modes<PLAW, FAST>(g, J, T, ky, lG, x, act, z0, z1, false, [&](const SweepMode &m) {
        if (!m.live) return;  // (a zeroed position of a FAST wave, lanes beyond the row among them: nothing is read)
        const double d2 = FAST ? fma(m.dr, m.dr, m.di * m.di) : m.dr * m.dr + m.di * m.di;
        const double q = g.fundamental * m.ik2;
        const double sj[3] = {(double) m.kx * q, (double) ky * q, (double) m.kz * q};
        const int xs = m.kx < 0 ? m.kx + N : m.kx, zs = m.kz < 0 ? m.kz + N : m.kz;  // the generated mode's own indices
        double q2r[3] = {0.0, 0.0, 0.0}, q2i[3] = {0.0, 0.0, 0.0}, q3r[3] = {0.0, 0.0, 0.0}, q3i[3] = {0.0, 0.0, 0.0};
        if (!g.qonemode) lpt_amplitudes<O3>(g, ((long long) ky * N + zs) * N + xs, sj, q2r, q2i, q3r, q3i);  // (one plane wave: no higher order)
        double p1 = 0.0, p2 = 0.0, p3 = 0.0, pq = 0.0, pv = 0.0;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double q1r = sj[j] * m.dr, q1i = sj[j] * m.di;
            p1 += q1r * q1r + q1i * q1i;
            p2 += q2r[j] * q2r[j] + q2i[j] * q2i[j];
            p3 += q3r[j] * q3r[j] + q3i[j] * q3i[j];
            const double tr = q1r + q2r[j] + q3r[j], ti = q1i + q2i[j] + q3i[j];
            pq += tr * tr + ti * ti;
            const double vr = g.lpt2_alpha * q1r + f2 * q2r[j] + f3 * q3r[j], vi = g.lpt2_alpha * q1i + f2 * q2i[j] + f3 * q3i[j];
            pv += vr * vr + vi * vi;
        }
        const double root = FAST ? sqrt_pos((double) m.k2i) : sqrt((double) m.k2i);
        const int s = lpt_isqrt_fix(m.k2i, root);
        const int b = w == 1 ? s : s / w;
        if (b != run_b) {
            flush();
            run_b = b;
        }
        run_n++;
        run_v[0] += root * g.fundamental;
        run_v[1] += m.P;
        run_v[2] += d2;
        run_v[3] += p1;
        run_v[4] += p2;
        run_v[5] += p3;
        run_v[6] += pq;
        run_v[7] += pv;
    });
    flush();
    __syncthreads();
    for (int i = threadIdx.x; i < PK_WIN; i += PK_BX) {
        const unsigned n = wcnt[i];
        const int b = bmin + i;
        if (n == 0 || b >= nbins) continue;
        atomicAdd(&gcount[b], (unsigned long long) n * weight);
#pragma unroll
        for (int j = 0; j < PL_NV; j++) unsafeAtomicAdd(&gsum[(size_t) j * nbins + b], wsum[j * PK_WIN + i] * (double) weight);
    }
}

template <bool O3, bool PLAW, bool FAST>
int launch_pk_lpt_t(const GenConst &g, const SweepJumps &J, int ky_first, int nrows, int lG, int w, int nbins, double f2, double f3,
                    unsigned long long *gcount, double *gsum, hipStream_t st) {
    if (nrows <= 0) return 0;
    const int zc = std::min(g.N, PK_ZC);
    const size_t lds = sizeof(double) * ((FAST ? g.genf_n : 0) + PL_NV * PK_WIN) + sizeof(unsigned) * PK_WIN;
    set_dyn_lds<k_pk_lpt<O3, PLAW, FAST>>(lds > 65536 ? lds : 0);
    hipLaunchKernelGGL((k_pk_lpt<O3, PLAW, FAST>), dim3((g.N + PK_BX - 1) / PK_BX, (g.N + zc - 1) / zc, nrows), dim3(PK_BX), lds, st, g, J, ky_first,
                       lG, zc, w, nbins, f2, f3, gcount, gsum);
    ZD_LAUNCH_CHECK();
    return 0;
}

template <bool FAST>
int launch_pk_lpt(const GenConst &g, const SweepJumps &J, int ky_first, int nrows, int lG, int w, int nbins, double f2, double f3,
                  unsigned long long *gcount, double *gsum, hipStream_t st) {
    const bool o3 = g.lpt3_p3 != nullptr, plaw = g.is_powerlaw != 0;
#define PCASE(a, b) \
    if (o3 == a && plaw == b) return launch_pk_lpt_t<a, b, FAST>(g, J, ky_first, nrows, lG, w, nbins, f2, f3, gcount, gsum, st)
    PCASE(false, false);
    PCASE(false, true);
    PCASE(true, false);
    PCASE(true, true);
#undef PCASE
    return 1;
}

// what the parameters of an LPT sum must satisfy, asked before a plan or the GPU is touched; NULL: accepted
const char *lpt_params_refusal(const zd_params &p, const char *what, char *buf, size_t cap) {
    if (p.q2LPT != 1) {
        snprintf(buf, cap, "%s needs a ZD_q2LPT = 1 job: it sums the first, second and third order of an LPT run", what);
        return buf;
    }
    const char *why = zd::lpt2_refusal(&p, p.ngpu > 1 ? p.ngpu : 1);
    if (!why) why = zd::lpt2_dealias_refusal(&p);
    if (!why) why = zd::lpt3_refusal(&p);
    return why;
}

const char *lpt_sites_refusal(const zd_params &p, int64_t nsites, const int64_t *sites, double *out18, char *buf, size_t cap) {
    if (!sites || !out18) return "zd_plan_lpt_direct_sum needs a site array and an output array";
    if (nsites < 1 || nsites > DS_MAX_SITES) {
        snprintf(buf, cap, "the LPT direct summation takes 1 to %d sites per call (got %lld)", DS_MAX_SITES, (long long) nsites);
        return buf;
    }
    for (int64_t i = 0; i < 3 * nsites; i++)
        if (sites[i] < 0 || sites[i] >= p.ppd) {
            snprintf(buf, cap, "site %lld = (%lld, %lld, %lld) lies outside the lattice [0, %lld)^3", (long long) (i / 3), (long long) sites[i / 3 * 3],
                     (long long) sites[i / 3 * 3 + 1], (long long) sites[i / 3 * 3 + 2], (long long) p.ppd);
            return buf;
        }
    return nullptr;
}

const char *lpt_bins_refusal(const zd_params &p, int32_t bin_width, int64_t nbins, const int64_t *count, const double *sums8, char *buf, size_t cap) {
    if (!count || !sums8) return "zd_plan_lpt_power needs a count array and a sums array";
    const int64_t need = bin_width >= 1 ? zd_power_nbins(p.ppd, bin_width) : 0;
    if (need <= 0 || nbins < need) {
        snprintf(buf, cap, "the LPT band power at PPD = %lld needs bin_width >= 1 and room for zd_power_nbins = %lld bins (got width %d, %lld bins)",
                 (long long) p.ppd, (long long) need, (int) bin_width, (long long) nbins);
        return buf;
    }
    return nullptr;
}

// an LPT plan as zd_plan_create leaves it: the final pass's GenConst with the spectra resident (PhiK beside them only as the modes of a
// caller-supplied field, zd_plan_create_field_lpt: the sweeps then read D there instead of drawing it)
bool lpt_plan_ready(const zd_plan *pl) {
    const GenConst &g = pl->g;
    if (!g.lpt2_sk || (g.phik && !pl->field) || g.gen_phi || g.v1dev || g.qPLT || !pl->d_twN || pl->nranks != 1) return false;
    return !pl->p.q3LPT || (g.lpt3_p3 && g.lpt3_c[0] && g.lpt3_c[1] && g.lpt3_c[2]);
}

// the plan of a one-call form, rounds included (zd_direct_sum's way); NULL: refused, message printed
zd_plan *lpt_one_call_plan(const zd_params *p_in, const zd_pk *pk) {
    zd_params p = *p_in;
    p.ngpu = 0;
    if (p.stream_factor <= 0) {  // any factor whose plan the library accepts: the sums do not use the store
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
            fprintf(stderr, "zeldovich_hip: no GPU\n");
            return nullptr;
        }
        const int R = zd_choose_stream_factor(&p, 1, (int64_t) free_b - ((int64_t) 16 << 30));
        if (R > 0) p.stream_factor = R;
    }
    zd_plan *pl = nullptr;
    if (zd_plan_create(&p, pk, nullptr, 0, 0, 1, &pl)) return nullptr;
    return pl;
}

}  // namespace

extern "C" int zd_plan_lpt_direct_sum(zd_plan *pl, int64_t nsites, const int64_t *sites_zyx, double *out18, void *hip_stream) {
    if (!pl) {
        fprintf(stderr, "zeldovich_hip: zd_plan_lpt_direct_sum needs a plan\n");
        return 1;
    }
    const zd_params &p = pl->p;
    char buf[256];
    const char *why = lpt_params_refusal(p, "zd_plan_lpt_direct_sum", buf, sizeof(buf));
    if (!why) why = lpt_sites_refusal(p, nsites, sites_zyx, out18, buf, sizeof(buf));
    if (why) {
        fprintf(stderr, "zeldovich_hip: %s\n", why);
        return 1;
    }
    if (!lpt_plan_ready(pl)) {
        fprintf(stderr, "zeldovich_hip: this plan does not hold the spectra of an LPT run (no LPT direct summation)\n");
        return 1;
    }
    hipStream_t st = (hipStream_t) hip_stream;
    const GenConst &g = pl->g;
    const bool o3 = g.lpt3_p3 != nullptr;
    const int N = pl->N, nrows = pl->half, NV = DS_NS * (o3 ? 6 : 3);
    // order 1: k_ds_sweep on this plan's GenConst (the refusal of zd_plan_direct_sum concerns the higher orders, summed below)
    std::vector<double> first(7 * (size_t) nsites);
    if (zdsweep::ds_sweep_sites(pl, nsites, sites_zyx, g.lpt2_alpha, first.data(), st)) return 1;
    const int ngroups = (int) ((nsites + DS_NS - 1) / DS_NS);
    const long long nwg = (long long) ((N + DS_BX - 1) / DS_BX) * nrows;  // workgroups = partials of a launch group
    zdown::DevBuf<double> part, sums;
    if (part.alloc((size_t) NV * nwg) != hipSuccess || sums.alloc((size_t) NV * ngroups) != hipSuccess) {
        fprintf(stderr, "zeldovich_hip: LPT direct summation: no device memory for %lld partial sums\n", nwg * NV);
        return 1;
    }
    std::vector<double> h((size_t) NV * ngroups, 0.0);
    for (int grp = 0; grp < ngroups && !g.qonemode; grp++) {  // (one plane wave: no higher order, the sums stay zero)
        const DsSites<DS_NS> S = zdsweep::make_ds_sites(N, nsites, sites_zyx, grp);
        const int rc = o3 ? launch_ds_lpt_t<true>(g, S, nrows, pl->d_twN, part, st) : launch_ds_lpt_t<false>(g, S, nrows, pl->d_twN, part, st);
        if (rc || zdsweep::launch_ds_reduce(part, nwg, NV, sums + (size_t) grp * NV, st)) return 1;
    }
    if (!g.qonemode &&
        (hipMemcpyAsync(h.data(), sums, sizeof(double) * h.size(), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)) {
        fprintf(stderr, "zeldovich_hip: LPT direct summation failed: %s\n", hipGetErrorString(hipGetLastError()));
        return 1;
    }
    const double f2 = zd::lpt2_f2(&p), f3 = zd::lpt3_f3(&p);
    const int nq = o3 ? 6 : 3;
    for (int64_t i = 0; i < nsites; i++) {  // [group][site of the group][nq] = [site][nq]
        double *o = out18 + 18 * i;
        for (int j = 0; j < 6; j++) o[j] = first[7 * i + j];
        for (int j = 0; j < 3; j++) {
            const double q2 = h[(size_t) nq * i + j], q3 = o3 ? h[(size_t) nq * i + 3 + j] : 0.0;
            o[6 + j]  = q2;
            o[9 + j]  = f2 * q2;
            o[12 + j] = q3;
            o[15 + j] = f3 * q3;
        }
    }
    return 0;
}

extern "C" int zd_lpt_direct_sum(const zd_params *p_in, const zd_pk *pk, int64_t nsites, const int64_t *sites_zyx, double *out18) {
    if (!p_in || !pk) {
        fprintf(stderr, "zeldovich_hip: zd_lpt_direct_sum needs parameters and a power spectrum\n");
        return 1;
    }
    char buf[256];
    const char *why = lpt_params_refusal(*p_in, "zd_lpt_direct_sum", buf, sizeof(buf));  // (before a plan — the rounds — is made)
    if (!why) why = lpt_sites_refusal(*p_in, nsites, sites_zyx, out18, buf, sizeof(buf));
    if (why) {
        fprintf(stderr, "zeldovich_hip: %s\n", why);
        return 1;
    }
    zd_plan *pl = lpt_one_call_plan(p_in, pk);
    if (!pl) return 1;
    const zdown::PlanPtr plan(pl);
    return zd_plan_lpt_direct_sum(pl, nsites, sites_zyx, out18, nullptr);
}

extern "C" int zd_plan_lpt_power(zd_plan *pl, int32_t bin_width, int64_t nbins, int64_t *count, double *sums8, void *hip_stream) {
    if (!pl) {
        fprintf(stderr, "zeldovich_hip: zd_plan_lpt_power needs a plan\n");
        return 1;
    }
    const zd_params &p = pl->p;
    char buf[256];
    const char *why = lpt_params_refusal(p, "zd_plan_lpt_power", buf, sizeof(buf));
    if (!why) why = lpt_bins_refusal(p, bin_width, nbins, count, sums8, buf, sizeof(buf));
    if (why) {
        fprintf(stderr, "zeldovich_hip: %s\n", why);
        return 1;
    }
    if (!lpt_plan_ready(pl)) {
        fprintf(stderr, "zeldovich_hip: this plan does not hold the spectra of an LPT run (no LPT band power)\n");
        return 1;
    }
    hipStream_t st = (hipStream_t) hip_stream;
    const GenConst &g = pl->g;
    const size_t nb = (size_t) nbins;
    zdown::DevBuf<double> dbuf;  // counts (as uint64), then the PL_NV sums
    if (dbuf.alloc(nb * (1 + PL_NV)) != hipSuccess || hipMemsetAsync(dbuf, 0, nb * 8 * (1 + PL_NV), st) != hipSuccess) {
        fprintf(stderr, "zeldovich_hip: LPT band power: no device memory for %lld bins\n", (long long) nbins);
        return 1;
    }
    unsigned long long *gcount = (unsigned long long *) dbuf.get();
    double *gsum = dbuf + nb;
    const SweepJumps J = zdsweep::make_sweep_jumps(pl->N);
    const double f2 = zd::lpt2_f2(&p), f3 = zd::lpt3_f3(&p);
    const int nrows = pl->half;
    const bool fast = g.genf_tab && !g.qonemode && !g.phik;  // (the table arithmetic draws; a field's modes are read by the general form)
    int rc;
    if (fast) {  // the plane ky = 0 through the general form, every other row through the table arithmetic
        rc = launch_pk_lpt<false>(g, J, 0, 1, pl->S.lG, bin_width, (int) nbins, f2, f3, gcount, gsum, st);
        if (!rc) rc = launch_pk_lpt<true>(g, J, 1, nrows - 1, pl->S.lG, bin_width, (int) nbins, f2, f3, gcount, gsum, st);
    } else {
        rc = launch_pk_lpt<false>(g, J, 0, nrows, pl->S.lG, bin_width, (int) nbins, f2, f3, gcount, gsum, st);
    }
    if (rc) return 1;
    std::vector<double> h(nb * (1 + PL_NV));
    if (hipMemcpyAsync(h.data(), dbuf, nb * 8 * (1 + PL_NV), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        fprintf(stderr, "zeldovich_hip: LPT band power sweep failed: %s\n", hipGetErrorString(hipGetLastError()));
        return 1;
    }
    const unsigned long long *hc = (const unsigned long long *) h.data();
    for (size_t b = 0; b < nb; b++) {
        count[b] = (int64_t) hc[b];
        for (int j = 0; j < PL_NV; j++) sums8[PL_NV * b + j] = h[nb * (1 + j) + b];
    }
    return 0;
}

extern "C" int zd_lpt_power(const zd_params *p_in, const zd_pk *pk, int32_t bin_width, int64_t nbins, int64_t *count, double *sums8) {
    if (!p_in || !pk) {
        fprintf(stderr, "zeldovich_hip: zd_lpt_power needs parameters and a power spectrum\n");
        return 1;
    }
    char buf[256];
    const char *why = lpt_params_refusal(*p_in, "zd_lpt_power", buf, sizeof(buf));  // (before a plan — the rounds — is made)
    if (!why) why = lpt_bins_refusal(*p_in, bin_width, nbins, count, sums8, buf, sizeof(buf));
    if (why) {
        fprintf(stderr, "zeldovich_hip: %s\n", why);
        return 1;
    }
    zd_plan *pl = lpt_one_call_plan(p_in, pk);
    if (!pl) return 1;
    const zdown::PlanPtr plan(pl);
    return zd_plan_lpt_power(pl, bin_width, nbins, count, sums8, nullptr);
}
