// zd_kernels_pk.hip — band power of the realised modes: one sweep over the modes a plan generates that bins |D(k)|^2, the input
// P(k) and the displacement / velocity power per |k| shell instead of storing anything (zd_plan_measure_power / zd_measure_power,
// include/zeldovich_hip.h).  No FFT, no block store, no y / x stage: the sweep does not depend on the transform family and takes
// every even PPD the library accepts.
//
// DEFINITION OF THE MEASUREMENT
//   Bins.  kx, ky, kz are the signed integer wavenumbers (-N/2 < k_i <= N/2), w = bin_width (an integer >= 1, in fundamentals).
//          Mode k lies in bin b iff (b w)^2 <= kx^2 + ky^2 + kz^2 < ((b + 1) w)^2: an exact integer shell, decided in integer
//          arithmetic.  zd_power_nbins(ppd, w) = isqrt(3 (N/2)^2) / w + 1 bins hold every mode of the cube.
//   Sums.  Over all N^3 wavevectors of the cube — each Hermitian pair counted twice — restricted to the modes the zero rule of
//          src/zeldovich.cpp:350-356 leaves alive (|k_i| == kmax, the spherical ZD_k_cutoff unless ZD_CornerModes, the one-mode
//          filter); k = 0 is excluded.  Per bin:
//              count      modes                                                       (int64, exact)
//              sum_k      sum |k| fundamental
//              sum_dens   sum |D(k)|^2          D as the generators form it: cgauss<2> of the pcg64 draws at the mode's counter
//                                               (ZD_qPk_fix_to_mean: fixed amplitude); ZD_f_NL != 0: D = PhiK(k) M(k) of the plan's PhiK
//              sum_input  sum P(|k|)            PowerSpectrum::power (zd_pk_power): <|D|^2>, and |D|^2 itself with fixed amplitudes
//              sum_disp   sum_j |q_j(k)|^2      q_j = i s_j D; ZA: s_j = k_j fundamental / k^2; PLT: s_j = rescale e_j fundamental / (k.e)
//              sum_vel    sum_j |v_j(k)|^2      ZA: v = vnorm q (src/output.cpp:78-82); PLT: v_j = f q_j, its own field
//   Refusals.  Configurations whose Nyquist-plane modes stay alive (the nyquist_dead condition of pack_mode, zd_route.h: there the
//          delivered fields are not transforms of real fields and "power per wavevector" has no single meaning), and
//          ZD_Version = 1, whose draws are sequential; ZD_q2LPT jobs, whose delivered fields hold a second-order part the sweep
//          does not regenerate (their band power, order by order: zd_plan_lpt_power, zd_kernels_lpt_ds.hip).
//
// A rank sweeps the half-space rows it owns, ky = rank (mod nranks), ky < N/2, every (kx, kz); a row ky >= 1 stands for itself and
// its Hermitian twin (weight 2), the plane ky = 0 is visited position by position with the conjugate "loser" rule of k_gen.  The
// sums of the ranks add up to the whole.
//
// k_pk_sweep<PLT, PLAW, FAST>: one thread owns one x and walks PK_ZC consecutive z with ONE RNG state (the z-major walk of k_gen at
// stream factor 1).  FAST = the table arithmetic of k_genf (zd_genmath.h: ln / exp / sincos / sqrt and P(k) from the LDS image, the
// eigenmode lookup of eigenmode_fast, waves of zeroed modes only move the RNG) for the rows ky >= 1; the general form = the per-mode
// arithmetic of k_gen (ky = 0, ZD_f_NL, the one-mode filter, splines too large for the LDS image).
// A wave's 64 modes fall into unrelated bins, so nothing is reduced across lanes: a thread sums the run of modes that stay in one
// bin in registers, adds the run into an LDS window of PK_WIN bins that starts at the workgroup's smallest |k| (a tile of 256 x 256
// modes spans < 362 fundamentals; a mode outside the window — wide tiles cannot happen, this is a guard — goes to global memory
// directly), and the workgroup flushes its window once with global double atomics.  Counts are integer atomics: exact.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "zd_plan.h"
#include "zd_launch.h"
#include "zd_genmath.h"
#include "zd_sweep.h"

using namespace zd;
using zdfft::cplx;
using zdpcg::u128;
using namespace zdgen;
using zdsweep::SweepJumps;
using zdsweep::SweepMode;

namespace {

constexpr int PK_BX  = 256;  // threads (consecutive x) per workgroup
constexpr int PK_ZC  = 256;  // z indices one thread walks
constexpr int PK_WIN = 384;  // bins of the LDS window: sqrt(255^2 + 255^2) + 2 = 363 at w = 1
constexpr int PK_NV  = 5;    // sum_k, sum_dens, sum_input, sum_disp, sum_vel

// floor(sqrt(k2i)) from an approximate root
__device__ __forceinline__ int pk_isqrt_fix(int k2i, double root) {
    int s = (int) root;
    if (s * s > k2i) s--;
    else if ((s + 1) * (s + 1) <= k2i) s++;
    return s;
}

// the run of consecutive modes of one thread that share a bin
struct PkRun {
    int b;
    unsigned n;
    double v[PK_NV];
};

template <bool PLT, bool PLAW, bool FAST>
__global__ __launch_bounds__(PK_BX) void k_pk_sweep(GenConst g, SweepJumps J, int ky_first, int ky_stride, int lG, int zc, int w, int nbins,
                                                     double vnorm2, unsigned long long *__restrict__ gcount, double *__restrict__ gsum) {
    extern __shared__ double pk_lds[];
    const int ntab = FAST ? g.genf_n : 0;
    double *T      = pk_lds;                      // LDS image of k_genf (FAST)
    double *wsum   = pk_lds + ntab;               // [PK_NV][PK_WIN]
    unsigned *wcnt = reinterpret_cast<unsigned *>(wsum + PK_NV * PK_WIN);
    const int N = g.N, half = g.half;
    for (int i = threadIdx.x; i < ntab; i += PK_BX) T[i] = g.genf_tab[i];
    for (int i = threadIdx.x; i < PK_NV * PK_WIN; i += PK_BX) wsum[i] = 0.0;
    for (int i = threadIdx.x; i < PK_WIN; i += PK_BX) wcnt[i] = 0u;
    const int ky  = ky_first + (int) blockIdx.z * ky_stride;
    const int x0  = (int) blockIdx.x * PK_BX, xl = min(N - 1, x0 + PK_BX - 1);
    const int z0  = (int) blockIdx.y * zc, z1 = min(N, z0 + zc);
    const bool act = x0 + (int) threadIdx.x < N;
    const int x   = act ? x0 + (int) threadIdx.x : 0;
    const int kx  = x > half ? x - N : x;
    // first bin of the window: |k_i| of an index is a tent, so its minimum over a range sits at an end
    int bmin;
    {
        auto tent = [&](int i) { return i > half ? N - i : i; };
        const int ax = min(tent(x0), tent(xl)), az = min(tent(z0), tent(z1 - 1));
        const int k2 = ax * ax + ky * ky + az * az;
        const int s  = pk_isqrt_fix(k2, sqrt((double) k2));
        bmin = w == 1 ? s : s / w;
    }
    __syncthreads();
    const unsigned weight = ky != 0 ? 2u : 1u;  // a half-space row ky >= 1 stands for itself and its Hermitian twin
    PkRun run;
    run.b = -1;
    run.n = 0;
#pragma unroll
    for (int j = 0; j < PK_NV; j++) run.v[j] = 0.0;
    auto flush = [&]() {
        if (run.n == 0) return;
        const int i = run.b - bmin;
        if (i >= 0 && i < PK_WIN) {
            atomicAdd(&wcnt[i], run.n);
#pragma unroll
            for (int j = 0; j < PK_NV; j++) unsafeAtomicAdd(&wsum[j * PK_WIN + i], run.v[j]);
        } else if (run.b < nbins) {
            atomicAdd(&gcount[run.b], (unsigned long long) run.n * weight);
#pragma unroll
            for (int j = 0; j < PK_NV; j++) unsafeAtomicAdd(&gsum[(size_t) j * nbins + run.b], run.v[j] * (double) weight);
        }
        run.n = 0;
#pragma unroll
        for (int j = 0; j < PK_NV; j++) run.v[j] = 0.0;
    };
    auto add = [&](int k2i, double root, double d2, double P, double disp, double vel) {
        const int s = pk_isqrt_fix(k2i, root);
        const int b = w == 1 ? s : s / w;
        if (b != run.b) {
            flush();
            run.b = b;
        }
        run.n++;
        run.v[0] += root * g.fundamental;
        run.v[1] += d2;
        run.v[2] += P;
        run.v[3] += disp;
        run.v[4] += vel;
    };

    // what the sweep takes from a visited mode (the walk: zd_sweep.h)
    EigXY exy = {};
    EigAxis eax = {0, 0, 0.0}, eay = {0, 0, 0.0};
    if constexpr (PLT) {
        eax = eig_axis(g, eig_index_x(g, kx));
        eay = eig_axis(g, ky);
        if constexpr (FAST) exy = eig_xy(g, eax, eay);
    }
    zdsweep::sweep_modes<PLAW, FAST>(g, J, T, ky, lG, x, act, z0, z1, false, [&](const SweepMode &m) {
        const double d2 = FAST ? fma(m.dr, m.dr, m.di * m.di) : m.dr * m.dr + m.di * m.di;
        double disp, vel;
        if constexpr (PLT) {
            double e[4];
            double f, rescale = 1.0, sx, sy, sz;
            if constexpr (FAST) {
                eigenmode_fast(g, m.kx, ky, m.kz, exy, eig_axis(g, eig_index_z(g, m.kz)), e);
                f = (sqrt_pos(1. + 24 * e[3] * g.f_cluster) - 1) * .25;
                if (g.qPLTrescale) rescale = fexp(g.ln_growth_ratio * (g.target_f - f), T);
                sx = rescale * e[0], sy = rescale * e[1], sz = rescale * e[2];
            } else {
                const EigAxis eaz = eig_axis(g, eig_index_z(g, m.kz));
                if (m.cj)  // mirrored source mode (ky = 0 plane only): its own x axis
                    get_eigenmode_dev(g, m.kx, ky, m.kz, eig_axis(g, eig_index_x(g, m.kx)), eay, eaz, e);
                else
                    get_eigenmode_dev(g, m.kx, ky, m.kz, eax, eay, eaz, e);
                f = (sqrt(1. + 24 * e[3] * g.f_cluster) - 1) * .25;
                if (g.qPLTrescale) rescale = exp(g.ln_growth_ratio * (g.target_f - f));
                sx = rescale * e[0] * g.fundamental * m.ik2, sy = rescale * e[1] * g.fundamental * m.ik2, sz = rescale * e[2] * g.fundamental * m.ik2;
            }
            disp = (sx * sx + sy * sy + sz * sz) * d2;
            vel  = f * f * disp;
        } else {
            const double q = g.fundamental * m.ik2;
            disp = (double) m.k2i * (q * q) * d2;
            vel  = vnorm2 * disp;
        }
        if (m.live) add(m.k2i, FAST ? sqrt_pos((double) m.k2i) : sqrt((double) m.k2i), d2, m.P, disp, vel);
    });
    flush();
    __syncthreads();
    for (int i = threadIdx.x; i < PK_WIN; i += PK_BX) {
        const unsigned n = wcnt[i];
        const int b = bmin + i;
        if (n == 0 || b >= nbins) continue;
        atomicAdd(&gcount[b], (unsigned long long) n * weight);
#pragma unroll
        for (int j = 0; j < PK_NV; j++) unsafeAtomicAdd(&gsum[(size_t) j * nbins + b], wsum[j * PK_WIN + i] * (double) weight);
    }
}

template <bool PLT, bool PLAW, bool FAST>
int launch_pk_t(const GenConst &g, const SweepJumps &J, int ky_first, int ky_stride, int nrows, int lG, int w, int nbins, double vnorm2,
                unsigned long long *gcount, double *gsum, hipStream_t st) {
    if (nrows <= 0) return 0;
    const int zc = std::min(g.N, PK_ZC);
    const size_t lds = sizeof(double) * ((FAST ? g.genf_n : 0) + PK_NV * PK_WIN) + sizeof(unsigned) * PK_WIN;
    set_dyn_lds<k_pk_sweep<PLT, PLAW, FAST>>(lds > 65536 ? lds : 0);
    hipLaunchKernelGGL((k_pk_sweep<PLT, PLAW, FAST>), dim3((g.N + PK_BX - 1) / PK_BX, (g.N + zc - 1) / zc, nrows), dim3(PK_BX), lds, st, g, J,
                       ky_first, ky_stride, lG, zc, w, nbins, vnorm2, gcount, gsum);
    ZD_LAUNCH_CHECK();
    return 0;
}

template <bool FAST>
int launch_pk(const GenConst &g, const SweepJumps &J, int ky_first, int ky_stride, int nrows, int lG, int w, int nbins, double vnorm2,
              unsigned long long *gcount, double *gsum, hipStream_t st) {
    const bool plt = g.qPLT != 0, plaw = g.is_powerlaw != 0;
#define PCASE(a, b) \
    if (plt == a && plaw == b) return launch_pk_t<a, b, FAST>(g, J, ky_first, ky_stride, nrows, lG, w, nbins, vnorm2, gcount, gsum, st)
    PCASE(false, false);
    PCASE(false, true);
    PCASE(true, false);
    PCASE(true, true);
#undef PCASE
    return 1;
}

}  // namespace

extern "C" int zd_plan_measure_power(zd_plan *pl, int32_t bin_width, int64_t nbins, int64_t *count, double *sum_k, double *sum_dens,
                                     double *sum_input, double *sum_disp, double *sum_vel, void *hip_stream) {
    if (!pl || !count || !sum_k || !sum_dens || !sum_input || !sum_disp || !sum_vel) {
        fprintf(stderr, "zeldovich_hip: zd_plan_measure_power needs a plan and six output arrays\n");
        return 1;
    }
    const zd_params &p = pl->p;
    const int64_t need = zd_power_nbins(p.ppd, bin_width);
    if (need <= 0 || nbins < need) {
        fprintf(stderr, "zeldovich_hip: band power at PPD = %lld needs bin_width >= 1 and room for zd_power_nbins = %lld bins (got width %d, %lld bins)\n",
                (long long) p.ppd, (long long) need, (int) bin_width, (long long) nbins);
        return 1;
    }
    if (p.version == 1) {
        fprintf(stderr, "zeldovich_hip: band power is not measured with ZD_Version = 1: its mt19937 draws are sequential, no mode can be "
                        "regenerated from a counter\n");
        return 1;
    }
    if (p.q2LPT) {
        fprintf(stderr, "zeldovich_hip: band power is not measured on a ZD_q2LPT plan: the sweep regenerates the first-order modes only\n");
        return 1;
    }
    const GenConst &g = pl->g;
    if (!(g.kmax == pl->half || (!p.corner_modes && p.k_cutoff >= 1.0))) {
        fprintf(stderr, "zeldovich_hip: band power is not measured while modes on the Nyquist planes stay alive (ZD_CornerModes with "
                        "ZD_k_cutoff = %g): the fields are then not transforms of real fields\n", p.k_cutoff);
        return 1;
    }
    if (g.gen_phi || g.v1dev || (g.qPLT && !g.eig) || (p.f_NL != 0. && !g.phik)) {
        fprintf(stderr, "zeldovich_hip: this plan does not generate the modes of a run (no band power)\n");
        return 1;
    }
    hipStream_t st = (hipStream_t) hip_stream;
    const size_t nb = (size_t) nbins;
    zdown::DevBuf<double> buf;  // counts (as uint64), then the PK_NV sums
    if (buf.alloc(nb * (1 + PK_NV)) != hipSuccess || hipMemsetAsync(buf, 0, nb * 8 * (1 + PK_NV), st) != hipSuccess) {
        fprintf(stderr, "zeldovich_hip: band power: no device memory for %lld bins\n", (long long) nbins);
        return 1;
    }
    unsigned long long *gcount = (unsigned long long *) buf.get();
    double *gsum = buf + nb;
    const SweepJumps J = zdsweep::make_sweep_jumps(pl->N);
    const int G = pl->nranks, rank = pl->rank, Hq = pl->Hq;  // rows ky = rank + G i, i < Hq
    const double vnorm2 = pl->ec.vnorm * pl->ec.vnorm;
    const bool fast = g.genf_tab && !g.phik && !g.qonemode;
    int rc = 0;
    if (fast) {  // the plane ky = 0 (rank 0) through the general form, every other row through the table arithmetic
        const int skip = rank == 0 ? 1 : 0;
        if (skip) rc = launch_pk<false>(g, J, 0, G, 1, pl->S.lG, bin_width, (int) nbins, vnorm2, gcount, gsum, st);
        if (!rc) rc = launch_pk<true>(g, J, rank + skip * G, G, Hq - skip, pl->S.lG, bin_width, (int) nbins, vnorm2, gcount, gsum, st);
    } else {
        rc = launch_pk<false>(g, J, rank, G, Hq, pl->S.lG, bin_width, (int) nbins, vnorm2, gcount, gsum, st);
    }
    if (rc) return 1;
    std::vector<double> h(nb * (1 + PK_NV));
    if (hipMemcpyAsync(h.data(), buf, nb * 8 * (1 + PK_NV), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        fprintf(stderr, "zeldovich_hip: band power sweep failed: %s\n", hipGetErrorString(hipGetLastError()));
        return 1;
    }
    const unsigned long long *hc = (const unsigned long long *) h.data();
    double *outs[PK_NV] = {sum_k, sum_dens, sum_input, sum_disp, sum_vel};
    for (size_t b = 0; b < nb; b++) {
        count[b] = (int64_t) hc[b];
        for (int j = 0; j < PK_NV; j++) outs[j][b] = h[nb * (1 + j) + b];
    }
    return 0;
}

extern "C" int zd_measure_power(const zd_params *p_in, const zd_pk *pk, const double *eig, int64_t eig_ppd, int32_t bin_width, int64_t nbins,
                                int64_t *count, double *sum_k, double *sum_dens, double *sum_input, double *sum_disp, double *sum_vel) {
    zd_params p = *p_in;
    p.ngpu = 0;
    if (p.q2LPT) {  // (before a plan — and with it the second-order round — is made)
        fprintf(stderr, "zeldovich_hip: band power is not measured on a ZD_q2LPT job: the sweep regenerates the first-order modes only\n");
        return 1;
    }
    if (p.stream_factor <= 0) {  // any factor whose plan the library accepts: the sweep does not use the store
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
            fprintf(stderr, "zeldovich_hip: no GPU\n");
            return 1;
        }
        const int R = zd_choose_stream_factor(&p, 1, (int64_t) free_b - ((int64_t) 16 << 30));
        if (R > 0) p.stream_factor = R;
    }
    zd_plan *pl = nullptr;
    if (zd_plan_create(&p, pk, eig, eig_ppd, 0, 1, &pl)) return 1;
    const zdown::PlanPtr plan(pl);
    return zd_plan_measure_power(pl, bin_width, nbins, count, sum_k, sum_dens, sum_input, sum_disp, sum_vel, nullptr);
}
