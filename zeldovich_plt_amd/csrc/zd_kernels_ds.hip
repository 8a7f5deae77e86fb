// zd_kernels_ds.hip — direct summation at sample sites: one sweep over the modes a plan generates that accumulates
// F(k) e^{2 pi i k.x / N} at a handful of lattice sites instead of storing anything (zd_plan_direct_sum / zd_direct_sum,
// include/zeldovich_hip.h).  No FFT, no block store, no fold, no packing, no epilogue: the sums are independent of everything
// between the generator and the delivered records, do not depend on the transform family and take every even PPD the library
// accepts.
//
// DEFINITION OF THE SUMS
//   Sites.  A lattice site s = (z, y, x), 0 <= z, y, x < N, in the (z, y, x) order of the records.  out[s][0..6] = qx, qy, qz, vx, vy,
//          vz, density: the fields an RVdoubleZel run with ZD_qdensity = 1 delivers at that site ([nsites][7] doubles).
//   Sums.  field(s) = sum_k F(k) e^{+2 pi i (kx x + ky y + kz z) / N} over all N^3 signed wavevectors (-N/2 < k_i <= N/2), the
//          unnormalised inverse transform, with the amplitudes the generators form:
//              density   F = D(k)          cgauss<2> of the pcg64 draws at the mode's counter (ZD_qPk_fix_to_mean: fixed amplitude);
//                                          ZD_f_NL != 0: D = PhiK(k) M(k) of the plan's PhiK
//              q_j       F = i s_j D       ZA: s_j = k_j fundamental / k^2; PLT: s_j = rescale e_j fundamental / (k.e)
//              v_j       F = i f s_j D     ZA: f = vnorm (src/output.cpp:78-82); PLT: f of the mode's eigenvalue, its own field
//          restricted to the modes the zero rule of src/zeldovich.cpp:350-356 leaves alive (|k_i| == kmax, the spherical
//          ZD_k_cutoff unless ZD_CornerModes, the one-mode filter); k = 0 is excluded.  This is oracle/zdo.py: direct_sum.
//   Refusals.  Configurations whose Nyquist-plane modes stay alive (the nyquist_dead condition of pack_mode, zd_route.h: the
//          delivered fields are then not transforms of Hermitian fields), ZD_Version = 1, whose draws are sequential, and ZD_q2LPT
//          plans, whose delivered fields hold a second-order part the sweep does not regenerate; a site outside [0, N)^3, fewer
//          than 1 or more than 64 sites, NULL arrays.
//          (A ZD_q2LPT / ZD_q3LPT plan has entry points of its own, zd_plan_lpt_direct_sum / zd_lpt_direct_sum in zd_kernels_lpt_ds.hip: its
//          first order is this sweep, run through ds_sweep_sites with the velocity factor lpt2_alpha, its higher orders are summed from
//          the spectra the plan keeps.)
//
//   ZD_f_NL plans.  The second pass of the reference forms D = PhiK M for every mode but k = 0 (src/zeldovich.cpp:393-400: no zero
//          rule), and so do k_gen and this sweep; the row ky = N/2 stays unread, as in the y stage.  Modes on the planes |kx| = N/2,
//          |kz| = N/2 are then alive, with the signed wavenumber +N/2 in s_j.
//
// A rank sweeps the half-space rows it owns, ky = rank (mod nranks), ky < N/2, every (kx, kz); a row ky >= 1 contributes
// 2 Re(F e^{i theta}), itself and its Hermitian twin (the twin rows of the stores are written as conjugates).  The plane ky = 0 is
// visited position by position with the conjugate "loser" rule of k_gen, and every position adds what the reference's arrays
// density + i qx = (1 - s_x) D, qy + i qz = (-s_z + i s_y) D, i vx = -f s_x D, vy + i vz = f (-s_z + i s_y) D hold of it: real and
// imaginary part of the position's term, each into its field.  For a position and its mirror image together that is Re(F e^{i theta})
// twice; the Nyquist positions of an f_NL plan, which are their own mirror images in one coordinate, land where the records have them.
// The sums of the ranks add up to the whole.
//
// k_ds_sweep<PLT, PLAW, FAST, NS>: the walk of k_pk_sweep (zd_sweep.h), one thread per x over all z of a row, NS = 8 sites per
// launch (more sites: more sweeps), 7 NS sums per thread in registers.
//   Phase.  m = (kx x + ky y + kz z) mod N in integers (position indices stand for the wavenumbers: they agree mod N) and
//          e^{2 pi i m / N} from the plan's length-N table (make_twiddles: rounded from long double).  The general form looks every
//          phase up; the FAST rows re-seed from the table every DS_RESEED steps of the z run and rotate by the site's
//          e^{2 pi i z_s / N} in between (a wave's 64 lanes would otherwise gather 8 unrelated table lines per mode): at most 31
//          rotations, 7e-15 relative whatever N is.  No sincos of an unreduced argument anywhere.
//   Sums.  thread -> wave (shuffles, fixed order) -> workgroup (LDS, wave 0..3 in order) -> one partial per workgroup in a
//          buffer; k_ds_reduce adds the partials of a launch group in a fixed order.  No floating-point atomics: two calls on one
//          plan return the same bits.
// Shared with zd_kernels_lpt_ds.hip through zd_sweep.h: the sites of a launch group (DsSites, make_ds_sites), k_ds_reduce's launcher
// (any number of sums per site) and ds_sweep_sites, the launches of zd_plan_direct_sum behind its refusals.
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

using namespace zd;
using zdfft::cplx;
using namespace zdgen;
using zdsweep::SweepJumps;
using zdsweep::SweepMode;
using zdsweep::DsSites;
using zdsweep::DS_BX;
using zdsweep::DS_NS;
using zdsweep::DS_RESEED;
using zdsweep::DS_MAX_SITES;

namespace {

constexpr int DS_NQ = 7;          // qx, qy, qz, vx, vy, vz, density
constexpr int DS_RB = 256;        // threads of k_ds_reduce

template <bool PLT, bool PLAW, bool FAST, int NS>
__global__ __launch_bounds__(DS_BX) void k_ds_sweep(GenConst g, SweepJumps J, DsSites<NS> S, int ky_first, int ky_stride, int lG, double vnorm,
                                                     const cplx *__restrict__ twN, double *__restrict__ partial) {
    extern __shared__ double ds_lds[];
    constexpr int NV = NS * DS_NQ;
    const int ntab = FAST ? g.genf_n : 0;
    double *T     = ds_lds;         // LDS image of k_genf (FAST)
    double *stage = ds_lds + ntab;  // [waves][NV]
    const int N = g.N, half = g.half;
    for (int i = threadIdx.x; i < ntab; i += DS_BX) T[i] = g.genf_tab[i];
    const int ky = ky_first + (int) blockIdx.y * ky_stride;
    const int x0 = (int) blockIdx.x * DS_BX;
    const bool act = x0 + (int) threadIdx.x < N;
    const int x  = act ? x0 + (int) threadIdx.x : 0;
    const int kx = x > half ? x - N : x;
    __syncthreads();
    const double weight = ky != 0 ? 2.0 : 1.0;  // a half-space row ky >= 1 stands for itself and its Hermitian twin
    double acc[NS][DS_NQ];
#pragma unroll
    for (int s = 0; s < NS; s++)
#pragma unroll
        for (int q = 0; q < DS_NQ; q++) acc[s][q] = 0.0;
    // Re(D e^{i t}) into the density, Re(i s_j D e^{i t}) into q_j, f times it into v_j, for the phase (c, sn) of site s
    auto add = [&](int s, double c, double sn, double Dr, double Di, const double (&sj)[3], const double (&fsj)[3]) {
        const double dre = Dr * c - Di * sn;
        const double fim = -(Dr * sn + Di * c);
#pragma unroll
        for (int j = 0; j < 3; j++) {
            acc[s][j]     = fma(sj[j], fim, acc[s][j]);
            acc[s][3 + j] = fma(fsj[j], fim, acc[s][3 + j]);
        }
        acc[s][6] += dre;
    };
    EigXY exy = {};
    EigAxis eax = {0, 0, 0.0}, eay = {0, 0, 0.0};
    if constexpr (PLT) {
        eax = eig_axis(g, eig_index_x(g, kx));
        eay = eig_axis(g, ky);
        if constexpr (FAST) exy = eig_xy(g, eax, eay);
    }
    cplx ph[NS];  // FAST: the sites' phases at position (x, zlast)
    int zlast = -2, zseed = 0;
    zdsweep::sweep_modes<PLAW, FAST>(g, J, T, ky, lG, x, act, 0, N, g.phik != nullptr, [&](const SweepMode &m) {
        double sj[3], fsj[3];
        if constexpr (PLT) {
            double e[4], f, rescale = 1.0;
            if constexpr (FAST) {
                eigenmode_fast(g, m.kx, ky, m.kz, exy, eig_axis(g, eig_index_z(g, m.kz)), e);
                f = (sqrt_pos(1. + 24 * e[3] * g.f_cluster) - 1) * .25;
                if (g.qPLTrescale) rescale = fexp(g.ln_growth_ratio * (g.target_f - f), T);
            } else {
                const EigAxis eaz = eig_axis(g, eig_index_z(g, m.kz));
                if (m.cj)  // mirrored source mode (ky = 0 plane only): its own x axis
                    get_eigenmode_dev(g, m.kx, ky, m.kz, eig_axis(g, eig_index_x(g, m.kx)), eay, eaz, e);
                else
                    get_eigenmode_dev(g, m.kx, ky, m.kz, eax, eay, eaz, e);
                f = (sqrt(1. + 24 * e[3] * g.f_cluster) - 1) * .25;
                if (g.qPLTrescale) rescale = exp(g.ln_growth_ratio * (g.target_f - f));
                rescale *= g.fundamental * m.ik2;
            }
#pragma unroll
            for (int j = 0; j < 3; j++) {
                sj[j]  = rescale * e[j];
                fsj[j] = f * sj[j];
            }
        } else {
            const double q = g.fundamental * m.ik2;
            sj[0] = (double) m.kx * q, sj[1] = (double) ky * q, sj[2] = (double) m.kz * q;
#pragma unroll
            for (int j = 0; j < 3; j++) fsj[j] = vnorm * sj[j];
        }
        const double Dr = weight * m.dr, Di = weight * m.di;  // zeroed positions of a FAST wave carry D = 0
        if constexpr (FAST) {
            if (m.z != zlast + 1 || m.z - zseed >= DS_RESEED) {  // (wave-uniform: whole waves skip, never single lanes)
#pragma unroll
                for (int s = 0; s < NS; s++) ph[s] = twN[modn(N, x * S.x[s] + ky * S.y[s] + m.z * S.z[s])];
                zseed = m.z;
            } else {
#pragma unroll
                for (int s = 0; s < NS; s++) {
                    const double c = ph[s].x, sn = ph[s].y;
                    ph[s].x = fma(c, S.wr[s], -sn * S.wi[s]);
                    ph[s].y = fma(c, S.wi[s], sn * S.wr[s]);
                }
            }
            zlast = m.z;
#pragma unroll
            for (int s = 0; s < NS; s++) add(s, ph[s].x, ph[s].y, Dr, Di, sj, fsj);
        } else {  // the generated mode's own indices
            const int xs = m.kx < 0 ? m.kx + N : m.kx, zs = m.kz < 0 ? m.kz + N : m.kz;
#pragma unroll
            for (int s = 0; s < NS; s++) {
                const cplx p = twN[modn(N, xs * S.x[s] + ky * S.y[s] + zs * S.z[s])];
                if (ky != 0) {
                    add(s, p.x, p.y, Dr, Di, sj, fsj);
                } else {  // the plane ky = 0, position by position: what the reference's packed arrays deliver (see the definition)
                    const double sg = m.cj ? -1.0 : 1.0;  // the conjugated copy of the mode at -k: D -> conj D, s -> -s
                    const double er = Dr * p.x - Di * p.y, ei = sg * (Dr * p.y + Di * p.x);  // D e^{i t} at the position
                    const double tx = sg * sj[0], ty = sg * sj[1], tz = sg * sj[2];
                    acc[s][6] += (1.0 - tx) * er;
                    acc[s][0] += (1.0 - tx) * ei;
                    acc[s][1] += -tz * er - ty * ei;
                    acc[s][2] += -tz * ei + ty * er;
                    const double ux = sg * fsj[0], uy = sg * fsj[1], uz = sg * fsj[2];
                    acc[s][3] += -ux * ei;
                    acc[s][4] += -uz * er - uy * ei;
                    acc[s][5] += -uz * ei + uy * er;
                }
            }
        }
    });
    // thread -> wave -> workgroup, every step in a fixed order
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int s = 0; s < NS; s++)
#pragma unroll
        for (int q = 0; q < DS_NQ; q++) {
            double v = acc[s][q];
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
            if (lane == 0) stage[wave * NV + s * DS_NQ + q] = v;
        }
    __syncthreads();
    if (threadIdx.x < NV) {
        double v = stage[threadIdx.x];
        for (int w = 1; w < DS_BX / 64; w++) v += stage[w * NV + threadIdx.x];
        partial[((size_t) blockIdx.y * gridDim.x + blockIdx.x) * NV + threadIdx.x] = v;
    }
}

// out[o] = sum of partial[i * nv + o] over the nwg partials of a launch group, in an order that depends on nothing but nwg
__global__ __launch_bounds__(DS_RB) void k_ds_reduce(const double *__restrict__ partial, long long nwg, int nv, double *__restrict__ out) {
    __shared__ double sh[DS_RB];
    const int o = blockIdx.x;
    double v = 0.0;
    for (long long i = threadIdx.x; i < nwg; i += DS_RB) v += partial[i * nv + o];
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int h = DS_RB / 2; h >= 1; h >>= 1) {
        if ((int) threadIdx.x < h) sh[threadIdx.x] += sh[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[o] = sh[0];
}

template <bool PLT, bool PLAW, bool FAST>
int launch_ds_t(const GenConst &g, const SweepJumps &J, const DsSites<DS_NS> &S, int ky_first, int ky_stride, int nrows, int lG, double vnorm,
                const cplx *twN, double *partial, hipStream_t st) {
    if (nrows <= 0) return 0;
    const size_t lds = sizeof(double) * ((FAST ? g.genf_n : 0) + (DS_BX / 64) * DS_NS * DS_NQ);
    set_dyn_lds<k_ds_sweep<PLT, PLAW, FAST, DS_NS>>(lds > 65536 ? lds : 0);
    hipLaunchKernelGGL((k_ds_sweep<PLT, PLAW, FAST, DS_NS>), dim3((g.N + DS_BX - 1) / DS_BX, nrows), dim3(DS_BX), lds, st, g, J, S, ky_first,
                       ky_stride, lG, vnorm, twN, partial);
    ZD_LAUNCH_CHECK();
    return 0;
}

// the instantiations: (PLT, PLAW), each in the FAST and the general form
#define DS_VARIANTS(X) X(false, false) X(false, true) X(true, false) X(true, true)

template <bool FAST>
int launch_ds(const GenConst &g, const SweepJumps &J, const DsSites<DS_NS> &S, int ky_first, int ky_stride, int nrows, int lG, double vnorm,
              const cplx *twN, double *partial, hipStream_t st) {
    const bool plt = g.qPLT != 0, plaw = g.is_powerlaw != 0;
#define DCASE(a, b) \
    if (plt == a && plaw == b) return launch_ds_t<a, b, FAST>(g, J, S, ky_first, ky_stride, nrows, lG, vnorm, twN, partial, st);
    DS_VARIANTS(DCASE)
#undef DCASE
    return 1;
}

// what both entry points refuse before a plan or the GPU is touched; NULL: nothing
const char *ds_refusal(const zd_params &p, int64_t nsites, const int64_t *sites, double *out7, char *buf, size_t cap) {
    if (!sites || !out7) return "zd_plan_direct_sum needs a site array and an output array";
    if (nsites < 1 || nsites > DS_MAX_SITES) {
        snprintf(buf, cap, "direct summation takes 1 to %d sites per call (got %lld)", DS_MAX_SITES, (long long) nsites);
        return buf;
    }
    for (int64_t i = 0; i < 3 * nsites; i++)
        if (sites[i] < 0 || sites[i] >= p.ppd) {
            snprintf(buf, cap, "site %lld = (%lld, %lld, %lld) lies outside the lattice [0, %lld)^3", (long long) (i / 3), (long long) sites[i / 3 * 3],
                     (long long) sites[i / 3 * 3 + 1], (long long) sites[i / 3 * 3 + 2], (long long) p.ppd);
            return buf;
        }
    if (p.version == 1)
        return "no direct summation with ZD_Version = 1: its mt19937 draws are sequential, no mode can be regenerated from a counter";
    if (p.q2LPT) return "no direct summation on a ZD_q2LPT plan: the sweep regenerates the first-order modes only";
    return nullptr;
}

}  // namespace

namespace zdsweep {

int launch_ds_reduce(const double *partial, long long nwg, int nv, double *out, hipStream_t st) {
    hipLaunchKernelGGL(k_ds_reduce, dim3(nv), dim3(DS_RB), 0, st, partial, nwg, nv, out);
    ZD_LAUNCH_CHECK();
    return 0;
}

DsSites<DS_NS> make_ds_sites(int N, int64_t nsites, const int64_t *sites_zyx, int grp) {
    const long double TWO_PI = 2.0L * 3.14159265358979323846264338327950288L;
    DsSites<DS_NS> S;
    for (int s = 0; s < DS_NS; s++) {  // a short last group sums its first site again; those sums are dropped
        const int64_t i = (int64_t) grp * DS_NS + s < nsites ? (int64_t) grp * DS_NS + s : (int64_t) grp * DS_NS;
        S.z[s] = (int) sites_zyx[3 * i], S.y[s] = (int) sites_zyx[3 * i + 1], S.x[s] = (int) sites_zyx[3 * i + 2];
        const long double a = TWO_PI * (long double) S.z[s] / (long double) N;
        S.wr[s] = (double) cosl(a), S.wi[s] = (double) sinl(a);
    }
    return S;
}

int ds_sweep_sites(zd_plan *pl, int64_t nsites, const int64_t *sites_zyx, double vnorm, double *out7, hipStream_t st) {
    const GenConst &g = pl->g;
    const int N = pl->N, G = pl->nranks, rank = pl->rank, Hq = pl->Hq;  // rows ky = rank + G i, i < Hq
    constexpr int NV = DS_NS * DS_NQ;
    const int ngroups = (int) ((nsites + DS_NS - 1) / DS_NS);
    const long long nwg = (long long) ((N + DS_BX - 1) / DS_BX) * Hq;  // workgroups = partials of a launch group
    zdown::DevBuf<double> part, sums;
    if (part.alloc(NV * (size_t) nwg) != hipSuccess || sums.alloc((size_t) NV * ngroups) != hipSuccess) {
        fprintf(stderr, "zeldovich_hip: direct summation: no device memory for %lld partial sums\n", nwg * NV);
        return 1;
    }
    const SweepJumps J = zdsweep::make_sweep_jumps(N);
    const bool fast = g.genf_tab && !g.phik && !g.qonemode;
    for (int grp = 0; grp < ngroups; grp++) {
        const DsSites<DS_NS> S = make_ds_sites(N, nsites, sites_zyx, grp);
        double *partial = part;
        const size_t per_row = (size_t) ((N + DS_BX - 1) / DS_BX) * NV;
        int rc = 0;
        if (fast) {  // the plane ky = 0 (rank 0) through the general form, every other row through the table arithmetic
            const int skip = rank == 0 ? 1 : 0;
            if (skip) rc = launch_ds<false>(g, J, S, 0, G, 1, pl->S.lG, vnorm, pl->d_twN, partial, st);
            if (!rc) rc = launch_ds<true>(g, J, S, rank + skip * G, G, Hq - skip, pl->S.lG, vnorm, pl->d_twN, partial + skip * per_row, st);
        } else {
            rc = launch_ds<false>(g, J, S, rank, G, Hq, pl->S.lG, vnorm, pl->d_twN, partial, st);
        }
        if (rc || launch_ds_reduce(partial, nwg, NV, sums + (size_t) grp * NV, st)) return 1;
    }
    std::vector<double> h((size_t) NV * ngroups);
    if (hipMemcpyAsync(h.data(), sums, sizeof(double) * h.size(), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        fprintf(stderr, "zeldovich_hip: direct summation failed: %s\n", hipGetErrorString(hipGetLastError()));
        return 1;
    }
    std::copy(h.begin(), h.begin() + DS_NQ * nsites, out7);  // [group][site of the group][7] = [site][7]
    return 0;
}

}  // namespace zdsweep

extern "C" int zd_plan_direct_sum(zd_plan *pl, int64_t nsites, const int64_t *sites_zyx, double *out7, void *hip_stream) {
    if (!pl) {
        fprintf(stderr, "zeldovich_hip: zd_plan_direct_sum needs a plan\n");
        return 1;
    }
    const zd_params &p = pl->p;
    char buf[256];
    if (const char *why = ds_refusal(p, nsites, sites_zyx, out7, buf, sizeof(buf))) {
        fprintf(stderr, "zeldovich_hip: %s\n", why);
        return 1;
    }
    const GenConst &g = pl->g;
    if (!(g.kmax == pl->half || (!p.corner_modes && p.k_cutoff >= 1.0))) {
        fprintf(stderr, "zeldovich_hip: no direct summation while modes on the Nyquist planes stay alive (ZD_CornerModes with "
                        "ZD_k_cutoff = %g): the fields are then not transforms of Hermitian fields\n", p.k_cutoff);
        return 1;
    }
    if (g.gen_phi || g.v1dev || (g.qPLT && !g.eig) || (p.f_NL != 0. && !g.phik) || !pl->d_twN) {
        fprintf(stderr, "zeldovich_hip: this plan does not generate the modes of a run (no direct summation)\n");
        return 1;
    }
    return zdsweep::ds_sweep_sites(pl, nsites, sites_zyx, pl->ec.vnorm, out7, (hipStream_t) hip_stream);
}

extern "C" int zd_direct_sum(const zd_params *p_in, const zd_pk *pk, const double *eig, int64_t eig_ppd, int64_t nsites, const int64_t *sites_zyx,
                             double *out7) {
    if (!p_in || !pk) {
        fprintf(stderr, "zeldovich_hip: zd_direct_sum needs parameters and a power spectrum\n");
        return 1;
    }
    zd_params p = *p_in;
    p.ngpu = 0;
    char buf[256];
    if (const char *why = ds_refusal(p, nsites, sites_zyx, out7, buf, sizeof(buf))) {  // (before a plan — a second-order or phi round — is made)
        fprintf(stderr, "zeldovich_hip: %s\n", why);
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
    return zd_plan_direct_sum(pl, nsites, sites_zyx, out7, nullptr);
}
