// zd_kernels_glass.hip — the delivered field at arbitrary positions: displacements and velocities for glass, tiled-glass, BCC / FCC
// and other off-lattice particle loads (zd_interp_*, zd_plan_interp, zd_displace; include/zeldovich_hip.h).  A pure consumer of
// delivered planes: it reads the records a plan's x stage writes and nothing else, so it serves every row of the README table —
// ZA, PLT, f_NL, composite and convolution grids, 2LPT, 3LPT — without touching the route or a parameter struct.
//
// DEFINITION
//   Particle load.  npart positions p = (x, y, z), float64, in box units, every coordinate in [0, 1); anything else, NaN included, is
//          refused on the host before the GPU is touched.  x is the fastest index of the records, z the plane index.
//   Tiling.  With tile = t >= 1 the load is replicated t^3 times: particle ((a t + b) t + c) npart + i sits at (p_i + (c, b, a)) / t,
//          and results come back in that index order.  (The sum p + c and the quotient are rounded as float64 arithmetic rounds them;
//          a quotient that rounds up to 1.0 lands on cell 0 with tau = 0 by the rule below.)
//   Lattice coordinate.  Per axis, N = PPD: u = p N in float64, i0 = floor(u), tau = u - i0; indices are taken mod N, so u == N gives
//          cell 0 with tau = 0.
//   Weights of order 1 (trilinear).  Offsets 0, 1 get 1 - tau, tau.
//   Weights of order 3 (cubic Lagrange through four points: it interpolates, it is no smoothing B-spline).  Offsets -1, 0, 1, 2 get
//              -tau (tau - 1) (tau - 2) / 6,   (tau + 1) (tau - 1) (tau - 2) / 2,   -(tau + 1) tau (tau - 2) / 2,   (tau + 1) tau (tau - 1) / 6
//   Result.  psi(p) = sum_z sum_y sum_x w_z w_y w_x rec[z][y][x] for the three displacement components and, in RVZel and RVdoubleZel,
//          the three velocity components of the delivered records; out6 = qx, qy, qz, vx, vy, vz (the order of zd_direct_sum; the
//          records hold (z, y, x)).  Accumulation is in float64 whatever the record format; Zeldovich and ZelSimple carry no velocity:
//          their velocity columns are exact zeros.  The records are the plan's own: units, vnorm, PLT and LPT content are unchanged.
//   What follows.  At lattice sites every weight is exactly 0 or 1 and the result equals the record.  Every particle's sums are owned by
//          one thread: there are no floating-point atomics, and two calls with the same stream factor (the same order of planes) return
//          the same bits; another order of planes adds a particle's z terms in another order, within rounding.
//   Accuracy is the user's choice through oversampling: the field at PPD = m N with ZD_k_cutoff = m is the band-limited field of the N
//          run sampled m times as finely, and the interpolation converges to it as m grows.  No window is divided out in k space.
//
// BINNING (at creation).  Cell indices are computed on the device; a counting sort — integer histogram (atomics), exclusive scan,
// scatter — puts the particles into bins (z cell, tile of T x T cells in y, x), z leading, T = 8 or the next power of two that keeps
// the histogram at 2^26 bins.  The order inside a bin is whatever the atomics give; it changes no result, because a particle owns its
// sums.  The sorted arrays hold u = p N per axis (24 bytes), the permutation (4) and the accumulators (24 or 48); results return in
// input order through the permutation.
//
// k_interp_plane<ORDER, FMT>.  For a delivered plane z: the particles whose z stencil holds z, i.e. the bins z and z - 1 (order 1) or
// z - 2 ... z + 1 (order 3), all mod N — one contiguous range of the sorted arrays per bin, blockIdx.y choosing the bin.  One thread
// per particle: the 4 or 16 records of its (y, x) stencil, times its z weight, into its own six accumulators with plain loads and
// stores.  The ranges of one launch are distinct bins (N >= 4), successive planes are ordered by the stream, and nothing assumes that
// successive planes are neighbours in z (residue order, pairs z, z + R / 2 of the two-residue passes).
//
// A staged form — one wave per bin copying the tile's records plus halo into LDS and serving the bin's particles from there — was
// built and measured against this one and is not kept: within 4 % either way.  The accumulators' read-modify-write
// per touched plane is most of the traffic; the records of neighbouring particles already come from L2.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../include/zeldovich_hip.h"
#include "zd_glass.h"
#include "zd_launch.h"
#include "zd_own.h"

namespace {

constexpr int GL_BX      = 256;        // threads per workgroup, one particle each
constexpr int GL_SCAN_E  = 16;         // histogram entries per thread of the scan
constexpr int GL_SCAN_B  = GL_BX * GL_SCAN_E;
constexpr long long GL_MAX_BINS = 1LL << 26;

// bins: key = (z cell * nt + (y cell >> tshift)) * nt + (x cell >> tshift)
struct GlassGrid {
    int N, tshift, nt;
};

// the particles of an object: global indices [first, first + n) of the tiled load; base positions [base0, base0 + ...) are on the device
struct GlassLoad {
    const double *base;  // [..][3] = x, y, z
    long long npart, base0, first;
    int tile;
};

// u = p N of particle g (definition: Tiling, Lattice coordinate)
__device__ __forceinline__ void glass_u(const GlassLoad &L, int N, long long g, double (&u)[3]) {
    const long long cell = g / L.npart, i = g - cell * L.npart;
    const long long t = L.tile;
    const double off[3] = {(double) (cell % t), (double) ((cell / t) % t), (double) (cell / (t * t))};
    const double *p = L.base + 3 * (i - L.base0);
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const double q = (p[j] + off[j]) / (double) t;
        u[j] = q * (double) N;
    }
}

// cell (mod N) and tau of one coordinate
__device__ __forceinline__ int glass_cell(double u, int N, double &tau) {
    const double f = floor(u);
    tau = u - f;
    const int c = (int) f;
    return c >= N ? c - N : c;
}

__device__ __forceinline__ unsigned glass_key(const GlassGrid &G, const double (&u)[3]) {
    double t;
    const int xc = glass_cell(u[0], G.N, t), yc = glass_cell(u[1], G.N, t), zc = glass_cell(u[2], G.N, t);
    return (unsigned) ((zc * G.nt + (yc >> G.tshift)) * G.nt + (xc >> G.tshift));
}

__global__ __launch_bounds__(GL_BX) void k_glass_hist(GlassLoad L, GlassGrid G, long long n, unsigned *__restrict__ hist) {
    const long long i = (long long) blockIdx.x * GL_BX + threadIdx.x;
    if (i >= n) return;
    double u[3];
    glass_u(L, G.N, L.first + i, u);
    atomicAdd(&hist[glass_key(G, u)], 1u);
}

// exclusive scan of hist[nb] in three steps: sums of blocks of GL_SCAN_B entries, their scan by one workgroup, the blocks again
__global__ __launch_bounds__(GL_BX) void k_glass_scan_sums(const unsigned *__restrict__ hist, long long nb, unsigned *__restrict__ bsum) {
    __shared__ unsigned sh[GL_BX];
    const long long i0 = (long long) blockIdx.x * GL_SCAN_B + (long long) threadIdx.x * GL_SCAN_E;
    unsigned v = 0;
    for (int e = 0; e < GL_SCAN_E; e++)
        if (i0 + e < nb) v += hist[i0 + e];
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int h = GL_BX / 2; h >= 1; h >>= 1) {
        if ((int) threadIdx.x < h) sh[threadIdx.x] += sh[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) bsum[blockIdx.x] = sh[0];
}

// exclusive scan over the threads of a workgroup (Hillis-Steele in LDS); returns the exclusive prefix of v, *total = the sum
__device__ __forceinline__ unsigned glass_block_scan(unsigned v, unsigned *sh, unsigned *total) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int d = 1; d < GL_BX; d <<= 1) {
        const unsigned a = (int) threadIdx.x >= d ? sh[threadIdx.x - d] : 0u;
        __syncthreads();
        sh[threadIdx.x] += a;
        __syncthreads();
    }
    const unsigned incl = sh[threadIdx.x];
    *total = sh[GL_BX - 1];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(GL_BX) void k_glass_scan_top(unsigned *__restrict__ bsum, long long nblocks) {
    __shared__ unsigned sh[GL_BX];
    unsigned carry = 0;
    for (long long c0 = 0; c0 < nblocks; c0 += GL_BX) {
        const long long i = c0 + threadIdx.x;
        const unsigned v = i < nblocks ? bsum[i] : 0u;
        unsigned total;
        const unsigned ex = glass_block_scan(v, sh, &total);
        if (i < nblocks) bsum[i] = carry + ex;
        carry += total;
    }
}

__global__ __launch_bounds__(GL_BX) void k_glass_scan_blocks(unsigned *__restrict__ hist, long long nb, const unsigned *__restrict__ bsum) {
    __shared__ unsigned sh[GL_BX];
    const long long i0 = (long long) blockIdx.x * GL_SCAN_B + (long long) threadIdx.x * GL_SCAN_E;
    unsigned v[GL_SCAN_E], sum = 0;
#pragma unroll
    for (int e = 0; e < GL_SCAN_E; e++) {
        v[e] = i0 + e < nb ? hist[i0 + e] : 0u;
        sum += v[e];
    }
    unsigned total;
    unsigned run = bsum[blockIdx.x] + glass_block_scan(sum, sh, &total);
#pragma unroll
    for (int e = 0; e < GL_SCAN_E; e++) {
        if (i0 + e < nb) hist[i0 + e] = run;
        run += v[e];
    }
}

// first sorted slot of every z cell (the scanned histogram at the first bin of the cell); zstart[N] = n
__global__ __launch_bounds__(GL_BX) void k_glass_zstart(const unsigned *__restrict__ hist, GlassGrid G, unsigned n, unsigned *__restrict__ zstart) {
    const int z = blockIdx.x * GL_BX + threadIdx.x;
    if (z < G.N) zstart[z] = hist[(long long) z * G.nt * G.nt];
    if (z == G.N) zstart[z] = n;
}

// hist holds the first free slot of every bin and is advanced by the atomics
__global__ __launch_bounds__(GL_BX) void k_glass_scatter(GlassLoad L, GlassGrid G, long long n, unsigned *__restrict__ hist, unsigned *__restrict__ perm,
                                                         double *__restrict__ su) {
    const long long i = (long long) blockIdx.x * GL_BX + threadIdx.x;
    if (i >= n) return;
    double u[3];
    glass_u(L, G.N, L.first + i, u);
    const unsigned slot = atomicAdd(&hist[glass_key(G, u)], 1u);
    perm[slot] = (unsigned) i;
#pragma unroll
    for (int j = 0; j < 3; j++) su[(size_t) j * n + slot] = u[j];
}

// weights of the definition; offset of weight j from the cell: j (order 1), j - 1 (order 3)
template <int ORDER>
__device__ __forceinline__ void glass_weights(double t, double (&w)[ORDER + 1]) {
    if constexpr (ORDER == 1) {
        w[0] = 1.0 - t;
        w[1] = t;
    } else {
        w[0] = -t * (t - 1.0) * (t - 2.0) / 6.0;
        w[1] = (t + 1.0) * (t - 1.0) * (t - 2.0) / 2.0;
        w[2] = -(t + 1.0) * t * (t - 2.0) / 2.0;
        w[3] = (t + 1.0) * t * (t - 1.0) / 6.0;
    }
}

template <int FMT> constexpr int glass_nq = (FMT == ZD_FMT_RVZEL || FMT == ZD_FMT_RVDOUBLEZEL) ? 6 : 3;
template <int FMT> constexpr int glass_recsize = FMT == ZD_FMT_ZEL ? 32 : FMT == ZD_FMT_RVZEL ? 32 : FMT == ZD_FMT_RVDOUBLEZEL ? 56 : 12;

// record `idx` of a plane as float64 qx, qy, qz (, vx, vy, vz); the records hold (z, y, x) components (zd_epi.h emit_record)
template <int FMT>
__device__ __forceinline__ void glass_record(const char *__restrict__ plane, size_t idx, double (&v)[glass_nq<FMT>]) {
    const char *rec = plane + idx * glass_recsize<FMT>;
    if constexpr (FMT == ZD_FMT_ZEL) {
        const double2 a = reinterpret_cast<const double2 *>(rec)[0], b = reinterpret_cast<const double2 *>(rec)[1];
        v[2] = a.y, v[1] = b.x, v[0] = b.y;
    } else if constexpr (FMT == ZD_FMT_RVZEL) {
        const float4 a = reinterpret_cast<const float4 *>(rec)[0], b = reinterpret_cast<const float4 *>(rec)[1];
        v[2] = a.z, v[1] = a.w, v[0] = b.x, v[5] = b.y, v[4] = b.z, v[3] = b.w;
    } else if constexpr (FMT == ZD_FMT_RVDOUBLEZEL) {
        const double *d = reinterpret_cast<const double *>(rec + 8);
        v[2] = d[0], v[1] = d[1], v[0] = d[2], v[5] = d[3], v[4] = d[4], v[3] = d[5];
    } else {
        const float *d = reinterpret_cast<const float *>(rec);
        v[2] = d[0], v[1] = d[1], v[0] = d[2];
    }
}

template <int ORDER, int FMT>
__global__ __launch_bounds__(GL_BX) void k_interp_plane(int N, zdglass::PlaneJob job, long long n, const double *__restrict__ su,
                                                        const char *__restrict__ plane, double *__restrict__ acc) {
    constexpr int NW = ORDER + 1, NQ = glass_nq<FMT>, LO = ORDER == 3 ? 1 : 0;
    const int j = blockIdx.y;  // the z weight this workgroup's bin takes from the plane
    const unsigned i = blockIdx.x * GL_BX + threadIdx.x;
    if (i >= job.count[j]) return;
    const size_t s = (size_t) job.start[j] + i;
    double tx, ty, tz;
    const int xc = glass_cell(su[s], N, tx), yc = glass_cell(su[(size_t) n + s], N, ty);
    glass_cell(su[2 * (size_t) n + s], N, tz);
    double wx[NW], wy[NW], wz[NW];
    glass_weights<ORDER>(tx, wx);
    glass_weights<ORDER>(ty, wy);
    glass_weights<ORDER>(tz, wz);
    int xs[NW];
#pragma unroll
    for (int a = 0; a < NW; a++) {
        const int x = xc + a - LO;
        xs[a] = x < 0 ? x + N : x >= N ? x - N : x;
    }
    double sum[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) sum[q] = 0.0;
#pragma unroll
    for (int b = 0; b < NW; b++) {
        const int y = yc + b - LO;
        const size_t row = (size_t) (y < 0 ? y + N : y >= N ? y - N : y) * N;
#pragma unroll
        for (int a = 0; a < NW; a++) {
            double v[NQ];
            glass_record<FMT>(plane, row + xs[a], v);
            const double w = wy[b] * wx[a];
#pragma unroll
            for (int q = 0; q < NQ; q++) sum[q] = fma(w, v[q], sum[q]);
        }
    }
    const double w = wz[j];
#pragma unroll
    for (int q = 0; q < NQ; q++) {
        double *a = acc + (size_t) q * n + s;
        *a = fma(w, sum[q], *a);
    }
}

// sorted accumulators -> out[(g - g0) * 6 + q] for the particles g0 <= g < g0 + gn (input order); velocity columns a format lacks: 0
__global__ __launch_bounds__(GL_BX) void k_glass_unsort(long long n, int nq, const unsigned *__restrict__ perm, const double *__restrict__ acc, long long g0,
                                                        long long gn, double *__restrict__ out) {
    const long long s = (long long) blockIdx.x * GL_BX + threadIdx.x;
    if (s >= n) return;
    const long long g = (long long) perm[s] - g0;
    if (g < 0 || g >= gn) return;
    for (int q = 0; q < 6; q++) out[g * 6 + q] = q < nq ? acc[(size_t) q * n + s] : 0.0;
}

inline unsigned blocks_of(long long n) { return (unsigned) ((n + GL_BX - 1) / GL_BX); }

int launch_glass_hist(const GlassLoad &L, const GlassGrid &G, long long n, unsigned *hist, hipStream_t st) {
    hipLaunchKernelGGL(k_glass_hist, dim3(blocks_of(n)), dim3(GL_BX), 0, st, L, G, n, hist);
    ZD_LAUNCH_CHECK();
    return 0;
}

int launch_glass_scan(unsigned *hist, long long nb, unsigned *bsum, hipStream_t st) {
    const long long nblocks = (nb + GL_SCAN_B - 1) / GL_SCAN_B;
    hipLaunchKernelGGL(k_glass_scan_sums, dim3((unsigned) nblocks), dim3(GL_BX), 0, st, hist, nb, bsum);
    ZD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_glass_scan_top, dim3(1), dim3(GL_BX), 0, st, bsum, nblocks);
    ZD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_glass_scan_blocks, dim3((unsigned) nblocks), dim3(GL_BX), 0, st, hist, nb, bsum);
    ZD_LAUNCH_CHECK();
    return 0;
}

int launch_glass_scatter(const GlassLoad &L, const GlassGrid &G, long long n, unsigned *hist, unsigned *zstart, unsigned *perm, double *su, hipStream_t st) {
    hipLaunchKernelGGL(k_glass_zstart, dim3(blocks_of(G.N + 1)), dim3(GL_BX), 0, st, hist, G, (unsigned) n, zstart);
    ZD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_glass_scatter, dim3(blocks_of(n)), dim3(GL_BX), 0, st, L, G, n, hist, perm, su);
    ZD_LAUNCH_CHECK();
    return 0;
}

template <int ORDER, int FMT>
int launch_interp_plane_t(int N, const zdglass::PlaneJob &job, long long n, const double *su, const void *plane, double *acc, hipStream_t st) {
    unsigned most = 0;
    for (int j = 0; j <= ORDER; j++) most = std::max(most, job.count[j]);
    if (most == 0) return 0;  // no particle's stencil holds this plane
    hipLaunchKernelGGL((k_interp_plane<ORDER, FMT>), dim3(blocks_of(most), ORDER + 1), dim3(GL_BX), 0, st, N, job, n, su, (const char *) plane, acc);
    ZD_LAUNCH_CHECK();
    return 0;
}

int launch_interp_plane(int order, int fmt, int N, const zdglass::PlaneJob &job, long long n, const double *su, const void *plane, double *acc,
                        hipStream_t st) {
#define GCASE(o, f) \
    if (order == o && fmt == f) return launch_interp_plane_t<o, f>(N, job, n, su, plane, acc, st);
    GCASE(1, ZD_FMT_ZEL) GCASE(1, ZD_FMT_RVZEL) GCASE(1, ZD_FMT_RVDOUBLEZEL) GCASE(1, ZD_FMT_ZELSIMPLE)
    GCASE(3, ZD_FMT_ZEL) GCASE(3, ZD_FMT_RVZEL) GCASE(3, ZD_FMT_RVDOUBLEZEL) GCASE(3, ZD_FMT_ZELSIMPLE)
#undef GCASE
    fprintf(stderr, "zeldovich_hip: no interpolation kernel of order %d for ICFormat %d\n", order, fmt);
    return 1;
}

int launch_glass_unsort(long long n, int nq, const unsigned *perm, const double *acc, long long g0, long long gn, double *out, hipStream_t st) {
    hipLaunchKernelGGL(k_glass_unsort, dim3(blocks_of(n)), dim3(GL_BX), 0, st, n, nq, perm, acc, g0, gn, out);
    ZD_LAUNCH_CHECK();
    return 0;
}

int fail(const char *what) {
    fprintf(stderr, "zeldovich_hip: %s\n", what);
    return 1;
}

}  // namespace

// the consumer object: the sorted load of one sweep and its accumulators
struct zd_interp {
    int N = 0, fmt = 0, order = 0, nq = 0;
    long long n = 0;
    zdown::DevBuf<double> d_su, d_acc;  // [3][n] u = p N of the sorted particles; [nq][n] sums
    zdown::DevBuf<unsigned> d_perm;     // sorted slot -> index in the object's input order
    std::vector<unsigned> zstart;       // [N + 1] first sorted slot of every z cell
    std::vector<char> seen;             // [N] planes added so far
    int nseen = 0;
};

namespace zdglass {

const char *load_refusal(int64_t ppd, int32_t icformat, int32_t order, int64_t npart, const double *pos_xyz, int64_t tile, char *buf, size_t cap) {
    if (order != 1 && order != 3) {
        snprintf(buf, cap, "order = %d: the interpolation has order 1 (trilinear) or 3 (cubic Lagrange)", order);
        return buf;
    }
    if (npart < 1) {
        snprintf(buf, cap, "npart = %lld: a particle load has at least one particle", (long long) npart);
        return buf;
    }
    if (tile < 1 || tile > 65536) {
        snprintf(buf, cap, "tile = %lld: the load is replicated tile^3 times, 1 <= tile <= 65536", (long long) tile);
        return buf;
    }
    if ((double) npart * (double) tile * (double) tile * (double) tile > 4e18) {
        snprintf(buf, cap, "npart = %lld with tile = %lld: more particles than an index holds", (long long) npart, (long long) tile);
        return buf;
    }
    if (!pos_xyz) return "pos_xyz is a null pointer: the load needs its positions";
    if (ppd < 4 || ppd > ZD_MAX_PPD) {
        snprintf(buf, cap, "ppd = %lld: planes of an interpolation have 4 to %d points per side", (long long) ppd, ZD_MAX_PPD);
        return buf;
    }
    if (icformat < ZD_FMT_ZEL || icformat > ZD_FMT_ZELSIMPLE) {
        snprintf(buf, cap, "icformat = %d is no record format (ZD_FMT_*)", icformat);
        return buf;
    }
    for (int64_t i = 0; i < 3 * npart; i++)
        if (!(pos_xyz[i] >= 0.0 && pos_xyz[i] < 1.0)) {  // (NaN fails both)
            snprintf(buf, cap, "pos_xyz: particle %lld = (%.17g, %.17g, %.17g) lies outside [0, 1)^3", (long long) (i / 3), pos_xyz[i / 3 * 3],
                     pos_xyz[i / 3 * 3 + 1], pos_xyz[i / 3 * 3 + 2]);
            return buf;
        }
    return nullptr;
}

long long hist_bins(int64_t ppd) {
    int tshift = 3;
    long long nt = (ppd + 7) >> 3;
    while (ppd * nt * nt > GL_MAX_BINS) tshift++, nt = (ppd + (1LL << tshift) - 1) >> tshift;
    return ppd * nt * nt;
}

int create(int64_t ppd, int32_t icformat, int32_t order, int64_t npart, const double *pos_xyz, int64_t tile, int64_t first, int64_t count,
           zd_interp **out) {
    if (count < 1 || count > MAX_SWEEP) {
        fprintf(stderr, "zeldovich_hip: an interpolation object takes 1 to %lld particles (got %lld)\n", MAX_SWEEP, (long long) count);
        return 1;
    }
    std::unique_ptr<zd_interp> it(new zd_interp);
    it->N = (int) ppd, it->fmt = icformat, it->order = order, it->n = count;
    it->nq = icformat == ZD_FMT_RVZEL || icformat == ZD_FMT_RVDOUBLEZEL ? 6 : 3;
    GlassGrid G = {(int) ppd, 3, 0};
    G.nt = (G.N + 7) >> 3;
    while ((long long) G.N * G.nt * G.nt > GL_MAX_BINS) G.tshift++, G.nt = (G.N + (1 << G.tshift) - 1) >> G.tshift;
    const long long nb = (long long) G.N * G.nt * G.nt, nblocks = (nb + GL_SCAN_B - 1) / GL_SCAN_B;
    // the base positions this object's particles come from: all of them for a tiled load, else its own slice
    const int64_t base0 = tile == 1 ? first : 0, nbase = tile == 1 ? count : npart;
    zdown::DevBuf<double> d_base;
    zdown::DevBuf<unsigned> d_hist, d_bsum, d_zstart;
    const size_t n = (size_t) count;
    if (d_base.alloc(3 * (size_t) nbase) != hipSuccess || d_hist.alloc((size_t) nb) != hipSuccess || d_bsum.alloc((size_t) nblocks) != hipSuccess ||
        d_zstart.alloc((size_t) G.N + 1) != hipSuccess || it->d_su.alloc(3 * n) != hipSuccess || it->d_perm.alloc(n) != hipSuccess ||
        it->d_acc.alloc((size_t) it->nq * n) != hipSuccess) {
        fprintf(stderr, "zeldovich_hip: no device memory for an interpolation of %lld particles (%.2f GB)\n", (long long) count,
                (n * (28.0 + 8.0 * it->nq) + 24.0 * nbase + 4.0 * nb) / 1e9);
        return 1;
    }
    hipStream_t st = 0;
    const GlassLoad L = {d_base.get(), (long long) npart, (long long) base0, (long long) first, (int) tile};
    it->zstart.resize((size_t) G.N + 1);
    it->seen.assign((size_t) G.N, 0);
    if (hipMemcpyAsync(d_base, pos_xyz + 3 * base0, sizeof(double) * 3 * (size_t) nbase, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemsetAsync(d_hist, 0, sizeof(unsigned) * (size_t) nb, st) != hipSuccess ||
        hipMemsetAsync(it->d_acc, 0, sizeof(double) * (size_t) it->nq * n, st) != hipSuccess)
        return fail("interpolation: upload of the particle load failed");
    if (launch_glass_hist(L, G, count, d_hist, st) || launch_glass_scan(d_hist, nb, d_bsum, st) ||
        launch_glass_scatter(L, G, count, d_hist, d_zstart, it->d_perm, it->d_su, st))
        return 1;
    if (hipMemcpyAsync(it->zstart.data(), d_zstart, sizeof(unsigned) * ((size_t) G.N + 1), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
        fprintf(stderr, "zeldovich_hip: interpolation: binning the particle load failed: %s\n", hipGetErrorString(hipGetLastError()));
        return 1;
    }
    *out = it.release();
    return 0;
}

}  // namespace zdglass

extern "C" int zd_interp_create(int64_t ppd, int32_t icformat, int32_t order, int64_t npart, const double *pos_xyz, zd_interp **out) {
    char buf[256];
    if (!out) return fail("zd_interp_create: out is a null pointer");
    *out = nullptr;
    if (const char *why = zdglass::load_refusal(ppd, icformat, order, npart, pos_xyz, 1, buf, sizeof(buf))) {
        fprintf(stderr, "zeldovich_hip: zd_interp_create: %s\n", why);
        return 1;
    }
    return zdglass::create(ppd, icformat, order, npart, pos_xyz, 1, 0, npart, out);
}

extern "C" void zd_interp_destroy(zd_interp *it) { delete it; }

extern "C" int zd_interp_add_plane(zd_interp *it, int64_t z, const void *d_plane_records, void *hip_stream) {
    if (!it) return fail("zd_interp_add_plane needs an interpolation object");
    if (!d_plane_records) return fail("zd_interp_add_plane: d_plane_records is a null pointer");
    if (z < 0 || z >= it->N) {
        fprintf(stderr, "zeldovich_hip: zd_interp_add_plane: plane z = %lld lies outside [0, %d)\n", (long long) z, it->N);
        return 1;
    }
    if (it->seen[(size_t) z]) {
        fprintf(stderr, "zeldovich_hip: zd_interp_add_plane: plane z = %lld was added before\n", (long long) z);
        return 1;
    }
    zdglass::PlaneJob job = {};
    const int lo = it->order == 3 ? 1 : 0;
    for (int j = 0; j <= it->order; j++) {  // weight j belongs to the cell z - (j - lo)
        const int zc = (int) ((z - (j - lo) + it->N) % it->N);
        job.start[j] = it->zstart[(size_t) zc];
        job.count[j] = it->zstart[(size_t) zc + 1] - it->zstart[(size_t) zc];
    }
    if (launch_interp_plane(it->order, it->fmt, it->N, job, it->n, it->d_su, d_plane_records, it->d_acc, (hipStream_t) hip_stream)) return 1;
    it->seen[(size_t) z] = 1;
    it->nseen++;
    return 0;
}

extern "C" int zd_interp_result(zd_interp *it, double *out6) {
    if (!it) return fail("zd_interp_result needs an interpolation object");
    if (!out6) return fail("zd_interp_result: out6 is a null pointer");
    if (it->nseen != it->N) {
        int64_t z = 0;
        while (z < it->N && it->seen[(size_t) z]) z++;
        fprintf(stderr, "zeldovich_hip: zd_interp_result: %d of %d planes have not been added (the first is z = %lld)\n", it->N - it->nseen, it->N,
                (long long) z);
        return 1;
    }
    // input order through the permutation, in at most eight pieces of a device buffer
    const long long piece = std::max<long long>(1LL << 22, (it->n + 7) / 8);
    zdown::DevBuf<double> d_out;
    if (hipDeviceSynchronize() != hipSuccess || d_out.alloc(6 * (size_t) std::min(piece, it->n)) != hipSuccess)
        return fail("zd_interp_result: the planes' work failed or there is no device memory for the results");
    for (long long g0 = 0; g0 < it->n; g0 += piece) {
        const long long gn = std::min(piece, it->n - g0);
        if (launch_glass_unsort(it->n, it->nq, it->d_perm, it->d_acc, g0, gn, d_out, 0)) return 1;
        if (hipMemcpy(out6 + 6 * g0, d_out, sizeof(double) * 6 * (size_t) gn, hipMemcpyDeviceToHost) != hipSuccess)
            return fail("zd_interp_result: copying the results failed");
    }
    return 0;
}

void zdglass::shape(const zd_interp *it, int64_t *ppd, int32_t *icformat) { *ppd = it->N, *icformat = it->fmt; }
