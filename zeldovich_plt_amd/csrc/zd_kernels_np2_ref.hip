// zd_kernels_np2_ref.hip — composite-length (2^a 3^b 5^c 7^d) line transforms on the reference's arrays, for ZD_f_NL on the
// composite grids.
//
// f_NL's second pass bypasses the zero rule (D = PhiK * M on every mode but k = 0, src/zeldovich.cpp:393-400), so the modes
// on the Nyquist planes |k_i| = N/2 are live and the reference takes Re / Im of its mixed arrays: the Hermitian field stores of
// zd_kernels_np2.hip cannot carry them.  The convolution path (zd_kernels_any.hip) has the right store — [plane][array][y][x],
// general complex lines, the twin rules of k_any_scatter — but transforms every line as a Bluestein convolution of twice its
// length.  These kernels are its two transforms on the composite engine of zd_fft_q.h instead, with the same arguments and
// the same (unnormalised, e^{+2 pi i nk/n}) result:
//     k_refq_cols   in-place transform of strided lines: the z lines of the folded generator output, y columns of the store,
//                   the full-length z lines of the phi round (stream factor 1)
//     k_refq_lines  in-place transform of contiguous lines: the x lines
// The phi round (stream factor 1) keeps only the half-space rows ky < N/2 of its planes, [z][ky][x]: phi is a real field, so a
// y column is rebuilt from its half.  Its z lines go from the generator output into those planes and from the planes into PhiK
// (k_refq_cols_oop), and its y columns run inverse transform, phi + f_NL phi^2 and the second transform in one kernel (k_refq_yphi):
// 8 N^3 bytes of planes beside PhiK's 8 N^3 where the full store held 16 N^3.
// The generator, the scatter and the particle epilogue of the main pass are the convolution path's own.
// On several ranks (G > 1) the arrays are split over the ranks with the chunk semantics of the power-of-two store (AnyChunks,
// zd_device.h), so that zd_multi.cpp moves the bytes as it does there; the kernels that know that layout:
//     k_refq_scatter  the z lines of this rank's rows into the chunked send store (self and twin slots)
//     k_refq_ycols    y columns gathered over the G chunks of a ring slot (the main pass and the phi round)
//     k_refq_xphi     the phi round's x lines: inverse transform, phi + f_NL phi^2, second transform
//     k_refq_emit     the particle epilogue with the chunked row map
// x lines are whole rows (k_refq_lines per chunk); the phi round's forward z lines into PhiK[row slot][kz][x] are k_refq_cols_oop.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "zd_device.h"
#include "zd_epi.h"
#include "zd_fft_q.h"
#include "zd_launch.h"

using namespace zd;
using zdfft::cplx;

// line (batch, x): points data[batch * batch_stride + x + i * point_stride], i < P*Q, for the columns x < ncols.  zero_point >= 0:
// that input point counts as zero (the Nyquist row of the y stage, zeldovich.cpp:644-650).
//   grid: (ceil(ncols / W), nbatch)   block: W * Q * P / E
template <int P, int E, int Q, int W>
__global__ __launch_bounds__(W *Q *P / E) void k_refq_cols(const cplx *__restrict__ twP, const cplx *__restrict__ twN, const cplx *__restrict__ twQ,
                                                         cplx *__restrict__ data, long long batch_stride, long long point_stride, int ncols,
                                                         int zero_point) {
    using LQ = zdfft::LineQ<P, E, Q, W, false>;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr int T = LQ::T;
    const int c = threadIdx.x % (W * Q), t = threadIdx.x / (W * Q);
    const int w = c % W, n2 = c / W;
    const int x = blockIdx.x * W + w;
    const bool on = x < ncols;
    cplx *base = data + (long long) blockIdx.y * batch_stride + (on ? x : 0);
    double re[E], im[E];
#pragma unroll
    for (int e = 0; e < E; e++) {
        const int i = Q * (t + T * e) + n2;
        cplx v = cplx{0.0, 0.0};
        if (on && i != zero_point) v = base[(long long) i * point_stride];
        re[e] = v.x;
        im[e] = v.y;
    }
    LQ::run(re, im, t, w, n2, lds, twP, twN, twQ);  // (ends with a barrier: every point of the tile has been read)
    if (!on) return;
#pragma unroll
    for (int e = 0; e < E; e++) base[(long long) ((t + T * e) + P * n2) * point_stride] = cplx{re[e], im[e]};
}

// line l at data[l * pitch], l < nlines.   grid: ceil(nlines / W)   block: W * Q * P / E
template <int P, int E, int Q, int W>
__global__ __launch_bounds__(W *Q *P / E) void k_refq_lines(const cplx *__restrict__ twP, const cplx *__restrict__ twN, const cplx *__restrict__ twQ,
                                                          cplx *__restrict__ data, long long pitch, long long nlines) {
    using LQ = zdfft::LineQ<P, E, Q, W, true>;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr int T = LQ::T;
    const int t = threadIdx.x % T, c = threadIdx.x / T;
    const int w = c % W, n2 = c / W;
    const long long line = (long long) blockIdx.x * W + w;
    const bool on = line < nlines;
    cplx *base = data + (on ? line : 0) * pitch;
    double re[E], im[E];
#pragma unroll
    for (int e = 0; e < E; e++) {
        cplx v = cplx{0.0, 0.0};
        if (on) v = base[Q * (t + T * e) + n2];
        re[e] = v.x;
        im[e] = v.y;
    }
    LQ::run(re, im, t, w, n2, lds, twP, twN, twQ);
    if (!on) return;
#pragma unroll
    for (int e = 0; e < E; e++) base[(t + T * e) + P * n2] = cplx{re[e], im[e]};
}

// out-of-place strided lines: line (batch, x) read from in[batch * in_bs + x + i * in_ps], written (conjugated if CONJ) to
// out[batch * out_bs + x + k * out_ps].  The phi round on half-space planes: the z lines of the generator output into the store,
// and the last z lines of the store into PhiK[ky][kz][x].     grid: (ceil(ncols / W), nbatch)   block: W * Q * P / E
template <int P, int E, int Q, int W, bool CONJ>
__global__ __launch_bounds__(W *Q *P / E) void k_refq_cols_oop(const cplx *__restrict__ twP, const cplx *__restrict__ twN,
                                                             const cplx *__restrict__ twQ, const cplx *__restrict__ in, long long in_bs,
                                                             long long in_ps, cplx *__restrict__ out, long long out_bs, long long out_ps,
                                                             int ncols) {
    using LQ = zdfft::LineQ<P, E, Q, W, false>;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr int T = LQ::T;
    const int c = threadIdx.x % (W * Q), t = threadIdx.x / (W * Q);
    const int w = c % W, n2 = c / W;
    const int x = blockIdx.x * W + w;
    const bool on = x < ncols;
    const cplx *src = in + (long long) blockIdx.y * in_bs + (on ? x : 0);
    double re[E], im[E];
#pragma unroll
    for (int e = 0; e < E; e++) {
        cplx v = cplx{0.0, 0.0};
        if (on) v = src[(long long) (Q * (t + T * e) + n2) * in_ps];
        re[e] = v.x;
        im[e] = v.y;
    }
    LQ::run(re, im, t, w, n2, lds, twP, twN, twQ);
    if (!on) return;
    cplx *dst = out + (long long) blockIdx.y * out_bs + x;
#pragma unroll
    for (int e = 0; e < E; e++) dst[(long long) ((t + T * e) + P * n2) * out_ps] = cplx{re[e], CONJ ? -im[e] : im[e]};
}

// ZD_f_NL, phi round on half-space planes (store [z][ky < N/2][x], x already transformed): the y columns of the real field phi.  A
// column is rebuilt whole from its half — G[N - ky] = conj G[ky] (the twin rows of k_any_scatter), G[N/2] = 0 (the Nyquist row of the
// y stage, zeldovich.cpp:644-650) — transformed, phi = Re -> (phi + f_NL phi^2) / N^3 (k_any_phi_nl), transformed again as a real
// line (the conjugate of its forward transform, as on the full store) and its rows ky < N/2 written back.
//   grid: (ceil(N / W), N planes)   block: W * Q * P / E
template <int P, int E, int Q, int W>
__global__ __launch_bounds__(W *Q *P / E) void k_refq_yphi(const cplx *__restrict__ twP, const cplx *__restrict__ twN, const cplx *__restrict__ twQ,
                                                         cplx *__restrict__ store, long long pitch, double f_NL, double inv_ppd3) {
    using LQ = zdfft::LineQ<P, E, Q, W, false>;
    static_assert(LQ::LDS_DOUBLES >= W * P * Q, "the real column must fit the transform's LDS");
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr int T = LQ::T, N = P * Q, H = N / 2;
    const int c = threadIdx.x % (W * Q), t = threadIdx.x / (W * Q);
    const int w = c % W, n2 = c / W;
    const int x = blockIdx.x * W + w;
    const bool on = x < N;
    cplx *base = store + (long long) blockIdx.y * H * pitch + (on ? x : 0);
    double re[E], im[E];
#pragma unroll
    for (int e = 0; e < E; e++) {
        const int i = Q * (t + T * e) + n2;
        cplx v = cplx{0.0, 0.0};
        if (on && i < H) v = base[(long long) i * pitch];
        else if (on && i > H) {
            v = base[(long long) (N - i) * pitch];
            v.y = -v.y;
        }
        re[e] = v.x;
        im[e] = v.y;
    }
    LQ::run(re, im, t, w, n2, lds, twP, twN, twQ);  // (ends with a barrier)
    // output index (t + T e) + P n2 -> input index Q (t + T e) + n2 of the second transform: through the LDS, real parts only
#pragma unroll
    for (int e = 0; e < E; e++) {
        const double phi = re[e];
        lds[w * N + (t + T * e) + P * n2] = (phi + f_NL * phi * phi) * inv_ppd3;
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < E; e++) {
        re[e] = lds[w * N + Q * (t + T * e) + n2];
        im[e] = 0.0;
    }
    __syncthreads();
    LQ::run(re, im, t, w, n2, lds, twP, twN, twQ);
    if (!on) return;
#pragma unroll
    for (int e = 0; e < E; e++) {
        const int k = (t + T * e) + P * n2;
        if (k < H) base[(long long) k * pitch] = cplx{re[e], im[e]};
    }
}

// ---- several ranks: the arrays split over G ranks (AnyChunks, zd_device.h) ----
// Chunks are plane-major, so along z the store of a rank is one plane stride: plane z2 = c Zq + zl at (c Zq + zl) narray 2Hq pitch.
// The phi round's forward z lines into PhiK are therefore k_refq_cols_oop with that stride.

// z stage, second half: the z lines of rows ky = ky_first + G (r0 + kyl) (Y as in k_any_scatter) go to plane z2 = chunk z2 / Zq, local
// plane z2 % Zq; row slot r0 + kyl ("self") and Hq + r0 + kyl, column N - x ("twin"), the twin rules of k_any_scatter.
//   grid: (ceil(N / 256), L, njobs * nky)   block: 256
__global__ __launch_bounds__(256) void k_refq_scatter(JobList jobs, AnyChunks C, int ky_first, int r0, int nky, int L, const cplx *__restrict__ Y,
                                                     cplx *__restrict__ store) {
    const int N = C.N;
    const int x = blockIdx.x * 256 + threadIdx.x, z2 = blockIdx.y;
    const int j = blockIdx.z / nky, kyl = blockIdx.z % nky;
    if (x >= N) return;
    const int slot = r0 + kyl, ky = ky_first + C.G * slot;
    const int kind = jobs.kind[j], arr = jobs.arr[j];
    const bool twin_only = jobs.twin[j] != 0;
    if (ky == 0 && twin_only) return;  // ky = 0 is its own twin plane: every column written as "self"
    const cplx v = Y[(((long long) j * nky + kyl) * L + z2) * N + x];
    cplx *img = store + (long long) (z2 / C.Zq) * C.chunk + ((long long) (z2 % C.Zq) * C.narray + arr) * (2 * C.Hq) * C.pitch;
    if (!twin_only) img[(long long) slot * C.pitch + x] = v;
    if (ky != 0 && (twin_only || kind == JOB_C_BOTH || kind == JOB_DENS)) {
        const double sgr = (kind == JOB_C_BOTH) ? -1.0 : 1.0, sgi = (kind == JOB_C_BOTH) ? 1.0 : -1.0;  // -conj / conj
        img[(long long) (C.Hq + slot) * C.pitch + (x ? N - x : 0)] = cplx{sgr * v.x, sgi * v.y};
    }
}

// y columns over the G chunks of a store / ring slot (C.chunk = its chunk stride), in place: column (image b, x < ncols), b = local
// plane * narray + array, point ky at chunk / slot any_chunk_row(ky).  zero_point >= 0: that input point counts as zero (ky = N/2, the Nyquist
// row, zeldovich.cpp:644-650); outputs k >= out_limit are not written back (the phi round keeps the rows ky < N/2 only).
//   grid: (ceil(ncols / W), nbatch)   block: W * Q * P / E
template <int P, int E, int Q, int W>
__global__ __launch_bounds__(W *Q *P / E) void k_refq_ycols(const cplx *__restrict__ twP, const cplx *__restrict__ twN, const cplx *__restrict__ twQ,
                                                          AnyChunks C, cplx *__restrict__ data, int ncols, int zero_point, int out_limit) {
    using LQ = zdfft::LineQ<P, E, Q, W, false>;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr int T = LQ::T;
    const int c = threadIdx.x % (W * Q), t = threadIdx.x / (W * Q);
    const int w = c % W, n2 = c / W;
    const int x = blockIdx.x * W + w;
    const bool on = x < ncols;
    cplx *img = data + (long long) blockIdx.y * (2 * C.Hq) * C.pitch + (on ? x : 0);
    double re[E], im[E];
#pragma unroll
    for (int e = 0; e < E; e++) {
        const int i = Q * (t + T * e) + n2;
        cplx v = cplx{0.0, 0.0};
        if (on && i != zero_point) {
            int ch, s;
            any_chunk_row(C, i, ch, s);
            v = img[ch * C.chunk + (long long) s * C.pitch];
        }
        re[e] = v.x;
        im[e] = v.y;
    }
    LQ::run(re, im, t, w, n2, lds, twP, twN, twQ);  // (ends with a barrier: every point of the tile has been read)
    if (!on) return;
#pragma unroll
    for (int e = 0; e < E; e++) {
        const int k = (t + T * e) + P * n2;
        if (k >= out_limit) continue;
        int ch, s;
        any_chunk_row(C, k, ch, s);
        img[ch * C.chunk + (long long) s * C.pitch] = cplx{re[e], im[e]};
    }
}

// ZD_f_NL phi round on several ranks, x lines (whole rows, after the inverse y transform): inverse transform, phi = Re -> (phi + f_NL phi^2) / N^3
// (k_any_phi_nl), transformed again as a real line (the forward transform's conjugate; the conjugation happens in the last z lines,
// as on one rank).  Line l at data[l * pitch].   grid: ceil(nlines / W)   block: W * Q * P / E
template <int P, int E, int Q, int W>
__global__ __launch_bounds__(W *Q *P / E) void k_refq_xphi(const cplx *__restrict__ twP, const cplx *__restrict__ twN, const cplx *__restrict__ twQ,
                                                         cplx *__restrict__ data, long long pitch, long long nlines, double f_NL, double inv_ppd3) {
    using LQ = zdfft::LineQ<P, E, Q, W, true>;
    extern __shared__ __attribute__((aligned(16))) double lds[];  // max(LQ::LDS_DOUBLES, W N) doubles
    constexpr int T = LQ::T, N = P * Q;
    const int t = threadIdx.x % T, c = threadIdx.x / T;
    const int w = c % W, n2 = c / W;
    const long long line = (long long) blockIdx.x * W + w;
    const bool on = line < nlines;
    cplx *base = data + (on ? line : 0) * pitch;
    double re[E], im[E];
#pragma unroll
    for (int e = 0; e < E; e++) {
        cplx v = cplx{0.0, 0.0};
        if (on) v = base[Q * (t + T * e) + n2];
        re[e] = v.x;
        im[e] = v.y;
    }
    LQ::run(re, im, t, w, n2, lds, twP, twN, twQ);  // (ends with a barrier)
    // output index (t + T e) + P n2 -> input index Q (t + T e) + n2 of the second transform: through the LDS, real parts only
#pragma unroll
    for (int e = 0; e < E; e++) {
        const double phi = re[e];
        lds[w * N + (t + T * e) + P * n2] = (phi + f_NL * phi * phi) * inv_ppd3;
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < E; e++) {
        re[e] = lds[w * N + Q * (t + T * e) + n2];
        im[e] = 0.0;
    }
    __syncthreads();
    LQ::run(re, im, t, w, n2, lds, twP, twN, twQ);
    if (!on) return;
#pragma unroll
    for (int e = 0; e < E; e++) base[(t + T * e) + P * n2] = cplx{re[e], im[e]};
}

// WriteParticlesSlab (src/output.cpp:86-203) on planes [plane0, plane0 + nplanes) of an AnyChunks store / ring slot (x transformed):
// the epilogue of k_any_emit, row y found through any_chunk_row.   grid: (ceil(N / 256), N, nplanes)   block: 256
template <int NA>
__global__ __launch_bounds__(256) void k_refq_emit(AnyChunks C, EpiConst ec, const cplx *__restrict__ store, int plane0, int z_first, int z_step,
                                                  char *__restrict__ records, float *__restrict__ density, Reduce *__restrict__ red) {
    __shared__ double scr[7 * 4];
    const int N = C.N;
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, pl = plane0 + blockIdx.z;
    const int z = z_first + z_step * (int) blockIdx.z;
    double ssq = 0.0;
    MaxAbs mx;
    if (x < N) {
        int ch, s;
        any_chunk_row(C, y, ch, s);
        const long long astride = (long long) (2 * C.Hq) * C.pitch;
        const cplx *row = store + ch * C.chunk + (long long) pl * C.narray * astride + (long long) s * C.pitch + x;
        const cplx a0 = row[0];
        const long long pidx = (long long) blockIdx.z * N * N + (long long) y * N + x;
        ssq = a0.x * a0.x;
        if (density) density[pidx] = (float) a0.x;
        if constexpr (NA >= 2) {
            const cplx a1 = row[astride];
            const double pos[3] = {a0.y, a1.x, a1.y};
            double vel[3] = {pos[0] * ec.vnorm, pos[1] * ec.vnorm, pos[2] * ec.vnorm};
            if constexpr (NA == 4) {
                const cplx a2 = row[2 * astride], a3 = row[3 * astride];
                vel[0] = a2.y * ec.vnorm;
                vel[1] = a3.x * ec.vnorm;
                vel[2] = a3.y * ec.vnorm;
            }
            max_track(mx, pos, ((unsigned long long) z * N + (unsigned long long) y) * N + (unsigned long long) x);
            if (records) emit_record(records, pidx, ec, z, y, x, pos, vel);
        }
    }
    xfft_reduce<256, NA>(scr, red, ssq, mx);
}

namespace zd {

template <int P, int E, int Q, int W>
static int launch_refq_ycols_t(const cplx *tw, const AnyChunks &C, void *data, int ncols, int nbatch, int zero_point, int out_limit,
                               hipStream_t st) {
    constexpr int threads = W * Q * P / E;
    const size_t shmem = sizeof(double) * zdfft::LineQ<P, E, Q, W, false>::LDS_DOUBLES;
    if (shmem > 160 * 1024 || nbatch < 1 || nbatch > 65535) return 2;
    ZD_PROBE_RETURN();
    set_dyn_lds<k_refq_ycols<P, E, Q, W>>(shmem);
    hipLaunchKernelGGL((k_refq_ycols<P, E, Q, W>), dim3((ncols + W - 1) / W, nbatch), dim3(threads), shmem, st, tw, tw + P, tw + P + P * Q, C,
                       (cplx *) data, ncols, zero_point, out_limit);
    ZD_LAUNCH_CHECK();
    return 0;
}
template <int P, int E, int Q, int W>
static int launch_refq_xphi_t(const cplx *tw, void *data, long long pitch, long long nlines, double f_NL, hipStream_t st) {
    constexpr int threads = W * Q * P / E, N = P * Q;
    constexpr size_t ld = zdfft::LineQ<P, E, Q, W, true>::LDS_DOUBLES;
    const size_t shmem = sizeof(double) * (ld > (size_t) W * N ? ld : (size_t) W * N);
    if (shmem > 160 * 1024) return 2;
    ZD_PROBE_RETURN();
    set_dyn_lds<k_refq_xphi<P, E, Q, W>>(shmem);
    hipLaunchKernelGGL((k_refq_xphi<P, E, Q, W>), dim3((unsigned) ((nlines + W - 1) / W)), dim3(threads), shmem, st, tw, tw + P, tw + P + N,
                       (cplx *) data, pitch, nlines, f_NL, 1. / N / N / N);
    ZD_LAUNCH_CHECK();
    return 0;
}

template <int P, int E, int Q, int W, bool CONJ>
static int launch_refq_cols_oop_t(const cplx *tw, const void *in, long long in_bs, long long in_ps, void *out, long long out_bs,
                                  long long out_ps, int ncols, int nbatch, hipStream_t st) {
    constexpr int threads = W * Q * P / E;
    const size_t shmem = sizeof(double) * zdfft::LineQ<P, E, Q, W, false>::LDS_DOUBLES;
    if (shmem > 160 * 1024 || nbatch < 1 || nbatch > 65535) return 2;
    ZD_PROBE_RETURN();
    set_dyn_lds<k_refq_cols_oop<P, E, Q, W, CONJ>>(shmem);
    hipLaunchKernelGGL((k_refq_cols_oop<P, E, Q, W, CONJ>), dim3((ncols + W - 1) / W, nbatch), dim3(threads), shmem, st, tw, tw + P,
                       tw + P + P * Q, (const cplx *) in, in_bs, in_ps, (cplx *) out, out_bs, out_ps, ncols);
    ZD_LAUNCH_CHECK();
    return 0;
}
template <int P, int E, int Q, int W>
static int launch_refq_yphi_t(const cplx *tw, void *store, long long pitch, int nplanes, double f_NL, hipStream_t st) {
    constexpr int threads = W * Q * P / E, N = P * Q;
    const size_t shmem = sizeof(double) * zdfft::LineQ<P, E, Q, W, false>::LDS_DOUBLES;
    if (shmem > 160 * 1024 || nplanes < 1 || nplanes > 65535) return 2;
    ZD_PROBE_RETURN();
    set_dyn_lds<k_refq_yphi<P, E, Q, W>>(shmem);
    hipLaunchKernelGGL((k_refq_yphi<P, E, Q, W>), dim3((N + W - 1) / W, nplanes), dim3(threads), shmem, st, tw, tw + P, tw + P + N,
                       (cplx *) store, pitch, f_NL, 1. / N / N / N);
    ZD_LAUNCH_CHECK();
    return 0;
}

template <int P, int E, int Q, int W>
static int launch_refq_cols_t(const cplx *tw, void *data, long long batch_stride, long long point_stride, int ncols, int nbatch,
                              int zero_point, hipStream_t st) {
    constexpr int threads = W * Q * P / E;
    static_assert(threads <= 1024, "workgroup too large");
    const size_t shmem = sizeof(double) * zdfft::LineQ<P, E, Q, W, false>::LDS_DOUBLES;
    if (shmem > 160 * 1024 || nbatch < 1 || nbatch > 65535) return 2;
    ZD_PROBE_RETURN();
    set_dyn_lds<k_refq_cols<P, E, Q, W>>(shmem);
    hipLaunchKernelGGL((k_refq_cols<P, E, Q, W>), dim3((ncols + W - 1) / W, nbatch), dim3(threads), shmem, st, tw, tw + P, tw + P + P * Q,
                       (cplx *) data, batch_stride, point_stride, ncols, zero_point);
    ZD_LAUNCH_CHECK();
    return 0;
}
template <int P, int E, int Q, int W>
static int launch_refq_lines_t(const cplx *tw, void *data, long long pitch, long long nlines, hipStream_t st) {
    constexpr int threads = W * Q * P / E;
    static_assert(threads <= 1024, "workgroup too large");
    const size_t shmem = sizeof(double) * zdfft::LineQ<P, E, Q, W, true>::LDS_DOUBLES;
    if (shmem > 160 * 1024) return 2;
    ZD_PROBE_RETURN();
    set_dyn_lds<k_refq_lines<P, E, Q, W>>(shmem);
    hipLaunchKernelGGL((k_refq_lines<P, E, Q, W>), dim3((unsigned) ((nlines + W - 1) / W)), dim3(threads), shmem, st, tw, tw + P,
                       tw + P + P * Q, (cplx *) data, pitch, nlines);
    ZD_LAUNCH_CHECK();
    return 0;
}

// line lengths P * Q with a transform here (P >= 16: sixteen elements per thread), lines per workgroup W: every PPD of
// zd_kernels_np2.hip's table with its W there, and the z lines of 16 * Q that its stream factors reach
#define REFQ_SIZES(X)                                                                                                          \
    X(16, 3, 16) X(32, 3, 16) X(64, 3, 16) X(128, 3, 16) X(256, 3, 8) X(512, 3, 8) X(1024, 3, 4)                               \
    X(16, 9, 16) X(32, 9, 16) X(64, 9, 16) X(128, 9, 8) X(256, 9, 4) X(512, 9, 2)                                              \
    X(16, 27, 16) X(32, 27, 8) X(64, 27, 8) X(128, 27, 4) X(256, 27, 2)                                                        \
    X(16, 5, 16) X(32, 5, 16) X(64, 5, 16) X(128, 5, 16) X(256, 5, 8) X(512, 5, 4) X(1024, 5, 2)                               \
    X(16, 15, 16) X(32, 15, 16) X(64, 15, 16) X(128, 15, 8) X(256, 15, 4) X(512, 15, 2)                                        \
    X(16, 25, 16) X(32, 25, 16) X(64, 25, 8) X(128, 25, 4) X(256, 25, 2)                                                       \
    X(16, 45, 8) X(32, 45, 8) X(64, 45, 4) X(128, 45, 2)                                                                       \
    X(16, 75, 8) X(32, 75, 4) X(64, 75, 2)                                                                                     \
    X(16, 125, 4) X(32, 125, 4) X(64, 125, 2)                                                                                  \
    X(16, 7, 16) X(32, 7, 16) X(64, 7, 16) X(128, 7, 16) X(256, 7, 8) X(512, 7, 4) X(1024, 7, 2)                               \
    X(16, 21, 16) X(32, 21, 16) X(64, 21, 8) X(128, 21, 4) X(256, 21, 2)                                                       \
    X(16, 35, 16) X(32, 35, 8) X(64, 35, 4) X(128, 35, 2)                                                                      \
    X(16, 49, 16) X(32, 49, 8) X(64, 49, 4) X(128, 49, 2)                                                                      \
    X(16, 135, 4) X(32, 135, 2) X(64, 135, 1)

bool refq_supported_len(int n) {
#define RS(p, q, w) \
    if (n == (p) * (q)) return true;
    REFQ_SIZES(RS)
#undef RS
    return false;
}
int launch_refq_cols(int n, const void *tw, void *data, long long batch_stride, long long point_stride, int ncols, int nbatch, int zero_point,
                     hipStream_t st) {
#define RC(p, q, w)     \
    if (n == (p) * (q)) \
        return launch_refq_cols_t<p, 16, q, w>((const cplx *) tw, data, batch_stride, point_stride, ncols, nbatch, zero_point, st);
    REFQ_SIZES(RC)
#undef RC
    ZD_TABLE_MISS("zeldovich_hip: no composite transform of strided lines of length %d\n", n);
    return 2;
}
int launch_refq_cols_oop(int n, const void *tw, const void *in, long long in_bs, long long in_ps, void *out, long long out_bs, long long out_ps,
                         int ncols, int nbatch, bool conj, hipStream_t st) {
#define RO(p, q, w)                                                                                                                    \
    if (n == (p) * (q))                                                                                                                \
        return conj ? launch_refq_cols_oop_t<p, 16, q, w, true>((const cplx *) tw, in, in_bs, in_ps, out, out_bs, out_ps, ncols, nbatch, st) \
                    : launch_refq_cols_oop_t<p, 16, q, w, false>((const cplx *) tw, in, in_bs, in_ps, out, out_bs, out_ps, ncols, nbatch, st);
    REFQ_SIZES(RO)
#undef RO
    ZD_TABLE_MISS("zeldovich_hip: no composite transform of strided lines of length %d\n", n);
    return 2;
}
int launch_refq_yphi(int n, const void *tw, void *store, long long pitch, int nplanes, double f_NL, hipStream_t st) {
#define RY(p, q, w) \
    if (n == (p) * (q)) return launch_refq_yphi_t<p, 16, q, w>((const cplx *) tw, store, pitch, nplanes, f_NL, st);
    REFQ_SIZES(RY)
#undef RY
    ZD_TABLE_MISS("zeldovich_hip: no composite phi column transform of length %d\n", n);
    return 2;
}
int launch_refq_lines(int n, const void *tw, void *data, long long pitch, long long nlines, hipStream_t st) {
#define RL(p, q, w) \
    if (n == (p) * (q)) return launch_refq_lines_t<p, 16, q, w>((const cplx *) tw, data, pitch, nlines, st);
    REFQ_SIZES(RL)
#undef RL
    ZD_TABLE_MISS("zeldovich_hip: no composite transform of contiguous lines of length %d\n", n);
    return 2;
}

int launch_refq_ycols(int n, const void *tw, const AnyChunks &C, void *data, int ncols, int nbatch, int zero_point, int out_limit,
                      hipStream_t st) {
#define RYC(p, q, w) \
    if (n == (p) * (q) && C.N == n) return launch_refq_ycols_t<p, 16, q, w>((const cplx *) tw, C, data, ncols, nbatch, zero_point, out_limit, st);
    REFQ_SIZES(RYC)
#undef RYC
    ZD_TABLE_MISS("zeldovich_hip: no composite transform of chunked y columns of length %d\n", n);
    return 2;
}
int launch_refq_xphi(int n, const void *tw, void *data, long long pitch, long long nlines, double f_NL, hipStream_t st) {
#define RXP(p, q, w) \
    if (n == (p) * (q)) return launch_refq_xphi_t<p, 16, q, w>((const cplx *) tw, data, pitch, nlines, f_NL, st);
    REFQ_SIZES(RXP)
#undef RXP
    ZD_TABLE_MISS("zeldovich_hip: no composite phi line transform of length %d\n", n);
    return 2;
}
int launch_refq_scatter(const JobList &jobs, const AnyChunks &C, int ky_first, int r0, int nky, int L, const void *Y, void *store, hipStream_t st) {
    if (jobs.n * nky > 65535) return 2;
    hipLaunchKernelGGL(k_refq_scatter, dim3((C.N + 255) / 256, L, jobs.n * nky), dim3(256), 0, st, jobs, C, ky_first, r0, nky, L,
                       (const cplx *) Y, (cplx *) store);
    ZD_LAUNCH_CHECK();
    return 0;
}
int launch_refq_emit(const AnyChunks &C, const EpiConst &ec, const void *store, int plane0, int nplanes, int z_first, int z_step, void *records,
                     float *density, Reduce *red, hipStream_t st) {
    dim3 grid((C.N + 255) / 256, C.N, nplanes), block(256);
    if (C.narray == 1) {
        hipLaunchKernelGGL(k_refq_emit<1>, grid, block, 0, st, C, ec, (const cplx *) store, plane0, z_first, z_step, (char *) records, density, red);
        ZD_LAUNCH_CHECK();
    } else if (C.narray == 2) {
        hipLaunchKernelGGL(k_refq_emit<2>, grid, block, 0, st, C, ec, (const cplx *) store, plane0, z_first, z_step, (char *) records, density, red);
        ZD_LAUNCH_CHECK();
    } else {
        hipLaunchKernelGGL(k_refq_emit<4>, grid, block, 0, st, C, ec, (const cplx *) store, plane0, z_first, z_step, (char *) records, density, red);
        ZD_LAUNCH_CHECK();
    }
    return 0;
}

}  // namespace zd
