// zd_kernels_lpt2q.hip — the de-aliased second-order round (ZD_2LPT_dealias, step 2' of the definition in zd_kernels_lpt2.hip): the
// source on the lattice of M = 3 N / 2 points per side, M = P * 3 with P a power of two, on the composite line transforms of
// zd_fft_q.h.  The generator (k_gen_lpt2<2> at lattice M), the z lines, the scatter and the y columns are those of the
// reference-array family (zd_kernels_lpt2.hip, zd_kernels_any.hip, zd_kernels_np2_ref.hip); what the round needs beside them:
//     k_xlpt2q      k_xlpt2's contract on the x lines of the one-array store [z][y][x]: inverse transform in registers, the pass's term
//                   of the source into the real M^3 accumulator; on pass 4, S / M^3 through the x transform, in place
//     k_lpt2q_zsrc  the last z lines: the columns |kx| < N/2, 0 <= ky < N/2 of the store, truncated to |kz| < N/2, conjugated, into
//                   S(k)[ky][kz][x] of the N layout that the final pass reads
// A forward transform of a real field is the conjugate of its inverse transform: pass 4 of k_xlpt2q, the y columns (k_refq_cols) and
// k_lpt2q_zsrc are three inverse transforms, and the conjugation happens once, where S(k) is written.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "zd_device.h"
#include "zd_fft_q.h"
#include "zd_launch.h"

using namespace zd;
using zdfft::cplx;

// line l (= z M + y) at data[l * pitch], l < nlines, in gradient pass `pass`: inverse x transform; the line now holds A(x) + i B(x) of
// the pass's two gradient fields.  acc[l M + x] = A B (pass 1), += A B (pass 2), -= A^2 + B^2 (passes 3, 4).  Pass 4 goes on: the line
// takes S(x) / M^3 — from the output order (t + T e) + P n2 to the input order Q (t + T e) + n2 through the LDS, real parts only, as
// k_refq_xphi does — and is transformed again, in place.     grid: ceil(nlines / W)   block: W * Q * P / E
template <int P, int E, int Q, int W>
__global__ __launch_bounds__(W *Q *P / E) void k_xlpt2q(const cplx *__restrict__ twP, const cplx *__restrict__ twN, const cplx *__restrict__ twQ,
                                                      cplx *__restrict__ data, long long pitch, long long nlines, int pass, double inv_m3,
                                                      double *__restrict__ acc) {
    using LQ = zdfft::LineQ<P, E, Q, W, true>;
    extern __shared__ __attribute__((aligned(16))) double lds[];  // max(LQ::LDS_DOUBLES, W M) doubles
    constexpr int T = LQ::T, M = P * Q;
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
    double *a = acc + (on ? line : 0) * M;
#pragma unroll
    for (int e = 0; e < E; e++) {
        const int xx = (t + T * e) + P * n2;
        double s = (pass == 1 || !on) ? 0.0 : a[xx];
        s = pass <= 2 ? fma(re[e], im[e], s) : s - fma(re[e], re[e], im[e] * im[e]);
        if (pass < 4) {
            if (on) a[xx] = s;
        } else {
            lds[w * M + xx] = s * inv_m3;
        }
    }
    if (pass < 4) return;  // (uniform over the launch)
    __syncthreads();
#pragma unroll
    for (int e = 0; e < E; e++) {
        re[e] = lds[w * M + Q * (t + T * e) + n2];
        im[e] = 0.0;
    }
    __syncthreads();
    LQ::run(re, im, t, w, n2, lds, twP, twN, twQ);
    if (!on) return;
#pragma unroll
    for (int e = 0; e < E; e++) base[(t + T * e) + P * n2] = cplx{re[e], im[e]};
}

// z line (ky, x) of the store [z][y][x] on the M lattice, for the columns of the N layout: x < N/2 is kx = x at store column x,
// x > N/2 is kx = x - N at store column x + M - N, x = N/2 (the Nyquist plane of N) reads zeros.  Output kz of the transform goes,
// conjugated, to sk[(ky N + kz') N + x] with kz' = kz for kz < N/2 and kz - (M - N) for kz > M - N/2; kz' = N/2 takes zeros (the final
// pass never reads that plane alive, but what it reads must be finite); the outputs between are the de-aliasing's discard.
//   grid: (N / W, N / 2)   block: W * Q * P / E
template <int P, int E, int Q, int W>
__global__ __launch_bounds__(W *Q *P / E) void k_lpt2q_zsrc(const cplx *__restrict__ twP, const cplx *__restrict__ twN, const cplx *__restrict__ twQ,
                                                          const cplx *__restrict__ store, long long pitch, int N, cplx *__restrict__ sk) {
    using LQ = zdfft::LineQ<P, E, Q, W, false>;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr int T = LQ::T, M = P * Q;
    const int c = threadIdx.x % (W * Q), t = threadIdx.x / (W * Q);
    const int w = c % W, n2 = c / W;
    const int x = blockIdx.x * W + w, ky = blockIdx.y, H = N / 2;
    const bool on = x < N, live = on && x != H;
    const int xs = x < H ? x : x + (M - N);
    const cplx *src = store + (long long) ky * pitch + (live ? xs : 0);
    const long long plane = (long long) M * pitch;
    double re[E], im[E];
#pragma unroll
    for (int e = 0; e < E; e++) {
        cplx v = cplx{0.0, 0.0};
        if (live) v = src[(long long) (Q * (t + T * e) + n2) * plane];
        re[e] = v.x;
        im[e] = v.y;
    }
    LQ::run(re, im, t, w, n2, lds, twP, twN, twQ);
    if (!on) return;
    cplx *dst = sk + (long long) ky * N * N + x;
#pragma unroll
    for (int e = 0; e < E; e++) {
        const int k = (t + T * e) + P * n2;
        if (k < H) dst[(long long) k * N] = cplx{re[e], -im[e]};
        else if (k == H) dst[(long long) k * N] = cplx{0.0, 0.0};
        else if (k > M - H) dst[(long long) (k - (M - N)) * N] = cplx{re[e], -im[e]};
    }
}

namespace zd {

template <int P, int E, int Q, int W>
static int launch_lpt2q_xsrc_t(const cplx *tw, int pass, void *data, long long pitch, long long nlines, double *acc, hipStream_t st) {
    constexpr int threads = W * Q * P / E, M = P * Q;
    static_assert(threads <= 1024, "workgroup too large");
    constexpr size_t ld = zdfft::LineQ<P, E, Q, W, true>::LDS_DOUBLES;
    const size_t shmem = sizeof(double) * (ld > (size_t) W * M ? ld : (size_t) W * M);
    if (shmem > 160 * 1024 || pitch < M) return 2;
    ZD_PROBE_RETURN();
    set_dyn_lds<k_xlpt2q<P, E, Q, W>>(shmem);
    hipLaunchKernelGGL((k_xlpt2q<P, E, Q, W>), dim3((unsigned) ((nlines + W - 1) / W)), dim3(threads), shmem, st, tw, tw + P, tw + P + M,
                       (cplx *) data, pitch, nlines, pass, 1. / M / M / M, acc);
    ZD_LAUNCH_CHECK();
    return 0;
}
template <int P, int E, int Q, int W>
static int launch_lpt2q_zsrc_t(const cplx *tw, int N, const void *store, long long pitch, void *sk, hipStream_t st) {
    constexpr int threads = W * Q * P / E, M = P * Q;
    const size_t shmem = sizeof(double) * zdfft::LineQ<P, E, Q, W, false>::LDS_DOUBLES;
    if (shmem > 160 * 1024 || 2 * M != 3 * N || N % W || pitch < M) return 2;
    ZD_PROBE_RETURN();
    set_dyn_lds<k_lpt2q_zsrc<P, E, Q, W>>(shmem);
    hipLaunchKernelGGL((k_lpt2q_zsrc<P, E, Q, W>), dim3(N / W, N / 2), dim3(threads), shmem, st, tw, tw + P, tw + P + M, (const cplx *) store, pitch,
                       N, (cplx *) sk);
    ZD_LAUNCH_CHECK();
    return 0;
}

// the lattices M = 3 N / 2 of PPD = 32 .. 1024: (P, Q, lines per workgroup of the x kernel, of the z kernel).  The z kernel keeps the
// widths of REFQ_SIZES (zd_kernels_np2_ref.hip): its W neighbouring columns are what coalesces.  An x line is contiguous whatever W is,
// and at P = 512 eight lines are 768 threads, which caps a thread at 168 registers (404 bytes of scratch per lane); four lines are 384
// threads with the whole register file and half the LDS, so two workgroups share a CU.  PPD = 2048 (M = 3072) does not fit one GPU
// (zd_capi_sizing.cpp lpt2_round_bytes).
#define LPT2Q_SIZES(X) X(16, 3, 16, 16) X(32, 3, 16, 16) X(64, 3, 16, 16) X(128, 3, 16, 16) X(256, 3, 8, 8) X(512, 3, 4, 8)

int launch_lpt2q_xsrc(int m, const void *tw, int pass, void *data, long long pitch, long long nlines, double *acc, hipStream_t st) {
    if (pass < 1 || pass > 4) return 2;
#define XCASE(p, q, w, wz) \
    if (m == (p) * (q)) return launch_lpt2q_xsrc_t<p, 16, q, w>((const cplx *) tw, pass, data, pitch, nlines, acc, st);
    LPT2Q_SIZES(XCASE)
#undef XCASE
    ZD_TABLE_MISS("zeldovich_hip: the de-aliased second-order round has x lines of 48 .. 1536 points (PPD = 32 .. 1024), got %d\n", m);
    return 2;
}
int launch_lpt2q_zsrc(int m, int n, const void *tw, const void *store, long long pitch, void *sk, hipStream_t st) {
#define ZCASE(p, q, wx, w) \
    if (m == (p) * (q)) return launch_lpt2q_zsrc_t<p, 16, q, w>((const cplx *) tw, n, store, pitch, sk, st);
    LPT2Q_SIZES(ZCASE)
#undef ZCASE
    ZD_TABLE_MISS("zeldovich_hip: the de-aliased second-order round has z lines of 48 .. 1536 points (PPD = 32 .. 1024), got %d\n", m);
    return 2;
}

}  // namespace zd
