// zd_kernels_field.hip — intake of a caller-supplied real field: a[z][y][x] -> PhiK[ky][kz][x], the half-space array every generator
// form reads as D = PhiK * fnl_M (GenConst::phik; fnl_M is a table of ones on such a plan).  gfx950.
//
// Definition (also in include/zeldovich_hip.h and the README).  The caller gives a real field a[z][y][x], N = PPD points per side,
// float32 or float64, on the host or on the device, and says what it is:
//   density  the linear density delta in the run's own units (what ZD_qdensity = 1 delivers):
//              D(k) = (1 / N^3) sum_x a(x) exp(-2 pi i k.x / N)
//   white    unit-variance white noise: D(k) = W(k) sqrt(power(|k|) / N^3), W the unnormalised forward sum and power = zd_pk_power
//            (normalisation and 1 / V included); with <|W|^2> = N^3 this is <|D|^2> = power(k), the variance of a seeded run
// and D(k) is then cleared by the run's zero rule, mode_is_zero (zd_device.h): the |k_i| = kmax planes, k^2 >= k^2_cutoff without
// ZD_CornerModes, ZD_qonemode, and k = 0.  The planes |k_i| = N/2 are cleared as well: the rule does that by itself whenever
// kmax = N/2, and where it does not (ZD_CornerModes with ZD_k_cutoff != 1) PhiK has no row ky = N/2 to keep the modes in, and a real
// field has no gradient on the other two.  So with ZD_qdensity = 1 the density the run delivers is the imposed field with those modes
// removed, and displacements and velocities are what the path makes of these D(k), exactly as if the draws had produced them.
// ZD_Seed is ignored; no draw is made.
//
// Three stages on the radix-16 engine (zd_fft.h).  The engine's transforms have sign +1; the forward transform of a REAL field is the
// conjugate of its sign +1 transform, so the lines run as they are and the last store conjugates.
//   k_field_x  rows of a chunk of planes, float32 or float64, straight from the caller's layout (ROWS rows per workgroup, LineInner):
//              one real row per complex line with a zero imaginary part.  (Two rows per line would halve the x arithmetic, but the
//              untangling pairs element k with N - k, which sit in different threads AND different register slots of the engine's
//              fixed-point distribution t + T e: one more LDS exchange per line, for a stage that is bound by its 16-byte stores.)
//              Output: the workspace [plane of the chunk][y][x], complex.
//   k_field_y  columns of a workspace plane (W columns per workgroup, ColsInner); only the outputs ky < N/2 are stored, as
//              PhiK[ky][z][x] with z still the lattice plane.
//   k_field_z  columns of PhiK along z, in place: a workgroup holds its W lines in registers before it stores any of them.  The store
//              epilogue conjugates, applies the zero rule and multiplies by amp[kx^2 + ky^2 + kz^2]: 1 / N^3 (density) or
//              sqrt(power / N^3) (white), a table by integer |k|^2 as pk_tab is.
// Memory: PhiK (8 N^3 bytes) is the only N^3-sized allocation.  The workspace holds FIELD_WS_PLANES(N) planes (4 at N = 2048; at most
// 256 MB at every size); a host field is uploaded through a staging buffer of as many real planes and never resident as a whole; a
// device field is read where it lies.
#include <hip/hip_runtime.h>

#include "zd_device.h"
#include "zd_fft.h"
#include "zd_launch.h"

using zdfft::cplx;

namespace zd {

template <int N, int E, int ROWS>
__global__ __launch_bounds__(ROWS *N / E) void k_field_x(const void *__restrict__ src, int is_f32, const cplx *__restrict__ tw,
                                                        cplx *__restrict__ work) {
    using PL  = zdfft::Plan<N, E>;
    using LDS = zdfft::LineInner<N, ROWS>;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr int T = PL::T;
    const int t = threadIdx.x % T, row = threadIdx.x / T;
    const long long line = ((long long) blockIdx.y * N + blockIdx.x * ROWS + row) * N;  // (plane of the chunk, y)
    double re[E], im[E];
    if (is_f32) {
        const float *p = (const float *) src + line;
#pragma unroll
        for (int e = 0; e < E; e++) re[e] = (double) p[t + T * e];
    } else {
        const double *p = (const double *) src + line;
#pragma unroll
        for (int e = 0; e < E; e++) re[e] = p[t + T * e];
    }
#pragma unroll
    for (int e = 0; e < E; e++) im[e] = 0.0;
    zdfft::fft_line<PL, LDS>(re, im, t, row, lds, tw);
    int t2 = t;
    asm volatile("" : "+v"(t2));  // keep the address arithmetic behind the transform (register pressure, as in k_xphi)
    cplx *q = work + line;
#pragma unroll
    for (int e = 0; e < E; e++) q[t2 + T * e] = cplx{re[e], im[e]};
}

template <int N, int E, int W>
__global__ __launch_bounds__(W *N / E) void k_field_y(const cplx *__restrict__ tw, const cplx *__restrict__ work, int z0,
                                                     cplx *__restrict__ phik) {
    using PL  = zdfft::Plan<N, E>;
    using LDS = zdfft::ColsInner<N, W>;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr int T = PL::T;
    const int w = threadIdx.x % W, t = threadIdx.x / W;
    const int x = blockIdx.x * W + w, pl = blockIdx.y;
    const cplx *p = work + (long long) pl * N * N + x;
    double re[E], im[E];
#pragma unroll
    for (int e = 0; e < E; e++) {
        const cplx v = p[(long long) (t + T * e) * N];
        re[e] = v.x;
        im[e] = v.y;
    }
    zdfft::fft_line<PL, LDS>(re, im, t, w, lds, tw);
    int t2 = t;
    asm volatile("" : "+v"(t2));
    cplx *q = phik + (long long) (z0 + pl) * N + x;
#pragma unroll
    for (int e = 0; e < E / 2; e++) q[(long long) (t2 + T * e) * N * N] = cplx{re[e], im[e]};  // ky = t + T e < N/2
}

template <int N, int E, int W>
__global__ __launch_bounds__(W *N / E) void k_field_z(GenConst g, const cplx *__restrict__ tw, const double *__restrict__ amp,
                                                     cplx *__restrict__ phik) {
    using PL  = zdfft::Plan<N, E>;
    using LDS = zdfft::ColsInner<N, W>;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr int T = PL::T, half = N / 2;
    const int w = threadIdx.x % W, t = threadIdx.x / W;
    const int x = blockIdx.x * W + w, ky = blockIdx.y;
    cplx *p = phik + (long long) ky * N * N + x;
    double re[E], im[E];
#pragma unroll
    for (int e = 0; e < E; e++) {
        const cplx v = p[(long long) (t + T * e) * N];
        re[e] = v.x;
        im[e] = v.y;
    }
    zdfft::fft_line<PL, LDS>(re, im, t, w, lds, tw);  // (every line of the workgroup is in registers from here on)
    int t2 = t;
    asm volatile("" : "+v"(t2));
    const int kx = x > half ? x - N : x;
    const bool col_dead = x == half || ky == half;  // (ky < N/2 by the grid)
    const int kxy2 = kx * kx + ky * ky;
#pragma unroll
    for (int e = 0; e < E; e++) {
        const int z = t2 + T * e, kz = z > half ? z - N : z;
        const int k2i = kxy2 + kz * kz;
        double a = 0.0;
        if (!col_dead && z != half && k2i != 0 && !mode_is_zero(g, kx, ky, kz, (double) k2i * g.fundamental2)) a = amp[k2i];
        p[(long long) z * N] = cplx{re[e] * a, -im[e] * a};
    }
}

template <int N, int E, int ROWS>
static int launch_field_x_t(const void *src, int is_f32, const void *tw, void *work, int nplanes, hipStream_t st) {
    ZD_PROBE_RETURN();
    const size_t shmem = sizeof(double) * zdfft::LineInner<N, ROWS>::SIZE;
    set_dyn_lds<k_field_x<N, E, ROWS>>(shmem);
    hipLaunchKernelGGL((k_field_x<N, E, ROWS>), dim3(N / ROWS, nplanes), dim3(ROWS * N / E), shmem, st, src, is_f32, (const cplx *) tw,
                       (cplx *) work);
    ZD_LAUNCH_CHECK();
    return 0;
}
template <int N, int E, int W>
static int launch_field_y_t(const void *tw, const void *work, int z0, int nplanes, void *phik, hipStream_t st) {
    ZD_PROBE_RETURN();
    const size_t shmem = sizeof(double) * zdfft::ColsInner<N, W>::SIZE;
    set_dyn_lds<k_field_y<N, E, W>>(shmem);
    hipLaunchKernelGGL((k_field_y<N, E, W>), dim3(N / W, nplanes), dim3(W * N / E), shmem, st, (const cplx *) tw, (const cplx *) work, z0,
                       (cplx *) phik);
    ZD_LAUNCH_CHECK();
    return 0;
}
template <int N, int E, int W>
static int launch_field_z_t(const GenConst &g, const void *tw, const double *amp, void *phik, hipStream_t st) {
    ZD_PROBE_RETURN();
    const size_t shmem = sizeof(double) * zdfft::ColsInner<N, W>::SIZE;
    set_dyn_lds<k_field_z<N, E, W>>(shmem);
    hipLaunchKernelGGL((k_field_z<N, E, W>), dim3(N / W, N / 2), dim3(W * N / E), shmem, st, g, (const cplx *) tw, amp, (cplx *) phik);
    ZD_LAUNCH_CHECK();
    return 0;
}

// the tile shapes of the f_NL round's forward stages (launch_fnl_stage): rows per x workgroup, columns per y / z workgroup
#define FIELD_SIZES(X) X(32, 16, 32, 32) X(64, 16, 32, 32) X(128, 16, 32, 32) X(256, 16, 16, 16) X(512, 16, 16, 8) X(1024, 16, 8, 4) X(2048, 16, 8, 2)

// rows of the planes [0, nplanes) of src (real, float32 or float64, [plane][y][x]) -> work[plane][y][x]
int launch_field_x(int N, const void *src, int is_f32, const void *tw, void *work, int nplanes, hipStream_t st) {
#define FCASE(n, e, w, rows) \
    case n: return launch_field_x_t<n, e, rows>(src, is_f32, tw, work, nplanes, st);
    switch (N) { FIELD_SIZES(FCASE) }
#undef FCASE
    ZD_TABLE_MISS("zeldovich_hip: ZD_Field: the intake has x lines for PPD = 32 ... 2048 (powers of two), got %d\n", N);
    return 2;
}
// columns of the workspace planes [0, nplanes) -> PhiK[ky < N/2][z0 + plane][x]
int launch_field_y(int N, const void *tw, const void *work, int z0, int nplanes, void *phik, hipStream_t st) {
#define FCASE(n, e, w, rows) \
    case n: return launch_field_y_t<n, e, w>(tw, work, z0, nplanes, phik, st);
    switch (N) { FIELD_SIZES(FCASE) }
#undef FCASE
    ZD_TABLE_MISS("zeldovich_hip: ZD_Field: the intake has y lines for PPD = 32 ... 2048 (powers of two), got %d\n", N);
    return 2;
}
// z lines of PhiK in place; the zero rule of g (N, half, kmax, corner_modes, k2_cutoff, fundamental2, qonemode, one_mode) and
// amp[|k|^2] in the store epilogue
int launch_field_z(const GenConst &g, const void *tw, const double *amp, void *phik, hipStream_t st) {
#define FCASE(n, e, w, rows) \
    case n: return launch_field_z_t<n, e, w>(g, tw, amp, phik, st);
    switch (g.N) { FIELD_SIZES(FCASE) }
#undef FCASE
    ZD_TABLE_MISS("zeldovich_hip: ZD_Field: the intake has z lines for PPD = 32 ... 2048 (powers of two), got %d\n", g.N);
    return 2;
}

}  // namespace zd
