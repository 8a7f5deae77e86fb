// zd_kernels_field_adj.hip — adjoint of a run on a caller-supplied field (zd_kernels_field.hip): the gradient of a scalar loss with
// respect to the field a, from its gradients with respect to the displacements, the velocities and the delivered density.  gfx950.
//
// Definition (also in include/zeldovich_hip.h and the README).  All arrays are [z][y][x]; components in the order of the records'
// d / v members, (q_z, q_y, q_x); fftn is the forward sum (exp(-i)), N = PPD.  The forward map of a field run is linear in a:
//   D(k)  = alive(k) A(|k|^2) fftn(a)(k)     A = 1 / N^3 (density) or sqrt(power(|k|) / N^3) (white): the intake's amp table
//   q_j   = N^3 ifftn(i s_j D).real          v_j = N^3 ifftn(i f s_j D).real          delivered density = N^3 ifftn(D).real
// alive is the intake's zero rule (mode_is_zero and the |k_i| = N/2 planes, asked on the half space the path reads and mirrored), and
// s_j(k), f(k) are the generator's per-mode coefficients (zd_kernels.hip k_gen):
//   ZA   s_j = k_j fundamental / k^2,                f = (sqrt(1 + 24 f_cluster) - 1) / 4
//   PLT  s_j = rescale e_j fundamental / k^2,        f = (sqrt(1 + 24 e_3 f_cluster) - 1) / 4, the eigenmode of a winner mode (ky > 0;
//        on ky = 0: kz > 0; on ky = kz = 0: kx > 0) from its own lookup, the mirrored half from s(-k) = -s(k), f(-k) = f(k)
// The adjoint takes three real cotangents, each optional (absent = an exact zero): g_q[z][y][x][3], g_v[z][y][x][3], g_dens[z][y][x],
//   H(k)  = alive(k) A(|k|^2) [ sum_j conj(i s_j(k)) ( fftn(g_q,j)(k) + f(k) fftn(g_v,j)(k) ) + fftn(g_dens)(k) ]
//   abar  = N^3 ifftn(H).real                                                                     float64 [z][y][x]
// so that <q, g_q> + <v, g_v> + <dens, g_dens> = <a, abar> for every a.  ZD_Seed, ICFormat, ZD_qdensity, ZD_qoneslab, the stream
// factor and the store mode do not enter: this is the adjoint of the exact float64 map.
//
// Stages, on the radix-16 engine (zd_fft.h; sign +1, so the forward transform of a real array is the conjugate of the engine's):
//   forward, one pass per real component array c (ZA: three passes of g_q,j + f g_v,j, f being one number; PLT: three of g_q,j and
//   three of g_v,j; one more for g_dens):
//     k_fadj_x   rows of a chunk of planes: a lane reads its elements' component out of the row's 3 N contiguous values (one wave load
//                covers one contiguous run of the row; every line of the row is fetched once per pass), float32 or float64, forms
//                fa a + fb b on load, one real row per complex line -> work[plane of the chunk][y][x]
//     k_field_y  (the intake's) columns of the workspace; ky < N/2 only -> T[ky][z][x]
//     k_fadj_z   z lines of T; the store epilogue conjugates, evaluates alive, A, s_j (and f) of its mode — mode_is_zero, eig_axis /
//                get_eigenmode_dev with the generator's cj treatment of the plane ky = 0 — and adds conj(i s_j) ... into H[ky][kz][x]:
//                the first pass writes, the later ones read, add and write.  One thread owns an element: no atomics, and two calls
//                return the same bits.
//   inverse: abar = Re sum over the stored rows with weight 1 on ky = 0 and 2 on 0 < ky < N/2, the rows ky >= N/2 taken as zeros (ky =
//   N/2 is dead).  The plane ky = 0 of H is Hermitian in (kx, kz) by construction — the cotangents are real, alive and A are even, s is
//   odd and f even under the mirror — so its sum is real as it stands; tests/test_gpu_field_adj.py holds that.
//     k_fadj_iz  z lines of H in place; the store multiplies by the row's weight
//     k_fadj_iy  columns of a chunk of planes: N/2 inputs, the upper half zeros -> work[plane of the chunk][y][x]
//     k_fadj_ix  rows of the workspace; the real part -> abar[z][y][x], float64
// Memory: H and T, 8 N^3 bytes each — T is dead before the inverse writes the result, which is as large: a result on the device lends
// its storage to T; the workspace of the intake (FIELD_WS_PLANES(N) planes); host cotangents and a host result go through staging
// buffers of as many planes.
#include <hip/hip_runtime.h>

#include "zd_device.h"
#include "zd_fft.h"
#include "zd_genmath.h"
#include "zd_launch.h"

using zdfft::cplx;

namespace zd {

using zdgen::eig_axis;
using zdgen::eig_index_x;
using zdgen::eig_index_z;
using zdgen::EigAxis;
using zdgen::get_eigenmode_dev;

// component `comp` of `nc` interleaved ones, fa a + fb b (b may be NULL)
template <int N, int E, int ROWS>
__global__ __launch_bounds__(ROWS *N / E) void k_fadj_x(const void *__restrict__ a, const void *__restrict__ b, double fa, double fb, int is_f32,
                                                       int nc, int comp, const cplx *__restrict__ tw, cplx *__restrict__ work) {
    using PL  = zdfft::Plan<N, E>;
    using LDS = zdfft::LineInner<N, ROWS>;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr int T = PL::T;
    const int t = threadIdx.x % T, row = threadIdx.x / T;
    const long long line = ((long long) blockIdx.y * N + blockIdx.x * ROWS + row) * N;  // (plane of the chunk, y)
    const long long src  = line * nc + comp;
    double re[E], im[E];
    if (is_f32) {
        const float *p = (const float *) a + src, *q = (const float *) b + src;
#pragma unroll
        for (int e = 0; e < E; e++) re[e] = fa * (double) p[(long long) (t + T * e) * nc] + (b ? fb * (double) q[(long long) (t + T * e) * nc] : 0.0);
    } else {
        const double *p = (const double *) a + src, *q = (const double *) b + src;
#pragma unroll
        for (int e = 0; e < E; e++) re[e] = fa * p[(long long) (t + T * e) * nc] + (b ? fb * q[(long long) (t + T * e) * nc] : 0.0);
    }
#pragma unroll
    for (int e = 0; e < E; e++) im[e] = 0.0;
    zdfft::fft_line<PL, LDS>(re, im, t, row, lds, tw);
    int t2 = t;
    asm volatile("" : "+v"(t2));  // keep the address arithmetic behind the transform (register pressure, as in k_field_x)
    cplx *o = work + line;
#pragma unroll
    for (int e = 0; e < E; e++) o[t2 + T * e] = cplx{re[e], im[e]};
}

// coef: 0 = conj(i s_comp), 1 = f conj(i s_comp) (PLT velocities), 2 = 1 (density)
template <int N, int E, int W, bool PLT>
__global__ __launch_bounds__(W *N / E) void k_fadj_z(GenConst g, const cplx *__restrict__ tw, const double *__restrict__ amp,
                                                    const cplx *__restrict__ T_, cplx *__restrict__ H, int comp, int coef, int first) {
    using PL  = zdfft::Plan<N, E>;
    using LDS = zdfft::ColsInner<N, W>;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr int T = PL::T, half = N / 2;
    const int w = threadIdx.x % W, t = threadIdx.x / W;
    const int x = blockIdx.x * W + w, ky = blockIdx.y;
    const long long col = (long long) ky * N * N + x;
    const cplx *p = T_ + col;
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
    cplx *h = H + col;
    const int kx = x > half ? x - N : x;
    const bool col_dead = x == half;  // (ky < N/2 by the grid)
    EigAxis eax = {0, 0, 0.0}, eay = {0, 0, 0.0};
    if constexpr (PLT) {
        eax = eig_axis(g, eig_index_x(g, kx));
        eay = eig_axis(g, ky);
    }
#pragma unroll
    for (int e = 0; e < E; e++) {
        const int z = t2 + T * e, kz = z > half ? z - N : z;
        // the mode the generator reads for this position: on the plane ky = 0 the losers are the conjugated copies of their mirror images
        const bool cj = ky == 0 && (kz < 0 || (kz == 0 && kx < 0));
        const int kxm = cj ? -kx : kx, kzm = cj ? -kz : kz;
        const int k2i = kxm * kxm + ky * ky + kzm * kzm;
        const double k2v = (double) k2i * g.fundamental2;
        const bool alive = !col_dead && z != half && k2i != 0 && !mode_is_zero(g, kxm, ky, kzm, k2v);
        double cr = 0.0, ci = 0.0;  // this pass's term of H: coefficient x conj(line)
        if (alive) {
            const double a = amp[k2i], gr = re[e], gi = -im[e];
            if (coef == 2) {
                cr = a * gr;
                ci = a * gi;
            } else {
                const double ik2 = 1.0 / k2v;
                double s;
                if constexpr (PLT) {
                    double ev[4];
                    const EigAxis eaz = eig_axis(g, eig_index_z(g, kzm));
                    if (cj)  // mirrored source mode (ky = 0 plane only): its own x axis
                        get_eigenmode_dev(g, kxm, ky, kzm, eig_axis(g, eig_index_x(g, kxm)), eay, eaz, ev);
                    else
                        get_eigenmode_dev(g, kxm, ky, kzm, eax, eay, eaz, ev);
                    const double f = (sqrt(1. + 24 * ev[3] * g.f_cluster) - 1) * .25;
                    double rescale = 1.0;
                    if (g.qPLTrescale) rescale = exp(g.ln_growth_ratio * (g.target_f - f));
                    s = rescale * (comp == 0 ? ev[2] : comp == 1 ? ev[1] : ev[0]) * g.fundamental * ik2;
                    if (coef == 1) s *= f;
                } else {
                    s = (double) (comp == 0 ? kzm : comp == 1 ? ky : kxm) * g.fundamental * ik2;
                }
                if (cj) s = -s;  // conjugated copy of the mode at -k: s -> -s(-k)
                s *= a;
                cr = s * gi;   // conj(i s) (gr + i gi) = s gi - i s gr
                ci = -s * gr;
            }
        }
        cplx *o = h + (long long) z * N;
        if (first) {
            *o = cplx{cr, ci};
        } else if (alive) {
            const cplx v = *o;
            *o = cplx{v.x + cr, v.y + ci};
        }
    }
}

template <int N, int E, int W>
__global__ __launch_bounds__(W *N / E) void k_fadj_iz(const cplx *__restrict__ tw, cplx *__restrict__ H) {
    using PL  = zdfft::Plan<N, E>;
    using LDS = zdfft::ColsInner<N, W>;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr int T = PL::T;
    const int w = threadIdx.x % W, t = threadIdx.x / W;
    const int x = blockIdx.x * W + w, ky = blockIdx.y;
    cplx *p = H + (long long) ky * N * N + x;
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
    const double wgt = ky ? 2.0 : 1.0;  // a row 0 < ky < N/2 stands for itself and its Hermitian twin
#pragma unroll
    for (int e = 0; e < E; e++) p[(long long) (t2 + T * e) * N] = cplx{re[e] * wgt, im[e] * wgt};
}

template <int N, int E, int W>
__global__ __launch_bounds__(W *N / E) void k_fadj_iy(const cplx *__restrict__ tw, const cplx *__restrict__ H, int z0, cplx *__restrict__ work) {
    using PL  = zdfft::Plan<N, E>;
    using LDS = zdfft::ColsInner<N, W>;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr int T = PL::T;
    const int w = threadIdx.x % W, t = threadIdx.x / W;
    const int x = blockIdx.x * W + w, pl = blockIdx.y;
    const cplx *p = H + (long long) (z0 + pl) * N + x;
    double re[E], im[E];
#pragma unroll
    for (int e = 0; e < E; e++) {
        if (e < E / 2) {  // ky = t + T e < N/2
            const cplx v = p[(long long) (t + T * e) * N * N];
            re[e] = v.x;
            im[e] = v.y;
        } else {
            re[e] = im[e] = 0.0;
        }
    }
    zdfft::fft_line<PL, LDS>(re, im, t, w, lds, tw);
    int t2 = t;
    asm volatile("" : "+v"(t2));
    cplx *q = work + (long long) pl * N * N + x;
#pragma unroll
    for (int e = 0; e < E; e++) q[(long long) (t2 + T * e) * N] = cplx{re[e], im[e]};
}

template <int N, int E, int ROWS>
__global__ __launch_bounds__(ROWS *N / E) void k_fadj_ix(const cplx *__restrict__ tw, const cplx *__restrict__ work, double *__restrict__ out) {
    using PL  = zdfft::Plan<N, E>;
    using LDS = zdfft::LineInner<N, ROWS>;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr int T = PL::T;
    const int t = threadIdx.x % T, row = threadIdx.x / T;
    const long long line = ((long long) blockIdx.y * N + blockIdx.x * ROWS + row) * N;  // (plane of the chunk, y)
    const cplx *p = work + line;
    double re[E], im[E];
#pragma unroll
    for (int e = 0; e < E; e++) {
        const cplx v = p[t + T * e];
        re[e] = v.x;
        im[e] = v.y;
    }
    zdfft::fft_line<PL, LDS>(re, im, t, row, lds, tw);
    int t2 = t;
    asm volatile("" : "+v"(t2));
    double *q = out + line;
#pragma unroll
    for (int e = 0; e < E; e++) q[t2 + T * e] = re[e];
}

template <int N, int E, int ROWS>
static int launch_fadj_x_t(const void *a, const void *b, double fa, double fb, int is_f32, int nc, int comp, const void *tw, void *work, int nplanes,
                           hipStream_t st) {
    ZD_PROBE_RETURN();
    const size_t shmem = sizeof(double) * zdfft::LineInner<N, ROWS>::SIZE;
    set_dyn_lds<k_fadj_x<N, E, ROWS>>(shmem);
    hipLaunchKernelGGL((k_fadj_x<N, E, ROWS>), dim3(N / ROWS, nplanes), dim3(ROWS * N / E), shmem, st, a, b, fa, fb, is_f32, nc, comp,
                       (const cplx *) tw, (cplx *) work);
    ZD_LAUNCH_CHECK();
    return 0;
}
template <int N, int E, int W, bool PLT>
static int launch_fadj_z_t(const GenConst &g, const void *tw, const double *amp, const void *T, void *H, int comp, int coef, int first,
                           hipStream_t st) {
    ZD_PROBE_RETURN();
    const size_t shmem = sizeof(double) * zdfft::ColsInner<N, W>::SIZE;
    set_dyn_lds<k_fadj_z<N, E, W, PLT>>(shmem);
    hipLaunchKernelGGL((k_fadj_z<N, E, W, PLT>), dim3(N / W, N / 2), dim3(W * N / E), shmem, st, g, (const cplx *) tw, amp, (const cplx *) T,
                       (cplx *) H, comp, coef, first);
    ZD_LAUNCH_CHECK();
    return 0;
}
template <int N, int E, int W>
static int launch_fadj_iz_t(const void *tw, void *H, hipStream_t st) {
    ZD_PROBE_RETURN();
    const size_t shmem = sizeof(double) * zdfft::ColsInner<N, W>::SIZE;
    set_dyn_lds<k_fadj_iz<N, E, W>>(shmem);
    hipLaunchKernelGGL((k_fadj_iz<N, E, W>), dim3(N / W, N / 2), dim3(W * N / E), shmem, st, (const cplx *) tw, (cplx *) H);
    ZD_LAUNCH_CHECK();
    return 0;
}
template <int N, int E, int W>
static int launch_fadj_iy_t(const void *tw, const void *H, int z0, int nplanes, void *work, hipStream_t st) {
    ZD_PROBE_RETURN();
    const size_t shmem = sizeof(double) * zdfft::ColsInner<N, W>::SIZE;
    set_dyn_lds<k_fadj_iy<N, E, W>>(shmem);
    hipLaunchKernelGGL((k_fadj_iy<N, E, W>), dim3(N / W, nplanes), dim3(W * N / E), shmem, st, (const cplx *) tw, (const cplx *) H, z0,
                       (cplx *) work);
    ZD_LAUNCH_CHECK();
    return 0;
}
template <int N, int E, int ROWS>
static int launch_fadj_ix_t(const void *tw, const void *work, double *out, int nplanes, hipStream_t st) {
    ZD_PROBE_RETURN();
    const size_t shmem = sizeof(double) * zdfft::LineInner<N, ROWS>::SIZE;
    set_dyn_lds<k_fadj_ix<N, E, ROWS>>(shmem);
    hipLaunchKernelGGL((k_fadj_ix<N, E, ROWS>), dim3(N / ROWS, nplanes), dim3(ROWS * N / E), shmem, st, (const cplx *) tw, (const cplx *) work, out);
    ZD_LAUNCH_CHECK();
    return 0;
}

// the intake's tile shapes (FIELD_SIZES of zd_kernels_field.hip): rows per x workgroup, columns per y / z workgroup
#define FADJ_SIZES(X) X(32, 16, 32, 32) X(64, 16, 32, 32) X(128, 16, 32, 32) X(256, 16, 16, 16) X(512, 16, 16, 8) X(1024, 16, 8, 4) X(2048, 16, 8, 2)

// rows of the planes [0, nplanes) of the cotangents a, b (b may be NULL; real, float32 or float64, [plane][y][x][nc]), component comp:
// fa a + fb b -> work[plane][y][x]
int launch_field_adj_x(int N, const void *a, const void *b, double fa, double fb, int is_f32, int nc, int comp, const void *tw, void *work,
                       int nplanes, hipStream_t st) {
#define FCASE(n, e, w, rows) \
    case n: return launch_fadj_x_t<n, e, rows>(a, b, fa, fb, is_f32, nc, comp, tw, work, nplanes, st);
    switch (N) { FADJ_SIZES(FCASE) }
#undef FCASE
    ZD_TABLE_MISS("zeldovich_hip: ZD_Field: the adjoint has x lines for PPD = 32 ... 2048 (powers of two), got %d\n", N);
    return 2;
}
// z lines of T[ky][z][x]; this pass's term into H[ky][kz][x] (first: written; otherwise added).  g: the zero rule and, with g.qPLT, the
// eigenmode table and the growth constants; amp as for launch_field_z
int launch_field_adj_z(const GenConst &g, const void *tw, const double *amp, const void *T, void *H, int comp, int coef, int first, hipStream_t st) {
#define FCASE(n, e, w, rows)                                                                              \
    case n:                                                                                               \
        return g.qPLT ? launch_fadj_z_t<n, e, w, true>(g, tw, amp, T, H, comp, coef, first, st)           \
                      : launch_fadj_z_t<n, e, w, false>(g, tw, amp, T, H, comp, coef, first, st);
    switch (g.N) { FADJ_SIZES(FCASE) }
#undef FCASE
    ZD_TABLE_MISS("zeldovich_hip: ZD_Field: the adjoint has z lines for PPD = 32 ... 2048 (powers of two), got %d\n", g.N);
    return 2;
}
// inverse: z lines of H in place, weighted by row
int launch_field_adj_iz(int N, const void *tw, void *H, hipStream_t st) {
#define FCASE(n, e, w, rows) \
    case n: return launch_fadj_iz_t<n, e, w>(tw, H, st);
    switch (N) { FADJ_SIZES(FCASE) }
#undef FCASE
    ZD_TABLE_MISS("zeldovich_hip: ZD_Field: the adjoint has z lines for PPD = 32 ... 2048 (powers of two), got %d\n", N);
    return 2;
}
// inverse: columns of the planes [z0, z0 + nplanes) of H (rows ky < N/2; the rest zeros) -> work[plane][y][x]
int launch_field_adj_iy(int N, const void *tw, const void *H, int z0, int nplanes, void *work, hipStream_t st) {
#define FCASE(n, e, w, rows) \
    case n: return launch_fadj_iy_t<n, e, w>(tw, H, z0, nplanes, work, st);
    switch (N) { FADJ_SIZES(FCASE) }
#undef FCASE
    ZD_TABLE_MISS("zeldovich_hip: ZD_Field: the adjoint has y lines for PPD = 32 ... 2048 (powers of two), got %d\n", N);
    return 2;
}
// inverse: rows of the workspace planes [0, nplanes); the real part -> out[plane][y][x]
int launch_field_adj_ix(int N, const void *tw, const void *work, double *out, int nplanes, hipStream_t st) {
#define FCASE(n, e, w, rows) \
    case n: return launch_fadj_ix_t<n, e, rows>(tw, work, out, nplanes, st);
    switch (N) { FADJ_SIZES(FCASE) }
#undef FCASE
    ZD_TABLE_MISS("zeldovich_hip: ZD_Field: the adjoint has x lines for PPD = 32 ... 2048 (powers of two), got %d\n", N);
    return 2;
}

}  // namespace zd
