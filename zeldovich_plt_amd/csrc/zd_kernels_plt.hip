// zd_kernels_plt.hip — the PLT eigenmode table computed on the GPU (zd_make_eigenmodes, include/zeldovich_hip.h): the table a
// ZD_qPLT run reads (src/zeldovich.cpp:149-276 and :794-830 only READ it; the program that made the reference's `eigmodes128` is not
// part of its sources).  This definition is the contract.
//
// DEFINITION
//   Layout.  float64 [n][n][n/2 + 1][4] = (e_x, e_y, e_z, lambda), indexed [ikx][iky][ikz].  Signed integer wavenumber m = i for
//          i <= n/2 (index n/2 is +n/2), else i - n; ikz = 0 .. n/2.  |e| = 1.  A file is an int32 n followed by the doubles.
//   Matrix.  Simple cubic lattice of spacing 1 under periodic gravity (Marcos et al. 2006), k = 2 pi m / n.  The normalised dynamical
//          matrix, in units of 4 pi G rho_0:
//              D_ab(k) = delta_ab / 3 - S_ab(k) / (4 pi),     S_ab(k) = sum_{R != 0} cos(k.R) d_a d_b (1/r) at R,
//          the conditionally convergent sum taken in its Ewald form with splitting parameter alpha and shells R, m' in [-s, s]^3:
//              S_ab = sum_{R != 0} cos(k.R) [A(R) R_a R_b - B(R) delta_ab] + 4 alpha^3 / (3 sqrt pi) delta_ab
//                     - 4 pi sum_m' q_a q_b exp(-q^2 / 4 alpha^2) / q^2,        q = 2 pi m' + k
//              A(R) = [3 erfc(alpha R) / R^3 + (2 alpha / sqrt pi) exp(-alpha^2 R^2) (3 / R^2 + 2 alpha^2)] / R^2
//              B(R) = erfc(alpha R) / R^3 + (2 alpha / sqrt pi) exp(-alpha^2 R^2) / R^2
//          Product values alpha = 2, s = 4: the omitted terms are below 1e-20.
//   Mode.  Eigenvalues within 1e-9 of each other (chained) form one eigenspace.  lambda is the eigenvalue (the mean over its
//          eigenspace) whose eigenspace carries the largest projection of khat = m / |m|; e is that projection, normalised, so e.khat > 0.
//          In an exactly degenerate space (the zone corner, D = delta / 3) e is therefore khat, not whatever a solver returns.
//          Entry [0][0][0] is (0, 0, 0, 1): the reader blends it into the neighbours of k = 0 when it interpolates — a zero vector
//          leaves their direction alone — and 1 is the k -> 0 limit of lambda.
//   Known limitation.  Whether `eigmodes128` was built with exactly this selection rule cannot be checked: its generator is not
//          published.  The rule follows Garrison et al. 2016 ("most longitudinal") and the comment at get_eigenmode
//          (src/zeldovich.cpp: "upweights each mode by 1/(khat.e)").
//   What it gives (tests/plt_eigen_ref.py, tests/test_plt_eigen.py): tr D = 1 (Kohn sum rule) to 4e-15; D -> khat khat as k -> 0;
//          at (pi, 0, 0) lambda = 1.10423556, transverse -0.05211778; at (pi, pi, pi) three times 1/3; over whole tables lambda in
//          [0.3265, 1.1043] and e.khat >= 0.63.
//
// AS BUILT
//   k_plt_modes<S>: one thread per wavevector, a launch per chunk of kx planes, a fixed summation order (two calls return the same
//   bits).  No erfc and no transcendental in the inner loops:
//     * A(R), B(R) do not depend on k: the host forms them for the half shell (std::erfc; R and -R contribute equally: 364 vectors at
//       s = 4) and the workgroup keeps them in LDS, every lane reading the same entry.
//     * cos(k.R) = Re prod_a e^{i k_a R_a}: per axis s sincos of 2 pi j / n with the INTEGER j = m_a R_a mod n folded to (-n/2, n/2];
//       no sincos of an unreduced argument.  The x factor is formed once per R_x plane (a rolled loop), y and z sit in registers.
//     * exp(-q^2 / 4 alpha^2) = prod_a exp(-q_a^2 / 4 alpha^2): 3 (2 s + 1) exp per mode.
//   The eigenproblem: cyclic Jacobi on the 3 x 3 in registers, PLT_SWEEPS sweeps whatever the matrix (orthonormal vectors at
//   degeneracy too), then the selection rule.  Plain C++ and vector stores only.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "zd_launch.h"
#include "zd_plt.h"

namespace zd {

PltConst plt_const(int n, double alpha) {
    PltConst c;
    c.n      = n;
    c.inv4a2 = 1.0 / (4.0 * alpha * alpha);
    c.self   = 4.0 * alpha * alpha * alpha / (3.0 * sqrt(M_PI));
    return c;
}

// A(R) | B(R) interleaved, in the order the kernels walk the half shell: the plane R_x = 0 (R_y = 0: R_z = 1 .. s; R_y = 1 .. s: every
// R_z), then the planes R_x = 1 .. s (every R_y, R_z)
std::vector<double> plt_shell_table(double alpha, int s) {
    std::vector<double> tab;
    tab.reserve(2 * (size_t) plt_half_shell(s));
    const double g0 = 2.0 * alpha / sqrt(M_PI);
    for (int rx = 0; rx <= s; rx++)
        for (int ry = rx == 0 ? 0 : -s; ry <= s; ry++)
            for (int rz = rx == 0 && ry == 0 ? 1 : -s; rz <= s; rz++) {
                const double r2 = (double) (rx * rx + ry * ry + rz * rz), r = sqrt(r2), r3 = r2 * r;
                const double ec = std::erfc(alpha * r), g = g0 * exp(-alpha * alpha * r2);
                tab.push_back((3.0 * ec / r3 + g * (3.0 / r2 + 2.0 * alpha * alpha)) / r2);
                tab.push_back(ec / r3 + g / r2);
            }
    return tab;
}

namespace {

constexpr int PLT_BX       = 256;  // threads (consecutive wavevectors of the chunk, kz fastest) per workgroup
constexpr int PLT_SWEEPS   = 8;    // cyclic Jacobi sweeps: a 3 x 3 is at rounding after 5
constexpr double PLT_GROUP = 1e-9; // eigenvalues closer than this form one eigenspace

// e^{2 pi i m r / n} from the integer m r mod n, folded to (-n/2, n/2]
__device__ __forceinline__ void plt_phase(int n, int m, int r, double &c, double &s) {
    int j = (m * r) % n;  // |m| <= n/2 <= 256 (the test hook: <= 2^20), r <= 5
    if (j < 0) j += n;
    if (2 * j > n) j -= n;
    sincospi((double) (2 * j) / (double) n, &s, &c);
}

// one plane R_x = rx of the real-space sum (HALF: the plane R_x = 0, of which the half R_y > 0 or R_y = 0, R_z > 0 is walked);
// (exr, exi) = e^{i k_x R_x}; tp: the plane's A | B entries
template <int S, bool HALF>
__device__ __forceinline__ void plt_real_plane(double rx, double exr, double exi, const double (&cy)[S + 1], const double (&sy)[S + 1],
                                               const double (&cz)[S + 1], const double (&sz)[S + 1], const double2 *tp, double (&acc)[6],
                                               double &accB) {
    int t = 0;
#pragma unroll
    for (int ry = HALF ? 0 : -S; ry <= S; ry++) {
        const int ay     = ry < 0 ? -ry : ry;
        const double eyr = cy[ay], eyi = ry < 0 ? -sy[ay] : sy[ay];
        const double cr = exr * eyr - exi * eyi, ci = exr * eyi + exi * eyr;
        double T0 = 0.0, T1 = 0.0, T2 = 0.0, U = 0.0;
#pragma unroll
        for (int rz = (HALF && ry == 0) ? 1 : -S; rz <= S; rz++) {
            const int az     = rz < 0 ? -rz : rz;
            const double ezi = rz < 0 ? -sz[az] : sz[az];
            const double cc  = cr * cz[az] - ci * ezi;  // cos(k.R)
            const double2 ab = tp[t++];
            const double a   = ab.x * cc;
            U  = fma(ab.y, cc, U);
            T0 += a;
            T1 = fma(a, (double) rz, T1);
            T2 = fma(a, (double) (rz * rz), T2);
        }
        acc[0] = fma(rx * rx, T0, acc[0]);
        acc[1] = fma((double) (ry * ry), T0, acc[1]);
        acc[2] += T2;
        acc[3] = fma(rx * (double) ry, T0, acc[3]);
        acc[4] = fma(rx, T1, acc[4]);
        acc[5] = fma((double) ry, T1, acc[5]);
        accB += U;
    }
}

// the six distinct elements xx, yy, zz, xy, xz, yz of D at k = 2 pi (mx, my, mz) / n; tab: LDS image of plt_shell_table(alpha, S)
template <int S>
__device__ __forceinline__ void plt_matrix(const PltConst &c, int mx, int my, int mz, const double2 *tab, double (&D)[6]) {
    constexpr int W = 2 * S + 1;
    const int n = c.n;
    const double TWO_PI = 6.283185307179586476925286766559;
    // ---- real space: 2 sum over the half shell ----
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, accB = 0.0;
    {
        double cy[S + 1], sy[S + 1], cz[S + 1], sz[S + 1];
        cy[0] = cz[0] = 1.0;
        sy[0] = sz[0] = 0.0;
#pragma unroll
        for (int r = 1; r <= S; r++) {
            plt_phase(n, my, r, cy[r], sy[r]);
            plt_phase(n, mz, r, cz[r], sz[r]);
        }
        plt_real_plane<S, true>(0.0, 1.0, 0.0, cy, sy, cz, sz, tab, acc, accB);
        const double2 *tp = tab + (S + S * W);
#pragma unroll 1
        for (int rx = 1; rx <= S; rx++, tp += W * W) {
            double exr, exi;
            plt_phase(n, mx, rx, exr, exi);
            plt_real_plane<S, false>((double) rx, exr, exi, cy, sy, cz, sz, tp, acc, accB);
        }
    }
    // ---- reciprocal space: sum_m' q_a q_b exp(-q^2 / 4 alpha^2) / q^2 over [-S, S]^3; q = 0 (k = 0, m' = 0) is no term ----
    double rec[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    {
        const double fx = (double) mx / (double) n, fy = (double) my / (double) n, fz = (double) mz / (double) n;
        double qy[W], gy[W], qz[W], gz[W];
#pragma unroll
        for (int i = 0; i < W; i++) {
            qy[i] = TWO_PI * ((double) (i - S) + fy);
            gy[i] = exp(-qy[i] * qy[i] * c.inv4a2);
            qz[i] = TWO_PI * ((double) (i - S) + fz);
            gz[i] = exp(-qz[i] * qz[i] * c.inv4a2);
        }
#pragma unroll 1
        for (int ix = 0; ix < W; ix++) {
            const double qx = TWO_PI * ((double) (ix - S) + fx);
            const double gx = exp(-qx * qx * c.inv4a2);
#pragma unroll
            for (int iy = 0; iy < W; iy++) {
                const double gxy = gx * gy[iy], qxy2 = fma(qx, qx, qy[iy] * qy[iy]);
                double W0 = 0.0, W1 = 0.0, W2 = 0.0;
#pragma unroll
                for (int iz = 0; iz < W; iz++) {
                    const double q2 = fma(qz[iz], qz[iz], qxy2);
                    const double w  = q2 > 0.0 ? gxy * gz[iz] / q2 : 0.0;
                    W0 += w;
                    W1 = fma(w, qz[iz], W1);
                    W2 = fma(w, qz[iz] * qz[iz], W2);
                }
                rec[0] = fma(qx * qx, W0, rec[0]);
                rec[1] = fma(qy[iy] * qy[iy], W0, rec[1]);
                rec[2] += W2;
                rec[3] = fma(qx * qy[iy], W0, rec[3]);
                rec[4] = fma(qx, W1, rec[4]);
                rec[5] = fma(qy[iy], W1, rec[5]);
            }
        }
    }
    // D = delta / 3 - S / (4 pi),  S = 2 (acc - accB delta) + self delta - 4 pi rec
    const double inv4pi = 1.0 / (2.0 * TWO_PI);
#pragma unroll
    for (int j = 0; j < 3; j++) D[j] = 1.0 / 3.0 - (2.0 * (acc[j] - accB) + c.self) * inv4pi + rec[j];
#pragma unroll
    for (int j = 3; j < 6; j++) D[j] = rec[j] - 2.0 * acc[j] * inv4pi;
}

// one Jacobi rotation that zeroes a[P][Q]; v collects the rotations (columns = eigenvectors)
template <int P, int Q>
__device__ __forceinline__ void plt_rotate(double (&a)[3][3], double (&v)[3][3]) {
    constexpr int R  = 3 - P - Q;
    const double apq = a[P][Q];
    if (apq == 0.0) return;
    const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);  // +-inf for a tiny a[P][Q]: t = 0, nothing moves
    const double t     = copysign(1.0, theta) / (fabs(theta) + sqrt(fma(theta, theta, 1.0)));
    const double cs    = 1.0 / sqrt(fma(t, t, 1.0)), sn = t * cs;
    a[P][P] -= t * apq;
    a[Q][Q] += t * apq;
    a[P][Q] = a[Q][P] = 0.0;
    const double arp = a[R][P], arq = a[R][Q];
    a[R][P] = a[P][R] = cs * arp - sn * arq;
    a[R][Q] = a[Q][R] = sn * arp + cs * arq;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double vp = v[i][P], vq = v[i][Q];
        v[i][P] = cs * vp - sn * vq;
        v[i][Q] = sn * vp + cs * vq;
    }
}

// (e_x, e_y, e_z, lambda) of the definition from D's six elements at the signed wavenumber m != 0
__device__ __forceinline__ void plt_select(const double (&D)[6], int mx, int my, int mz, double (&out)[4]) {
    double a[3][3] = {{D[0], D[3], D[4]}, {D[3], D[1], D[5]}, {D[4], D[5], D[2]}};
    double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
#pragma unroll 1
    for (int sweep = 0; sweep < PLT_SWEEPS; sweep++) {
        plt_rotate<0, 1>(a, v);
        plt_rotate<0, 2>(a, v);
        plt_rotate<1, 2>(a, v);
    }
    const double w[3] = {a[0][0], a[1][1], a[2][2]};
    const double kn = 1.0 / sqrt((double) (mx * mx + my * my + mz * mz));
    const double kh[3] = {mx * kn, my * kn, mz * kn};
    double p[3];
#pragma unroll
    for (int i = 0; i < 3; i++) p[i] = v[0][i] * kh[0] + v[1][i] * kh[1] + v[2][i] * kh[2];
    // eigenspaces: the connected components of "closer than PLT_GROUP"
    const bool c01 = fabs(w[0] - w[1]) < PLT_GROUP, c02 = fabs(w[0] - w[2]) < PLT_GROUP, c12 = fabs(w[1] - w[2]) < PLT_GROUP;
    bool same[3][3];
    same[0][0] = same[1][1] = same[2][2] = true;
    same[0][1] = same[1][0] = c01 || (c02 && c12);
    same[0][2] = same[2][0] = c02 || (c01 && c12);
    same[1][2] = same[2][1] = c12 || (c01 && c02);
    double weight[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        weight[i] = 0.0;
#pragma unroll
        for (int j = 0; j < 3; j++) weight[i] += same[i][j] ? p[j] * p[j] : 0.0;
    }
    int best = 0;  // the first of equal weights (members of one eigenspace have the same)
    double wbest = weight[0];
    if (weight[1] > wbest) best = 1, wbest = weight[1];
    if (weight[2] > wbest) best = 2;
    double e[3] = {0.0, 0.0, 0.0}, lam = 0.0, cnt = 0.0;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const bool in = best == 0 ? same[0][j] : best == 1 ? same[1][j] : same[2][j];
        const double pj = in ? p[j] : 0.0;
#pragma unroll
        for (int i = 0; i < 3; i++) e[i] = fma(pj, v[i][j], e[i]);
        lam += in ? w[j] : 0.0;
        cnt += in ? 1.0 : 0.0;
    }
    const double en = 1.0 / sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
    out[0] = e[0] * en, out[1] = e[1] * en, out[2] = e[2] * en;
    out[3] = lam / cnt;
}

template <int S>
__device__ __forceinline__ void plt_load_table(const double *__restrict__ tab, double2 *lds) {
    for (int i = threadIdx.x; i < plt_half_shell(S); i += PLT_BX) lds[i] = make_double2(tab[2 * i], tab[2 * i + 1]);
    __syncthreads();
}

// grid: ceil(nkx n (n/2 + 1) / PLT_BX)  block: PLT_BX; out[(ikx - kx0)][iky][ikz][4]
template <int S>
__global__ __launch_bounds__(PLT_BX) void k_plt_modes(PltConst c, const double *__restrict__ tab, int kx0, int nkx, double *__restrict__ out) {
    __shared__ double2 lds[plt_half_shell(S)];
    plt_load_table<S>(tab, lds);
    const int n = c.n, h = n / 2 + 1;
    const long long id = (long long) blockIdx.x * PLT_BX + threadIdx.x;
    if (id >= (long long) nkx * n * h) return;
    const int iz = (int) (id % h), iy = (int) (id / h % n), ix = kx0 + (int) (id / ((long long) h * n));
    const int mx = ix <= n / 2 ? ix : ix - n, my = iy <= n / 2 ? iy : iy - n, mz = iz;
    double r[4] = {0.0, 0.0, 0.0, 1.0};
    if (mx != 0 || my != 0 || mz != 0) {
        double D[6];
        plt_matrix<S>(c, mx, my, mz, lds, D);
        plt_select(D, mx, my, mz, r);
    }
    double2 *o = reinterpret_cast<double2 *>(out + 4 * id);
    o[0] = make_double2(r[0], r[1]);
    o[1] = make_double2(r[2], r[3]);
}

#ifdef ZD_TESTING
// grid: ceil(nmodes / PLT_BX); out6[mode][6]
template <int S>
__global__ __launch_bounds__(PLT_BX) void k_test_plt_matrix(PltConst c, const double *__restrict__ tab, long long nmodes, const int *__restrict__ m_xyz,
                                                            double *__restrict__ out6) {
    __shared__ double2 lds[plt_half_shell(S)];
    plt_load_table<S>(tab, lds);
    const long long id = (long long) blockIdx.x * PLT_BX + threadIdx.x;
    if (id >= nmodes) return;
    double D[6];
    plt_matrix<S>(c, m_xyz[3 * id], m_xyz[3 * id + 1], m_xyz[3 * id + 2], lds, D);
#pragma unroll
    for (int j = 0; j < 6; j++) out6[6 * id + j] = D[j];
}

template <int S>
int launch_test_plt_matrix_t(const PltConst &c, const double *tab, long long nmodes, const int *m_xyz, double *out6, hipStream_t st) {
    hipLaunchKernelGGL(k_test_plt_matrix<S>, dim3((unsigned) ((nmodes + PLT_BX - 1) / PLT_BX)), dim3(PLT_BX), 0, st, c, tab, nmodes, m_xyz, out6);
    ZD_LAUNCH_CHECK();
    return 0;
}
#endif

}  // namespace

int launch_plt_modes(const PltConst &c, const double *tab, int kx0, int nkx, double *out, hipStream_t st) {
    const long long nmodes = (long long) nkx * c.n * (c.n / 2 + 1);
    if (nmodes <= 0) return 0;
    hipLaunchKernelGGL(k_plt_modes<PLT_SHELLS>, dim3((unsigned) ((nmodes + PLT_BX - 1) / PLT_BX)), dim3(PLT_BX), 0, st, c, tab, kx0, nkx, out);
    ZD_LAUNCH_CHECK();
    return 0;
}

#ifdef ZD_TESTING
int launch_test_plt_matrix(const PltConst &c, int shells, const double *tab, long long nmodes, const int *m_xyz, double *out6, hipStream_t st) {
    if (nmodes <= 0) return 0;
    if (shells == 3) return launch_test_plt_matrix_t<3>(c, tab, nmodes, m_xyz, out6, st);
    if (shells == 4) return launch_test_plt_matrix_t<4>(c, tab, nmodes, m_xyz, out6, st);
    if (shells == 5) return launch_test_plt_matrix_t<5>(c, tab, nmodes, m_xyz, out6, st);
    return 1;
}
#endif

}  // namespace zd
