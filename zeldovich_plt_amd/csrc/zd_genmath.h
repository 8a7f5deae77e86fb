// zd_genmath.h — per-mode device arithmetic shared by the generator kernels (zd_kernels.hip: k_gen / k_genf; zd_kernels_fz.hip:
// the fused generator + z FFT of the packed PLT store): table forms of ln / exp / sincos / sqrt, PowerSpectrum::power from the
// LDS image, the per-axis part of the eigenmode lookup.  Moved out of zd_kernels.hip unchanged (round 5).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "zd_device.h"

namespace zdgen {
using zd::GenConst;

// i mod N for 0 <= i < 2^31 (N a power of two on the production path; PPD = 2^a 3^b takes the division)
__device__ __forceinline__ int modn(int N, int i) { return (N & (N - 1)) == 0 ? (i & (N - 1)) : (int) ((unsigned) i % (unsigned) N); }

// interp_eigmode + get_eigenmode (src/zeldovich.cpp:154-276); out = e_x,e_y,e_z (weighted), lambda.
// The per-axis part of the lookup (table index or lower/upper corner + fraction, incl. the "never
// interpolate across the +-Nyquist seam" rule :176-183 and the wrap :194-198) depends on one wavenumber
// only, so the generator hoists x (fixed per thread) and y (fixed per row) out of its mode loop.
struct EigAxis {
    int l, h;   // exact stride: l = table index, h unused; interpolation: lower / upper corner
    double f;   // fraction towards h
};
__device__ __forceinline__ EigAxis eig_axis(const GenConst &g, int ik) {  // ik = table-space index 0..N-1
    EigAxis a;
    const int N = g.N, ep = (int) g.eig_ppd;
    if (ep % N == 0) {
        a.l = ik * (ep / N);
        a.h = a.l;
        a.f = 0.0;
        return a;
    }
    const int halfppd = ep / 2 + 1, ppdhalf = ep / 2;
    double f = ((double) ep) / N * ik;
    if (f > ppdhalf && f < halfppd) f = floor(f + 1);
    a.l = (int) f;
    a.h = a.l + 1;
    if (a.h == ep) a.h = 0;
    a.f = f - a.l;
    return a;
}
__device__ __forceinline__ int eig_index_x(const GenConst &g, int kx) { return kx < 0 ? g.N + kx : kx; }
__device__ __forceinline__ int eig_index_z(const GenConst &g, int kz) {
    const int i = kz < 0 ? g.N + kz : kz;
    return i > g.N / 2 ? g.N - i : i;  // +k half-space of the rfft layout
}
// ------------------------------------------------------------------------------------------------
// k_genf arithmetic.  The generator is VALU-bound (2 x 128-bit LCG steps + Box-Muller + P(k) per mode,
// redone for every z-residue pass), and a wave's 64 modes have 64 unrelated |k|^2: gathering {P, 1/k^2}
// from the by-|k|^2 table costs 64 cache-line fills per wave-instruction and was measured to take as
// long as all the arithmetic together.  So k_genf evaluates everything from small LDS tables
// (GenfTab, ~22 KB, built on the host in long double):
//   * one_rand<2> (power_spectrum.cpp:284-308) is kept as the exact integer m = r + 1 (m = 0 <=> r = 2^64-1,
//     i.e. the value 1.0) and its correctly rounded double; the 2^-64 scale is folded into the callers;
//   * ln x: x = 2^e f, f in [sqrt(1/2), sqrt(2)), bin j of width 1/256 with c_j ~ 1/centre, ln f = -ln c_j +
//     log1p(f c_j - 1) (7 terms; the two bins around f = 1 have c = 1 so that ln stays relatively exact near 1);
//   * e^x = 2^k 2^(j/64) e^r, |r| <= ln2/128 (6 terms);
//   * cos/sin(2 pi theta): nearest of 512 tabulated directions + a 3-term rotation;
//   * P(k): SplineFunction::val with per-segment records {x_lo, 1/h, y_lo, y_hi, y2_lo h^2/6, y2_hi h^2/6}.
// Each is within 4e-16 (relative) of the correctly rounded result; cgauss<2> itself evaluates
// cos/sin(fl(2*M_PI*theta)), 4e-16 away from the exact angle.
struct GenfTab {  // offsets in doubles inside the LDS image (zd_capi.cpp: build_genf_table)
    static constexpr int SC = 0, LG = 1024, EX = 1392, SEG = 1456, GLUT = 1024;
    static constexpr int lut(int nseg) { return SEG + 6 * nseg; }
    static constexpr int size(int nseg) { return SEG + 6 * nseg + GLUT / 4; }
};

// a*b + c as the three-address VOP3 form.  Left to itself the compiler picks the two-address v_fmac_f64 for the
// Horner steps below and then copies every coefficient into the destination first (a quarter of the loop's vector
// instructions were such v_mov_b64; the asm form makes the generator ~7 % faster).
// HAZARD: the compiler's hazard recognizer does not look at the operands of asm statements.  gfx950 needs a wait
// state between a transcendental VALU op (v_rcp_f64, v_rsq_f64, ...) and the first read of its result; with an asm
// v_fma_f64 as that first reader the wait state was missing whenever the scheduler happened to put the two back to
// back (round 1: 1/k^2 wrong -> PLT displacements 15 % off, NaN in the packed ZA kernel; the parity tests caught both).
// Two guards, neither by convention:
//   * every transcendental builtin used next to asm FMAs goes through trans_rcp / trans_rsq below, which carry their
//     own wait state (an `s_nop 0` tied to the result register: one issue cycle per reciprocal, ~3 per mode);
//   * build() runs check_trans_hazard.py on the gfx950 ISA of this file: no instruction may read a TRANS result in
//     the next issue slot.
// -DZD_NO_FMA_ASM builds the plain-fma() version of everything (A/B parity runs).
__device__ __forceinline__ double trans_rcp(double d) {
    double r = __builtin_amdgcn_rcp(d);
    asm volatile("s_nop 0" : "+v"(r));
    return r;
}
__device__ __forceinline__ double trans_rsq(double d) {
    double r = __builtin_amdgcn_rsq(d);
    asm volatile("s_nop 0" : "+v"(r));
    return r;
}
__device__ __forceinline__ double fma3(double a, double b, double c) {
#ifdef ZD_NO_FMA_ASM
    return fma(a, b, c);
#endif
    double d;
    asm volatile("v_fma_f64 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}

__device__ __forceinline__ double fnma3(double a, double b, double c) {  // -a*b + c
#ifdef ZD_NO_FMA_ASM
    return fma(-a, b, c);
#endif
    double d;
    asm volatile("v_fma_f64 %0, -%1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}
__device__ __forceinline__ double fmas3(double a, double b, double c) {  // a*b - c
#ifdef ZD_NO_FMA_ASM
    return fma(a, b, -c);
#endif
    double d;
    asm volatile("v_fma_f64 %0, %1, %2, -%3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}

__device__ __forceinline__ double u64_to_double(uint64_t m) {  // round-to-nearest: both halves are exact, one rounding in the fma
    return fma((double) (uint32_t) (m >> 32), 4294967296.0, (double) (uint32_t) m);
}

// ln(x * 2^-ebias) for a normal x > 0
__device__ __forceinline__ double flog(double x, int ebias, const double *T) {
    double f = __builtin_amdgcn_frexp_mant(x);  // [0.5, 1)
    int e    = __builtin_amdgcn_frexp_exp(x);
    const bool lo = f < 0.70710678118654752440;
    f = lo ? f + f : f;  // [sqrt(1/2), sqrt(2))
    e = lo ? e - 1 : e;
    const int j     = (int) (f * 256.0) - 181;
    const double2 t = reinterpret_cast<const double2 *>(T + GenfTab::LG)[j];  // {c_j, -ln c_j}
    const double r  = fma(f, t.x, -1.0);
    double p = fma3(r, 1.0 / 7.0, -1.0 / 6.0);
    p = fma3(r, p, 0.2);
    p = fma3(r, p, -0.25);
    p = fma3(r, p, 1.0 / 3.0);
    p = fma3(r, p, -0.5);
    p = fma3(r, p, 1.0);
    const double de = (double) (e - ebias);
    return fma3(de, 0.69314716756343842, fma3(de, 1.2996506893901347e-08, fma3(r, p, t.y)));
}

__device__ __forceinline__ double fexp(double x, const double *T) {
    x = fmin(fmax(x, -745.0), 709.0);
    const double n = __builtin_rint(x * 92.332482616893656877);  // 64 / ln 2
    double r = fma3(n, -0.010830424493178725, x);
    r = fma3(n, -2.0307042021720854e-10, r);
    const int ni = (int) n;
    double p = fma3(r, 1.0 / 720, 1.0 / 120);
    p = fma3(r, p, 1.0 / 24);
    p = fma3(r, p, 1.0 / 6);
    p = fma3(r, p, 0.5);
    p = fma3(r, p, 1.0);
    p = fma3(r, p, 1.0);
    return ldexp(T[GenfTab::EX + (ni & 63)] * p, ni >> 6);
}

__device__ __forceinline__ double frcp(double d) {
    double r = trans_rcp(d);
    const double e = fma(-d, r, 1.0);
    r = fma3(e, r, r);
    return fma3(fnma3(d, r, 1.0), r, r);
}

// sqrt(v) for v >= 0 (v = 0 -> 0); v is far from the subnormal range (P(k) |ln R| of a mode that carries power)
__device__ __forceinline__ double sqrt_pos(double v) {
    const double r = trans_rsq(v);
    double g = v * r, h = 0.5 * r;
    const double e = fnma3(h, g, 0.5);
    g = fma3(g, e, g);
    h = fma3(h, e, h);
    g = fma3(fnma3(g, g, v), h, g);
    g = fma3(fnma3(g, g, v), h, g);
    return v > 0.0 ? g : 0.0;
}

// cos/sin(2 pi m 2^-64) from sc[j] = {cos, sin}(2 pi j / 512)
__device__ __forceinline__ void sincos_u01(double md, const double *T, double &sn, double &cs) {
    const double t = md * 2.77555756156289135e-17;  // m * 2^-55 = theta * 512, exact
    const double j = __builtin_rint(t);
    const double b = (t - j) * 1.22718463030851298e-02;  // 2 pi / 512 * (theta*512 - j), |b| <= pi/512
    const double2 a = reinterpret_cast<const double2 *>(T + GenfTab::SC)[((int) j) & 511];
    const double b2 = b * b;
    const double sb = fma3(b * b2, fma3(b2, 8.33333333333333322e-03, -1.66666666666666657e-01), b);          // sin b
    const double cm = b2 * fma3(b2, fma3(b2, -1.38888888888888894e-03, 4.16666666666666644e-02), -0.5);     // cos b - 1
    cs = a.x + fmas3(a.x, cm, a.y * sb);
    sn = a.y + fma3(a.y, cm, a.x * sb);
}

// PowerSpectrum::power (src/power_spectrum.cpp:225-261) for k2 = |k|^2 > 0, from the LDS image
template <bool PLAW>
__device__ __forceinline__ double genf_power(const GenConst &g, const double *T, double k2) {
    const double v = 0.5 * flog(k2, 0, T);  // ln k
    double val;
    if constexpr (PLAW) {
        val = g.powerlaw_index * v;
    } else {
        const int nseg = g.genf_nseg;
        const unsigned short *lut = reinterpret_cast<const unsigned short *>(T + GenfTab::lut(nseg));
        int c = (int) ((v - g.glut_x0) * g.glut_inv_dx);
        c     = c < 0 ? 0 : (c >= GenfTab::GLUT ? GenfTab::GLUT - 1 : c);
        int klo = lut[c];
        const double *seg = T + GenfTab::SEG;
        while (klo < nseg - 1 && seg[6 * (klo + 1)] <= v) klo++;  // largest klo with x[klo] <= v (spline_function.h:146-152)
        const double2 *rec = reinterpret_cast<const double2 *>(seg + 6 * klo);
        const double2 q0 = rec[0], q1 = rec[1], q2 = rec[2];  // {x_lo, 1/h}, {y_lo, y_hi}, {c_lo, c_hi}
        const double b = (v - q0.x) * q0.y, a = 1.0 - b;
        val = fma3(a, q1.x, b * q1.y) + fma3(fmas3(a * a, a, a), q2.x, fmas3(b * b, b, b) * q2.y);
    }
    return fexp(fma(-k2, g.pk_smooth2, val), T) * g.pk_norm;
}

__device__ __forceinline__ void cmac(double &ar, double &ai, double c, double dr, double di) {
    ar = fma(c, dr, ar);
    ai = fma(c, di, ai);
}


// ------------------------------------------------------------------------------------------------
// Per-mode arithmetic of the general generator (k_gen) and the eigenmode lookups of k_genf, shared with the band-power sweep
// (zd_kernels_pk.hip).  Moved out of zd_kernels.hip unchanged.

// PowerSpectrum::power (src/power_spectrum.cpp:225-261) with SplineFunction::val
// (include/spline_function.h:141-163).  The reference bisects for the segment; here a uniform-cell
// table over ln k gives a start index and a short forward scan lands on exactly the segment the
// bisection would return (largest klo with x[klo] <= v, clamped to [0, n-2]).
template <bool PLAW>
__device__ __forceinline__ double pk_power(const GenConst &g, double k2) {  // k2 = |k|^2
    if (k2 <= 0.0) return 0.0;
    if constexpr (PLAW) {
        const double k = sqrt(k2);
        return pow(k, g.powerlaw_index) * exp(-k2 * g.pk_smooth2) * g.pk_norm;
    } else {
        const double v = 0.5 * log(k2);  // = log(sqrt(k2)) to 1 ulp
        int c   = (int) ((v - g.lut_x0) * g.lut_inv_dx);
        c       = c < 0 ? 0 : (c >= zd::PK_LUT ? zd::PK_LUT - 1 : c);
        int klo = g.pk_lut[c];
        const int last = g.pk_n - 2;
        while (klo < last && g.pk_x[klo + 1] <= v) klo++;
        const int khi = klo + 1;
        const double xl = g.pk_x[klo], xh = g.pk_x[khi];
        const double h = xh - xl;
        const double a = (xh - v) / h, b = (v - xl) / h;
        const double val = a * g.pk_y[klo] + b * g.pk_y[khi]
                           + ((a * a * a - a) * g.pk_y2[klo] + (b * b * b - b) * g.pk_y2[khi]) * (h * h) / 6.0;
        return exp(val - k2 * g.pk_smooth2) * g.pk_norm;
    }
}

// sin and cos of 2*pi*theta for theta in (0,1]: exact octant reduction (theta*8 is exact), then the
// fdlibm kernel polynomials on [0, pi/4].  cgauss<2> (power_spectrum.cpp:353-356) evaluates
// cos/sin(fl(2*M_PI*theta)); the two differ by the rounding of that product, ~4e-16 absolute.
__device__ __forceinline__ void sincos2pi(double theta, double &sn, double &cs) {
    const double t8 = theta * 8.0;
    const int q     = (int) t8;
    const double f  = t8 - (double) q;
    const int k     = q & 7;
    const double r  = (k & 1) ? 1.0 - f : f;
    const double a  = 0.78539816339744830962 * r;  // pi/4 * r
    const double z  = a * a;
    // __kernel_sin / __kernel_cos coefficients (fdlibm k_sin.c, k_cos.c)
    const double sp = -1.66666666666666324348e-01 + z * (8.33333333332248946124e-03 + z * (-1.98412698298579493134e-04
                      + z * (2.75573137070700676789e-06 + z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10))));
    const double s0 = a + a * z * sp;
    const double cp = 4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * (2.48015872894767294178e-05
                      + z * (-2.75573143513906633035e-07 + z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11))));
    const double c0 = 1.0 - (0.5 * z - z * z * cp);
    const bool swap = ((k + 1) & 2) != 0;  // k = 1,2,5,6
    const double sv = swap ? c0 : s0, cv = swap ? s0 : c0;
    sn = (k >= 4) ? -sv : sv;                      // k = 4..7: sin < 0
    cs = (k >= 2 && k <= 5) ? -cv : cv;            // k = 2..5: cos < 0
}

// cgauss<2> (power_spectrum.cpp:338-359) given P(k) and the two raw draws
__device__ __forceinline__ void gauss_from_pk(const GenConst &g, double Pk, uint64_t r1, uint64_t r2, double &dr,
                                              double &di) {
    double R           = zdpcg::u01(r1);
    const double theta = zdpcg::u01(r2);
    if ZD_TUNE(g.ablate & 2) {
        dr = R * Pk;
        di = theta * Pk;
        return;
    }
    if (!g.fixed_power)
        R = sqrt(-Pk * log(R));
    else
        R = sqrt(Pk);
    double sn, cs;
    sincos2pi(theta, sn, cs);
    dr = R * cs;
    di = R * sn;
}
template <bool PLAW>
__device__ __forceinline__ void gauss_mode(const GenConst &g, double k2, uint64_t r1, uint64_t r2, double &dr,
                                           double &di) {
    gauss_from_pk(g, ZD_TUNE(g.ablate & 1) ? 1e-9 * k2 : pk_power<PLAW>(g, k2), r1, r2, dr, di);
}

__device__ __forceinline__ void get_eigenmode_dev(const GenConst &g, int kx, int ky, int kz, const EigAxis &ax,
                                                  const EigAxis &ay, const EigAxis &az, double (&out)[4]) {
    const int ep = (int) g.eig_ppd, halfppd = ep / 2 + 1;
    const double k2 = (double) (kx * kx + ky * ky + kz * kz);
    double eh[4];
    const double2 *E = reinterpret_cast<const double2 *>(g.eig);  // [x][y][z][4] doubles = 2 double2 per entry
    if (ep % g.N == 0) {
        const int i = ((ax.l * ep + ay.l) * halfppd + az.l) * 2;
        const double2 q0 = E[i], q1 = E[i + 1];
        eh[0] = q0.x;
        eh[1] = q0.y;
        eh[2] = q1.x;
        eh[3] = q1.y;
    } else {
        // trilinear weights and corners in the reference's order f[0..7] = (x l/h, y l/h, z l/h) with z
        // fastest; accumulated left to right like the single expression of zeldovich.cpp:218-225.
        // Corners with zero weight are not read (the reference reads them: same value unless non-finite).
        eh[0] = eh[1] = eh[2] = eh[3] = 0.0;
#pragma unroll 2
        for (int c = 0; c < 8; c++) {
            const double wx = (c & 4) ? ax.f : 1 - ax.f, wy = (c & 2) ? ay.f : 1 - ay.f, wz = (c & 1) ? az.f : 1 - az.f;
            const double wgt = wx * wy * wz;
            if (wgt != 0) {
                const int cx = (c & 4) ? ax.h : ax.l, cy = (c & 2) ? ay.h : ay.l, cz = (c & 1) ? az.h : az.l;
                const int i  = ((cx * ep + cy) * halfppd + cz) * 2;
                const double2 q0 = E[i], q1 = E[i + 1];
                eh[0] += wgt * q0.x;
                eh[1] += wgt * q0.y;
                eh[2] += wgt * q1.x;
                eh[3] += wgt * q1.y;
            }
        }
    }
    eh[2] *= (kz < 0 ? -1.0 : 1.0);  // copysign(1, kz) for an int: kz = 0 -> +1
    const double imag = 1.0 / sqrt(eh[0] * eh[0] + eh[1] * eh[1] + eh[2] * eh[2]);
    eh[0] *= imag;  // the reference divides each component (zeldovich.cpp:257-259): <= 1 ulp apart
    eh[1] *= imag;
    eh[2] *= imag;
    double norm = k2 / (kx * eh[0] + ky * eh[1] + kz * eh[2]);
    if (k2 == 0.0 || !isfinite(norm)) norm = 0.0;
    out[0] = norm * eh[0];
    out[1] = norm * eh[1];
    out[2] = norm * eh[2];
    out[3] = eh[3];
}

// Tail of the k_genf eigenmode lookups: from the blended (un-normalised) table entry eh = (e_x, e_y, e_z, lambda) of |kz| to the
// coefficient of the displacement, out[j] = s_j = e_j k^2 / (k.e) x fundamental / k^2 = e_j / ((k.e) fundamental) (round 5: neither
// |e| nor k^2 enters — the reference normalises e, src/zeldovich.cpp:255-262, forms e k^2 / (k.e) and LoadPlane multiplies by
// fundamental / k^2, :428-434; one reciprocal instead of an inverse square root with two Newton steps and two reciprocals: 25 of a
// PLT mode's ~350 instructions); k.e = 0 or not finite -> 0 as there (:262-263; k = 0 does not occur: ky >= 1); out[3] = lambda
__device__ __forceinline__ void eig_coeff_tail(double fundamental, int kx, int ky, int kz, double (&eh)[4], double (&out)[4]) {
    eh[2] *= (kz < 0 ? -1.0 : 1.0);
    const double dot = kx * eh[0] + ky * eh[1] + kz * eh[2];
    double inv = frcp(dot * fundamental);
    if (!isfinite(inv)) inv = 0.0;
    out[0] = inv * eh[0];
    out[1] = inv * eh[1];
    out[2] = inv * eh[2];
    out[3] = eh[3];
}

// get_eigenmode for k_genf: the (x, y) part of the lookup — table offsets of the 4 corner columns and the products
// w_x w_y — depends on the thread's kx and the row's ky only and is prepared once per tile; per mode remain the two
// z corners, 1/|e| by rsq + Newton and k^2/(k.e) by reciprocal (get_eigenmode_dev: sqrt + two divisions).
// Accumulation order and weight association are those of get_eigenmode_dev / zeldovich.cpp:218-225.
struct EigXY {
    int base[4];   // ((cx*ep + cy)*halfppd)*2 in double2 units, corners (l,l), (l,h), (h,l), (h,h)
    double w[4];   // w_x * w_y
};
__device__ __forceinline__ EigXY eig_xy(const GenConst &g, const EigAxis &ax, const EigAxis &ay) {
    const int ep = (int) g.eig_ppd, halfppd = ep / 2 + 1;
    EigXY q;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const int cx = (c & 2) ? ax.h : ax.l, cy = (c & 1) ? ay.h : ay.l;
        q.base[c] = ((cx * ep + cy) * halfppd) * 2;
        q.w[c]    = ((c & 2) ? ax.f : 1 - ax.f) * ((c & 1) ? ay.f : 1 - ay.f);
    }
    return q;
}
__device__ __forceinline__ void eigenmode_fast(const GenConst &g, int kx, int ky, int kz, const EigXY &q, const EigAxis &az,
                                               double (&out)[4]) {
    const double fundamental = g.fundamental;
    const double2 *E = reinterpret_cast<const double2 *>(g.eig);
    double eh[4];
    if ((int) g.eig_ppd % g.N == 0) {
        const int i = q.base[0] + az.l * 2;
        const double2 q0 = E[i], q1 = E[i + 1];
        eh[0] = q0.x;
        eh[1] = q0.y;
        eh[2] = q1.x;
        eh[3] = q1.y;
    } else {
        eh[0] = eh[1] = eh[2] = eh[3] = 0.0;
#pragma unroll
        for (int c = 0; c < 8; c++) {
            const double wgt = q.w[c >> 1] * ((c & 1) ? az.f : 1 - az.f);
            if (wgt != 0) {
                const int i = q.base[c >> 1] + ((c & 1) ? az.h : az.l) * 2;
                const double2 q0 = E[i], q1 = E[i + 1];
                eh[0] += wgt * q0.x;
                eh[1] += wgt * q0.y;
                eh[2] += wgt * q1.x;
                eh[3] += wgt * q1.y;
            }
        }
    }
    eig_coeff_tail(fundamental, kx, ky, kz, eh, out);
}
}  // namespace zdgen
