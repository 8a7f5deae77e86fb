// TEST INFRASTRUCTURE ONLY: the plain DFT behind the FFTW3 interface (see fftw3.h).
#include <cmath>
#include <cstdlib>
#include <vector>

#include "fftw3.h"

struct fftw_plan_shim {
    int rank, n0, n1, sign;
    std::vector<long double> c, s;    // e^{sign 2 pi i m / n1}, m = 0 .. n1-1: the lines along the last index
    std::vector<long double> c0, s0;  // the same for n0: the columns of a 2-D plan (empty in a 1-D plan)
};

static void table(int n, int sign, std::vector<long double> &c, std::vector<long double> &s) {
    c.resize(n);
    s.resize(n);
    const long double twopi = 2.0L * acosl(-1.0L);
    for (int m = 0; m < n; m++) {
        long double a = twopi * (long double) m / (long double) n;
        c[m] = cosl(a);
        s[m] = sign * sinl(a);
    }
}

// one line of n points at the given stride: the input is copied to (xr, xi) first, so in and out may be the same line
static void line(int n, const std::vector<long double> &c, const std::vector<long double> &s, const fftw_complex *in,
                 fftw_complex *out, long stride, std::vector<long double> &xr, std::vector<long double> &xi) {
    for (int j = 0; j < n; j++) {
        xr[j] = in[j * stride][0];
        xi[j] = in[j * stride][1];
    }
    for (int k = 0; k < n; k++) {
        long double ar = 0.0L, ai = 0.0L;
        long m = 0;  // j k mod n
        for (int j = 0; j < n; j++) {
            ar += xr[j] * c[m] - xi[j] * s[m];
            ai += xr[j] * s[m] + xi[j] * c[m];
            m += k;
            if (m >= n) m -= n;
        }
        out[k * stride][0] = (double) ar;
        out[k * stride][1] = (double) ai;
    }
}

extern "C" fftw_plan fftw_plan_dft_1d(int n, fftw_complex *, fftw_complex *, int sign, unsigned) {
    if (n <= 0 || (sign != 1 && sign != -1)) return NULL;
    fftw_plan p = new fftw_plan_shim;
    p->rank = 1;
    p->n0 = 1;
    p->n1 = n;
    p->sign = sign;
    table(n, sign, p->c, p->s);
    return p;
}

extern "C" fftw_plan fftw_plan_dft_2d(int n0, int n1, fftw_complex *, fftw_complex *, int sign, unsigned) {
    if (n0 <= 0 || n1 <= 0 || (sign != 1 && sign != -1)) return NULL;
    fftw_plan p = new fftw_plan_shim;
    p->rank = 2;
    p->n0 = n0;
    p->n1 = n1;
    p->sign = sign;
    table(n1, sign, p->c, p->s);
    table(n0, sign, p->c0, p->s0);
    return p;
}

extern "C" void fftw_execute_dft(const fftw_plan p, fftw_complex *in, fftw_complex *out) {
    // scratch is per call: the reference executes one plan from many threads at once
    int nmax = p->n0 > p->n1 ? p->n0 : p->n1;
    std::vector<long double> xr(nmax), xi(nmax);
    if (p->rank == 1) {
        line(p->n1, p->c, p->s, in, out, 1, xr, xi);
        return;
    }
    for (int r = 0; r < p->n0; r++)  // rows
        line(p->n1, p->c, p->s, in + (long) r * p->n1, out + (long) r * p->n1, 1, xr, xi);
    for (int q = 0; q < p->n1; q++)  // then columns, in place in the output
        line(p->n0, p->c0, p->s0, out + q, out + q, p->n1, xr, xi);
}

extern "C" void fftw_destroy_plan(fftw_plan p) { delete p; }
extern "C" int fftw_import_wisdom_from_filename(const char *) { return 0; }
extern "C" int fftw_export_wisdom_to_filename(const char *) { return 0; }
