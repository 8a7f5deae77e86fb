/* TEST INFRASTRUCTURE ONLY.  This project's stand-in for the FFTW3 entry points the reference program calls.  Written
 * here behind FFTW's interface; no FFTW code.  The transform is the definition itself: an O(n^2) sum per line,
 * Y[k] = sum_j X[j] exp(sign 2 pi i j k / n), unnormalised, with an n-entry twiddle table and the accumulation in long
 * double -- the dullest correct transform, so that what the reference program writes with it carries no FFT
 * library's rounding.  2-D plans transform the rows (last index), then the columns.  Planning never touches its
 * arrays (NULL is fine).  Checked against numpy.fft in tests/test_reference_runs.py. */
#ifndef ZD_SHIM_FFTW3_H
#define ZD_SHIM_FFTW3_H
#ifdef __cplusplus
extern "C" {
#endif

typedef double fftw_complex[2];
typedef struct fftw_plan_shim *fftw_plan;

#define FFTW_FORWARD (-1)
#define FFTW_BACKWARD (+1)
#define FFTW_MEASURE (0U)
#define FFTW_PATIENT (1U << 5)
#define FFTW_ESTIMATE (1U << 6)

fftw_plan fftw_plan_dft_1d(int n, fftw_complex *in, fftw_complex *out, int sign, unsigned flags);
fftw_plan fftw_plan_dft_2d(int n0, int n1, fftw_complex *in, fftw_complex *out, int sign, unsigned flags);
void fftw_execute_dft(const fftw_plan p, fftw_complex *in, fftw_complex *out);
void fftw_destroy_plan(fftw_plan p);
int fftw_import_wisdom_from_filename(const char *filename); /* always 0: there is no wisdom */
int fftw_export_wisdom_to_filename(const char *filename);   /* always 0: nothing is written */

#ifdef __cplusplus
}
#endif
#endif
