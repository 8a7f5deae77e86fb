// zd_testing.h — entry points that exist only in the -DZD_TESTING library (make testing ->
// build/libzeldovich_hip_testing.so): device test hooks and the in-process emulation of the RCCL calls.  They are test
// scaffolding, not part of the product C ABI (include/zeldovich_hip.h); tests/ reach them through
// zeldovich_plt_amd.api.load_testing_library().
#pragma once
#include "../../include/zeldovich_hip.h"
#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)
/* ---- host hook (no GPU) -------------------------------------- */
/* the route (zd_route.h) plan creation takes for (p, stream factor R — 0: none given —, nranks), main pass: out[0 .. 11] = family,
 * pack, narray, pstep, npass, R, L, Hq, Zq, dens, dens_only, composite twiddles; `why` (cap bytes) gets the refusal text, "" if the
 * route is accepted.  Returns 0 if accepted, 1 if refused */
int zd_test_route(const zd_params *p, int32_t R, int32_t nranks, int32_t *out, char *why, int64_t cap);
/* the dispatch tables the stages of the job as given consult (zd_route.h route_stages; role: 0 main, 1 phi pass, 2 second f_NL pass,
 * 3 gradient passes of the second-order round), whatever the route says about the job: `text` (cap bytes) gets the line
 * "route <TAB> 1 accepted | 0 refused <TAB> refusal", then one line per stage, "stage <TAB> launcher <TAB> key <TAB> 1 | 0" — the launcher
 * and key as zd_dispatch_report names the instantiation, 1 if the table has a kernel for the key.  text may be NULL.  Returns the
 * number of stages without a kernel if the route accepts the job; -1 if it is refused by its parameters alone, -2 if only because a
 * stage has no kernel; -3 for an unknown role */
int zd_test_route_kernels(const zd_params *p, int32_t R, int32_t nranks, int32_t role, char *text, int64_t cap);
/* the coefficients a ZD_q2LPT job runs with (zd_route.h): out[0 .. 2] = alpha (= vnorm), lpt2_ratio and lpt2_f2 with their defaults
 * resolved */
void zd_test_lpt2_coefficients(const zd_params *p, double *out);
/* device buffers, pinned buffers, events and streams the library's owning handles (zd_own.h) hold at this moment, plus the plans alive:
 * 0 once everything the library made has been given back */
int64_t zd_test_live_handles(void);
/* ---- device test hooks (each needs a GPU) -------------------- */
/* n counter-addressed draws: out[2*i], out[2*i+1] = the two uint64 of mode (kx,ky,kz)[i] */
int zd_test_draws(int64_t seed, int64_t n, const int32_t *kxyz, uint64_t *out);
/* Gaussian amplitudes D(k) for the same mode list (cgauss<2>, src/power_spectrum.cpp:338-359) */
int zd_test_modes(const zd_params *p, const zd_pk *pk, int64_t n, const int32_t *kxyz, double *D);
/* the same through the arithmetic the production generator k_genf uses (LDS-table ln / exp / sincos / spline segments,
 * integer zero rule, Newton reciprocal): out[3*i] = {Re D, Im D, fundamental / |k|^2}; ky >= 0 */
int zd_test_modes_table(const zd_params *p, const zd_pk *pk, int64_t n, const int32_t *kxyz, double *out);
/* zd_generate with p->ngpu ranks as threads on the visible GPU(s), running the RCCL branch of the exchange code (buffer
 * offsets, grouped send / receive order, stream and event ordering) on an in-process emulation of the ncclSend / ncclRecv /
 * ncclGroup calls — real RCCL refuses two ranks on one device, and test boxes have one */
int zd_test_generate_loopback(const zd_params *p, const zd_pk *pk, const double *eig, int64_t eig_ppd, zd_slab_cb cb, void *user,
                              zd_stats *out);
/* ZD_Version = 1: the first 624 * nblocks words of gsl_rng_mt19937 seeded with `seed`, from the workgroup-parallel
 * regeneration the stream kernel uses (src/power_spectrum.cpp:18-25) */
int zd_test_v1_words(int64_t seed, int32_t nblocks, uint32_t *out);
/* batch of `lines` independent length-n inverse FFTs, host in/out [lines][n] complex double;
 * axis_kind 0: the contiguous-line kernel path (x pass), 1: the strided-line path (y/z passes; host layout [n][lines]);
 * 3 / 4: the composite transforms of the reference's arrays (ZD_f_NL on composite grids, zd_kernels_np2_ref.hip), strided lines
 * (host layout [n][lines]) / contiguous lines, any n of its table and any number of lines */
int zd_test_fft(int32_t n, int64_t lines, int32_t axis_kind, const double *in, double *out);
/* the y columns of the reference's arrays split over G ranks (ZD_f_NL on composite grids, several ranks: k_refq_ycols) on host
 * columns [nimg][n][ncols] complex double, through a chunked store of nimg planes per chunk; mode 0: ky = n/2 read as zero, every
 * output written; 1: every input read, outputs ky < n/2 only (the other rows of out keep their input) */
int zd_test_ycols(int32_t n, int32_t G, int32_t ncols, int32_t nimg, int32_t mode, const double *in, double *out);
/* on != 0: every store / exchange ring / phi field the library allocates from now on starts out as NaN bytes */
void zd_test_poison(int on);
/* w = 4: plans of the ZA field store at PPD = 1024 created from now on pair their ring rows in groups of 4 — two column pairs per y
 * workgroup, the form PPD = 4096 runs — instead of 8 (zd_device.h ring_pair_w); 0: back to the table */
void zd_test_ring_pair_w(int w);
/* rank >= 0: that rank of the thread-per-GPU driver (zd_generate with ngpu > 1, zd_test_generate_loopback) fails BEFORE its first
 * pass — its peers are then blocked inside their first grouped send / receive, which only an abort ends; -1: nobody */
void zd_test_fail_rank(int rank);
/* the PLT dynamical matrix (zd_kernels_plt.hip) at nmodes signed wavenumbers m_xyz[nmodes][3] of a table of n points per side, for the
 * splitting parameter alpha and `shells` (3, 4 or 5) shells: out6[nmodes][6] = D_xx, D_yy, D_zz, D_xy, D_xz, D_yz */
int zd_test_plt_matrix(int64_t n, double alpha, int32_t shells, int64_t nmodes, const int32_t *m_xyz, double *out6);
#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
