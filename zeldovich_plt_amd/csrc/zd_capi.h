// zd_capi.h — what the units of the C ABI (zd_capi*.cpp: include/zeldovich_hip.h, zd_testing.h, zd_tuning.h) share: one unit per job,
// every function one of them lends another declared here, once.  Internal to the library: nothing here is exported.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/zeldovich_hip.h"
#include "zd_device.h"
#include "zd_launch.h"
#include "zd_plan.h"
#include "zd_route.h"
#ifdef ZD_TUNING
#include "zd_tuning.h"
#endif
#ifdef ZD_TESTING
#include <atomic>

#include "zd_testing.h"
#endif

using zdfft::cplx;
using zdpcg::u128;
using zd::is_pow2;
using zd::Route;
using zd::route;
using zd::split_routes;  // (zd_route.h)
using zdown::DevBuf;
using zdown::Event;
using zdown::PinnedBuf;
using zdown::PlanPtr;
using zdown::Stream;
using zdown::upload;

#define HIPCHECK(call)                                                                               \
    do {                                                                                             \
        hipError_t e__ = (call);                                                                     \
        if (e__ != hipSuccess) {                                                                     \
            fprintf(stderr, "zeldovich_hip: %s failed at %s:%d: %s\n", #call, __FILE__, __LINE__,    \
                    hipGetErrorString(e__));                                                         \
            return 1;                                                                                \
        }                                                                                            \
    } while (0)

// ---- zd_capi_sizing.cpp: sizes of the stores and rounds ----
// complex elements of padding per row of a store (384 B from PPD = 512 on: de-aliases the y stage's strided rows)
int store_row_pad(int64_t N);
// Block table of the field store (zd_device.h FieldLayout) for `nranks` ranks; returns the elements per (plane, field) image
int64_t field_rows(const zd_params *p, int nranks, std::vector<zd::FieldRow> *rows);
// ring between the y and x stages of the field store: planes of the three PACK_ZAPAIR arrays
int field_ring_planes(int64_t N, int64_t Zq);
// ZD_f_NL memory: PhiK (half-space rows, [ky][kz][x])
int64_t fnl_phik_bytes(int64_t N);
// ZD_q2LPT memory: the source S(k) (half-space rows, PhiK's layout), and the peak of the second-order round before it
int64_t lpt2_sk_bytes(int64_t N);
int64_t lpt2_round_bytes(const zd_params *p);
// second order on a caller-supplied field: the round's peak with D(k) resident beside it
int64_t field_lpt2_round_bytes(const zd_params *p);
// ZD_q3LPT memory: the peak of the third-order round
int64_t lpt3_round_bytes(int64_t N);

// ---- zd_capi.cpp: plan construction ----
std::vector<cplx> make_twiddles(int n);
// Bluestein tables of a length-n transform on the engine of size M = 2^m >= 2n - 1 (zd_kernels_any.hip)
int any_make_tab(int n, zd::AnyTab *tab, DevBuf<cplx> *d_bufs);
// twiddles of a composite transform (zd_fft_q.h) of length len = P * Q: exp(2 pi i k / P) | exp(2 pi i k / len) | exp(2 pi i k / Q)
std::vector<cplx> make_twq(int len);  // (empty: no such transform)
int upload_twq(int len, DevBuf<cplx> &dst);
// a zeroed GenConst with the constants of the zero rule (zeldovich.cpp:299-320, 350; zd_device.h mode_is_zero)
void gen_zero_rule(zd::GenConst &g, const zd_params *p);
// the growth constants of the per-mode coefficients (zeldovich.cpp:403-434): every plan's, and those of zd_field_vjp
void gen_growth(zd::GenConst &g, const zd_params *p);
// phi_mode 1: first f_NL pass (one array holding phi = D/M); phik != NULL: second pass (D = phik * M).  ZD_q2LPT: phi_mode 2 = the
// plan of the second-order round's gradient passes; phik != NULL with phi_mode 0 = the final pass, phik holding the source S(k)
// field_d != NULL (ZD_q2LPT only): the modes D(k) of a caller-supplied field, PhiK's layout; the plan reads them (GenConst::phik with a
// table of ones) where it would draw, in the gradient passes and in the final pass, beside S(k)
int plan_create_ex(const zd_params *p, const zd_pk *pk, const double *eig, int64_t eig_ppd, int rank, int nranks, int phi_mode,
                   const cplx *phik, PlanPtr &out, bool field = false, const cplx *field_d = nullptr);
// a plan that was made goes to a caller of the C ABI; *out is left alone otherwise
int hand_over(int rc, PlanPtr &pl, zd_plan **out);

// ---- zd_capi_stages.cpp: the stages and their timing ----
void collect_events(zd_plan *pl);
// the line transforms of the reference-array store (pl->any): composite (zd_kernels_np2_ref.hip) where the route says so (pl->twr),
// else convolutions (zd_kernels_any.hip).  zlen: lines of length L (the z lines of a pass), else N.
int any_cols(const zd_plan *pl, bool zlen, void *data, long long batch_stride, long long point_stride, int ncols, int nbatch,
             int zero_point, hipStream_t st);
int any_lines(const zd_plan *pl, void *data, long long pitch, long long nlines, hipStream_t st);
// the layouts of a ring slot whose chunks are `chunk_planes` planes long instead of Zq (zd_multi.cpp exchanges in plane groups)
zd::StoreLayout layout_for_chunks(const zd_plan *pl, int chunk_planes);
zd::AnyChunks any_chunks(const zd_plan *pl, int chunk_planes);

// ---- zd_capi_rounds.cpp: the rounds before the first pass ----
// f_NL: the phi round, run once; *d_phik = PhiK[ky][kz][x] for the half-space rows (owned by the caller, untouched on failure)
int make_phik(const zd_params *p, const zd_pk *pk, DevBuf<cplx> &d_phik);
// the round's peak against the free memory, asked before anything is built (the figure is the message)
int lpt2_round_fits(const zd_params *p, int64_t free_bytes);
// ZD_q2LPT: the second-order round (zd_kernels_lpt2.hip), run once; d_sk = S(k)[ky][kz][x], scaled by N^-3 (handed to the caller).
// field_d != NULL: the gradient passes read D(k) of a caller-supplied field there (zd_kernels_lpt2_field.hip) instead of drawing it
int make_lpt2_source(const zd_params *p, const zd_pk *pk, DevBuf<cplx> &d_sk, const cplx *field_d = nullptr);
// ZD_q3LPT: the third-order round (zd_kernels_lpt3.hip), run once after the second; d_out[0 .. 3] = P3(k), C_x(k), C_y(k), C_z(k)
int make_lpt3_sources(const zd_params *p, const zd_pk *pk, const cplx *d_sk, DevBuf<cplx> (&d_out)[4]);
// a plan of the final pass takes the four spectra over and points its generator at them
void adopt_lpt3(zd_plan *pl, DevBuf<cplx> (&d_spec)[4]);
// a ZD_q2LPT job the route takes for this call (the refusal printed otherwise), asked BEFORE the second-order round is run
int lpt2_route_check(const zd_params *p, int nranks, int rank);

// ---- zd_capi_field.cpp: a caller-supplied field ----
struct FieldSpec {
    int32_t kind, dtype;  // ZD_FIELD_DENSITY / _WHITE, ZD_FIELD_F32 / _F64
    const void *field;    // a[z][y][x], C-contiguous
    int32_t on_device;
    int32_t order = 1;  // 2: second order on the field (zd_generate_field_lpt, zd_plan_create_field_lpt)
};
// The field -> d_phik = D(k)[ky][kz][x] for the half-space rows, zero rule and amplitude applied (owned by the caller, untouched on
// failure)
int make_field_phik(const zd_params *p, const zd_pk *pk, const FieldSpec &f, DevBuf<cplx> &d_phik);
// order 2: the second-order round with D(k) resident beside it against the free memory (the figure is the message)
int field_lpt2_fits(const zd_params *p, int64_t free_bytes);

// ---- zd_capi_generate.cpp ----
// zd_generate, and zd_generate_field (fs != NULL: the modes come from the caller's field; its refusals have been asked)
int generate_impl(const zd_params *p_in, const zd_pk *pk, const double *eig, int64_t eig_ppd, zd_slab_cb cb, void *user, zd_stats *out,
                  const FieldSpec *fs);

// ---- zd_capi_diag.cpp ----
#ifdef ZD_TESTING
extern std::atomic<int> g_ring_pair_w;  // zd_test_ring_pair_w
#endif
