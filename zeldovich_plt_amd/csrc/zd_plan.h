// zd_plan.h — the plan object behind the staged C ABI (include/zeldovich_hip.h), shared by the zd_capi*.cpp units (single-rank
// stages) and zd_multi.cpp (the in-library multi-GPU driver).
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/zeldovich_hip.h"
#include "zd_device.h"
#include "zd_own.h"

struct EventPair {
    hipEvent_t a, b;
    int kind;
};

struct zd_plan {
    zd_plan() { zdown::live(+1); }
    ~zd_plan();  // zd_capi.cpp: collects the timing events; the members below release themselves
    zd_params p;
    int rank = 0, nranks = 1;
    int N = 0, half = 0, narray = 0, R = 1, L = 0, Hq = 0, Zq = 0;
    int family = 0;            // the kernel family of the route this plan was built from (zd_route.h FAM_*): the stages pick their kernels by it
    bool twr = false;          // reference arrays (family FAM_REF_COMPOSITE): the lines use the composite twiddles d_twr_*, else the Bluestein tables
    int pack = zd::PACK_NONE;  // what the store holds (zd_device.h PACK_*)
    int npass = 1, pstep = 1;  // passes per run; planes a store plane delivers (2 with PACK_ZAPAIR)
    bool var_pending = true;   // packed stores: the next Z stage accumulates sum |D|^2
    zd::GenConst g;
    zd::GenJumps J;
    zd::JobList jobs;
    zd::StoreLayout S;
    zd::EpiConst ec;
    // events and worker streams of the Z stage (declared before the buffers: released after them, as zd_plan_destroy always did)
    zdown::Event ev_fork;
    zdown::Event ev_pipe[5];  // one rank, two stores (zd_plan_run_passes): start, Z done x2, XY done x2
    std::vector<zdown::Event> ev_gen, ev_fft;  // per slab of d_Y
    zdown::Stream s_gen, s_fft;
    // field store (PACK_ZAFIELD): layout of the store, and the ring the y stage fills for the x stage
    zd::FieldLayout F;
    zdown::DevBuf<zd::FieldRow> d_fieldrows;
    zd::StoreLayout SR;             // the ring as a single-rank block store of 3 arrays
    zdown::DevBuf<zdfft::cplx> d_ring;
    bool dens = false;              // ZD_qdensity = 1 on the six-field store (composite grids): fields 4, 5 = D of the two residues
    bool dens_only = false;         // ZD_qdensity = 2 there: density planes only, no records
    zdown::DevBuf<zdfft::cplx> d_ring_dens;  // ... and their array delta_r0 + i delta_r1 for the ring's planes
    // PLT + ZD_qdensity = 1 on the composite grids (one rank): the density planes of a pass come from a second, density-only plan at
    // stream factor 2R (its pass j = residues j, j + R = exactly the planes of this plan's pass j), run at the head of the Z stage on
    // the same store; they wait here, in delivery order, for the x stage's calls
    zdown::PlanPtr dens_sub;
    zdown::DevBuf<float> d_dens_pass;
    int dens_pass = -1;  // the pass whose density planes d_dens_pass holds (the latest Z stage's; -1: none yet)
    int ring_planes = 0;
    int64_t store_bytes_ = 0;       // bytes of the send (= receive) buffer per pass
    // device tables
    zdown::DevBuf<double> d_pk;  // x | y | y2
    zdown::DevBuf<int> d_lut;
    zdown::DevBuf<double> d_pktab;
    zdown::DevBuf<double> d_fnlM;  // f_NL: M(k) by integer |k|^2
    zdown::DevBuf<double> d_eig;
    zdown::DevBuf<double> d_eiglines;  // PLT with an interpolated table: (x, y)-interpolated lines of the slab being generated
    zdown::DevBuf<zdpcg::u128> d_rowstate;
    zdown::DevBuf<zdfft::cplx> d_twN, d_twL;
    zdown::DevBuf<zdfft::cplx> d_twq_n, d_twq_l;  // PPD = 2^a 3^b: twiddle sets of the composite transforms (lengths N, L)
    zdown::DevBuf<double> d_genf;  // LDS image of k_genf
    zdown::DevBuf<unsigned> d_tilectr;  // one work counter per k_genf launch of a pass
    int n_tilectr = 0, gen_max_wgs = 0;
    zdown::DevBuf<zd::Reduce> d_red;
    // folded FFT inputs of one slab of half-space rows: Y[job][row][k2][x]; double-buffered so that
    // k_gen (VALU-bound) of slab s+1 runs beside k_zfft (HBM-bound) of slab s on a second stream
    // folded FFT inputs: a ring of slabs Y[job][row][k2][x].  Two slabs suffice for the gen || zfft overlap inside a
    // pass; whatever HBM the store leaves free holds more of them, so that the (VALU-bound) generator of pass p+1
    // runs ahead on its own stream while the (HBM-bound) y and x passes of pass p are still working
    std::vector<zdown::DevBuf<zdfft::cplx>> d_Y;
    int slab_rows = 0;        // rows generated per k_gen launch
    long long next_g = 0;     // running slab number: slab g lives in ring slot g % K
    int pass_step = 1;        // distance to this rank's next pass (pass groups: zd_plan_run_passes deals passes first, first + step, ...)
    int ahead_pass = -1;      // pass whose first `ahead_n` slabs (numbers ahead_g0...) are already being generated
    long long ahead_g0 = 0;
    int ahead_n = 0;
    bool overlap = true;
    // fused Z stage of the packed PLT store (zd_kernels_fz.hip): work items (row, first column, columns), longest first
    bool fused_z = false;
    zdown::DevBuf<zd::FzItem> d_fzitems;
    unsigned n_fzitems = 0;
    int ncu = 256;
    // ZD_Version = 1 (zd_kernels_v1.hip): mt19937 streams, one per yres; accepted pairs of the slab being generated
    int v1_block = 0;               // PPD / NumBlock streams (0: version 2)
    zdown::DevBuf<zd::V1Stream> d_v1streams;
    zdown::DevBuf<double2> d_v1dev;     // [slab row][z][x]
    zdown::DevBuf<int> d_v1err;
    zdown::DevBuf<zdfft::cplx> d_phik_owned;  // ZD_f_NL: PhiK of the phi round; ZD_q2LPT: the source S(k) — whoever ran the round hands it over
    bool field = false;  // PhiK is a caller-supplied field (zd_plan_create_field): D = PhiK itself, d_fnlM a table of ones
    // second order on such a field (zd_plan_create_field_lpt, order 2): d_phik_owned holds D(k) (GenConst::phik) and this the source
    // S(k) (GenConst::lpt2_sk)
    zdown::DevBuf<zdfft::cplx> d_lpt2_sk_owned;
    zdown::DevBuf<zdfft::cplx> d_lpt3_owned[4];  // ZD_q3LPT: P3(k), C_x(k), C_y(k), C_z(k) of the third-order round, handed over likewise
    // any even PPD (zd_kernels_any.hip): Bluestein tables for the lengths L (z lines) and N (y, x lines)
    bool any = false;  // family >= FAM_REF_COMPOSITE: the reference's arrays as a [plane][array][y][x] store
    zd::AnyTab tabL = {}, tabN = {};
    zd::AnyLayout AL = {};
    zdown::DevBuf<zdfft::cplx> d_any[6];
    // ZD_f_NL on a composite grid (zd_kernels_np2_ref.hip): the same store and steps, the lines through the composite transforms
    // (twiddle sets of zd_fft_q.h for the lengths N and L) instead of the Bluestein tables above
    zdown::DevBuf<zdfft::cplx> d_twr_n, d_twr_l;
    bool phi_half = false;  // the phi round's Z stage writes the half-space planes [z][ky < N/2][x] (make_phik), no twin rows
    // the same arrays split over several ranks (nranks > 1): the chunked store of zd_device.h AnyChunks (chunk = Zq planes; a ring
    // slot of chunk_planes planes per chunk only changes AC.chunk)
    zd::AnyChunks AC = {};
    // timing
    std::vector<EventPair> events;
    double kernel_ms[ZD_K_COUNT] = {};
    int64_t launches[ZD_K_COUNT] = {};
    int64_t bytes_sent = 0;  // N > 1 ranks: accounted by zd_plan_run_pass, reported and reset by zd_plan_stats
};

// internal entry points shared by the zd_capi*.cpp units and zd_multi.cpp
extern "C" {
int zd_plan_stage_y_group(zd_plan *pl, void *d_recv, int chunk_planes, int nplanes, void *hip_stream);
int zd_plan_stage_x_group(zd_plan *pl, int residue, const void *d_recv, int chunk_planes, int64_t plane0, int64_t gplane0,
                          int64_t nplanes, void *d_records, float *d_density, void *hip_stream);
// f_NL on several ranks (zd_multi.cpp)
int zd_plan_create_phi(const zd_params *p, const zd_pk *pk, int rank, int nranks, zd_plan **out);
int zd_plan_create_phik(const zd_params *p, const zd_pk *pk, const double *eig, int64_t eig_ppd, int rank, int nranks, const void *d_phik,
                        zd_plan **out);
int zd_plan_phi_xy_group(zd_plan *pl, void *d_slot, int chunk_planes, int nplanes, double f_NL, void *hip_stream);
int zd_plan_phi_zfwd(zd_plan *pl, void *d_store, void *d_phik, void *hip_stream);
// NULL if ZD_f_NL with these parameters runs on several ranks, else why not
const char *zd_fnl_multi_unsupported(const zd_params *p);
// hipEvent pair around something on `hip_stream` that is not a kernel of this file (zd_multi.cpp: the wait for an exchanged
// plane group); summed into kernel_ms[kind] by zd_plan_stats when the plan profiles
void zd_plan_tick(zd_plan *pl, int kind, void *hip_stream, int begin);
int zd_plan_stage_z_detached(zd_plan *pl, int residue, void *d_send, void *hip_stream, void *wait_event, void *done_event);
}
int zd_generate_multi(const zd_params *p, const zd_pk *pk, const double *eig, int64_t eig_ppd, zd_slab_cb cb, void *user,
                      zd_stats *out, int transport);
