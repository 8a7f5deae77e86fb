/* zeldovich_hip.h — C ABI of the MI355X-native grid->displacements path.
 *
 * The reference (abacusorg/zeldovich-PLT, mounted at /root/reference; citations are relative to it)
 * has no plugin / FFI interface: the path sits behind three C++ call sites in main()
 * (src/zeldovich.cpp:938 Setup_FFTW, :962-971 BlockArray + ZeldovichZ, :982 ZeldovichXY, which calls
 * back WriteParticlesSlab once per z plane, :667-681).  This header is the C-ABI a maintainer binds
 * in their place — plain pointers and sizes, no C++ / torch types.  INTEGRATION.md shows the binding.
 *
 * Library: zeldovich_plt_amd/csrc/build/libzeldovich_hip.so (HIP, gfx950 only).  All entry points
 * return 0 on success and non-zero on failure after printing a message to stderr (the reference's
 * convention is message + exit(1); the CLI wrapper turns a non-zero return into exit(1)).
 */
#ifndef ZELDOVICH_HIP_H
#define ZELDOVICH_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: exactly the declarations of this header are exported */
#pragma GCC visibility push(default)

#define ZD_MAX_PPD 65536 /* include/zeldovich.h:34 — fixes the RNG addressing */

/* ICFormat -> record layout (include/output.h:19-49) */
enum { ZD_FMT_ZEL = 0, ZD_FMT_RVZEL = 1, ZD_FMT_RVDOUBLEZEL = 2, ZD_FMT_ZELSIMPLE = 3 };

/* The subset of `Parameters` (include/parameters.h:9-86) that the path reads, with the derived
 * quantities of Parameters::setup (src/parameters.cpp:172-174) already filled in. */
typedef struct zd_params {
    int64_t ppd;        /* cbrt(NP): a power of two in [32, 16384] (above 8192: ZA field store only; 8192 with PLT: its field store only, i.e. no ZD_qdensity / ZD_f_NL), or 2^a Q with a >= 5 and Q one of 3, 9, 27, 5, 15,
                         * 25, 45, 75, 125, 135, 7, 21, 35, 49 (sizes: csrc/zd_kernels_np2.hip NP2_SIZES; the composite-transform kernels: ZA and PLT, also with ZD_qdensity = 1 or 2 — PLT with a density on one rank per pass group), or ANY other even number in [8, 8192]
                         * (one rank: convolution transforms on the power-of-two engine, ~6x slower).  ZD_f_NL on the composite sizes: the
                         * reference's arrays with composite-length transforms (csrc/zd_kernels_np2_ref.hip), on one rank or split over several
                         * (ZD_NumGPU = G, a power of two dividing PPD/2 and PPD/R; not with ZD_StoreMode = reference) */
    int32_t numblock;   /* ZD_NumBlock: v2 output does not depend on it; version 1: PPD / numblock random streams */
    int32_t cpd;        /* CPD: only used by the writer for ic_{z*cpd/ppd} */
    double boxsize;     /* BoxSize */
    double fundamental; /* 2 pi / boxsize */
    double nyquist;     /* pi / (boxsize/ppd) */
    double k_cutoff;    /* ZD_k_cutoff */
    double f_cluster;   /* ZD_f_cluster */
    double z_initial;   /* InitialRedshift */
    double PLT_target_z;
    int64_t seed;        /* ZD_Seed widened int -> unsigned long as src/power_spectrum.cpp:14 does */
    int32_t corner_modes;/* ZD_CornerModes */
    int32_t qdensity;    /* ZD_qdensity: 0 none, 1 also density plane, 2 density only */
    int32_t qoneslab;    /* ZD_qoneslab: -1 all, else only this z is delivered */
    int32_t qonemode;    /* ZD_qonemode */
    int32_t one_mode[3]; /* ZD_one_mode */
    int32_t qPLT;        /* ZD_qPLT */
    int32_t qPLTrescale; /* ZD_qPLT_rescale */
    int32_t icformat;    /* ZD_FMT_* */
    /* --- optional MI355X knobs (0 = let the library decide); not present in the reference --- */
    int32_t stream_factor; /* R: number of z-residue classes (a power of two; composite PPDs: any even divisor whose z lines PPD/R have a transform) */
    int32_t profile;       /* 1: bracket every kernel with hipEvents and report per-kernel ms */
    int32_t store_mode;    /* ZD_STORE_*: what the block store between the z and y passes holds (0 = best available) */
    int32_t serial_z;      /* 1: generator and z FFT on ONE stream (per-kernel timing runs); 0: two overlapped streams */
    int32_t ngpu;          /* ZD_NumGPU: GPUs of this node that zd_generate / the CLI drive (0 or 1 = one) */
    int32_t exchange_planes; /* store planes per exchange group between ranks (0 = ~4 GB ring slots) */
    /* --- local primordial non-Gaussianity (include/parameters.h:56-58); f_NL = 0 disables the path --- */
    double f_NL, n_s, Omega_M;
    /* --- ZD_Version (include/parameters.h:67-72): 0 or 2 = the pcg64 counter streams; 1 = the legacy phases: one
     * gsl_rng_mt19937 per yres (seed + yres) with rejection sampling (src/power_spectrum.cpp:18-25,310-332), which makes
     * the field depend on `numblock` — pass the value AFTER the reader's adjustment numblock = numblock * k_cutoff + .5
     * (src/parameters.cpp:129-141; zd_read_params does it) --- */
    int32_t version;
    int32_t pass_groups;   /* ZD_PassGroups, with ngpu > 1: the GPUs work as `pass_groups` independent groups of ngpu / pass_groups
                            * ranks; group j takes the residue passes j, j + pass_groups, ... and nothing travels between
                            * groups (the z-residue classes of the streaming are independent partitions of the output).
                            * Inside a group the rows / planes are sharded with the exchange described below.  0 = automatic:
                            * one GPU per group while the job has at least ngpu passes (2 and 4 GPUs at PPD = 4096: no
                            * exchange at all, where a pairwise exchange would be bound by ONE xGMI link), else one group
                            * of all GPUs (the all-to-all of 8 GPUs, every link of the mesh busy) */
    /* --- second-order Lagrangian perturbation theory (not in the reference; definition: csrc/zd_kernels_lpt2.hip) ---
     * q2LPT = 1 (ZD_q2LPT): displacement = psi1 + psi2, velocity = vnorm psi1 + lpt2_f2 psi2, with psi2 the Fourier-space 2LPT
     * displacement of the ZA field, scaled by lpt2_ratio = D2 / D1^2.  The two coefficients (ZD_2LPT_D2, ZD_2LPT_f2): 0 = the
     * values of the ZD_f_cluster background, -(2 vnorm + 1) / (6 vnorm + 1) (-3/7 at f_cluster = 1) and 2 vnorm.
     * ZD_Version 2, one GPU, PPD a power of two in [32, 2048]; not with ZD_qPLT, ZD_f_NL, ZD_qdensity, or ZD_CornerModes
     * together with ZD_k_cutoff != 1.
     * lpt2_dealias = 1 (ZD_2LPT_dealias, needs q2LPT = 1): the source of the second order is formed on the lattice of 3 PPD / 2 points
     * per side (Orszag's 3/2 rule, step 2' of the definition), so that no product mode folds back into the band that is kept; one
     * GPU holds ~81 PPD^3 bytes for that round (PPD <= 1024 on 288 GB); not with ZD_CornerModes.  The field sits in what was the
     * alignment gap between q2LPT and lpt2_ratio: no other member moves and the size of the struct is unchanged, so a caller built
     * against the earlier header that zero-fills the struct (as every reader here does) runs as before */
    int32_t q2LPT;
    int32_t lpt2_dealias;
    double lpt2_ratio;
    /* --- third-order Lagrangian perturbation theory (not in the reference; definition: csrc/zd_kernels_lpt3.hip) ---
     * q3LPT = 1 (ZD_q3LPT, needs q2LPT = 1): displacement = psi1 + psi2 + psi3, velocity = vnorm psi1 + lpt2_f2 psi2 + lpt3_f3 psi3, with
     * psi3_j(k) = i k_j P3 / k^2 - lpt3_g3c i (k x C)_j / k^2, P3 the transform of lpt3_g3a det T[D] + lpt3_g3b S3b and C the transverse
     * source.  The coefficients (ZD_3LPT_D3a, ZD_3LPT_D3b, ZD_3LPT_D3c, ZD_3LPT_f3): 0 = the default, which exists at f_cluster = 1 only:
     * -1/3, +10/21, +1/7 and 3 vnorm; any other f_cluster needs every enabled term's coefficient and lpt3_f3 given.  lpt3_terms
     * (ZD_3LPT_terms) leaves terms out: bit 1 = 3a, bit 2 = 3b, bit 4 = 3c, 0 = all (7).  What q2LPT refuses is refused; also
     * lpt2_dealias = 1 and PPD > 1024 (the third-order round holds ~120 PPD^3 bytes on one GPU; afterwards 40 PPD^3 stay resident).
     * The six members sit between lpt2_ratio and lpt2_f2: lpt2_f2 stays the LAST member of the struct, as tests/test_lpt2.py pins it, and
     * every member up to lpt2_ratio keeps its offset.  The struct grows by 40 bytes and lpt2_f2 moves by as much: callers are rebuilt
     * against this header (a caller that fills the struct by hand zeroes the new members; memset of the struct does). */
    int32_t q3LPT;
    int32_t lpt3_terms;
    double lpt3_g3a, lpt3_g3b, lpt3_g3c, lpt3_f3;
    double lpt2_f2;
} zd_params;

/* zd_params.store_mode */
enum {
    ZD_STORE_AUTO = 0,
    ZD_STORE_REFERENCE = 1, /* the reference's 1 / 2 / 4 complex arrays (density transformed; include/block_array.h:26-35) */
    ZD_STORE_PACKED = 2,    /* 3 arrays without the density field: ZA two z-residues per pass, PLT qx+i vx | qy+i qz | vy+i vz */
    ZD_STORE_FIELDS = 3     /* ZA only: the two potentials E = sum D/k^2, Z = sum kz D/k^2 of two z-residues for the
                             * half-space rows (no Hermitian twins), zero columns not stored; the y pass derives the
                             * displacement arrays plane by plane */
};

/* PowerSpectrum state after InitFromFile/InitFromPowerLaw + Normalize (src/power_spectrum.cpp:130-223).
 * Tables are the (ln k, ln P, y'') arrays of SplineFunction (include/spline_function.h). */
typedef struct zd_pk {
    int32_t n;
    const double *x, *y, *y2;
    double normalization;
    double Pk_smooth2;
    int32_t fixed_power; /* ZD_qPk_fix_to_mean */
    int32_t is_powerlaw;
    double powerlaw_index;
    double kmax; /* largest tabulated k (extrapolation warning only) */
    double kmin; /* smallest positive tabulated k (1e-4 for a power law): anchors primordial_norm, f_NL only */
} zd_pk;

/* Names of the kernels in timing arrays */
enum { ZD_K_GEN = 0, ZD_K_ZFFT = 1, ZD_K_YFFT = 2, ZD_K_XFFT = 3,
       ZD_K_ZSTAGE = 4, /* the Z stage as one unit: first generator launch .. last z FFT of a pass (the two kernels overlap
                         * on two streams, so their own spans include each other) */
       ZD_K_XWAIT = 5,  /* N > 1 ranks: time the compute stream stood waiting for an exchanged plane group to arrive */
       ZD_K_COUNT = 6 };

typedef struct zd_stats {
    double max_disp[3];      /* output.cpp:28: signed value of the largest |displacement| per axis (x,y,z) */
    double density_variance; /* output.cpp:30: sum of dens^2 over delivered planes */
    double seconds_total;    /* wall time of the grid->displacements interval (host clock, synced) */
    double kernel_ms[ZD_K_COUNT];      /* summed hipEvent time per kernel (profile=1) */
    int64_t kernel_launches[ZD_K_COUNT];
    int64_t bytes_intermediate; /* size of the z-FFT'd block store held in HBM per residue pass */
    int32_t stream_factor;      /* R actually used */
    int32_t modes_cached;       /* 1 if the Gaussian mode amplitudes were kept in HBM across passes */
    int64_t bytes_sent;         /* N > 1 ranks: bytes sent to OTHER ranks since the last zd_plan_stats / by this zd_generate call
                                 * (zd_generate: summed over the ranks) */
    int64_t max_disp_index[3];  /* lattice site (z * ppd + y) * ppd + x of max_disp[j]: the FIRST site in the reference's (z, y, x)
                                 * loop order that holds the largest |displacement| (output.cpp:190-193 compares with a strict >);
                                 * -1 if the field is identically zero */
} zd_stats;

/* Replacement for the per-plane callback WriteParticlesSlab (src/output.cpp:41-234).
 *   z          plane index (reference calls in increasing z; with stream_factor R > 1 planes arrive in
 *              residue order r, r+R, ... and `z` tells the consumer where they belong)
 *   n_records  ppd*ppd
 *   records    HOST pointer to n_records packed records (ICFormat layout), valid during the call only
 *   density    HOST pointer to n_records float32 densities, or NULL unless qdensity != 0
 * Return non-zero to abort. */
typedef int (*zd_slab_cb)(void *user, int64_t z, int64_t n_records, const void *records,
                          const float *density);

/* One call = ZeldovichZ + ZeldovichXY (src/zeldovich.cpp:517-695) on one GPU, or on p->ngpu GPUs of this node (one host thread
 * per GPU inside the library, the block exchange over RCCL / xGMI; the callback still comes from one thread at a time).
 *   eig / eig_ppd: PLT eigenmode table as loaded by load_eigmodes (src/zeldovich.cpp:794-830),
 *                  [eig_ppd][eig_ppd][eig_ppd/2+1][4] doubles; NULL/0 unless qPLT.
 *   cb may be NULL: planes are then produced in HBM and dropped (benchmark sink). */
int zd_generate(const zd_params *p, const zd_pk *pk, const double *eig, int64_t eig_ppd, zd_slab_cb cb,
                void *user, zd_stats *out);

/* Smallest stream factor R (a power of two; composite PPDs: any even divisor with a supported z length) whose block store of one pass (+ the y->x ring of the field store, + the exchange
 * ring for nranks > 1) fits in budget_bytes; -1 if none. */
int zd_choose_stream_factor(const zd_params *p, int nranks, int64_t budget_bytes);
/* How `ngpu` GPUs share the job (zd_params.pass_groups, 0 = automatic): *groups independent groups of ngpu / *groups ranks
 * and the stream factor *stream_factor whose number of passes is a multiple of *groups (budget_bytes: free HBM per rank, as
 * for zd_choose_stream_factor).  zd_generate applies it; one-process-per-GPU drivers call it so that every rank arrives at
 * the same split.  Returns non-zero if nothing fits. */
int zd_choose_pass_groups(const zd_params *p, int ngpu, int64_t budget_bytes, int32_t *groups, int32_t *stream_factor);
/* The same with a MEASURED link rate (zd_comm_probe: GB/s one link carries per direction while every link of a GPU works; <= 0 = not
 * measured, i.e. zd_choose_pass_groups).  Where the automatic choice would be one GPU per pass group (no exchange), the time of a
 * step is estimated for both splits from the per-particle unit times of one MI355X (generation, z FFT, y + x stages)
 * and the exchange's bytes per link at that rate, and the single group with the all-to-all (block store transposed between the z and
 * the y / x passes, the reference's StoreBlock / LoadBlock: src/block_array.cpp:387-414,466-504) is taken when it comes out faster —
 * about 45 GB/s per link at PPD = 4096 on 8 GPUs.  est_seconds (may be NULL): [0] pass groups, [1] all-to-all. */
int zd_choose_pass_groups_measured(const zd_params *p, int ngpu, int64_t budget_bytes, double link_GBps, int32_t *groups,
                                   int32_t *stream_factor, double *est_seconds);

/* ---- staged API (device pointers) for one-process-per-GPU drivers and for tests ---------------
 * Rank `rank` of `nranks` (a power of two) owns the half-space rows ky = rank, rank + nranks, ... (H = ppd/2/nranks
 * of them; cyclic, because the rows near ky = 0 carry most of the non-zero modes), plus their Hermitian twins,
 * during the Z stage, and z planes [rank*Zq, (rank+1)*Zq) of every residue
 * pass (Zq = ppd/R/nranks) during the XY stage.  Between the two, the caller exchanges equal
 * chunks (all-to-all): chunk d of the send buffer goes to rank d and is received as chunk `rank`…
 * of the receive buffer (exactly torch.distributed.all_to_all_single / ncclAllToAll semantics).
 * With nranks == 1 the send buffer IS the receive buffer.
 * ZD_f_NL != 0 (one rank): zd_plan_create runs the phi round of the reference (src/zeldovich.cpp:945-960) once and the plan
 * keeps PhiK; its Z stages then read D = PhiK * M.  On several ranks zd_generate (ZD_NumGPU) runs the phi round across them —
 * powers of two up to 4096 and the composite sizes whose lines have composite transforms — each rank keeping PhiK of its rows
 * (PPD^3 / (2 G) complex). */
typedef struct zd_plan zd_plan;

int zd_plan_create(const zd_params *p, const zd_pk *pk, const double *eig, int64_t eig_ppd, int rank,
                   int nranks, zd_plan **out);
void zd_plan_destroy(zd_plan *plan);

int32_t zd_plan_narray(const zd_plan *plan);       /* arrays of the store: 1, 2 or 4 (src/zeldovich.cpp:871-876), or 3:
                                                     * without ZD_qdensity the density field is not transformed and the
                                                     * remaining 3 (ZA) / 6 (PLT) real fields are packed into 3 arrays —
                                                     * ZA packs TWO z-residues per pass (qy+i qz of each, qx_r0 + i qx_r1),
                                                     * PLT packs qx+i vx | qy+i qz | vy+i vz; density_variance then comes
                                                     * from sum |D(k)|^2 (Parseval) */
int32_t zd_plan_store_mode(const zd_plan *plan);   /* ZD_STORE_REFERENCE / _PACKED / _FIELDS: what the store of this plan holds */
int32_t zd_plan_stream_factor(const zd_plan *plan);/* R: z-residue classes */
int32_t zd_plan_passes(const zd_plan *plan);       /* passes per run: R, or R/2 when a pass carries two residues */
int32_t zd_plan_plane_step(const zd_plan *plan);   /* 1, or 2 when a pass carries two residues: stage_x plane ranges
                                                     * must be multiples of it */
int32_t zd_plan_record_size(const zd_plan *plan);  /* bytes per particle record */
int64_t zd_plan_exchange_bytes(const zd_plan *plan); /* bytes of the send (= receive) buffer per pass */
int64_t zd_plan_local_planes(const zd_plan *plan);   /* Zq: z planes this rank finishes per pass */
int64_t zd_plan_plane_z(const zd_plan *plan, int residue, int64_t local_plane); /* global z */

/* Z stage for residue pass `residue`: mode generation (or cache reuse) + folded z FFT for the rows
 * this rank owns, written into `d_send` (device pointer, zd_plan_exchange_bytes). */
int zd_plan_stage_z(zd_plan *plan, int residue, void *d_send, void *hip_stream);

/* XY stage: in-place y FFT on `d_recv`, then x FFT + particle epilogue for local planes
 * [plane0, plane0+nplanes).  d_records: nplanes*ppd*ppd records; d_density: float32 or NULL.
 * Call zd_plan_stage_x ONCE per plane and pass: for the PPDs that run as convolutions (neither 2^a nor 2^a 3^b) the x transform
 * of a plane is done in place in `d_recv`.  ZD_qPLT with ZD_qdensity = 1 on a 2^a 3^b grid (one rank) keeps the density planes of
 * ONE pass inside the plan: only the pass of the most recent zd_plan_stage_z can deliver d_density; asking another pass for it
 * fails (its records, with d_density NULL, can still be taken from its own store). */
int zd_plan_stage_y(zd_plan *plan, void *d_recv, void *hip_stream);
int zd_plan_stage_x(zd_plan *plan, int residue, const void *d_recv, int64_t plane0, int64_t nplanes,
                    void *d_records, float *d_density, void *hip_stream);

/* ---- N > 1 ranks: exchange + pipelined XY stages inside the library --------------------------------
 * Replaces the per-block StoreBlock / LoadBlock traffic of src/zeldovich.cpp:583-587,634-637 between ZeldovichZ and
 * ZeldovichXY.  The send store is [destination rank][plane]...: plane groups of every chunk are contiguous, group j+1
 * travels (RCCL grouped ncclSend/ncclRecv over xGMI) while the y and x stages of group j run.  zd_generate with
 * zd_params.ngpu > 1 (`ZD_NumGPU` in the parameter file) drives all of this with one host thread per GPU; the entry
 * points below serve one-process-per-GPU drivers (bench.py under torch.distributed.run). */
typedef struct zd_comm zd_comm;
int zd_comm_unique_id(void *id128);  /* rank 0: 128-byte RCCL id, to be made known to all ranks by the launcher */
int zd_comm_create(int rank, int nranks, const void *id128, zd_comm **out); /* ncclCommInitRank on the current device */
void zd_comm_destroy(zd_comm *comm);
/* A rank that cannot go on (failed allocation, consumer error, ...) calls this before returning its error: ncclCommAbort on
 * its communicator, so that the send / receive kernels it has already queued drain instead of spinning on peers for ever.
 * zd_plan_run_pass does it by itself on every failure path; the launcher is expected to stop the other ranks when one
 * process exits non-zero (torch.distributed.run does). */
void zd_comm_abort(zd_comm *comm);
/* bytes this rank has sent to / received from other ranks since the communicator was created (or since the last call with
 * reset != 0) */
void zd_comm_traffic(zd_comm *comm, int64_t *bytes_sent, int64_t *bytes_received, int reset);
/* timed probe of the links: bytes_per_peer to and from every peer at once (grouped send / receive), one warm-up + reps repetitions;
 * *GBps_per_peer = what one link carries per direction meanwhile (0: no peers).  Every rank of the communicator calls it. */
int zd_comm_probe(zd_comm *comm, int64_t bytes_per_peer, int32_t reps, double *GBps_per_peer);
/* bytes of the two-slot receive ring zd_plan_run_pass allocates (0 for one rank) and the planes per exchange group */
int64_t zd_plan_ring_bytes(const zd_plan *plan, int32_t *group_planes);
/* consumer of finished planes: `nplanes` delivered planes starting at local plane `first_local_plane` of the pass lie
 * in d_records, produced by work still queued on hip_stream (order yourself after it, or synchronise) */
typedef int (*zd_group_cb)(void *user, int64_t first_local_plane, int64_t nplanes, const void *d_records, void *hip_stream);
/* One residue pass of this rank: Z stage into d_store (zd_plan_exchange_bytes), exchange and XY stages plane group by
 * plane group through d_records (room for rec_planes planes, a multiple of zd_plan_plane_step).  comm == NULL for one
 * rank.  cb may be NULL (benchmark sink). */
int zd_plan_run_pass(zd_plan *plan, zd_comm *comm, int pass, void *d_store, void *d_records, int64_t rec_planes,
                     zd_group_cb cb, void *user, void *hip_stream);

/* The passes first, first + step, ... of this rank (step = number of pass groups, first = this rank's group) in one call.
 * d_store2 (optional, as large as d_store): with a communicator of several ranks the passes are then PIPELINED — the Z stage of
 * the next pass runs into the other store while the planes of the current pass are exchanged and transformed; a store is
 * rewritten only after its sends have completed.  With ONE rank (comm == NULL) and a second store the Z stage of the next pass is
 * issued beside the y / x stages of the current one (measured slower than one store at PPD=4096 on an MI355X — DESIGN.md §8 —
 * and therefore not what zd_generate does; kept for A/B runs, bench.py --two-stores).  cb additionally receives the pass. */
typedef int (*zd_pass_cb)(void *user, int pass, int64_t first_local_plane, int64_t nplanes, const void *d_records, void *hip_stream);
int zd_plan_run_passes(zd_plan *plan, zd_comm *comm, int first, int step, void *d_store, void *d_store2, void *d_records,
                       int64_t rec_planes, zd_pass_cb cb, void *user, void *hip_stream);

/* Fetch + reset the device-side reductions (max_disp, density_variance) and kernel timers. Syncs. */
int zd_plan_stats(zd_plan *plan, zd_stats *out);

/* ---- host-side helpers mirroring the reference's setup code (no GPU needed) -------------------- */
/* Parameters(file) + setup(): src/parameters.cpp:11-197.  Fills zd_params; strings via out buffers. */
typedef struct zd_param_strings {
    char Pk_filename[1024];
    char output_dir[1024];
    char density_filename[1024];
    char PLT_filename[1024];
    char ICFormat[64];
    double Pk_scale, Pk_norm, Pk_sigma, Pk_sigma_ratio, Pk_smooth, Pk_powerlaw_index;
    int32_t qPk_fix_to_mean;
    int32_t version;
    double f_NL, n_s, Omega_M;
    int64_t np;
    char Pk_measured_filename[1024]; /* ZD_Pk_measured_filename (optional, not in the reference): the CLI writes the band-power table there */
    /* ZD_SelfCheck = n (optional, not in the reference; 0 < n <= 64, default 0 = off): after the run the CLI compares the records it
     * delivered at n lattice sites with zd_direct_sum and exits 1 if max |record - direct sum| / max|q| exceeds SelfCheck_tol
     * (ZD_SelfCheck_tol; default 1e-10 for the float64 formats, 1e-6 for the float32 ones); ZD_SelfCheck_filename: the site list
     * with both sets of values.  Refused by the reader together with what zd_direct_sum refuses, and with ZD_f_NL */
    double SelfCheck_tol;
    int32_t SelfCheck;
    char SelfCheck_filename[1024];
    /* ZD_PLT_compute_ppd = n (optional, not in the reference): with ZD_qPLT = 1 the CLI computes the eigenmode table of n points per
     * side on the GPU (zd_make_eigenmodes) instead of loading ZD_PLT_filename; exactly one of the two must be given, and n must be one
     * zd_make_eigenmodes accepts.  The member fills what was the padding at the end of the struct: its size is unchanged.
     * (ZD_PLT_write_filename, the file the CLI writes the table it used to, is read with zd_param_file_string.) */
    int32_t PLT_compute_ppd;
} zd_param_strings;
int zd_params_from_file(const char *path, zd_params *p, zd_param_strings *s);
/* The string a parameter file assigns to `key`, unquoted, into value[cap]; "" if the file does not assign it.  Non-zero (message) if the
 * file cannot be read or the string does not fit.  For optional keys that have no member in zd_param_strings (ZD_PLT_write_filename). */
int zd_param_file_string(const char *path, const char *key, char *value, int64_t cap);

/* PowerSpectrum: InitFromFile / InitFromPowerLaw + Normalize.  The handle owns the tables that
 * zd_pk points into. */
typedef struct zd_pk_handle zd_pk_handle;
int zd_pk_create_from_file(const char *path, double Pk_scale, double Pk_norm, double Pk_sigma,
                           double Pk_sigma_ratio, double Pk_smooth, int fix_to_mean, double boxsize,
                           zd_pk_handle **h, zd_pk *pk);
int zd_pk_create_powerlaw(double index, double Pk_norm, double Pk_sigma, double Pk_sigma_ratio,
                          double Pk_smooth, int fix_to_mean, double boxsize, zd_pk_handle **h, zd_pk *pk);
double zd_pk_power(const zd_pk *pk, double k);  /* PowerSpectrum::power, src/power_spectrum.cpp:225 */
double zd_pk_sigmaR(const zd_pk *pk, double R); /* PowerSpectrum::sigmaR, src/power_spectrum.cpp:60 */
void zd_pk_destroy(zd_pk_handle *h);

/* load_eigmodes: src/zeldovich.cpp:794-830.  Caller frees with zd_free. */
int zd_load_eigmodes(const char *path, double **eig, int64_t *eig_ppd);
void zd_free(void *p);
/* The inverse of zd_load_eigmodes: an int32 n followed by the n * n * (n/2 + 1) * 4 doubles of eig (no GPU needed).  A computed table
 * can then feed the reference program or a later run. */
int zd_write_eigmodes(const char *path, const double *eig, int64_t n);

/* ---- the PLT eigenmode table, computed ---------------------------------------------------------
 * Fills the HOST array eig[n][n][n/2 + 1][4] = (e_x, e_y, e_z, lambda) with the eigenmode table of the simple cubic lattice under
 * periodic gravity (Marcos et al. 2006): per wavevector the dynamical matrix as an Ewald sum and the most longitudinal eigenmode; the
 * definition is pinned in csrc/zd_kernels_plt.hip.  This is the table zd_generate takes as eig / eig_ppd = n; a run whose PPD is a
 * multiple of n reads it directly, any other interpolates (src/zeldovich.cpp:149-276).  n: even, in [4, ZD_PLT_MAX_PPD]; anything else
 * is refused (message, non-zero) before the array or the GPU is touched.  Two calls return the same bits. */
#define ZD_PLT_MAX_PPD 512
int zd_make_eigenmodes(int64_t n, double *eig);

/* ---- band power of the realised modes ---------------------------------------------------------
 * One sweep over the modes a run generates (no transform, no store) that bins instead of storing; the definition is pinned in
 * csrc/zd_kernels_pk.hip.  Bin b holds the modes with (b w)^2 <= kx^2 + ky^2 + kz^2 < ((b + 1) w)^2 (signed integer wavenumbers,
 * w = bin_width >= 1 fundamentals); zd_power_nbins = the number of bins that hold the whole cube (no GPU needed; 0 for invalid
 * arguments).  The sums run over all ppd^3 wavevectors, Hermitian pairs counted twice, restricted to the modes the zero rule
 * leaves alive, k = 0 excluded.  Outputs are HOST arrays of nbins >= zd_power_nbins entries:
 *   count      modes of the bin (exact)            sum_k      sum |k| fundamental
 *   sum_dens   sum |D(k)|^2                        sum_input  sum zd_pk_power(|k|)  (= <|D|^2>; with ZD_qPk_fix_to_mean |D|^2 itself)
 *   sum_disp   sum_j |q_j(k)|^2                    sum_vel    sum_j |v_j(k)|^2  (ZA: vnorm^2 sum_disp; PLT: its own field, rescale included)
 * zd_plan_measure_power measures the rows of this rank (ky = rank mod nranks): the sums of the ranks add up to the whole; a ZD_f_NL
 * plan measures D = PhiK M of its own PhiK.  The call returns when the sums are in the arrays.  zd_measure_power is the one-call
 * form on a one-rank plan.  Refused (message, non-zero): configurations whose Nyquist-plane modes stay alive (ZD_CornerModes with
 * ZD_k_cutoff != 1), ZD_Version = 1 and q2LPT plans (the sweep regenerates the first-order modes only). */
int64_t zd_power_nbins(int64_t ppd, int32_t bin_width);
int zd_plan_measure_power(zd_plan *plan, int32_t bin_width, int64_t nbins, int64_t *count, double *sum_k, double *sum_dens,
                          double *sum_input, double *sum_disp, double *sum_vel, void *hip_stream);
int zd_measure_power(const zd_params *p, const zd_pk *pk, const double *eig, int64_t eig_ppd, int32_t bin_width, int64_t nbins,
                     int64_t *count, double *sum_k, double *sum_dens, double *sum_input, double *sum_disp, double *sum_vel);

/* ---- direct summation at sample sites ----------------------------------------------------------
 * The same sweep accumulating F(k) e^{2 pi i k.x / ppd} at up to 64 lattice sites instead of binning: a check of the delivered records
 * that is independent of the stores, the fold, the transform passes, the packing and the epilogue, at any size and option; the
 * definition is pinned in csrc/zd_kernels_ds.hip.  sites_zyx: HOST array of nsites x (z, y, x), each in [0, ppd); out7: HOST array of
 * nsites x 7 doubles = qx, qy, qz, vx, vy, vz, density — what an RVdoubleZel run with ZD_qdensity = 1 delivers at those sites (formats
 * without velocities or runs without density simply ignore those columns).  zd_plan_direct_sum sums the rows of this rank (ky = rank
 * mod nranks): the results of the ranks add up to the whole; a ZD_f_NL plan uses its own PhiK.  The call returns when the sums are in
 * out7; two calls on one plan return the same bits.  zd_direct_sum is the one-call form on a one-rank plan.  Refused (message,
 * non-zero): configurations whose Nyquist-plane modes stay alive (ZD_CornerModes with ZD_k_cutoff != 1), ZD_Version = 1, q2LPT plans,
 * a site outside the lattice, nsites < 1 or > 64, NULL arrays. */
int zd_plan_direct_sum(zd_plan *plan, int64_t nsites, const int64_t *sites_zyx, double *out7, void *hip_stream);
int zd_direct_sum(const zd_params *p, const zd_pk *pk, const double *eig, int64_t eig_ppd, int64_t nsites, const int64_t *sites_zyx,
                  double *out7);

/* ---- ZD_q2LPT / ZD_q3LPT plans: direct summation and band power of the three orders ------------
 * An LPT plan keeps the spectra of its higher orders resident (S(k); with ZD_q3LPT also P3(k) and C_x,y,z(k)), and a delivered record
 * is the unnormalised inverse transform of amplitudes that are linear in them; the definition is pinned in
 * csrc/zd_kernels_lpt_ds.hip.  The sums pin the final pass of an LPT run — generator, z, y, x stages, epilogue, any stream factor —
 * and take the spectra as the plan holds them: they do not check the second- and third-order rounds.
 * (A ZD_qonemode plan is a single plane wave, which has no higher order: orders 2 and 3 are zero there, exactly.)
 *   zd_plan_lpt_direct_sum   sites_zyx as for zd_plan_direct_sum; out18: HOST array of nsites x 3 orders x (qx, qy, qz, vx, vy, vz):
 *                            order 1 (the ZA field, velocities alpha q), order 2, order 3 (zero without ZD_q3LPT).  The delivered
 *                            record is the sum over the orders.  Two calls on one plan return the same bits.
 *   zd_plan_lpt_power        bins and counting of zd_plan_measure_power; sums8: HOST array of nbins x (sum_k, sum_input, sum_dens,
 *                            sum_disp1, sum_disp2, sum_disp3, sum_disp, sum_vel): the displacement power of each order alone, then of
 *                            the delivered displacement and velocity (the sums over the orders, cross terms included).
 * zd_lpt_direct_sum and zd_lpt_power are the one-call forms: they create the plan, rounds included.  Refused (message, non-zero), before
 * a plan or the GPU is touched where possible: parameters without ZD_q2LPT = 1, whatever a ZD_q2LPT / ZD_2LPT_dealias / ZD_q3LPT plan
 * refuses, nsites < 1 or > 64, a site outside the lattice, bin_width < 1, nbins < zd_power_nbins, NULL arrays. */
int zd_plan_lpt_direct_sum(zd_plan *plan, int64_t nsites, const int64_t *sites_zyx, double *out18, void *hip_stream);
int zd_lpt_direct_sum(const zd_params *p, const zd_pk *pk, int64_t nsites, const int64_t *sites_zyx, double *out18);
int zd_plan_lpt_power(zd_plan *plan, int32_t bin_width, int64_t nbins, int64_t *count, double *sums8, void *hip_stream);
int zd_lpt_power(const zd_params *p, const zd_pk *pk, int32_t bin_width, int64_t nbins, int64_t *count, double *sums8);

/* ---- glass and other off-lattice particle loads: the delivered field at arbitrary positions ----
 * Displacements and velocities for particles that do not sit on the PPD^3 lattice (a glass, a tiled glass, BCC / FCC lattices, a
 * resampled region), by interpolating the delivered records; the definition is pinned in csrc/zd_kernels_glass.hip.  A pure consumer
 * of delivered planes: every configuration that delivers records is served, and the records are the plan's own (units, vnorm, PLT and
 * LPT content unchanged).
 *   positions  pos_xyz: HOST array of npart x (x, y, z) float64 in box units, every coordinate in [0, 1) (x: the fastest index of the
 *              records, z: the plane index); anything else, NaN included, is refused before the GPU is touched
 *   order      1: trilinear over the 2^3 surrounding sites; 3: cubic Lagrange over 4^3 sites (it interpolates: at a lattice site the
 *              result is the record itself)
 *   results    out6: HOST array of npart x (qx, qy, qz, vx, vy, vz) float64, in the order of the positions; formats without velocities
 *              (Zeldovich, ZelSimple) leave exact zeros in the velocity columns.  Sums are float64 whatever the record format, every
 *              particle is owned by one thread (no floating-point atomics): two runs return the same bits.
 * Accuracy is the caller's choice through oversampling: a run at PPD = m N with ZD_k_cutoff = m holds the band-limited field of the
 * PPD = N run sampled m times as finely, and the interpolation converges to the exact field as m grows.  No window is divided out.
 *
 * The consumer object, for any driver that has device planes: create it for a load, add every plane z in [0, ppd) once, in any order
 * (d_plane_records: DEVICE pointer to the ppd * ppd records of plane z in the layout of `icformat`, complete by the time work queued
 * on hip_stream runs; the launches are ordered by that stream), take the result.  About 80 bytes of HBM per particle.  Misuse — a
 * plane added twice, z outside [0, ppd), a result asked for while planes are missing, NULL arguments — prints one line and returns
 * non-zero.  The object does not care where a plane comes from, so a one-process-per-GPU driver can use it: each rank keeps an object
 * for a share of the PARTICLES and shows it every plane, its own and the ones its peers deliver.  zd_displace below drives one GPU. */
typedef struct zd_interp zd_interp;
int zd_interp_create(int64_t ppd, int32_t icformat, int32_t order, int64_t npart, const double *pos_xyz, zd_interp **out);
int zd_interp_add_plane(zd_interp *it, int64_t z, const void *d_plane_records, void *hip_stream);
int zd_interp_result(zd_interp *it, double *out6);
void zd_interp_destroy(zd_interp *it);
/* Every pass of a one-rank plan into the object (store and record buffers of its own, as zd_generate allocates them; each plane's z
 * from zd_plan_plane_z).  Returns when the planes' work is done.  Refused: plans of several ranks, plans that deliver no records
 * (ZD_qdensity = 2), an object made for another ppd or ICFormat. */
int zd_plan_interp(zd_plan *plan, zd_interp *it, void *hip_stream);
/* The one-call form.  The npart * tile^3 particles of the load replicated tile^3 times — particle ((a tile + b) tile + c) npart + i
 * sits at (p_i + (c, b, a)) / tile — are processed in sweeps of at most max_particles_per_sweep (0: as many as fit beside the plan in
 * free HBM); the plan's passes run again for every sweep (the draws are counter-addressed: regeneration is what the library does
 * anyway), and after each sweep cb receives first_particle, n and the HOST array out6 of n x 6 results, valid during the call (non-zero
 * return aborts).  A 2048^3-particle tiled glass therefore needs neither a host array nor HBM for all of its particles.  out (may be
 * NULL): the statistics of the last sweep's run, seconds_total = the whole call.  Refused with one line that names the argument, before
 * a plan or the GPU is touched: order not 1 or 3, npart < 1, tile < 1, NULL pointers, a position outside [0, 1), ZD_qoneslab >= 0,
 * ZD_qdensity = 2 (no records are delivered), ngpu > 1.  ZD_qdensity = 1 is accepted; the density plane is ignored. */
typedef int (*zd_particle_cb)(void *user, int64_t first_particle, int64_t n, const double *out6);
int zd_displace(const zd_params *p, const zd_pk *pk, const double *eig, int64_t eig_ppd, int32_t order, int64_t npart, const double *pos_xyz,
                int64_t tile, int64_t max_particles_per_sweep, zd_particle_cb cb, void *user, zd_stats *out);

/* ---- a caller-supplied density or white-noise field instead of ZD_Seed ---------------------------
 * The phases of a run come from a field the caller hands over — a white-noise cube shared with another code, a constrained
 * realisation, a field sampled by an inference chain, the density file an earlier ZD_qdensity = 1 run wrote — instead of the
 * counter-addressed draws; the definition is pinned in csrc/zd_kernels_field.hip.
 *   field     a real field a[z][y][x], ppd points per side, C-contiguous, float32 or float64 (dtype), a HOST pointer or, with
 *             field_on_device != 0, a DEVICE pointer (read where it lies, not copied; a host field is uploaded in chunks of planes)
 *   kind      ZD_FIELD_DENSITY: the linear density delta in the run's own units (what ZD_qdensity = 1 delivers):
 *                 D(k) = (1 / ppd^3) sum_x a(x) exp(-2 pi i k.x / ppd)
 *             ZD_FIELD_WHITE: unit-variance white noise: D(k) = W(k) sqrt(zd_pk_power(|k|) / ppd^3), W the unnormalised forward
 *                 sum; with <|W|^2> = ppd^3 this is <|D|^2> = power(k), the variance of a seeded run
 * D(k) is then cleared by the run's zero rule (src/zeldovich.cpp:350-356): the |k_i| = kmax planes, k^2 >= k^2_cutoff without
 * ZD_CornerModes, ZD_qonemode, k = 0 — and the planes |k_i| = ppd/2, which the rule clears by itself unless ZD_CornerModes meets
 * ZD_k_cutoff != 1.  With ZD_qdensity = 1 the density the run delivers is therefore the imposed field with those modes removed;
 * displacements and velocities are what the path makes of these D(k), exactly as if the draws had produced them (eigenmode direction,
 * f of the eigenvalue and the rescale under PLT, vnorm under ZA).  ZD_Seed is ignored; no draw is made.
 * The intake (three transform stages of its own) holds D(k) of the half space, 8 ppd^3 bytes, which the plan then owns, plus a workspace
 * of at most 256 MB (4 planes at ppd = 2048); the plan runs on the reference's arrays at any stream factor they take.
 * zd_plan_create_field creates a one-rank plan: the stage calls, zd_plan_run_passes, zd_plan_stats, zd_plan_interp, zd_plan_direct_sum and
 * zd_plan_measure_power work on it as on any plan.  zd_generate_field is the one-call form with zd_generate's callback.
 * Accepted: ppd a power of two in [32, 2048], one GPU; ZA, ZD_qPLT with or without ZD_qPLT_rescale; every ICFormat; ZD_qdensity 0 / 1 / 2;
 * ZD_k_cutoff, ZD_CornerModes, ZD_qonemode, ZD_f_cluster, ZD_qoneslab; any stream factor.  Refused before the GPU is touched, with one line
 * that starts "zeldovich_hip: ZD_Field" and names the other option: ZD_f_NL != 0, ZD_q2LPT / ZD_q3LPT, ZD_Version = 1,
 * ZD_qPk_fix_to_mean, ZD_NumGPU > 1, any other ppd, an unknown kind or dtype, a NULL field.  A job that does not fit is refused with
 * the byte figure in the message. */
enum { ZD_FIELD_DENSITY = 0, ZD_FIELD_WHITE = 1 };
enum { ZD_FIELD_F32 = 0, ZD_FIELD_F64 = 1 };
int zd_plan_create_field(const zd_params *p, const zd_pk *pk, const double *eig, int64_t eig_ppd, int32_t kind, int32_t dtype,
                         const void *field, int32_t field_on_device, zd_plan **out);
int zd_generate_field(const zd_params *p, const zd_pk *pk, const double *eig, int64_t eig_ppd, int32_t kind, int32_t dtype,
                      const void *field, int32_t field_on_device, zd_slab_cb cb, void *user, zd_stats *out);

/* ---- second order (2LPT) on a caller-supplied field: the order is an argument of the field call ------
 * Definition (pinned in csrc/zd_kernels_lpt2_field.hip).  Start from D(k), the modes of the supplied field exactly as a first-order field
 * run holds them (the intake above: zero rule, 1 / ppd^3 or the white-noise amplitude, the |k_i| = ppd/2 planes cleared), and apply steps
 * 1 - 5 of the DEFINITION in csrc/zd_kernels_lpt2.hip unchanged: gradients -k_a k_b D / k^2, S(x) on the ppd^3 lattice without
 * de-aliasing, S(k) = ppd^-3 x the forward sum times the alive mask with S(0) = 0, positions from D + gamma S, velocities from
 * alpha D + f2 gamma S; gamma = -lpt2_ratio, alpha and f2 resolved from lpt2_ratio, lpt2_f2 and f_cluster of the parameters as for
 * ZD_q2LPT.  It is the seeded ZD_q2LPT run with "D drawn from its counter" replaced by "D read from the field".  ZD_Seed is ignored.
 *   order   1: exactly zd_generate_field / zd_plan_create_field without an eigenmode table;  2: the above;  anything else is refused
 *           (3: third order on a field is not built).
 * The parameters come with q2LPT = q3LPT = lpt2_dealias = 0 (otherwise the refusal of a field run, in its words); inside, an order-2 job
 * runs as the q2LPT job it is, on the reference's four arrays at any stream factor, and the plan's parameters read back q2LPT = 1.
 * Accepted with order = 2: ppd a power of two in [32, 1024] (2048: the second-order round alone would hold ~275 GB), one GPU, ZA, every
 * ICFormat, ZD_k_cutoff, ZD_qonemode, ZD_f_cluster, ZD_qoneslab.  Refused with one line that starts "zeldovich_hip: ZD_Field" and names
 * the option: everything a field run refuses, and everything ZD_q2LPT refuses (ZD_qPLT, ZD_f_NL, a density output, ZD_Version = 1, live
 * Nyquist planes, several GPUs).  Memory: D(k) (8 ppd^3 bytes) stays resident through the round, whose peak is therefore ~32 ppd^3
 * bytes; afterwards D(k) and S(k) (16 ppd^3 bytes) sit beside the store of a pass; both belong to the plan.  A job that does not fit
 * is refused with the byte figure.  zd_plan_lpt_direct_sum and zd_plan_lpt_power work on such a plan (order 1 read from D, order 2 from
 * S); zd_plan_direct_sum and zd_plan_measure_power refuse it as they refuse every second-order plan; the stage calls,
 * zd_plan_run_passes, zd_plan_stats and zd_plan_interp work as on any plan.  zd_field_vjp is the adjoint of order 1 only. */
int zd_plan_create_field_lpt(const zd_params *p, const zd_pk *pk, int32_t kind, int32_t dtype, const void *field, int32_t field_on_device,
                             int32_t order, zd_plan **out);
int zd_generate_field_lpt(const zd_params *p, const zd_pk *pk, int32_t kind, int32_t dtype, const void *field, int32_t field_on_device,
                          int32_t order, zd_slab_cb cb, void *user, zd_stats *out);

/* ---- adjoint of a field run: the gradient with respect to the supplied field ------------------------
 * What a chain over the initial field needs beside the run itself: the vector-Jacobian product abar = J^T (dL/dq, dL/dv, dL/ddens) of a
 * scalar loss L.  The definition is pinned in csrc/zd_kernels_field_adj.hip.  All arrays are [z][y][x], components in the order of
 * the records' d / v members (q_z, q_y, q_x), fftn the forward sum (exp(-i)), N = ppd.  The forward map of a field run is linear:
 *     D(k) = alive(k) A(|k|^2) fftn(a)(k)       A = 1 / N^3 (ZD_FIELD_DENSITY) or sqrt(zd_pk_power(|k|) / N^3) (ZD_FIELD_WHITE)
 *     q_j  = N^3 ifftn(i s_j D).real            v_j = N^3 ifftn(i f s_j D).real            delivered density = N^3 ifftn(D).real
 * alive is the zero rule of a field run (above), asked on the half space the path reads (ky > 0; on ky = 0: kz > 0; on ky = kz = 0:
 * kx > 0) and mirrored; s_j(k) and f(k) are the generator's per-mode coefficients:
 *     ZA    s_j = k_j fundamental / k^2,            f = (sqrt(1 + 24 f_cluster) - 1) / 4
 *     PLT   s_j = rescale e_j fundamental / k^2,    f = (sqrt(1 + 24 e_3 f_cluster) - 1) / 4, the eigenmode of a mode of that half space
 *           from its own lookup; the mirrored half from s(-k) = -s(k), f(-k) = f(k)
 * The adjoint takes three real cotangents, each optional (NULL = an exact zero): g_q[z][y][x][3], g_v[z][y][x][3], g_dens[z][y][x], all of
 * one dtype (ZD_FIELD_F32 / _F64), all on the host or (cot_on_device != 0) all on the device, and writes
 *     H(k) = alive(k) A(|k|^2) [ sum_j conj(i s_j(k)) ( fftn(g_q,j)(k) + f(k) fftn(g_v,j)(k) ) + fftn(g_dens)(k) ]
 *     abar = N^3 ifftn(H).real                  float64 [z][y][x] into out_field (a device pointer with out_on_device != 0)
 * so that <q, g_q> + <v, g_v> + <dens, g_dens> = <a, abar> for every field a.  The call is stateless (the Jacobian does not depend on a:
 * no plan, no PhiK).  These enter exactly as in a field run: ZD_qPLT, ZD_qPLT_rescale, PLT_target_z, z_initial, ZD_f_cluster, ZD_k_cutoff,
 * ZD_CornerModes, ZD_qonemode, ZD_one_mode, the box, the power spectrum (white only) and the eigenmode table.  These do not:
 * ZD_Seed, ICFormat, ZD_qdensity, ZD_qoneslab, the stream factor, the store mode — it is the adjoint of the exact float64 map, whatever
 * format a forward run would round its records to.  No floating-point atomics: two calls return the same bits.
 * Memory: two half-space arrays of 8 ppd^3 bytes (one when the result lies on the device: its storage serves as the second until the
 * inverse writes it), the intake's workspace, staging buffers of as many planes for host arrays; a job that does not fit is refused
 * with the byte figure.  Refused before the GPU is touched, each with one line that starts
 * "zeldovich_hip: ZD_Field" and names the option: what zd_generate_field refuses, all three cotangents NULL, ZD_qPLT without a table.
 * stats (may be NULL): seconds_total and bytes_intermediate of the call. */
int zd_field_vjp(const zd_params *p, const zd_pk *pk, const double *eig, int64_t eig_ppd, int32_t kind, int32_t dtype, const void *g_q,
                 const void *g_v, const void *g_dens, int32_t cot_on_device, double *out_field, int32_t out_on_device, zd_stats *stats);

/* ---- diagnostics ------------------------------------------------------------------------------
 * Which kernel variants this process has launched so far, and how often: one line "count<TAB>line<TAB>launcher" per launch
 * site of the library, the launcher named with its template arguments (transform length, elements per thread, tile shape,
 * packing).  Writes at most cap - 1 bytes + a terminating 0 into buf (may be NULL) and returns the size a complete report
 * needs.  (The reference logs its FFTW plan sizes at start-up, src/zeldovich.cpp:39-135; here the variant depends on PPD,
 * store and stream factor, and the test-suite uses this report to prove that every variant it ships has been exercised.) */
int64_t zd_dispatch_report(char *buf, int64_t cap);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
