// zd_route.h — where routing lives: zd::route() maps (canonical parameters, stream factor, ranks, role) to the kernel family and the
// shape of the store that plan creation (zd_capi.cpp plan_create_one) builds and that the choosers (zd_choose_stream_factor,
// zd_choose_pass_groups) size.  Host only: no HIP call, no allocation; the environment only through tune_env (-DZD_TUNING).
#pragma once
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>

#include "../../include/zeldovich_hip.h"
#include "zd_device.h"
#include "zd_launch.h"
#include "zd_tables.h"

// Tuning / ablation knobs (environment variables ZD_ABLATE, ZD_PRUNE, ZD_NT, ZD_LAYOUT, ...) exist only in the
// -DZD_TUNING build (make tuning -> build/libzeldovich_hip_tuning.so, used by scripts/ through ZD_LIB_PATH).
// The product library never reads the environment: the names do not even reach its binary.  (Global, macro in the product: this
// header is for the zd_capi*.cpp units, and for zd_kernels_lpt_ds.hip, which asks the LPT refusals and coefficients.)
#ifdef ZD_TUNING
static inline const char *tune_env(const char *name) { return getenv(name); }
#else
#define tune_env(name) ((const char *) nullptr)
#endif

namespace zd {

inline bool is_pow2(int64_t n) { return n > 0 && (n & (n - 1)) == 0; }

// Four kernel families:
//   FAM_POW2           PPD = 2^a: the power-of-two engine (zd_kernels.hip), every store
//   FAM_COMPOSITE      PPD = 2^a 3^b 5^c 7^d of the kernel table: composite-transform kernels, field stores only (zd_kernels_np2.hip)
//   FAM_REF_COMPOSITE  ZD_f_NL on such a grid: the reference's arrays, every line through the composite transforms of
//                      zd_kernels_np2_ref.hip (the second pass keeps the Nyquist modes live, so the Hermitian field stores cannot
//                      carry it); several ranks split the arrays (AnyChunks)
//   FAM_CONVOLUTION    any other even PPD — or a composite one with options the composite kernels lack: the reference's arrays, one
//                      rank, the lines as convolutions on the power-of-two engine (zd_kernels_any.hip); R any divisor of PPD
enum { FAM_POW2 = 0, FAM_COMPOSITE = 1, FAM_REF_COMPOSITE = 2, FAM_CONVOLUTION = 3 };
// what a plan is for: the main pass, the first f_NL pass (one array holding phi = D/M), the second (D = PhiK * M), the gradient
// passes of the second-order round (one array holding two gradient fields of the ZA displacement; zd_kernels_lpt2.hip)
enum { ROLE_MAIN = 0, ROLE_PHI = 1, ROLE_PHIK = 2, ROLE_LPT2_GRAD = 3 };

struct Route {
    int family = FAM_POW2, pack = PACK_NONE, narray = 0, pstep = 1, npass = 1, R = 1, L = 0, Hq = 0, Zq = 0;
    bool dens = false;       // ZD_qdensity on the six-field ZA store (composite grids)
    bool dens_only = false;  // ZD_qdensity = 2 there: density planes only: no displacement arrays, no records (src/output.cpp:94,207)
    bool twr = false;        // reference arrays: the lines use the composite twiddles (else Bluestein tables)
    // The shape above is filled whatever is refused.  `legal`: family, stream factor, ranks and store take this job — what the
    // choosers ask; `why`: the first refusal in the order plan creation reports them ("" = none), which may also name an argument of
    // plan creation alone (eigenmode table, rank index, ZD_Version)
    bool legal = true;
    char why[320] = "";
    bool ok() const { return why[0] == 0; }
    void refuse(bool routing, const char *fmt, ...) {
        va_list ap;
        va_start(ap, fmt);
        if (!why[0]) vsnprintf(why, sizeof why, fmt, ap);
        va_end(ap);
        legal = legal && !routing;
    }
};

// ZD_qdensity = 2 (density only): the displacement arrays are never built (src/zeldovich.cpp:303,440), so the eigenmodes of ZD_qPLT
// never enter — the run IS the ZA density-only run, on every grid and path
inline zd_params canonical(const zd_params *p) {
    zd_params c = *p;
    if (c.qdensity == 2) c.qPLT = c.qPLTrescale = 0;
    return c;
}

// a composite PPD whose options (no f_NL, no ZD_qoneslab, store auto / fields) the composite kernels have
inline bool composite_options(const zd_params *p) {
    return p->f_NL == 0. && p->qoneslab < 0 && !is_pow2(p->ppd) && np2_supported_ppd((int) p->ppd)
           && (p->store_mode == ZD_STORE_AUTO || p->store_mode == ZD_STORE_FIELDS);
}
// ZD_qdensity = 1 on the composite grids (round 4): the ZA field store carries two more half-space sums — the density D of the two
// residues of a pass — and the y / x stages add one array, delta_r0 + i delta_r1 (zd_kernels_np2.hip).  The power-of-two grids keep
// the reference's arrays for ZD_qdensity (their kernels exist).  8640 = 64 * 135 included (tests/test_gpu_baseline_regime.py).
// ZD_qdensity = 2 (round 5): the same six-field store, the displacement arrays are simply not built and no records are written; the
// four potentials ride along unused, which still beats the convolution path by ~4x.
inline bool dens_fields(const zd_params *p) { return (p->qdensity == 1 || p->qdensity == 2) && !p->qPLT && composite_options(p); }
// PLT with ZD_qdensity = 1 on the composite grids, one rank (round 5): the PLT field store has no density field and its paired
// generator no registers for a seventh pair of sums, so the density planes come from a second plan — density only, ZA six-field
// store (dens_only) — at stream factor 2R: its pass j holds the residues j and j + R, i.e. exactly the planes z = j (mod R) of this
// plan's pass j, in the same delivery order.  It runs at the head of the Z stage on the same store (which the PLT pass then
// overwrites) and leaves N/R planes of float32 behind.  Before: the ~6x slower convolution path.
inline bool plt_dens_split(const zd_params *p, int nranks) {
    return p->qPLT && p->qdensity == 1 && nranks == 1 && composite_options(p) && !tune_env("ZD_NO_DENS_SPLIT");
}

// The largest wavenumber per axis that the zero rule keeps (zeldovich.cpp:350-353), and whether the rule leaves every mode with a
// component on the Nyquist plane |k_i| = N/2 at zero: the |k_i| == kmax rule does it when kmax == N/2 (k_cutoff = 1), the spherical cut
// when k_cutoff >= 1 and CornerModes is off.  Otherwise (e.g. CornerModes with k_cutoff = 2) the reference keeps independent,
// non-Hermitian draws there and takes Re/Im of the mixed field (zeldovich.cpp:350-356).
inline int kmax(int half, double k_cutoff) { return (int) ((double) half * (1.0 / k_cutoff) + .5); }
inline bool nyquist_dead(const zd_params *p) {
    const int half = (int) (p->ppd / 2);
    return kmax(half, p->k_cutoff) == half || (!p->corner_modes && p->k_cutoff >= 1.0);
}

// Second-order displacements (zd_params.q2LPT; definition in zd_kernels_lpt2.hip).  The second-order round keeps the whole field
// resident on one GPU, on the power-of-two engine, with the counter streams of ZD_Version 2; the final pass fills the reference's
// four arrays (the PLT shape: velocities are a field of their own), which carry no eigenmodes, no f_NL and no density output here.
// Live Nyquist planes (ZD_CornerModes with ZD_k_cutoff != 1) are not Hermitian: the source would not be real.  NULL: accepted.
inline const char *lpt2_refusal(const zd_params *p, int nranks) {
    if (!p->q2LPT) return nullptr;
    if (p->q2LPT != 1) return "ZD_q2LPT must be 0 or 1";
    if (p->qPLT) return "ZD_q2LPT = 1 is not supported together with ZD_qPLT";
    if (p->f_NL != 0.) return "ZD_q2LPT = 1 is not supported together with ZD_f_NL != 0";
    if (p->qdensity != 0) return "ZD_q2LPT = 1 is not supported together with a density output (ZD_qdensity)";
    if (p->version == 1) return "ZD_q2LPT = 1 needs the counter streams of ZD_Version = 2";
    if (nranks != 1 || p->ngpu > 1) return "ZD_q2LPT = 1 runs on one GPU (one rank)";
    if (!is_pow2(p->ppd) || p->ppd < 32 || p->ppd > 2048) return "ZD_q2LPT = 1 needs PPD a power of two in [32, 2048]";
    if (!nyquist_dead(p)) return "ZD_q2LPT = 1 is not supported with live Nyquist planes (ZD_CornerModes with ZD_k_cutoff != 1)";
    return nullptr;
}
// ZD_2LPT_dealias (zd_params.lpt2_dealias; step 2' of the definition, zd_kernels_lpt2.hip): the second-order round on the lattice of
// M = 3 PPD / 2 points per side, every line through the composite transforms of zd_kernels_np2_ref.hip (zd_kernels_lpt2q.hip).  The
// corner rule decided on that lattice would keep modes beyond the PPD cube.  NULL: accepted (asked after lpt2_refusal).
inline int64_t lpt2_dealias_lattice(int64_t N) { return 3 * N / 2; }
inline const char *lpt2_dealias_refusal(const zd_params *p) {
    if (!p->lpt2_dealias) return nullptr;
    if (p->lpt2_dealias != 1) return "ZD_2LPT_dealias must be 0 or 1";
    if (p->q2LPT != 1) return "ZD_2LPT_dealias = 1 needs ZD_q2LPT = 1";
    if (p->corner_modes) return "ZD_2LPT_dealias = 1 is not supported together with ZD_CornerModes";
    if (p->ppd % 2 || !refq_supported_len((int) lpt2_dealias_lattice(p->ppd)))
        return "ZD_2LPT_dealias = 1 needs a PPD whose 3 PPD / 2 has a composite line transform";
    return nullptr;
}
// its coefficients: alpha = vnorm of the f_cluster background (src/output.cpp:78-82); D2 / D1^2 and f2 as given, 0 = that background's
inline double lpt2_alpha(const zd_params *p) { return (sqrt(1. + 24 * p->f_cluster) - 1) * .25; }
inline double lpt2_ratio(const zd_params *p) { return p->lpt2_ratio != 0. ? p->lpt2_ratio : -(2 * lpt2_alpha(p) + 1) / (6 * lpt2_alpha(p) + 1); }
inline double lpt2_f2(const zd_params *p) { return p->lpt2_f2 != 0. ? p->lpt2_f2 : 2 * lpt2_alpha(p); }

// Third-order displacements (zd_params.q3LPT; definition in zd_kernels_lpt3.hip) ride on the second order: whatever lpt2_refusal refuses
// is refused before this is asked.  The cubic term of a de-aliased round would need the lattice of 2 PPD points per side; the round
// holds twelve real fields beside its store and S(k), 120 PPD^3 bytes; the default coefficients are those of the f_cluster = 1
// background.  NULL: accepted.
inline bool lpt3_term(const zd_params *p, int bit) { return ((p->lpt3_terms ? p->lpt3_terms : 7) & bit) != 0; }
inline const char *lpt3_refusal(const zd_params *p) {
    if (!p->q3LPT) return nullptr;
    if (p->q3LPT != 1) return "ZD_q3LPT must be 0 or 1";
    if (p->q2LPT != 1) return "ZD_q3LPT = 1 needs ZD_q2LPT = 1";
    if (p->lpt3_terms < 0 || p->lpt3_terms > 7) return "ZD_q3LPT = 1 takes ZD_3LPT_terms in 0 ... 7 (bit 1 = 3a, bit 2 = 3b, bit 4 = 3c)";
    if (p->lpt2_dealias) return "ZD_q3LPT = 1 is not supported together with ZD_2LPT_dealias = 1 (its cubic term would need the lattice of 2 PPD)";
    if (p->ppd > 1024) return "ZD_q3LPT = 1 needs PPD <= 1024 (the third-order round holds 120 PPD^3 bytes on one GPU)";
    if (p->f_cluster != 1.
        && ((lpt3_term(p, 1) && p->lpt3_g3a == 0.) || (lpt3_term(p, 2) && p->lpt3_g3b == 0.) || (lpt3_term(p, 4) && p->lpt3_g3c == 0.)
            || p->lpt3_f3 == 0.))
        return "ZD_q3LPT = 1 with ZD_f_cluster != 1 needs ZD_3LPT_f3 and the coefficient of every enabled term given (the defaults are "
               "those of f_cluster = 1)";
    return nullptr;
}
// its coefficients as the kernels take them: 0 for a term that is left out, else the given value or the default
inline double lpt3_g3a(const zd_params *p) { return !lpt3_term(p, 1) ? 0. : p->lpt3_g3a != 0. ? p->lpt3_g3a : -1. / 3.; }
inline double lpt3_g3b(const zd_params *p) { return !lpt3_term(p, 2) ? 0. : p->lpt3_g3b != 0. ? p->lpt3_g3b : 10. / 21.; }
inline double lpt3_g3c(const zd_params *p) { return !lpt3_term(p, 4) ? 0. : p->lpt3_g3c != 0. ? p->lpt3_g3c : 1. / 7.; }
inline double lpt3_f3(const zd_params *p) { return p->lpt3_f3 != 0. ? p->lpt3_f3 : 3 * lpt2_alpha(p); }

// reference arrays of a job: density only one (zeldovich.cpp:871-876), PLT — and the second order's own velocity field — four, else two
inline int ref_arrays(const zd_params *p) { return p->qdensity == 2 ? 1 : ((p->qPLT || p->q2LPT) ? 4 : 2); }

// Packed stores (zd_device.h PACK_*) the options ask for: without ZD_qdensity the density field is not transformed.
inline int pack_mode(const zd_params *p, int R) {
    if (p->store_mode == ZD_STORE_REFERENCE || p->q2LPT) return PACK_NONE;  // (second order: the final pass fills the reference's arrays)
    if ((p->qdensity != 0 && !dens_fields(p)) || p->f_NL != 0.) return PACK_NONE;
    if (p->qoneslab >= 0) return PACK_NONE;  // density_variance is then the sum over that one slab (output.cpp:197)
    // The packed stores treat every field as the transform of a REAL field (Hermitian modes) and take density_variance from
    // sum |D|^2.  That needs every mode with a component on the Nyquist plane to be zero (nyquist_dead): reference arrays otherwise.
    if (!nyquist_dead(p)) return PACK_NONE;
    // PLT: the three packed arrays by default; its field store (six half-space sums) only on request — measured slower
    // (PPD=2048 PLT+rescale 0.553 -> 0.609 s: every array of the y stage needs two potentials, each fetched twice, and the
    // 148-VGPR PLT generator leaves no room for the z FFT beside it anyway)
    // (PPD = 8192: the x pass of the packed arrays does not exist — three lines of a row are 1536 threads — so PLT runs on
    // its field store there, whose ring goes through k_xfft_two; ZA: only the field store has an x kernel that takes them in
    // sequence, k_xfft_seq)
    // composite PPD: the composite-transform kernels exist for the field stores only
    if (p->qPLT) return (p->ppd > 4096 || !is_pow2(p->ppd) || p->store_mode == ZD_STORE_FIELDS) ? PACK_PLTFIELD : PACK_PLT3;
    if (R < 2) return PACK_NONE;  // the ZA packings carry two z-residues per pass
    if (p->store_mode == ZD_STORE_PACKED) return p->ppd > 4096 ? PACK_NONE : PACK_ZAPAIR;
    return PACK_ZAFIELD;
}

// stream factors the composite (2^a 3^b 5^c 7^d) kernels take: any EVEN divisor of PPD (two residues r, r + R/2 share a ZA pass) — or
// 1 — whose z lines have a composite transform.  R = 36 gives PPD = 6912 z lines of 192 = 64 * 3 and 18 passes where the powers of two
// offer 64 (z lines of 108) and 32 passes: the store of a pass must fit, and between 128 GB and 260 GB there was nothing.
inline bool np2_stream_factor_ok(int64_t N, int R) {
    return R >= 1 && (R == 1 || R % 2 == 0) && N % R == 0 && np2_supported_zlen((int) (N / R));
}

// ZD_f_NL on a composite grid goes through the composite transforms where both line lengths — N (x, y; the phi round's z) and N / R
// (the z lines of a pass) — have one.  One rank: ZD_StoreMode = reference and ZD_qoneslab keep the convolution transforms, as does
// any stream factor outside fnl_np2_factor_ok.  Several ranks: the arrays split over the ranks (the z lines of a pass must deal out
// over them too) and nothing else — those configurations are refused with the reason given here (NULL: none).
inline const char *fnl_multi_refusal(const zd_params *p) {
    const int64_t N = p->ppd;
    if (is_pow2(N)) return N > 4096 ? "ZD_f_NL != 0 on several GPUs needs PPD <= 4096 on the powers of two" : nullptr;
    if (!np2_supported_ppd((int) N) || !refq_supported_len((int) N))
        return "ZD_f_NL != 0 on several GPUs needs a PPD with composite transforms (2^a 3^b 5^c 7^d of the kernel table); this PPD runs "
               "its lines as convolutions, on one GPU only";
    if (p->store_mode == ZD_STORE_REFERENCE)
        return "ZD_f_NL != 0 with ZD_StoreMode = reference runs the convolution transforms, on one GPU only";
    if (p->qoneslab >= 0) return "ZD_f_NL != 0 with ZD_qoneslab runs the convolution transforms, on one GPU only";
    if (tune_env("ZD_NO_NP2_FNL")) return "ZD_NO_NP2_FNL forces the convolution transforms, which run on one GPU only";
    return nullptr;
}
inline bool fnl_np2_factor_ok(const zd_params *p, int R) {
    return p->f_NL != 0. && !is_pow2(p->ppd) && !fnl_multi_refusal(p) && R >= 1 && p->ppd % R == 0 && refq_supported_len((int) (p->ppd / R));
}

// the next stream factor a family tries after R, and the shortest z line it takes: the powers of two double, the composite kernels
// take the even factors (or 1), the reference's arrays any divisor of PPD (their z-residue fold is a plain decimation)
inline int next_factor(int family, int R) { return family == FAM_POW2 ? 2 * R : family == FAM_COMPOSITE ? (R == 1 ? 2 : R + 2) : R + 1; }
inline int min_zlen(int family) { return family == FAM_POW2 ? 32 : family == FAM_COMPOSITE ? 12 : 3; }
// ... and the shortest a GIVEN stream factor may leave a job on the powers of two: the second-order final pass (its own generator and
// k_zfft on the reference's arrays, zd_kernels_lpt2.hip) also runs z lines of 16 points — one thread per line —, e.g. PPD = 64 at
// stream factor 4; every other job keeps 32 (the generators and field-store z transforms of zd_kernels.hip start there)
inline int given_min_zlen(const zd_params *p, int role) { return p->q2LPT && role == ROLE_MAIN ? 16 : min_zlen(FAM_POW2); }

// route_shape: family, store and shape of a job with the refusals that are arithmetic on the parameters; route() below adds the one
// that asks the dispatch tables.
// R <= 0: no factor given — plan creation's default (the first one whose z lines the composite kernels have, else 1).  rank and
// have_eig take part in plan creation's refusals only.
inline Route route_shape(const zd_params *p, int R_given, int nranks, int role, int rank = 0, bool have_eig = true) {
    Route r;
    const int64_t N = p->ppd;
    const int G = nranks < 1 ? 1 : nranks;
    const bool pow2 = is_pow2(N), main = role == ROLE_MAIN;
    int R = R_given > 0 ? R_given : 1;
    // (the plan of the second-order round's gradient passes belongs to a job that was asked as ROLE_MAIN before; with ZD_2LPT_dealias it
    // sits on the 3 PPD / 2 lattice, on the reference's arrays with the composite transforms)
    const bool grad = role == ROLE_LPT2_GRAD;
    if (!grad) {
        if (const char *why = lpt2_refusal(p, nranks)) r.refuse(true, "%s", why);
        if (const char *why = lpt2_dealias_refusal(p)) r.refuse(true, "%s", why);
        if (const char *why = lpt3_refusal(p)) r.refuse(true, "%s", why);
    }
    bool comp = false;
    if (!pow2) {
        int Rg = R_given > 0 ? R_given : 2;
        for (int c = 2; R_given <= 0 && N / c >= min_zlen(FAM_COMPOSITE); c += 2)
            if (np2_stream_factor_ok(N, c)) {
                Rg = c;
                break;
            }
        // the field stores deal row blocks of FIELD_RB rows to every rank
        comp = np2_supported_ppd((int) N) && main && np2_stream_factor_ok(N, Rg) && pack_is_fields(pack_mode(p, Rg))
               && (N / 2) % (G * FIELD_RB) == 0;
        if (comp) R = Rg;
    }
    r.twr    = !comp && (fnl_np2_factor_ok(p, R) || (grad && !pow2 && R == 1 && refq_supported_len((int) N)));
    r.family = pow2 ? FAM_POW2 : comp ? FAM_COMPOSITE : r.twr ? FAM_REF_COMPOSITE : FAM_CONVOLUTION;
    const bool any = !pow2 && !comp;
    if (pow2 && (N < 32 || N > 16384)) r.refuse(true, "PPD = %lld unsupported (powers of two: 32 ... 16384)", (long long) N);
    if (p->qPLT && !have_eig) r.refuse(false, "ZD_qPLT set but no eigenmode table given");
    if (any && nranks > 1 && p->f_NL != 0.) {  // ZD_f_NL on a composite grid, the arrays split over the ranks (AnyChunks)
        if (const char *why = fnl_multi_refusal(p)) r.refuse(true, "%s", why);
        else if (!(r.twr && (N / R) % G == 0 && (N / 2) % G == 0))
            r.refuse(true, "ZD_f_NL on %d ranks at PPD = %lld: stream factor %d has no composite z lines of length PPD / R dividing over the "
                           "ranks", nranks, (long long) N, R);
    } else if (any) {
        if (N % 2 || N < 8 || N > 8192 || nranks != 1 || R < 1 || N % R || N / R < min_zlen(FAM_CONVOLUTION))
            r.refuse(true, "PPD = %lld (neither 2^a nor a supported 2^a 3^b configuration) runs as convolutions on the power-of-two engine: "
                           "even PPD in [8, 8192], one rank, ZD_StreamFactor any divisor of PPD (got %d)", (long long) N, R);
    } else if (comp ? !np2_stream_factor_ok(N, R) : (!is_pow2(R) || N % R || N / R < given_min_zlen(p, role) || N / R > 4096)) {
        r.refuse(true, "stream factor %d invalid for PPD %lld", R, (long long) N);  // (z-FFT kernels exist up to length 4096)
    }
    const bool no_split = nranks < 1 || !is_pow2(nranks) || (N / 2) % G || (N / R) % G;
    if (no_split || rank < 0 || rank >= nranks)
        r.refuse(no_split, "cannot split PPD %lld (R=%d) over %d ranks (a power of two dividing PPD/2 and PPD/R is required)", (long long) N, R,
                 nranks);
    // legacy mt19937 streams, one per yres (power_spectrum.cpp:18-25); the second f_NL pass takes D from PhiK and draws nothing
    if (p->version != 0 && p->version != 1 && p->version != 2) r.refuse(false, "ZD_Version = %d (1 or 2 expected)", p->version);
    if (p->version == 1 && role != ROLE_PHIK && (p->numblock <= 0 || N % p->numblock || (N / p->numblock) % G))
        r.refuse(false, "ZD_Version = 1 needs ZD_NumBlock dividing PPD and PPD/NumBlock streams divisible by the number of ranks (%d)", nranks);
    // (density only rides on the six-field ZA store of the composite kernels; everywhere else it is one array)
    r.narray = (role == ROLE_PHI || role == ROLE_LPT2_GRAD) ? 1 : (p->qdensity == 2 && !any && dens_fields(p)) ? 2 : ref_arrays(p);
    if (main && r.narray >= 2 && !any) r.pack = pack_mode(p, R);
    // the field stores need row blocks of FIELD_RB rows per rank and a z FFT <= 2048; PPD > 4096 has no other store worth using
    if (pack_is_fields(r.pack) && (((N / 2) / G) % FIELD_RB || N / R > 2048))
        r.pack = N > 4096 ? PACK_NONE : (r.pack == PACK_PLTFIELD ? PACK_PLT3 : PACK_ZAPAIR);
    // a 16384-point line fills a workgroup: only the field store's kernels exist (also 8640 = 64 * 135: ZA)
    if (N > 8192 && r.pack != PACK_ZAFIELD)
        r.refuse(true, "PPD = %lld runs on the ZA field store only (ZD_StreamFactor >= 16; no ZD_qPLT / ZD_f_NL / ZD_qdensity = 2; "
                       "ZD_qdensity = 1 on the composite grid 8640 only)", (long long) N);
    // (launch_xfft_t would say so only after the Z and y stages of the first pass had run)
    if (r.pack == PACK_NONE && pow2 && (int64_t) r.narray * (N / 16) > 1024)
        r.refuse(true, "PPD = %lld on the reference's %d arrays (PLT with ZD_qdensity, ZD_f_NL or ZD_StoreMode = reference) has no x pass: the "
                       "lines of a row are %lld threads", (long long) N, r.narray, (long long) r.narray * (N / 16));
    if (r.pack != PACK_NONE) r.narray = 3;
    r.dens      = r.pack == PACK_ZAFIELD && dens_fields(p);
    r.dens_only = r.dens && p->qdensity == 2;
    r.pstep     = (r.pack == PACK_ZAPAIR || r.pack == PACK_ZAFIELD) ? 2 : 1;  // the ZA packings deliver two planes per store plane
    r.npass     = R / r.pstep;
    r.R         = R;
    r.L         = (int) (N / R);
    r.Hq        = (int) (N / 2) / G;
    r.Zq        = r.L / G;
    return r;
}

inline Route route(const zd_params *p, int R_given, int nranks, int role, int rank = 0, bool have_eig = true);

// The two halves of a PLT + density run (plt_dens_split) at the PLT half's stream factor R (<= 0: plan creation's default), and
// whether their shapes fit together: the PLT half on its field store, the density half density-only with the same passes and the
// same planes per pass.  (A refusal of either half is not asked here: plan creation then falls back by itself.)
inline bool split_routes(const zd_params *p, int R, zd_params *pa, zd_params *pb, Route *A, Route *B) {
    *pa = *pb          = *p;
    pa->qdensity       = 0;
    *A                 = route(pa, R, 1, ROLE_MAIN);
    pb->qPLT = pb->qPLTrescale = 0;
    pb->qdensity       = 2;
    pb->stream_factor  = 2 * A->R;
    *B                 = route(pb, 2 * A->R, 1, ROLE_MAIN);
    return A->family == FAM_COMPOSITE && A->pack == PACK_PLTFIELD && B->family == FAM_COMPOSITE && B->dens_only
           && B->npass == A->npass && B->pstep == 2 && 2 * B->Zq == A->Zq;
}

// ---- which dispatch table every stage of a job consults, and with which key ----
// One entry per (stage, launcher): the launcher as zd_dispatch_report names its instantiations (a prefix of them: launch_xfft stands
// for launch_xfft_t, _seq_t, _seq_plt_t, _two_t, _q2_plt_t), the key as it appears among their template arguments, and the answer of
// the table's predicate (zd_tables.h).  route_stages restates the selection code of the stages — launch_zstage_fft, fused_stage_z,
// any_stage_z, zd_plan_stage_y_group, zd_plan_stage_x_group, make_phik / zd_plan_phi_xy_group / zd_plan_phi_zfwd, make_lpt2_source,
// make_lpt3_sources (zd_capi_stages.cpp, zd_capi_rounds.cpp) — for the plan that plan_create_one builds from a Route; tests/test_gpu_route_edges.py holds it to what
// a run really launches.  Not listed: the generators (launch_gen takes every z line that is a multiple of 4, which every accepted
// family's are, and any length on the reference's arrays) and kernels without a size table (scatter, emit, pointwise).
struct StageKey {
    char stage[56], launcher[32], key[48];
    bool present;
};
struct StageList {
    enum { MAX = 48 };
    int n = 0;
    StageKey s[MAX];
    void add(const char *prefix, const char *stage, const char *launcher, bool present, const char *fmt, ...) {
        if (n >= MAX) return;
        StageKey &k = s[n++];
        snprintf(k.stage, sizeof k.stage, "%s%s", prefix, stage);
        snprintf(k.launcher, sizeof k.launcher, "%s", launcher);
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(k.key, sizeof k.key, fmt, ap);
        va_end(ap);
        k.present = present;
    }
    const StageKey *first_missing() const {
        for (int i = 0; i < n; i++)
            if (!s[i].present) return &s[i];
        return nullptr;
    }
};

// Fused Z stage of the packed PLT store (zd_kernels_fz.hip: generator + z FFT in one kernel), as far as parameters and route decide it:
// the packed store by the store mode's own choice, one rank with the rows of a plane in one block, z lines the kernel has, version-2
// streams, the whole field, the main pass, and a dead kz = N/2 plane that the cut — not the corner rule alone — leaves dead (the
// kernel never draws it).  plan_block_layout adds what only the plan knows (the table generator, every prune bit).  `pack` is
// PACK_PLT3 only on a main-role plan without ZD_q2LPT, so the other roles and a PhiK never get past the first term.
inline bool fused_z_route(const zd_params *p, int pack, int N, int L, int role, bool one_block) {
    return pack == PACK_PLT3 && p->store_mode == ZD_STORE_AUTO && one_block && genz_plt_supported(N, L) && p->version != 1
           && p->qoneslab < 0 && role == ROLE_MAIN && p->k_cutoff >= 1.0 && nyquist_dead(p) && !tune_env("ZD_NO_FUSED_Z");
}

// the stages of ONE plan of shape rt (no sub-rounds)
inline void plan_stages(const Route &rt, const zd_params *p, int role, int nranks, const char *prefix, StageList &out) {
    const int N = (int) p->ppd, L = rt.L, G = nranks < 1 ? 1 : nranks;
    const bool phi = role == ROLE_PHI, grad = role == ROLE_LPT2_GRAD;
    if (rt.family >= FAM_REF_COMPOSITE) {  // the reference's arrays: composite transforms (twr) or convolutions
        const bool phi_half = phi && rt.twr && G == 1;  // (make_phik: the z lines straight into half-space planes)
        if (phi_half) out.add(prefix, "z", "launch_refq_cols_oop_t", has_refq_cols_oop(L), "n = %d", L);
        else if (rt.twr) out.add(prefix, "z", "launch_refq_cols_t", has_refq_cols(L), "n = %d", L);
        else out.add(prefix, "z", "launch_any_cols_t", has_any_cols(L), "M = %d", any_engine_size(L));
        if (phi && G > 1) {  // zd_plan_phi_xy_group, zd_plan_phi_zfwd
            out.add(prefix, "phi y", "launch_refq_ycols_t", has_refq_ycols(N), "n = %d", N);
            out.add(prefix, "phi x", "launch_refq_xphi_t", has_refq_xphi(N), "n = %d", N);
            out.add(prefix, "phi z", "launch_refq_cols_oop_t", has_refq_cols_oop(N), "n = %d", N);
            return;
        }
        if (phi_half) {
            out.add(prefix, "phi x", "launch_refq_lines_t", has_refq_lines(N), "n = %d", N);
            out.add(prefix, "phi y", "launch_refq_yphi_t", has_refq_yphi(N), "n = %d", N);
            out.add(prefix, "phi z", "launch_refq_cols_oop_t", has_refq_cols_oop(N), "n = %d", N);
            return;
        }
        if (G > 1) out.add(prefix, "y", "launch_refq_ycols_t", has_refq_ycols(N), "n = %d", N);
        else if (rt.twr) out.add(prefix, "y", "launch_refq_cols_t", has_refq_cols(N), "n = %d", N);
        else out.add(prefix, "y", "launch_any_cols_t", has_any_cols(N), "M = %d", any_engine_size(N));
        if (grad) {  // the de-aliased second-order round on this lattice (make_lpt2_source): N is the lattice, 2 N / 3 the PPD
            out.add(prefix, "x", "launch_lpt2q_xsrc_t", has_lpt2q_xsrc(N), "n = %d", N);
            out.add(prefix, "source y", "launch_refq_cols_t", has_refq_cols(N), "n = %d", N);
            out.add(prefix, "source z", "launch_lpt2q_zsrc_t", has_lpt2q_zsrc(N, 2 * N / 3), "n = %d", N);
            return;
        }
        // x lines: of the main pass, or of the phi round on one rank (x, the 3-D transform back: lines, y columns, z columns)
        if (rt.twr || G > 1) out.add(prefix, phi ? "phi x" : "x", "launch_refq_lines_t", has_refq_lines(N), "n = %d", N);
        else out.add(prefix, phi ? "phi x" : "x", "launch_any_lines_t", has_any_lines(N), "M = %d", any_engine_size(N));
        return;
    }
    // slabs of the field stores are whole row blocks (plan_slabs) where the rows of a rank are (the route demotes the store otherwise)
    const int nky = rt.Hq % FIELD_RB ? rt.Hq : FIELD_RB;
    if (rt.family == FAM_COMPOSITE) {
        out.add(prefix, "z", "launch_zfft_fq_t", has_zfft_fields_np2(L, nky), "L = %d", L);
        if (!rt.dens_only) {
            out.add(prefix, "y", "launch_yfft_fq_t", has_yfft_fields_np2(N), "N = %d", N);
            out.add(prefix, "x", "launch_xfft_q_t", has_xfft_np2(N, rt.pack == PACK_PLTFIELD ? PACK_PLT3 : rt.pack), "N = %d, PLT = %s", N,
                    rt.pack == PACK_PLTFIELD ? "true" : "false");
        }
        if (rt.dens) {
            out.add(prefix, "density y", "launch_yfft_fq_t", has_yfft_fields_np2(N), "N = %d", N);
            out.add(prefix, "density x", "launch_xdens_q_t", has_xdens_np2(N), "N = %d", N);
        }
        return;
    }
    // the power-of-two engine
    const int one_block = G == 1 ? 1 : 0;  // (plan_block_layout: one rank keeps self and twin slots of a plane in one block)
    if (pack_is_fields(rt.pack)) {
        out.add(prefix, "z", "launch_zfft_f_t", has_zfft_fields(L, nky), "L = %d,", L);
        out.add(prefix, "y", "launch_yfft_f_t", has_yfft_fields(N, rt.Hq), "N = %d,", N);
        // the ring between the y and x stages: three arrays of a single-rank store, PLT3 order for the PLT field store
        out.add(prefix, "x", "launch_xfft", has_xfft(N, 3, rt.pack == PACK_PLTFIELD ? PACK_PLT3 : rt.pack, 0, 1), "N = %d,", N);
        return;
    }
    out.add(prefix, "z", "launch_zfft_t", has_zfft(L), "L = %d,", L);
    {   // the fused generator + z FFT of the packed PLT store (plan_block_layout) where the power table allows it (at most 512 spline
        // segments): plane-interleaved rows, 4 planes; the two-kernel stage on plain rows otherwise — a job needs both
        if (fused_z_route(p, rt.pack, N, L, role, one_block != 0)) {
            out.add(prefix, "z fused", "launch_genz_t", genz_plt_supported(N, L), "L = %d, R = %d,", L, rt.R);
            out.add(prefix, "y fused", "launch_yfft_t", has_yfft(N, 2, one_block, rt.Zq), "N = %d,", N);
            out.add(prefix, "x fused", "launch_xfft", has_xfft(N, rt.narray, rt.pack, 2, one_block), "N = %d,", N);
        }
    }
    out.add(prefix, "y", "launch_yfft_t", has_yfft(N, 0, one_block, rt.Zq), "N = %d,", N);
    if (phi) {  // make_phik / zd_plan_phi_xy_group, zd_plan_phi_zfwd: x (inverse, phi + f_NL phi^2, forward), y, z
        out.add(prefix, "phi x y z", "launch_fnl_t", has_fnl_stage(N), "N = %d,", N);
        return;
    }
    if (grad) {  // make_lpt2_source; make_lpt3_sources runs a plan of the same kind
        out.add(prefix, "x", "launch_lpt2_xsrc_t", has_lpt2_xsrc(N), "N = %d,", N);
        out.add(prefix, "source y z", "launch_fnl_t", has_fnl_stage(N), "N = %d,", N);
        if (p->q3LPT) {
            out.add(prefix, "third order x", "launch_lpt3_xpair_t", has_lpt3_xpair(N), "N = %d,", N);
            out.add(prefix, "third order source x", "launch_lpt3_xfwd_t", has_lpt3_xfwd(N), "N = %d,", N);
        }
        return;
    }
    out.add(prefix, "x", "launch_xfft", has_xfft(N, rt.narray, rt.pack, 0, one_block), "N = %d,", N);
}

// every stage of the job (p canonical): the plan of shape rt, the rounds that run before its first pass — the f_NL phi round, the
// second- and third-order rounds — and the density half of a PLT + density run on a composite grid.  A round whose own route is
// refused is listed with the stage "... route" and the refusal as its key.
inline void route_stages(const Route &rt, const zd_params *p, int R_given, int role, int nranks, StageList &out) {
    if (role != ROLE_MAIN) {
        plan_stages(rt, p, role, nranks, "", out);
        return;
    }
    auto round = [&](const zd_params &pp, int r_role, int r_ranks, const char *prefix) {
        const Route rr = route(&pp, 1, r_ranks, r_role);
        const int n0   = out.n;
        plan_stages(rr, &pp, r_role, r_ranks, prefix, out);
        bool missing = false;
        for (int i = n0; i < out.n; i++) missing = missing || !out.s[i].present;
        if (!rr.legal && !missing) out.add(prefix, "route", "route", false, "%.47s", rr.why);
    };
    if (p->f_NL != 0.) {  // make_phik (one rank) / zd_plan_create_phi (several): stream factor 1, no eigenmodes
        zd_params pp     = *p;
        pp.stream_factor = 1;
        pp.qPLT          = 0;
        round(pp, ROLE_PHI, nranks, "phi round: ");
    }
    if (p->q2LPT) {  // make_lpt2_source (with ZD_2LPT_dealias: a plan at the lattice of 3 PPD / 2), make_lpt3_sources
        zd_params pp     = *p;
        pp.stream_factor = 1;
        pp.qoneslab      = -1;
        if (p->lpt2_dealias) {
            pp.ppd          = lpt2_dealias_lattice(p->ppd);
            pp.k_cutoff     = p->k_cutoff * 1.5;
            pp.nyquist      = p->nyquist * 1.5;
            pp.lpt2_dealias = 0;
        }
        round(pp, ROLE_LPT2_GRAD, 1, "second-order round: ");
    }
    zd_params pa, pb;
    Route A, B;
    if (plt_dens_split(p, nranks) && split_routes(p, R_given, &pa, &pb, &A, &B) && A.ok() && B.ok()) {
        plan_stages(A, &pa, role, nranks, "", out);  // (plan_create_ex: the two halves; this route is the fall-back)
        plan_stages(B, &pb, role, nranks, "density half: ", out);
        return;
    }
    plan_stages(rt, p, role, nranks, "", out);
}

// The route of a job: its shape, and where nothing else refuses it, whether every stage has a kernel.  A job whose stages lack one is
// refused here, at plan creation, with the stage and the key named: the launch would otherwise fail with the step half issued.
inline Route route(const zd_params *p, int R_given, int nranks, int role, int rank, bool have_eig) {
    Route r = route_shape(p, R_given, nranks, role, rank, have_eig);
    if (!r.legal) return r;
    StageList st;
    route_stages(r, p, R_given, role, nranks, st);
    if (const StageKey *k = st.first_missing())
        r.refuse(true, "PPD = %lld: no kernel for the %s stage of this job (%s, %s): it is refused at plan creation", (long long) p->ppd,
                 k->stage, k->launcher, k->key);
    return r;
}

}  // namespace zd
