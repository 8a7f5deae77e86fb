// zd_capi_sizing.cpp — what a job's stores and rounds take in memory, and the two choosers built on it (zd_choose_stream_factor,
// zd_choose_pass_groups).  Host arithmetic on the parameters and zd::route only: no HIP call.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "zd_capi.h"

// Rows of the block store are N*16 B apart: at PPD >= 2048 that is a multiple of 32 KB and the strided accesses of
// the y pass pile onto a few HBM channels (PPD=4096: k_yfft 1.20 s -> 0.92 s with the pad, PPD=2048: 100 -> 93 ms).
// 384 B of padding per row de-aliases them (128 B and 640 B do as well; 256 B does not at PPD=2048) for 0.6-5 % more memory.
int store_row_pad(int64_t N) { return N >= 512 ? 24 : 0; }

// the zero rule of zeldovich.cpp:350-353 as the kernels prune by it (zd_device.h column_is_zero)
static void prune_rule(const zd_params *p, zd::StoreLayout &S) {
    const int half = (int) (p->ppd / 2);
    S.N         = (int) p->ppd;
    S.half      = half;
    S.prune     = 7;
    S.kmax      = zd::kmax(half, p->k_cutoff);
    S.fund2     = p->fundamental * p->fundamental;
    S.k2_cutoff = p->corner_modes ? 0.0 : p->nyquist * p->nyquist / (p->k_cutoff * p->k_cutoff);  // CornerModes: only |k_i| == kmax prunes
}

// Block table of the field store (zd_device.h FieldLayout) for `nranks` ranks: block b stands for the row slots 8b .. 8b+7
// (rows ky = c + nranks*slot) of every rank c and is sized by the longest of them (ky = nranks*8b).  Returns the elements
// per (plane, field) image.
int64_t field_rows(const zd_params *p, int nranks, std::vector<zd::FieldRow> *rows) {
    zd::StoreLayout S;
    memset(&S, 0, sizeof(S));
    prune_rule(p, S);
    const int N = S.N, half = S.half, Hq = half / nranks, CW = zd::FIELD_CW, NT = std::max(1, N / CW), RB = zd::FIELD_RB;
    const int nblk = (Hq + RB - 1) / RB;
    int64_t total = 0;
    if (rows) rows->resize(nblk);
    for (int i = 0; i < nblk; i++) {
        const int ky = i * RB * nranks;
        // live columns are kx in (-c, c): tiles [0, tl) on the low side, [th, NT) on the high side
        int tl = 0, th = NT;
        if (N >= 2 * CW) {
            while (tl < NT) {  // tile tl holds a live column?
                bool live = false;
                for (int x = tl * CW; x < (tl + 1) * CW && !live; x++) live = !zd::column_is_zero(S, x > half ? x - N : x, ky);
                if (!live) break;
                tl++;
            }
            while (th > tl) {
                bool live = false;
                for (int x = (th - 1) * CW; x < th * CW && !live; x++) live = !zd::column_is_zero(S, x > half ? x - N : x, ky);
                if (!live) break;
                th--;
            }
            // a live tile strictly between dead ones cannot happen for the symmetric interval rule, but the table must be
            // safe for any rule: if one exists, keep the whole row
            for (int tt = tl; tt < th; tt++)
                for (int x = tt * CW; x < (tt + 1) * CW; x++)
                    if (!zd::column_is_zero(S, x > half ? x - N : x, ky)) { tl = NT; th = NT; }
        } else {
            tl = NT;
        }
        zd::FieldRow r;
        r.base  = (int) total;
        r.split = (unsigned short) (tl >= th ? N : tl * CW);
        r.gap   = (unsigned short) (tl >= th ? 0 : (th - tl) * CW);
        if (rows) (*rows)[i] = r;
        // 384 B of padding per row as in the other stores: the first ~N/11 rows are complete (64 KiB apart at PPD = 4096)
        total += (int64_t) (N - r.gap + store_row_pad(N)) * RB;
    }
    return total;
}

// bytes of the block store one rank holds per pass (send side; nranks > 1 doubles it with the receive buffer).  Priced for the store the
// options ask for (pack_mode), also where the route demotes it or is refused: a finding (tests/test_route_agreement.py), kept
static int64_t store_bytes(const zd_params *p, int R, int nranks) {
    const int64_t N = p->ppd;
    const int pm = zd::pack_mode(p, R);
    if (zd::pack_is_fields(pm)) return (N / R) * (pm == zd::PACK_PLTFIELD || zd::dens_fields(p) ? 6 : 4) * field_rows(p, nranks, nullptr) * 16;
    return N * (N + store_row_pad(N)) * (N / R) / nranks * 16 * (pm != zd::PACK_NONE ? 3 : zd::ref_arrays(p));
}
// ring between the y and x stages of the field store: planes of the three PACK_ZAPAIR arrays
int field_ring_planes(int64_t N, int64_t Zq) {
    const int64_t plane_b = 3 * N * (N + store_row_pad(N)) * 16;
    return (int) std::max<int64_t>(1, std::min<int64_t>(Zq, ((int64_t) 6 << 30) / plane_b));
}

const char *zd_fnl_multi_unsupported(const zd_params *p) { return zd::fnl_multi_refusal(p); }

// ZD_f_NL on a composite grid, several ranks: bytes per rank of the two-slot exchange ring of a store with `narray` arrays and Zq
// planes per chunk (zd_plan_ring_bytes: a plane from every rank is narray N (N + pad) complex, ~4 GB per slot)
static int64_t fnl_multi_ring_bytes(const zd_params *p, int narray, int64_t Zq) {
    const int64_t N = p->ppd, per_plane = (int64_t) narray * N * (N + store_row_pad(N)) * 16;
    int64_t gp = std::max<int64_t>(1, std::min<int64_t>(Zq, ((int64_t) 4 << 30) / per_plane));
    if (p->exchange_planes > 0) gp = std::min<int64_t>(Zq, p->exchange_planes);
    return 2 * per_plane * gp;
}

// ZD_f_NL memory: PhiK (half-space rows, [ky][kz][x]) and the phi round's planes — half-space rows on the composite transforms
// (make_phik), the full store on the convolution ones
int64_t fnl_phik_bytes(int64_t N) { return (N / 2) * N * N * 16; }
static int64_t fnl_phi_bytes(const zd_params *p) {
    const int64_t N = p->ppd;
    return (route(p, 1, 1, zd::ROLE_PHI).twr ? N / 2 : N) * N * (N + store_row_pad(N)) * 16;
}

// ZD_q2LPT memory: the source S(k) (half-space rows, PhiK's layout) stays beside every pass's store; the second-order round before it
// peaks at its one-array store (every plane, self and twin slots) + the real N^3 accumulator, which S(k) then replaces
int64_t lpt2_sk_bytes(int64_t N) { return (N / 2) * N * N * 16; }
// ZD_2LPT_dealias: the same round on the lattice of M = 3 N / 2 points per side, (16 + 8) M^3 = 81 N^3 bytes (+ the row pad)
int64_t lpt2_round_bytes(const zd_params *p) {
    const int64_t M = p->lpt2_dealias ? zd::lpt2_dealias_lattice(p->ppd) : p->ppd;
    return M * M * (M + store_row_pad(M)) * 16 + M * M * M * 8;
}
// second order on a caller-supplied field: D(k) (PhiK, 8 N^3 bytes) stays resident through the round — about 32 N^3 bytes at the peak —
// and beside S(k) afterwards (16 N^3 bytes beside every pass's store)
int64_t field_lpt2_round_bytes(const zd_params *p) { return lpt2_round_bytes(p) + fnl_phik_bytes(p->ppd); }
// ZD_q3LPT memory: P3(k) and C_x,y,z(k) stay beside S(k), 40 N^3 bytes in all; the third-order round before them peaks at its one-array
// store + the twelve real Hessian fields + S(k) = 120 N^3 bytes (+ the row pad), of which the four new spectra then take 32 N^3
int64_t lpt3_round_bytes(int64_t N) { return N * N * (N + store_row_pad(N)) * 16 + 12 * N * N * N * 8 + lpt2_sk_bytes(N); }
static int64_t lpt_resident_bytes(const zd_params *p) { return p->q2LPT ? (p->q3LPT ? 5 : 1) * lpt2_sk_bytes(p->ppd) : 0; }

// the smallest stream factor whose stores fit the budget: first among those the family's own kernels take (power-of-two engine,
// composite kernels on the field stores), then — composite and other even PPDs — on the reference's arrays
static int choose_stream_factor_one(const zd_params *p, int nranks, int64_t budget_bytes) {
    const int64_t N = p->ppd, plane_b = N * (N + store_row_pad(N)) * 16;  // (one array of a plane)
    const int own = is_pow2(N) ? zd::FAM_POW2 : zd::FAM_COMPOSITE;
    // ZA without density: two residues share a pass, so R = 2 is preferred over R = 1 whenever the z FFT is long enough
    const Route r2 = route(p, 2, nranks, zd::ROLE_MAIN);
    if (p->q2LPT && lpt2_round_bytes(p) > budget_bytes) return -1;
    if (p->q3LPT && lpt3_round_bytes(N) > budget_bytes) return -1;
    const int64_t lpt2_resident = lpt_resident_bytes(p);  // (S(k); with the third order also P3(k), C_x,y,z(k))
    for (int R = r2.legal && r2.pstep == 2 ? 2 : 1; N / R >= zd::min_zlen(own); R = zd::next_factor(own, R)) {
        const Route rt = route(p, R, nranks, zd::ROLE_MAIN);
        if (!rt.legal || rt.family != own) continue;
        if (N > 4096 && rt.L > 2048) continue;  // the field store's z FFT stops at 2048 and PPD > 4096 has no other store worth using
        int64_t store = store_bytes(p, R, nranks);
        if (nranks > 1) store += std::min<int64_t>(store, (int64_t) 9 << 30);  // + the two-slot exchange ring (zd_multi.cpp), not a second store
        if (zd::pack_is_fields(zd::pack_mode(p, R)))  // + the y -> x ring (3 arrays; 4 with the density array); priced like the store
            store += (int64_t) field_ring_planes(N, rt.Zq) * (zd::dens_fields(p) ? 4 : 3) * plane_b;
        if (store + lpt2_resident <= budget_bytes) return R;
    }
    if (own == zd::FAM_POW2) return -1;
    // Reference arrays.  ZD_f_NL: PhiK stays beside every pass's store, and the phi round before it holds PhiK and the phi planes —
    // several ranks (the arrays split over them, AnyChunks): everything / G, plus the phi round's and each pass's exchange ring
    int64_t budget = budget_bytes;
    if (p->f_NL != 0.) {
        const int64_t phik = fnl_phik_bytes(N) / nranks;
        if (phik + (nranks > 1 ? N * plane_b / nranks + fnl_multi_ring_bytes(p, 1, N / nranks) : fnl_phi_bytes(p)) > budget) return -1;
        budget -= phik;
    }
    // f_NL on a composite grid: the smallest factor whose z lines the composite transforms take comes first
    for (int fam : {zd::FAM_REF_COMPOSITE, zd::FAM_CONVOLUTION})
        for (int R = 1; N / R >= zd::min_zlen(fam); R = zd::next_factor(fam, R)) {
            const Route rt = route(p, R, nranks, zd::ROLE_MAIN);
            if (!rt.legal || rt.family != fam) continue;
            if (rt.L * rt.narray * plane_b / nranks + (nranks > 1 ? fnl_multi_ring_bytes(p, rt.narray, rt.Zq) : 0) <= budget) return R;
        }
    return -1;
}

int zd_choose_stream_factor(const zd_params *p_in, int nranks, int64_t budget_bytes) {
    const zd_params pc = zd::canonical(p_in);
    if (zd::plt_dens_split(&pc, nranks)) {
        // the PLT half's own choice, with room for what the density half adds: N/R planes of float32, its two rings (3 + 1 arrays of
        // <= 6 GB / 3) and its tables; both R and 2R must have z lines the composite kernels transform
        const int64_t N = pc.ppd;
        for (int R = 1; N / R >= 24; R = zd::next_factor(zd::FAM_COMPOSITE, R)) {
            zd_params pa, pb;
            Route A, B;
            if (!split_routes(&pc, R, &pa, &pb, &A, &B)) continue;
            const int64_t ring = (int64_t) field_ring_planes(N, A.Zq) * N * (N + store_row_pad(N)) * 16;
            const int64_t need = store_bytes(&pa, R, 1) + 3 * ring                                             // the PLT half
                                 + A.L * N * N * 4 + 4 * ring + ((int64_t) 1 << 30);                           // + the density half
            if (need <= budget_bytes) return R;
        }
    }
    return choose_stream_factor_one(&pc, nranks, budget_bytes);
}

// the family whose stream factors the pass groups of a job step through.  One rank runs a job on the reference's arrays (PPD neither
// 2^a nor a composite size whose options the composite kernels have) with any divisor of PPD as R; several GPUs share it as pass groups only
static int group_family(const zd_params *p, int gsz) {
    const bool convolution_job = !zd::plt_dens_split(p, 1) && route(p, 0, 1, zd::ROLE_MAIN).family >= zd::FAM_REF_COMPOSITE;
    return is_pow2(p->ppd) ? zd::FAM_POW2 : (gsz == 1 && convolution_job) ? zd::FAM_CONVOLUTION : zd::FAM_COMPOSITE;
}
static bool group_factor_ok(int fam, int64_t N, int R) {
    return fam == zd::FAM_COMPOSITE ? zd::np2_stream_factor_ok(N, R) : (N % R == 0 && N / R >= zd::min_zlen(fam));
}

int zd_choose_pass_groups(const zd_params *p_in, int ngpu, int64_t budget_bytes, int32_t *groups, int32_t *stream_factor) {
    const zd_params pc = zd::canonical(p_in), *p = &pc;
    const int64_t N = p->ppd;
    if (ngpu < 1) ngpu = 1;
    const char *why = zd::lpt2_refusal(p, ngpu);  // (pass groups included: every GPU would run the second-order round)
    if (!why) why = zd::lpt2_dealias_refusal(p);
    if (!why) why = zd::lpt3_refusal(p);
    if (why) {
        fprintf(stderr, "zeldovich_hip: %s\n", why);
        return 1;
    }
    int g = p->pass_groups;
    if (g < 0 || (g > 0 && ngpu % g)) {
        fprintf(stderr, "zeldovich_hip: ZD_PassGroups = %d does not divide ZD_NumGPU = %d\n", g, ngpu);
        return 1;
    }
    if (p->f_NL != 0.) g = g > 0 ? g : 1;  // the phi round is one collective job
    if (g > 1 && p->f_NL != 0.) {
        fprintf(stderr, "zeldovich_hip: ZD_f_NL != 0 runs as one group of ranks (ZD_PassGroups = 1)\n");
        return 1;
    }
    const bool given = p->stream_factor > 0;
    if (g == 0) {  // automatic: one GPU per group — no exchange — while a single rank's job has, or can be given, that many passes
        g = 1;
        const int R1 = given ? p->stream_factor : zd_choose_stream_factor(p, 1, budget_bytes);
        if (R1 > 0 && ngpu > 1) {
            // A free stream factor may be doubled (smaller stores always fit): every rank then generates the modes once per
            // pass of its own instead of sharing one generation, and nothing travels.  PPD = 4096 ZA on 8 GPUs: R = 8 -> 16,
            // one pass per GPU, 0.36-0.38 s predicted against 0.30-0.33 s for the all-to-all — within the
            // uncertainty of the link rate, and independent of it.  More than one doubling is not worth the generations.
            // (reference arrays: any divisor of PPD is a stream factor there; up to four times the passes it needs)
            const int fam = group_family(p, 1);
            const int Rmax = given ? R1 : fam == zd::FAM_CONVOLUTION ? std::max(4 * R1, 2 * ngpu) : 2 * R1;
            for (int R2 = R1; R2 <= Rmax && N / R2 >= zd::min_zlen(fam); R2 = zd::next_factor(fam, R2)) {
                if (fam == zd::FAM_COMPOSITE && R2 > R1 && R1 % 2) break;  // (an odd R1 only ever stepped to odd factors: kept, a finding)
                if (!group_factor_ok(fam, N, R2)) continue;
                const int npass = route(p, R2, 1, zd::ROLE_MAIN).npass;
                if (npass >= ngpu && npass % ngpu == 0) {
                    g = ngpu;
                    break;
                }
            }
        }
    }
    const int gsz = ngpu / g;
    int R = given ? p->stream_factor : zd_choose_stream_factor(p, gsz, budget_bytes);
    if (R < 0) return 1;
    auto passes = [&](int r) { return route(p, r, gsz, zd::ROLE_MAIN).npass; };
    // Ranks that exchange pipeline their passes (zd_plan_run_passes: Z stage of pass p+1 beside the exchange of pass p, two
    // send stores): give every group at least four passes when the stream factor is free.  A larger factor always fits —
    // the stores shrink — and costs (passes / ranks per group) generations per rank, hidden behind the exchange.
    if (gsz > 1 && !given && is_pow2(N))
        while (passes(R) < 4 * g && N % (2 * R) == 0 && N / (2 * R) >= 256 && (N / (2 * R)) % gsz == 0) R *= 2;
    // the passes must deal out evenly over the groups: a larger stream factor (smaller stores) always fits
    const int fam = group_family(p, gsz);
    while (passes(R) % g) {
        if (given) {
            fprintf(stderr, "zeldovich_hip: ZD_StreamFactor = %d gives %d passes, not a multiple of the %d pass groups\n", R, passes(R), g);
            return 1;
        }
        if (fam == zd::FAM_COMPOSITE && R % 2) return 1;  // (from R = 1 the step was 1 -> 3 -> 5 ...: no even factor found; kept, a finding)
        do R = zd::next_factor(fam, R);
        while (N / R >= zd::min_zlen(fam) && !(group_factor_ok(fam, N, R) && (N / R) % gsz == 0));
        if (N / R < zd::min_zlen(fam)) return 1;
    }
    *groups        = g;
    *stream_factor = R;
    return 0;
}

// The choice with a measured link rate (zd_comm_probe).  Where zd_choose_pass_groups takes one GPU per pass group — nothing
// travels, every GPU generates all the modes once per pass of its own — the single group with the all-to-all is the alternative:
// the ranks share the generations (rows ky = rank mod G), the block store is transposed between the z and the y / x passes
// (src/block_array.cpp:387-414,466-504) in plane groups over every link of a GPU at once, passes pipelined over two send stores.
// Both are priced from unit times of ONE MI355X per particle of the grid (measured, DESIGN.md 4 / 5 — PPD = 4096: ZA a full
// generation 0.141 s, the z FFT beside it +0.185 s / 4 passes... per particle below; PLT from the PPD = 4096 PLT run; composite
// grids: y + x at 1.85x) and the exchange's bytes per link at the measured rate:
//   pass groups:  T = c_gen N^3 P / G + (c_zf + c_xy) N^3 / G                         P passes in all, P / G per GPU
//   all-to-all:   T = t_z / P' + max(t_ex, t_xy + t_z (P' - 1) / P') + 0.05 t_xy      t_z = (c_gen P' + c_zf) N^3 / G, t_xy = c_xy N^3 / G,
//                                                                                     t_ex = store bytes per rank and pass x P' / G / rate
// (first Z stage exposed, the others and the XY stages beside the exchange, the last plane group's XY behind it; P' = 1: t_z + max).
int zd_choose_pass_groups_measured(const zd_params *p_in, int ngpu, int64_t budget_bytes, double link_GBps, int32_t *groups,
                                   int32_t *stream_factor, double *est_seconds) {
    const zd_params pc = zd::canonical(p_in), *p = &pc;
    if (est_seconds) est_seconds[0] = est_seconds[1] = 0.0;
    if (zd_choose_pass_groups(p, ngpu, budget_bytes, groups, stream_factor)) return 1;
    if (!(link_GBps > 0.0) || ngpu < 2 || p->pass_groups != 0 || *groups != ngpu) return 0;  // nothing to decide
    zd_params q   = *p;
    q.pass_groups = 1;
    int32_t g1 = 0, R1 = 0;
    if (zd_choose_pass_groups(&q, ngpu, budget_bytes, &g1, &R1) || g1 != 1) return 0;  // no single group for this job: keep
    const double n3 = (double) p->ppd * (double) p->ppd * (double) p->ppd;
    const bool comp = !is_pow2(p->ppd);
    // (ZD_k_cutoff = c keeps 1 / c^3 of the modes and 1 / c^2 of the (kx, ky) columns: generation and z FFT shrink with them,
    // the y / x stages and the records do not)
    const double kc = p->k_cutoff > 1.0 ? p->k_cutoff : 1.0;
    const double c_gen = (p->qPLT ? 3.9e-12 : 2.05e-12) / (kc * kc * kc), c_zf = (p->qPLT ? 3.5e-12 : 2.7e-12) / (kc * kc);
    const double c_xy  = (p->qPLT ? 3.7e-11 : 2.0e-11) * (comp ? 1.85 : 1.0);
    const Route rq = route(&q, R1, ngpu, zd::ROLE_MAIN);
    const int P0 = route(p, *stream_factor, 1, zd::ROLE_MAIN).npass, P1 = rq.npass;
    const double t_pg = c_gen * n3 * P0 / ngpu + (c_zf + c_xy) * n3 / ngpu;
    const double t_z = (c_gen * P1 + c_zf) * n3 / ngpu, t_xy = c_xy * n3 / ngpu;
    const double t_ex = (double) store_bytes(&q, R1, ngpu) * P1 / ngpu / (link_GBps * 1e9);
    const double t_a2a = P1 >= 2 ? t_z / P1 + std::max(t_ex, t_xy + t_z * (P1 - 1) / P1) + 0.05 * t_xy : t_z + std::max(t_ex, t_xy) + 0.05 * t_xy;
    if (est_seconds) {
        est_seconds[0] = t_pg;
        est_seconds[1] = t_a2a;
    }
    if (t_a2a < t_pg) {
        *groups        = 1;
        *stream_factor = R1;
    }
    return 0;
}
