// zd_capi_rounds.cpp — the rounds that run before a job's first pass: the f_NL phi round (one rank here, its stages for several ranks),
// the second- and third-order rounds.
#include <cstdio>

#include "zd_capi.h"

// f_NL: phi field -> local transform phi + f_NL phi^2 -> Fourier space again (zeldovich.cpp:945-960, 699-790): the first
// ZeldovichZ / ZeldovichXY_Phi round of the reference, run once; *d_phik = PhiK[ky][kz][x] for the half-space rows (owned
// by the caller, untouched on failure).  One rank: the forward z transform needs every plane resident.
int make_phik(const zd_params *p, const zd_pk *pk, DevBuf<cplx> &d_phik) {
    const int64_t N  = p->ppd;
    zd_params pp     = *p;
    pp.stream_factor = 1;
    pp.qPLT          = 0;  // the phi pass never reaches the displacement algebra
    PlanPtr plan;
    if (plan_create_ex(&pp, pk, nullptr, 0, 0, 1, 1, nullptr, plan)) return 1;
    zd_plan *ph = plan.get();
    DevBuf<void> d_phi;
    DevBuf<cplx> d_out;  // PhiK, handed to the caller at the end: every early return frees it
    // composite transforms (fnl_np2): phi is a real field, so the planes keep the half-space rows ky < N/2 only (k_refq_yphi rebuilds
    // a column from its half) — 8 N^3 bytes beside PhiK's 8 N^3 where the full store held 16 N^3
    ph->phi_half = ph->twr && ph->jobs.n == 1 && ph->R == 1;
    const int64_t phi_bytes = ph->phi_half ? (N / 2) * N * ph->AL.pitch * 16 : zd_plan_exchange_bytes(ph);
    if (d_phi.store_alloc((size_t) phi_bytes) != hipSuccess || d_out.store_alloc((size_t) (N / 2) * N * N) != hipSuccess) {
        fprintf(stderr, "zeldovich_hip: f_NL needs %.1f GB of HBM for the phi field at PPD %lld\n",
                (phi_bytes + (N / 2) * N * N * 16) / 1e9, (long long) N);
        return 1;
    }
    fprintf(stderr, "Generating phi field\n");
    if (zd_plan_stage_z(ph, 0, d_phi, 0)) return 1;
    if (ph->phi_half) {  // x inverse, y inverse + phi + f_NL phi^2 + y, x, then z into PhiK (conjugated: see below)
        const long long pitch = ph->AL.pitch, plane = (long long) (N / 2) * pitch;
        if (any_lines(ph, d_phi, pitch, (long long) N * (N / 2), 0)) return 1;
        if (zd::launch_refq_yphi((int) N, ph->d_twr_n, d_phi, pitch, (int) N, p->f_NL, 0)) return 1;
        if (any_lines(ph, d_phi, pitch, (long long) N * (N / 2), 0)) return 1;
        if (zd::launch_refq_cols_oop((int) N, ph->d_twr_n, d_phi, pitch, plane, d_out, N * N, N, (int) N, (int) (N / 2), true, 0)) return 1;
    } else if (zd_plan_stage_y(ph, d_phi, 0)) {
        return 1;
    } else if (ph->any) {  // reference-array PPDs: x inverse, phi + f_NL phi^2, then the forward 3-D transform of that REAL field as the
                           // conjugate of its inverse transform (x, y, z in place; conjugated while PhiK is laid out).  The lines go
                           // through the composite transforms on the composite grids (fnl_np2), else as convolutions.
        const long long plane = (long long) N * ph->AL.pitch;
        if (any_lines(ph, d_phi, ph->AL.pitch, (long long) N * N, 0)) return 1;
        if (zd::launch_any_phi_nl(ph->AL, p->f_NL, d_phi, 0)) return 1;
        if (any_lines(ph, d_phi, ph->AL.pitch, (long long) N * N, 0)) return 1;
        if (any_cols(ph, false, d_phi, plane, ph->AL.pitch, (int) N, (int) N, -1, 0)) return 1;
        if (any_cols(ph, false, d_phi, ph->AL.pitch, plane, (int) N, (int) (N / 2), -1, 0)) return 1;  // along z, rows ky < N/2
        if (zd::launch_any_phik(ph->AL, d_phi, d_out, 0)) return 1;
    } else {
        int lN = 0;
        while ((1 << lN) < (int) N) lN++;
        if (zd::launch_fnl_stage(0, ph->S, p->f_NL, ph->d_twN, d_phi, nullptr, (int) N, lN, 0)) return 1;
        if (zd::launch_fnl_stage(1, ph->S, p->f_NL, ph->d_twN, d_phi, nullptr, (int) N, lN, 0)) return 1;
        if (zd::launch_fnl_stage(2, ph->S, p->f_NL, ph->d_twN, d_phi, d_out, (int) N, lN, 0)) return 1;
    }
    if (hipDeviceSynchronize() != hipSuccess) return 1;
    d_phik = std::move(d_out);
    return 0;
}

// the round's peak against the free memory, asked before anything is built (the figure is the message)
int lpt2_round_fits(const zd_params *p, int64_t free_bytes) {
    if (lpt2_round_bytes(p) <= free_bytes) return 1;
    fprintf(stderr, "zeldovich_hip: ZD_q2LPT%s needs %.1f GB of HBM for the second-order round at PPD %lld, %.1f GB are free\n",
            p->lpt2_dealias ? " with ZD_2LPT_dealias = 1" : "", lpt2_round_bytes(p) / 1e9, (long long) p->ppd, free_bytes / 1e9);
    return 0;
}
// ZD_q2LPT: the second-order round (definition and shape: zd_kernels_lpt2.hip), run once; d_sk = S(k)[ky][kz][x] for the half-space
// rows, already scaled by N^-3 (handed to the caller).  Four gradient passes over one one-array store — generator, z and y stages of
// the plan, then the x lines into the real accumulator — and the forward transforms of the f_NL phi round.  The accumulator is freed
// before S(k) is allocated: the peak is lpt2_round_bytes.
// ZD_2LPT_dealias = 1 (step 2' of the definition): the same round on the lattice of M = 3 N / 2 points per side.  The plan of the gradient
// passes is a plan AT M — ZD_k_cutoff x 1.5, the same box, the same seed: the counter-addressed draws and the zero rule give exactly the
// modes of the N run, at their signed wavenumbers — on a one-array store [z][y][x] of the reference-array family, every line through
// the composite transforms (Q = 3).  k_xlpt2q (zd_kernels_lpt2q.hip) forms S on the M^3 accumulator and, on pass 4, takes S / M^3 through
// the x transform; the y columns |kx| < N/2 follow in place, and the z lines of the columns |kx| < N/2, 0 <= ky < N/2 go, truncated
// to |kz| < N/2 and conjugated (three inverse transforms of a real field are the conjugate of its forward transform), straight
// into S(k)[ky][kz][x] of the N layout.
// field_d != NULL: D(k) of a caller-supplied field (PhiK's layout, resident beside the round); the gradient passes read it where they
// would draw (zd_kernels_lpt2_field.hip).  Not with the de-aliased round.
int make_lpt2_source(const zd_params *p, const zd_pk *pk, DevBuf<cplx> &d_sk, const cplx *field_d) {
    const bool dq   = p->lpt2_dealias != 0;
    const int64_t N = p->ppd, M = dq ? zd::lpt2_dealias_lattice(N) : N;  // points per side of the round's lattice
    if (dq && field_d) {
        fprintf(stderr, "zeldovich_hip: ZD_Field is not supported together with ZD_2LPT_dealias (the de-aliased round draws its modes)\n");
        return 1;
    }
    size_t free_b = 0, total_b = 0;
    if (dq && (hipMemGetInfo(&free_b, &total_b) != hipSuccess || !lpt2_round_fits(p, (int64_t) free_b))) return 1;
    zd_params pp     = *p;
    pp.stream_factor = 1;   // the forward z transform needs every plane of a row
    pp.qoneslab      = -1;  // (the source needs the whole field whatever is delivered)
    if (dq) {
        pp.ppd          = M;
        pp.k_cutoff     = p->k_cutoff * 1.5;
        pp.nyquist      = p->nyquist * 1.5;  // (k2_cutoff = nyquist^2 / k_cutoff^2 may move by an ulp: it decides differently only for an integer
                                             // |k|^2 ON the cut, and at k_cutoff = 1, 2 that is |k|^2 = kmax^2 = 4^a, the modes (kmax, 0, 0) the
                                             // |k_i| == kmax rule kills anyway; kmax itself is checked below)
        pp.lpt2_dealias = 0;
    }
    PlanPtr plan;
    if (plan_create_ex(&pp, pk, nullptr, 0, 0, 1, 2, nullptr, plan, field_d != nullptr, field_d)) return 1;
    zd_plan *ph = plan.get();
    if (dq && (!ph->twr || ph->N != M || ph->g.kmax != zd::kmax((int) (N / 2), p->k_cutoff))) {
        fprintf(stderr, "zeldovich_hip: ZD_2LPT_dealias: the plan on the %lld lattice does not carry the modes of PPD %lld\n", (long long) M,
                (long long) N);
        return 1;
    }
    DevBuf<cplx> d_grad, d_out;  // d_out: S(k), handed to the caller at the end: every early return frees it
    DevBuf<double> d_acc;
    if (d_grad.store_alloc((size_t) zd_plan_exchange_bytes(ph) / sizeof(cplx)) != hipSuccess || d_acc.store_alloc((size_t) M * M * M) != hipSuccess) {
        fprintf(stderr, "zeldovich_hip: ZD_q2LPT%s needs %.1f GB of HBM for the second-order round at PPD %lld\n",
                dq ? " with ZD_2LPT_dealias = 1" : "", lpt2_round_bytes(p) / 1e9, (long long) N);
        return 1;
    }
    const long long pitch = ph->AL.pitch, plane = M * pitch;  // (the de-aliased round's store)
    for (int pass = 1; pass <= 4; pass++) {
        ph->g.lpt2 = pass;
        if (zd_plan_stage_z(ph, 0, d_grad, 0) || zd_plan_stage_y(ph, d_grad, 0)) return 1;
        if (dq ? zd::launch_lpt2q_xsrc((int) M, ph->d_twr_n, pass, d_grad, pitch, M * M, d_acc, 0)
               : zd::launch_lpt2_xsrc(ph->S, pass, ph->d_twN, d_grad, d_acc, (int) N, 0))
            return 1;
    }
    if (hipDeviceSynchronize() != hipSuccess) return 1;
    d_acc.reset();
    if (d_out.store_alloc((size_t) lpt2_sk_bytes(N) / sizeof(cplx)) != hipSuccess) {
        fprintf(stderr, "zeldovich_hip: ZD_q2LPT needs %.1f GB of HBM for the second-order source at PPD %lld\n",
                lpt2_sk_bytes(N) / 1e9, (long long) N);
        return 1;
    }
    if (dq) {
        // y columns of the planes, only those that are kept: x = kx in [0, N/2) and x = M + kx, kx in (-N/2, 0)
        if (zd::launch_refq_cols((int) M, ph->d_twr_n, d_grad, plane, pitch, (int) (N / 2), (int) M, -1, 0)) return 1;
        if (zd::launch_refq_cols((int) M, ph->d_twr_n, d_grad + (M - N / 2 + 1), plane, pitch, (int) (N / 2 - 1), (int) M, -1, 0)) return 1;
        if (zd::launch_lpt2q_zsrc((int) M, (int) N, ph->d_twr_n, d_grad, pitch, d_out, 0)) return 1;
    } else {
        int lN = 0;
        while ((1 << lN) < (int) N) lN++;
        if (zd::launch_fnl_stage(1, ph->S, 0.0, ph->d_twN, d_grad, nullptr, (int) N, lN, 0)) return 1;
        if (zd::launch_fnl_stage(2, ph->S, 0.0, ph->d_twN, d_grad, d_out, (int) N, lN, 0)) return 1;
    }
    if (hipDeviceSynchronize() != hipSuccess) return 1;
    d_sk = std::move(d_out);
    return 0;
}
// ZD_q3LPT: the third-order round (definition and shape: zd_kernels_lpt3.hip), run once after the second-order round with its S(k) in
// d_sk; d_out[0 .. 3] = P3(k), C_x(k), C_y(k), C_z(k) in the layout of S(k), already scaled by N^-3 (handed to the caller).  Six pair
// passes over one one-array store — generator, z and y stages of a plan of the second-order round's kind, then the x lines into two
// real fields each —, the pointwise sources over four of the twelve fields, and four runs of the f_NL phi round's forward chain.  The
// eight fields that are no longer needed are freed before the four spectra are allocated: the peak is lpt3_round_bytes.
int make_lpt3_sources(const zd_params *p, const zd_pk *pk, const cplx *d_sk, DevBuf<cplx> (&d_out)[4]) {
    const int64_t N = p->ppd, n3 = N * N * N;
    zd_params pp     = *p;
    pp.stream_factor = 1;   // the forward z transform needs every plane of a row
    pp.qoneslab      = -1;  // (the sources need the whole field whatever is delivered)
    PlanPtr plan;
    if (plan_create_ex(&pp, pk, nullptr, 0, 0, 1, 2, nullptr, plan)) return 1;
    zd_plan *ph = plan.get();
    auto no_room = [&]() {
        fprintf(stderr, "zeldovich_hip: ZD_q3LPT needs %.1f GB of HBM for the third-order round at PPD %lld\n", lpt3_round_bytes(N) / 1e9,
                (long long) N);
        return 1;
    };
    DevBuf<cplx> d_pair, d_spec[4];  // d_spec: handed to the caller at the end: every early return frees them
    DevBuf<double> d_td[6], d_ts[6];
    zd::Lpt3Fields F;
    if (d_pair.store_alloc((size_t) zd_plan_exchange_bytes(ph) / sizeof(cplx)) != hipSuccess) return no_room();
    for (int f = 0; f < 6; f++) {
        if (d_td[f].store_alloc((size_t) n3) != hipSuccess || d_ts[f].store_alloc((size_t) n3) != hipSuccess) return no_room();
        F.d[f] = d_td[f];
        F.s[f] = d_ts[f];
    }
    ph->g.lpt2_sk = d_sk;
    for (int pass = 1; pass <= 6; pass++) {
        ph->g.lpt3 = pass;
        if (zd_plan_stage_z(ph, 0, d_pair, 0) || zd_plan_stage_y(ph, d_pair, 0)) return 1;
        if (zd::launch_lpt3_xpair(ph->S, ph->d_twN, d_pair, d_td[pass - 1], d_ts[pass - 1], (int) N, 0)) return 1;
    }
    if (zd::launch_lpt3_point(F, zd::lpt3_g3a(p), zd::lpt3_g3b(p), n3, 0)) return 1;
    if (hipDeviceSynchronize() != hipSuccess) return 1;
    for (int f = 0; f < 6; f++) {
        d_ts[f].reset();
        if (f >= 4) d_td[f].reset();
    }
    int lN = 0;
    while ((1 << lN) < (int) N) lN++;
    for (int f = 0; f < 4; f++) {
        if (d_spec[f].store_alloc((size_t) lpt2_sk_bytes(N) / sizeof(cplx)) != hipSuccess) return no_room();
        if (zd::launch_lpt3_xfwd(ph->S, ph->d_twN, d_td[f], d_pair, (int) N, 0)) return 1;
        if (zd::launch_fnl_stage(1, ph->S, 0.0, ph->d_twN, d_pair, nullptr, (int) N, lN, 0)) return 1;
        if (zd::launch_fnl_stage(2, ph->S, 0.0, ph->d_twN, d_pair, d_spec[f], (int) N, lN, 0)) return 1;
    }
    if (hipDeviceSynchronize() != hipSuccess) return 1;
    for (int f = 0; f < 4; f++) d_out[f] = std::move(d_spec[f]);
    return 0;
}
// a plan of the final pass takes the four spectra over and points its generator at them
void adopt_lpt3(zd_plan *pl, DevBuf<cplx> (&d_spec)[4]) {
    for (int f = 0; f < 4; f++) pl->d_lpt3_owned[f] = std::move(d_spec[f]);
    pl->g.lpt3_p3 = pl->d_lpt3_owned[0];
    for (int j = 0; j < 3; j++) pl->g.lpt3_c[j] = pl->d_lpt3_owned[1 + j];
}
// a ZD_q2LPT job the route takes for this call (the refusal printed otherwise), asked BEFORE the second-order round is run
int lpt2_route_check(const zd_params *p, int nranks, int rank) {
    const zd_params pc = zd::canonical(p);
    const Route rt = route(&pc, pc.stream_factor, nranks, zd::ROLE_MAIN, rank, true);
    if (rt.ok()) return 0;
    fprintf(stderr, "zeldovich_hip: %s\n", rt.why);
    return 1;
}

// ---- f_NL on several ranks (zd_multi.cpp): the plans of the phi round and of the main pass, and the stages of the phi round
// on a plane group / on the returned store ----
int zd_plan_create_phi(const zd_params *p, const zd_pk *pk, int rank, int nranks, zd_plan **out) {
    zd_params pp     = *p;
    pp.stream_factor = 1;  // the forward z transform needs every plane of a row: one pass
    pp.qPLT          = 0;
    PlanPtr pl;
    return hand_over(plan_create_ex(&pp, pk, nullptr, 0, rank, nranks, 1, nullptr, pl), pl, out);
}
int zd_plan_create_phik(const zd_params *p, const zd_pk *pk, const double *eig, int64_t eig_ppd, int rank, int nranks, const void *d_phik,
                        zd_plan **out) {
    PlanPtr pl;
    return hand_over(plan_create_ex(p, pk, eig, eig_ppd, rank, nranks, 0, (const cplx *) d_phik, pl), pl, out);
}
// planes [0, nplanes) of a ring slot with `chunk_planes` planes per chunk: inverse y, x (inverse, phi + f_NL phi^2, forward),
// forward y — ZeldovichXY_Phi (zeldovich.cpp:699-790)
int zd_plan_phi_xy_group(zd_plan *pl, void *d_slot, int chunk_planes, int nplanes, double f_NL, void *hip_stream) {
    hipStream_t st = (hipStream_t) hip_stream;
    if (pl->any) {  // composite grid (AnyChunks): y inverse (the Nyquist row read as zero), x lines with phi + f_NL phi^2 (every row of
                    // every chunk), y again — the rows ky < N/2 written back, all that the forward z lines into PhiK read
        const zd::AnyChunks C = any_chunks(pl, chunk_planes);
        if (zd::launch_refq_ycols(pl->N, pl->d_twr_n, C, d_slot, pl->N, nplanes, pl->N / 2, pl->N, st)) return 1;
        for (int c = 0; c < pl->nranks; c++)
            if (zd::launch_refq_xphi(pl->N, pl->d_twr_n, (cplx *) d_slot + c * C.chunk, C.pitch, (long long) nplanes * 2 * pl->Hq, f_NL, st))
                return 1;
        return zd::launch_refq_ycols(pl->N, pl->d_twr_n, C, d_slot, pl->N, nplanes, -1, pl->N / 2, st);
    }
    const zd::StoreLayout S = layout_for_chunks(pl, chunk_planes);
    if (zd::launch_yfft(S, nplanes, pl->d_twN, d_slot, st)) return 1;
    if (zd::launch_fnl_stage(0, S, f_NL, pl->d_twN, d_slot, nullptr, nplanes, 0, st)) return 1;
    return zd::launch_fnl_stage(1, S, f_NL, pl->d_twN, d_slot, nullptr, nplanes, 0, st);
}
// forward z over this rank's rows of the returned store -> PhiK[row slot][kz][x]
int zd_plan_phi_zfwd(zd_plan *pl, void *d_store, void *d_phik, void *hip_stream) {
    if (pl->any) {  // chunks are plane-major: plane z of this rank's rows sits at z (2 Hq pitch); conjugated, as make_phik does
        const long long pitch = pl->AC.pitch;
        return zd::launch_refq_cols_oop(pl->N, pl->d_twr_n, d_store, pitch, 2 * pl->Hq * pitch, d_phik, (long long) pl->N * pl->N, pl->N, pl->N,
                                        pl->Hq, true, (hipStream_t) hip_stream);
    }
    int lZq = 0;
    while ((1 << lZq) < pl->Zq) lZq++;
    return zd::launch_fnl_stage(2, pl->S, 0.0, pl->d_twN, d_store, d_phik, pl->N, lZq, (hipStream_t) hip_stream);
}
