// zd_capi_stages.cpp — the stages of a plan (zd_plan_stage_z, _y, _x and their plane-group forms), their timing spans, zd_plan_stats.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "zd_capi.h"

static void tick(zd_plan *pl, int kind, hipStream_t st, bool begin) {
    if (!pl->p.profile) return;
    if (begin) {
        EventPair ep;
        hipEventCreate(&ep.a);
        hipEventCreate(&ep.b);
        ep.kind = kind;
        hipEventRecord(ep.a, st);
        pl->events.push_back(ep);
    } else {
        hipEventRecord(pl->events.back().b, st);
    }
}

// span events (begin and end recorded at different places, other ticks in between)
static int span_begin(zd_plan *pl, int kind, hipStream_t st) {
    if (!pl->p.profile) return -1;
    EventPair ep;
    hipEventCreate(&ep.a);
    hipEventCreate(&ep.b);
    ep.kind = kind;
    hipEventRecord(ep.a, st);
    pl->events.push_back(ep);
    return (int) pl->events.size() - 1;
}
static void span_end(zd_plan *pl, int idx, hipStream_t st) {
    if (idx >= 0) hipEventRecord(pl->events[idx].b, st);
}

void collect_events(zd_plan *pl) {
    for (auto &ep : pl->events) {
        float ms = 0;
        hipEventSynchronize(ep.b);
        hipEventElapsedTime(&ms, ep.a, ep.b);
        pl->kernel_ms[ep.kind] += ms;
        pl->launches[ep.kind]++;
        hipEventDestroy(ep.a);
        hipEventDestroy(ep.b);
    }
    pl->events.clear();
}

static bool p_oneslab_off(const zd_plan *pl) { return pl->p.qoneslab < 0; }  // ZD_qoneslab runs finish a single pass

// the line transforms of the reference-array store (pl->any): composite (zd_kernels_np2_ref.hip) where the route says so
// (pl->twr), else convolutions (zd_kernels_any.hip).  zlen: lines of length L (the z lines of a pass), else N.
int any_cols(const zd_plan *pl, bool zlen, void *data, long long batch_stride, long long point_stride, int ncols, int nbatch,
             int zero_point, hipStream_t st) {
    if (pl->twr)
        return zd::launch_refq_cols(zlen ? pl->L : pl->N, zlen ? pl->d_twr_l : pl->d_twr_n, data, batch_stride, point_stride, ncols, nbatch,
                                    zero_point, st);
    return zd::launch_any_cols(zlen ? pl->tabL : pl->tabN, data, batch_stride, point_stride, ncols, nbatch, zero_point, st);
}
int any_lines(const zd_plan *pl, void *data, long long pitch, long long nlines, hipStream_t st) {
    if (pl->twr) return zd::launch_refq_lines(pl->N, pl->d_twr_n, data, pitch, nlines, st);
    return zd::launch_any_lines(pl->tabN, data, pitch, nlines, st);
}

// z FFT of one slab of generated rows into the block store (reference / packed arrays with Hermitian twins, or the
// potentials of the field store)
static int launch_zstage_fft(zd_plan *pl, int ky0, int kyloc0, int nky, const void *Y, void *d_send, hipStream_t st) {
    if (pl->family == zd::FAM_COMPOSITE) return zd::launch_zfft_fields_np2(pl->L, pl->F, pl->S, ky0, kyloc0, nky, Y, pl->d_twq_l, d_send, st);
    if (zd::pack_is_fields(pl->pack)) return zd::launch_zfft_fields(pl->L, pl->F, pl->S, ky0, kyloc0, nky, Y, pl->d_twL, d_send, st);
    return zd::launch_zfft(pl->L, pl->jobs, pl->S, ky0, kyloc0, nky, pl->Zq, Y, pl->d_twL, d_send, st);
}

// One slab of folded inputs, between its ZD_K_GEN ticks on `st`: rows r0 .. r0 + nky of this rank (half-space rows rank, rank + G,
// ...: cyclic) for the residues `residue` and `residue2` into Y, the generator's tiles counted on `ctr`.
static int gen_slab(zd_plan *pl, int r0, int nky, int residue, int residue2, void *Y, unsigned *ctr, hipStream_t st) {
    const int ky_first = pl->rank, G = pl->nranks;
    tick(pl, ZD_K_GEN, st, true);
    // ZD_Version = 1: every pass replays the streams from their seeds; rows that share a stream (block/G apart in this rank's row
    // order) are drawn by successive launches.  (Such plans never overlap: the worker streams do not come here with v1_block set.)
    if (pl->v1_block) {
        const int group = pl->v1_block / G;
        for (int i0 = 0; i0 < nky; i0 += group)
            if (zd::launch_v1_draw(pl->g, pl->v1_block, ky_first + G * (r0 + i0), G, std::min(group, nky - i0), pl->d_v1streams,
                                   pl->d_v1dev + (size_t) i0 * pl->N * pl->N, pl->d_v1err, st))
                return 1;
    }
    // (k_genf with walks of 16 / 4 / 2 z rows where the kernel exists, else the general generator)
    if (pl->d_eiglines && zd::launch_eig_lines(pl->g, ky_first + G * r0, G, nky, pl->d_eiglines, st)) return 1;
    if (zd::launch_gen(pl->g, pl->J, pl->jobs, pl->S, ky_first + G * r0, nky, pl->L, residue, residue2, pl->d_twN, Y, ctr, pl->gen_max_wgs, st))
        return 1;
    tick(pl, ZD_K_GEN, st, false);
    return 0;
}

// Z stage of the any-PPD path (zd_kernels_any.hip): general generator -> Y, convolution transform of Y along k2 in place,
// scatter into the [plane][array][y][x] store with the Hermitian twin rules
static int any_stage_z(zd_plan *pl, int residue, void *d_send, hipStream_t st) {
    const int zspan = span_begin(pl, ZD_K_ZSTAGE, st);
    if (pl->v1_block && zd::launch_v1_seed((unsigned long long) pl->p.seed, pl->v1_block, pl->d_v1streams, st)) return 1;
    HIPCHECK(hipMemsetAsync(pl->d_tilectr, 0, sizeof(unsigned) * pl->n_tilectr, st));
    const int ky_first = pl->rank, G = pl->nranks;  // this rank's half-space rows: rank, rank + G, ... (one rank: every row)
    int slab = 0;
    for (int r0 = 0; r0 < pl->Hq; r0 += pl->slab_rows, slab++) {
        const int nky = std::min(pl->slab_rows, pl->Hq - r0);
        if (gen_slab(pl, r0, nky, residue, residue, pl->d_Y[0], pl->d_tilectr + slab, st)) return 1;
        tick(pl, ZD_K_ZFFT, st, true);
        if (pl->phi_half) {  // phi round on half-space planes (one job, R = 1): the z lines straight into rows r0 .. of every plane
            if (zd::launch_refq_cols_oop(pl->L, pl->d_twr_l, pl->d_Y[0], (long long) pl->L * pl->N, pl->N, (cplx *) d_send + (long long) r0 * pl->AL.pitch,
                                         pl->AL.pitch, (long long) pl->half * pl->AL.pitch, pl->N, nky, false, st))
                return 1;
        } else {
            if (any_cols(pl, true, pl->d_Y[0], (long long) pl->L * pl->N, pl->N, pl->N, pl->jobs.n * nky, -1, st)) return 1;
            if (G > 1 ? zd::launch_refq_scatter(pl->jobs, pl->AC, ky_first, r0, nky, pl->L, pl->d_Y[0], d_send, st)
                      : zd::launch_any_scatter(pl->jobs, pl->AL, r0, nky, pl->L, pl->d_Y[0], d_send, st))
                return 1;
        }
        tick(pl, ZD_K_ZFFT, st, false);
    }
    span_end(pl, zspan, st);
    return 0;
}

static int stage_z_impl(zd_plan *pl, int residue, void *d_send, hipStream_t st, bool detached, hipEvent_t wait_ev, hipEvent_t done_ev);

// Z stage of a plan with the fused generator + z FFT (zd_kernels_fz.hip; one rank): the ky = 0 row — conjugate "loser" modes,
// zeldovich.cpp:485-503 — through the general generator and k_zfft (one row), every other row through k_genz_plt; one stream
static int fused_stage_z(zd_plan *pl, int residue, void *d_send, hipStream_t st, bool detached, hipEvent_t wait_ev, hipEvent_t done_ev) {
    if (detached && wait_ev) HIPCHECK(hipStreamWaitEvent(st, wait_ev, 0));
    pl->g.accum_var = pl->var_pending ? 1 : 0;  // once per run: every pass sees every mode
    pl->var_pending = false;
    const int zspan = span_begin(pl, ZD_K_ZSTAGE, st);
    HIPCHECK(hipMemsetAsync(pl->d_tilectr, 0, sizeof(unsigned), st));
    tick(pl, ZD_K_GEN, st, true);
    if (zd::launch_gen(pl->g, pl->J, pl->jobs, pl->S, 0, 1, pl->L, residue, residue, pl->d_twN, pl->d_Y[0], nullptr, pl->gen_max_wgs, st)) return 1;
    if (zd::launch_zfft(pl->L, pl->jobs, pl->S, 0, 0, 1, pl->Zq, pl->d_Y[0], pl->d_twL, d_send, st)) return 1;
    if (zd::launch_genz_plt(pl->g, pl->S, 0, pl->L, residue, pl->n_fzitems, pl->d_fzitems, pl->d_twN, pl->d_twL, d_send, pl->d_tilectr,
                            pl->ncu, st))
        return 1;
    tick(pl, ZD_K_GEN, st, false);
    span_end(pl, zspan, st);
    if (detached && done_ev) HIPCHECK(hipEventRecord(done_ev, st));
    return 0;
}

int zd_plan_stage_z(zd_plan *pl, int residue, void *d_send, void *hip_stream) {
    return stage_z_impl(pl, residue, d_send, (hipStream_t) hip_stream, false, nullptr, nullptr);
}

// The Z stage detached from the caller's stream (zd_multi.cpp pipelines passes with it): the z FFT — the only part that
// writes d_send — starts after `wait_ev` (NULL: at once) instead of after everything queued on `st`, nothing joins `st`, and
// `done_ev` is recorded behind the last z FFT.  Plans without the two worker streams (ZD_Version = 1, convolution PPDs,
// serial_z) run the stage on `st` as usual and record done_ev there.
int zd_plan_stage_z_detached(zd_plan *pl, int residue, void *d_send, void *hip_stream, void *wait_event, void *done_event) {
    return stage_z_impl(pl, residue, d_send, (hipStream_t) hip_stream, true, (hipEvent_t) wait_event, (hipEvent_t) done_event);
}

static int stage_z_impl(zd_plan *pl, int residue, void *d_send, hipStream_t st, bool detached, hipEvent_t wait_ev, hipEvent_t done_ev) {
    if (residue < 0 || residue >= pl->npass) return 1;
    if (pl->dens_sub) {
        // PLT + ZD_qdensity = 1 on a composite grid (plan_create_ex): first the whole density-only pass — Z stage into this store,
        // y / x stages of its density array — whose planes are the planes of this pass; then the PLT pass proper over the same
        // store.  All in stream order on st (a detached call included: the density planes are kept in ONE buffer).
        zd_plan *B = pl->dens_sub.get();
        if (detached && wait_ev) HIPCHECK(hipStreamWaitEvent(st, wait_ev, 0));
        B->pass_step = pl->pass_step;
        if (stage_z_impl(B, residue, d_send, st, false, nullptr, nullptr)) return 1;
        pl->dens_pass = -1;
        if (zd_plan_stage_x_group(B, residue, d_send, B->Zq, 0, 0, (int64_t) B->Zq * 2, nullptr, pl->d_dens_pass, st)) return 1;
        pl->dens_pass = residue;
        PlanPtr sub = std::move(pl->dens_sub);  // (the PLT pass itself)
        const int rc = stage_z_impl(pl, residue, d_send, st, false, nullptr, nullptr);
        pl->dens_sub = std::move(sub);
        if (rc) return rc;
        if (detached && done_ev) HIPCHECK(hipEventRecord(done_ev, st));
        return 0;
    }
    if (detached && (pl->any || !pl->overlap)) {  // no worker streams: in stream order on st
        if (wait_ev) HIPCHECK(hipStreamWaitEvent(st, wait_ev, 0));
        if (stage_z_impl(pl, residue, d_send, st, false, nullptr, nullptr)) return 1;
        if (done_ev) HIPCHECK(hipEventRecord(done_ev, st));
        return 0;
    }
    if (pl->any) return any_stage_z(pl, residue, d_send, st);
    if (pl->fused_z) return fused_stage_z(pl, residue, d_send, st, detached, wait_ev, done_ev);
    const int residue2 = pl->pstep == 2 ? residue + pl->R / 2 : residue;
    pl->g.accum_var = (pl->pack != zd::PACK_NONE && pl->var_pending) ? 1 : 0;  // once per run: every pass sees every mode
    pl->var_pending = false;
    const int ky_first = pl->rank, G = pl->nranks;  // this rank's half-space rows: rank, rank + G, ... (cyclic)
    const int zspan = span_begin(pl, ZD_K_ZSTAGE, detached ? pl->s_gen : st);
    if (!pl->overlap) {
        HIPCHECK(hipMemsetAsync(pl->d_tilectr, 0, sizeof(unsigned) * pl->n_tilectr, st));
        // ZD_Version = 1: every pass replays the streams from their seeds; rows that share a stream (block/G apart in
        // this rank's row order) are drawn by successive launches
        if (pl->v1_block && zd::launch_v1_seed((unsigned long long) pl->p.seed, pl->v1_block, pl->d_v1streams, st)) return 1;
        int slab = 0;
        for (int r0 = 0; r0 < pl->Hq; r0 += pl->slab_rows, slab++) {
            const int nky = std::min(pl->slab_rows, pl->Hq - r0);
            if (gen_slab(pl, r0, nky, residue, residue2, pl->d_Y[0], pl->d_tilectr + slab, st)) return 1;
            tick(pl, ZD_K_ZFFT, st, true);
            if (launch_zstage_fft(pl, ky_first + G * r0, r0, nky, pl->d_Y[0], d_send, st)) return 1;
            tick(pl, ZD_K_ZFFT, st, false);
        }
        span_end(pl, zspan, st);
        return 0;
    }
    // Two worker streams.  s_fft (k_zfft, writes the store) starts after everything already queued on the caller's
    // stream; s_gen (generator, writes ring slots only) is ordered by the ring alone and may be a pass ahead.
    const int K = (int) pl->d_Y.size(), nslab = pl->Hq / pl->slab_rows;
    if (!detached) {
        HIPCHECK(hipEventRecord(pl->ev_fork, st));
        HIPCHECK(hipStreamWaitEvent(pl->s_fft, pl->ev_fork, 0));
    } else if (wait_ev) {
        HIPCHECK(hipStreamWaitEvent(pl->s_fft, wait_ev, 0));
    }
    auto issue_gen = [&](int pass, int slab, long long gno, int accum) -> int {
        const int slot = (int) (gno % K), r0 = slab * pl->slab_rows;
        // the slot is free once the k_zfft that read its previous content (slab gno - K) has finished
        if (gno >= K) HIPCHECK(hipStreamWaitEvent(pl->s_gen, pl->ev_fft[slot], 0));
        unsigned *ctr = pl->d_tilectr + (pass & 1) * nslab;
        if (slab == 0) HIPCHECK(hipMemsetAsync(ctr, 0, sizeof(unsigned) * nslab, pl->s_gen));
        pl->g.accum_var = accum;
        if (gen_slab(pl, r0, pl->slab_rows, pass, pl->pstep == 2 ? pass + pl->R / 2 : pass, pl->d_Y[slot], ctr + slab, pl->s_gen)) return 1;
        HIPCHECK(hipEventRecord(pl->ev_gen[slot], pl->s_gen));
        return 0;
    };
    const int accum = pl->g.accum_var;
    // nothing (or something else) was started ahead; or the variance is summed in this Z stage (the first after zd_plan_stats),
    // which the slabs generated ahead — issued with accum = 0 — would leave out: they are generated again
    if (pl->ahead_pass != residue || accum) pl->ahead_n = 0;
    for (int slab = 0; slab < nslab; slab++) {
        long long gno;
        if (slab < pl->ahead_n)
            gno = pl->ahead_g0 + slab;
        else {
            gno = pl->next_g++;
            if (issue_gen(residue, slab, gno, accum)) return 1;
        }
        const int slot = (int) (gno % K), r0 = slab * pl->slab_rows;
        HIPCHECK(hipStreamWaitEvent(pl->s_fft, pl->ev_gen[slot], 0));
        tick(pl, ZD_K_ZFFT, pl->s_fft, true);
        if (launch_zstage_fft(pl, ky_first + G * r0, r0, pl->slab_rows, pl->d_Y[slot], d_send, pl->s_fft)) return 1;
        tick(pl, ZD_K_ZFFT, pl->s_fft, false);
        HIPCHECK(hipEventRecord(pl->ev_fft[slot], pl->s_fft));
    }
    pl->ahead_pass = -1;
    pl->ahead_n    = 0;
    // run ahead: the first slabs of the next pass go into the ring now; they execute while the caller's stream does
    // this pass's y and x transforms
    if (K > 2 && residue + pl->pass_step < pl->npass && p_oneslab_off(pl)) {
        const int n = std::min(nslab, K);
        pl->ahead_pass = residue + pl->pass_step;  // (this rank's next pass: with pass groups not residue + 1)
        pl->ahead_g0   = pl->next_g;
        for (int slab = 0; slab < n; slab++)
            if (issue_gen(residue + pl->pass_step, slab, pl->next_g++, 0)) return 1;
        pl->ahead_n = n;
    }
    if (detached) {  // nothing joins the caller's stream: whoever needs the store waits for done_ev
        if (done_ev) HIPCHECK(hipEventRecord(done_ev, pl->s_fft));
        span_end(pl, zspan, pl->s_fft);
        return 0;
    }
    // join: the caller's stream continues after the last k_zfft of this pass
    HIPCHECK(hipEventRecord(pl->ev_fork, pl->s_fft));
    HIPCHECK(hipStreamWaitEvent(st, pl->ev_fork, 0));
    span_end(pl, zspan, st);
    return 0;
}

// The XY stages address the store through its layout; after an exchange in plane groups (zd_multi.cpp) the data sits in
// a ring slot whose chunks are `chunk_planes` planes long instead of Zq.  Chunks are plane-major, so only the chunk stride
// changes.
zd::StoreLayout layout_for_chunks(const zd_plan *pl, int chunk_planes) {
    zd::StoreLayout S = pl->S;
    if (chunk_planes != pl->Zq) {
        S.kb_rows    = S.zb_rows * ((chunk_planes >> S.lq) >> S.lBz);
        S.chunk_rows = S.kb_rows * ((2 * pl->Hq) >> S.lBk);
    }
    return S;
}
zd::AnyChunks any_chunks(const zd_plan *pl, int chunk_planes) {
    zd::AnyChunks C = pl->AC;
    C.chunk         = (long long) chunk_planes * pl->narray * 2 * pl->Hq * pl->AC.pitch;
    return C;
}
static zd::FieldLayout fields_for_chunks(const zd_plan *pl, int chunk_planes) {
    zd::FieldLayout F = pl->F;
    F.chunk_elems     = (long long) chunk_planes * F.nfield * F.field_elems;
    return F;
}

// y stage on a store (or ring slot) whose chunks hold `chunk_planes` planes, for its planes [0, nplanes)
int zd_plan_stage_y_group(zd_plan *pl, void *d_recv, int chunk_planes, int nplanes, void *hip_stream) {
    hipStream_t st = (hipStream_t) hip_stream;
    if (zd::pack_is_fields(pl->pack)) return 0;  // field stores: the y transform runs plane group by plane group in stage_x
    if (pl->any) {  // every (plane, array) image: columns along y, the Nyquist row counted as zero (zeldovich.cpp:644-650)
        tick(pl, ZD_K_YFFT, st, true);
        if (pl->nranks > 1) {  // the columns gathered over the chunks of the ring slot
            if (zd::launch_refq_ycols(pl->N, pl->d_twr_n, any_chunks(pl, chunk_planes), d_recv, pl->N, nplanes * pl->narray, pl->N / 2, pl->N,
                                    st))
                return 1;
        } else if (any_cols(pl, false, d_recv, (long long) pl->N * pl->AL.pitch, pl->AL.pitch, pl->N, nplanes * pl->narray, pl->N / 2, st))
            return 1;
        tick(pl, ZD_K_YFFT, st, false);
        return 0;
    }
    tick(pl, ZD_K_YFFT, st, true);
    if (zd::launch_yfft(layout_for_chunks(pl, chunk_planes), nplanes, pl->d_twN, d_recv, st)) return 1;
    tick(pl, ZD_K_YFFT, st, false);
    return 0;
}
int zd_plan_stage_y(zd_plan *pl, void *d_recv, void *hip_stream) { return zd_plan_stage_y_group(pl, d_recv, pl->Zq, pl->Zq, hip_stream); }

// x stage (+ the y stage of the field store) for delivered planes [plane0, plane0 + nplanes) of a store / ring slot with
// `chunk_planes` planes per chunk; `gplane0` = the local plane index of the first one inside the pass (it fixes z)
int zd_plan_stage_x_group(zd_plan *pl, int residue, const void *d_recv, int chunk_planes, int64_t plane0, int64_t gplane0,
                          int64_t nplanes, void *d_records, float *d_density, void *hip_stream) {
    hipStream_t st = (hipStream_t) hip_stream;
    const int ps = pl->pstep;
    if (plane0 < 0 || nplanes < 1 || plane0 + nplanes > (int64_t) chunk_planes * ps || plane0 % ps || nplanes % ps || gplane0 % ps
        || gplane0 + nplanes > (int64_t) pl->Zq * ps) {
        fprintf(stderr, "zeldovich_hip: stage_x plane range [%lld, +%lld) invalid (multiples of %d inside [0, %lld))\n",
                (long long) plane0, (long long) nplanes, ps, (long long) chunk_planes * ps);
        return 1;
    }
    if (d_density && pl->dens_sub) {  // the planes the density-only half left behind at the head of this pass's Z stage
        if (pl->dens_pass != residue) {  // one buffer: a later Z stage has overwritten them (or no Z stage of this pass ran)
            fprintf(stderr, "zeldovich_hip: stage_x density of pass %d requested, but the last Z stage was pass %d: only that pass can "
                            "deliver density planes on this plan\n", residue, pl->dens_pass);
            return 1;
        }
        HIPCHECK(hipMemcpyAsync(d_density, pl->d_dens_pass + (size_t) gplane0 * pl->N * pl->N, (size_t) nplanes * pl->N * pl->N * sizeof(float),
                                hipMemcpyDeviceToDevice, st));
        d_density = nullptr;
    }
    if (d_density && pl->pack != zd::PACK_NONE && !pl->dens) return 1;  // packed stores carry no density field (but the six-field store)
    if (pl->any && pl->nranks > 1) {  // the same on a chunked ring slot: x lines per chunk, the epilogue finds row y by its slot
        const int z_first = (int) zd_plan_plane_z(pl, residue, gplane0);
        const zd::AnyChunks C = any_chunks(pl, chunk_planes);
        const long long img_rows = (long long) pl->narray * 2 * pl->Hq;
        tick(pl, ZD_K_XFFT, st, true);
        for (int c = 0; c < pl->nranks; c++)
            if (zd::launch_refq_lines(pl->N, pl->d_twr_n, (cplx *) const_cast<void *>(d_recv) + c * C.chunk + plane0 * img_rows * C.pitch,
                                      C.pitch, nplanes * img_rows, st))
                return 1;
        if (zd::launch_refq_emit(C, pl->ec, d_recv, (int) plane0, (int) nplanes, z_first, pl->R, d_records, d_density, pl->d_red, st)) return 1;
        tick(pl, ZD_K_XFFT, st, false);
        return 0;
    }
    if (pl->any) {  // x lines of the planes in place (each plane once), then the particle epilogue
        const int z_first = (int) zd_plan_plane_z(pl, residue, gplane0);
        cplx *first = (cplx *) const_cast<void *>(d_recv) + (long long) plane0 * pl->narray * pl->N * pl->AL.pitch;
        tick(pl, ZD_K_XFFT, st, true);
        if (any_lines(pl, first, pl->AL.pitch, (long long) nplanes * pl->narray * pl->N, st)) return 1;
        if (zd::launch_any_emit(pl->AL, pl->ec, d_recv, (int) plane0, (int) nplanes, z_first, pl->R, d_records, d_density, pl->d_red, st)) return 1;
        tick(pl, ZD_K_XFFT, st, false);
        return 0;
    }
    if (zd::pack_is_fields(pl->pack)) {
        // y stage (potentials -> the three displacement arrays of a group of store planes, into the ring) + x stage
        const zd::FieldLayout F = fields_for_chunks(pl, chunk_planes);
        const int p0 = (int) (plane0 / ps), np = (int) (nplanes / ps);
        const bool np2 = pl->family == zd::FAM_COMPOSITE;  // the composite-transform kernels (zd_kernels_np2.hip) and their twiddles d_twq_n
        for (int g0 = 0; g0 < np; g0 += pl->ring_planes) {
            const int ng = std::min(pl->ring_planes, np - g0);
            char *rec_g = d_records ? (char *) d_records + (size_t) g0 * ps * pl->N * pl->N * pl->ec.recsize : nullptr;
            const int z_first = (int) zd_plan_plane_z(pl, residue, gplane0 + (int64_t) g0 * ps);
            tick(pl, ZD_K_YFFT, st, true);
            if (!pl->dens_only
                && (np2 ? zd::launch_yfft_fields_np2(F, pl->S, pl->d_twq_n, d_recv, p0 + g0, ng, pl->SR.pitch, pl->d_ring, 0, st)
                        : zd::launch_yfft_fields(F, pl->S, pl->d_twN, d_recv, p0 + g0, ng, pl->SR.pitch, pl->d_ring, st)))
                return 1;
            if (pl->dens && d_density
                && zd::launch_yfft_fields_np2(F, pl->S, pl->d_twq_n, d_recv, p0 + g0, ng, pl->SR.pitch, pl->d_ring_dens, 1, st))
                return 1;
            tick(pl, ZD_K_YFFT, st, false);
            tick(pl, ZD_K_XFFT, st, true);
            if (!pl->dens_only
                && (np2 ? zd::launch_xfft_np2(pl->N, pl->ec, pl->d_twq_n, pl->d_ring, pl->SR.pitch, ng, z_first, pl->R, rec_g, pl->d_red, st)
                        : zd::launch_xfft(pl->SR, pl->ec, pl->d_twN, pl->d_ring, 0, ng, z_first, pl->R, rec_g, nullptr, pl->d_red, st)))
                return 1;
            if (pl->dens && d_density
                && zd::launch_xdens_np2(pl->N, pl->d_twq_n, pl->d_ring_dens, pl->SR.pitch, ng, d_density + (size_t) g0 * ps * pl->N * pl->N, st))
                return 1;
            tick(pl, ZD_K_XFFT, st, false);
        }
        return 0;
    }
    const int z_first = (int) zd_plan_plane_z(pl, residue, gplane0);
    tick(pl, ZD_K_XFFT, st, true);
    if (zd::launch_xfft(layout_for_chunks(pl, chunk_planes), pl->ec, pl->d_twN, d_recv, (int) (plane0 / ps), (int) (nplanes / ps), z_first,
                        pl->R, d_records, d_density, pl->d_red, st))
        return 1;
    tick(pl, ZD_K_XFFT, st, false);
    return 0;
}
int zd_plan_stage_x(zd_plan *pl, int residue, const void *d_recv, int64_t plane0, int64_t nplanes, void *d_records,
                    float *d_density, void *hip_stream) {
    return zd_plan_stage_x_group(pl, residue, d_recv, pl->Zq, plane0, plane0, nplanes, d_records, d_density, hip_stream);
}

void zd_plan_tick(zd_plan *pl, int kind, void *hip_stream, int begin) { tick(pl, kind, (hipStream_t) hip_stream, begin != 0); }

int zd_plan_stats(zd_plan *pl, zd_stats *out) {
    HIPCHECK(hipDeviceSynchronize());
    collect_events(pl);
    zd::Reduce h;
    HIPCHECK(hipMemcpy(&h, pl->d_red, sizeof(h), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemset(pl->d_red, 0, sizeof(zd::Reduce)));
    memset(out, 0, sizeof(*out));
    double ss = 0;
    for (int i = 0; i < zd::NSLOT; i++) ss += h.sumsq[i];
    // packed stores: ss = sum over the full k cube of |D(k)|^2 (generator); sum_x delta^2 = N^3 sum_k |D|^2
    out->density_variance = pl->pack != zd::PACK_NONE ? ss * (double) pl->N * (double) pl->N * (double) pl->N : ss;
    pl->var_pending       = true;
    for (int j = 0; j < 3; j++) {
        // output.cpp:190-193 keeps the signed value of the largest |pos|, the first one in (z, y, x) order on a tie: the slots hold
        // (|v|, (linear index << 1) | negative) of their best record
        unsigned long long babs = 0, bkey = 0;
        for (int i = 0; i < zd::NSLOT; i++)
            if (h.maxabs[j][i] > babs || (h.maxabs[j][i] == babs && babs != 0 && h.maxkey[j][i] < bkey)) {
                babs = h.maxabs[j][i];
                bkey = h.maxkey[j][i];
            }
        double a;
        memcpy(&a, &babs, 8);
        out->max_disp[j]       = (bkey & 1ULL) ? -a : a;
        out->max_disp_index[j] = babs ? (int64_t) (bkey >> 1) : -1;
    }
    for (int k = 0; k < ZD_K_COUNT; k++) {
        out->kernel_ms[k]       = pl->kernel_ms[k];
        out->kernel_launches[k] = pl->launches[k];
        pl->kernel_ms[k]        = 0;
        pl->launches[k]         = 0;
    }
    if (pl->dens_sub) {  // the density-only half of a PLT + ZD_qdensity = 1 run: its kernels belong to this run's time
        zd_stats sb;
        if (zd_plan_stats(pl->dens_sub.get(), &sb)) return 1;
        for (int k = 0; k < ZD_K_COUNT; k++) {
            out->kernel_ms[k] += sb.kernel_ms[k];
            out->kernel_launches[k] += sb.kernel_launches[k];
        }
    }
    out->bytes_intermediate = zd_plan_exchange_bytes(pl);
    out->bytes_sent         = pl->bytes_sent;
    pl->bytes_sent          = 0;
    out->stream_factor      = pl->R;
    out->modes_cached       = 0;  // modes are regenerated per residue pass (counter-addressed RNG)
    if (pl->d_v1err) {  // ZD_Version = 1: a stream that stopped accepting pairs (k_v1_draw's guard)
        int e = 0;
        HIPCHECK(hipMemcpy(&e, pl->d_v1err, sizeof(int), hipMemcpyDeviceToHost));
        if (e) {
            fprintf(stderr, "zeldovich_hip: ZD_Version = 1 stream generator failed\n");
            return 1;
        }
    }
    return 0;
}
