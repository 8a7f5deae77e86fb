// zd_capi_generate.cpp — the single-GPU driver zd_generate (= ZeldovichZ + ZeldovichXY, src/zeldovich.cpp:517-695): the record ring and
// the writer thread.
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <deque>
#include <functional>
#include <mutex>
#include <thread>

#include "zd_capi.h"

// ------------------------------------------------------------------------------------------------
// zd_generate, and zd_generate_field (fs != NULL: the modes come from the caller's field; its refusals have been asked)
int generate_impl(const zd_params *p_in, const zd_pk *pk, const double *eig, int64_t eig_ppd, zd_slab_cb cb, void *user, zd_stats *out,
                  const FieldSpec *fs) {
    // ZD_NumGPU: one host thread per GPU, exchange inside the library (zd_multi.cpp).  (ZD_qoneslab finishes ONE plane of one
    // pass and reports the reductions of that slab alone, output.cpp:197: that is this single-GPU path's job.)
    if ((p_in->q2LPT || p_in->lpt2_dealias || p_in->q3LPT) && lpt2_route_check(p_in, p_in->ngpu > 1 ? p_in->ngpu : 1, 0)) return 1;
    if (p_in->ngpu > 1 && p_in->qoneslab < 0) {
        int ndev = 0;
        HIPCHECK(hipGetDeviceCount(&ndev));
        // RCCL between distinct GPUs; when the ranks have to share devices (fewer GPUs than ranks: test boxes) they
        // pull their slices with device copies instead
        return zd_generate_multi(p_in, pk, eig, eig_ppd, cb, user, out, ndev >= p_in->ngpu ? 0 : 1);
    }
    zd_params p = *p_in;
    const int64_t N = p.ppd;
    size_t free_b = 0, total_b = 0;
    HIPCHECK(hipMemGetInfo(&free_b, &total_b));
    if (p.q2LPT && p.lpt2_dealias && !lpt2_round_fits(&p, (int64_t) free_b - ((int64_t) 16 << 30))) return 1;
    const bool field2 = fs && fs->order == 2;  // second order on the field: D(k) stays resident beside the round and beside S(k)
    if (field2 && !field_lpt2_fits(&p, (int64_t) free_b - ((int64_t) 16 << 30))) return 1;
    if (p.stream_factor <= 0) {
        // leave 16 GB for tables, the folded-input slabs (~3 GB), the record ring (8 GB) and the runtime
        int64_t budget = (int64_t) free_b - ((int64_t) 16 << 30);
        zd_params pq = p;
        if (fs) {  // a PhiK plan runs on the reference's arrays, beside PhiK (the intake's workspace is gone by then)
            pq.store_mode = ZD_STORE_REFERENCE;
            budget -= fnl_phik_bytes(N);
        }
        const int R = zd_choose_stream_factor(&pq, 1, budget);
        if (R < 0) {
            fprintf(stderr, "zeldovich_hip: PPD %lld does not fit in %.1f GB of free HBM at any stream factor\n",
                    (long long) N, free_b / 1e9);
            return 1;
        }
        p.stream_factor = R;
    }
    // ---- f_NL: phi field -> local transform -> Fourier space again (zeldovich.cpp:945-960) ----
    DevBuf<cplx> d_phik;  // PhiK or S(k), until the plan exists and owns it
    if (p.f_NL != 0.) {
        if (make_phik(&p, pk, d_phik)) return 1;
        HIPCHECK(hipMemGetInfo(&free_b, &total_b));
        if (p_in->stream_factor <= 0) {
            // (PhiK is allocated by now: it is part of what the chooser counts)
            const int R2 = zd_choose_stream_factor(&p, 1, (int64_t) free_b - ((int64_t) 16 << 30) + fnl_phik_bytes(N));
            if (R2 < 0) return 1;
            p.stream_factor = R2;
        }
    }
    // ---- second order on a caller-supplied field (zd_kernels_lpt2_field.hip): the intake first, the round reads its D(k) ----
    DevBuf<cplx> d_field;
    if (field2 && make_field_phik(&p, pk, *fs, d_field)) return 1;
    // ---- ZD_q2LPT: the second-order round (zd_kernels_lpt2.hip); the chooser has counted S(k) beside the passes' stores ----
    if (p.q2LPT && make_lpt2_source(&p, pk, d_phik, d_field)) return 1;
    // ---- ZD_q3LPT: the third-order round (zd_kernels_lpt3.hip); P3(k) and C_x,y,z(k) stay beside S(k), counted likewise ----
    DevBuf<cplx> d_lpt3[4];
    if (p.q3LPT && make_lpt3_sources(&p, pk, d_phik, d_lpt3)) return 1;
    // ---- a caller-supplied field (zd_kernels_field.hip): PhiK = its modes; no draw is made ----
    if (fs && !field2 && make_field_phik(&p, pk, *fs, d_phik)) return 1;
    PlanPtr plan;
    if (plan_create_ex(&p, pk, eig, eig_ppd, 0, 1, 0, d_phik, plan, fs != nullptr, d_field)) return 1;
    zd_plan *pl      = plan.get();
    if (field2) {  // the plan owns D(k) where PhiK goes, and S(k)
        pl->d_lpt2_sk_owned = std::move(d_phik);
        pl->d_phik_owned    = std::move(d_field);
    } else {
        pl->d_phik_owned = std::move(d_phik);
    }
    if (p.q3LPT) adopt_lpt3(pl, d_lpt3);
    const int R = pl->R, recsize = pl->ec.recsize, npass = pl->npass, pstep = pl->pstep;
    const int64_t Pp = zd_plan_local_planes(pl);  // planes delivered per pass
    const bool want_rec = pl->narray >= 2 && !pl->dens_only, want_dens = p.qdensity != 0;

    // Delivery (WriteParticlesSlab's role, src/output.cpp:207-224) is asynchronous: NB = 2 record buffers on the device
    // and in pinned host memory; chunk i is produced into buffer i % 2 on the compute stream, copied D2H on a copy stream
    // and handed to a writer thread that runs the callback plane by plane — the x stage of chunk i+1, the PCIe copy of
    // chunk i and the callback of chunk i-1 overlap (round 1 serialised the three).  The callback is still invoked
    // from ONE thread, in production order.
    constexpr int NB = 2;
    DevBuf<void> d_store, d_rec[NB];
    DevBuf<float> d_dens[NB];
    PinnedBuf<char> h_rec[NB];
    PinnedBuf<float> h_dens[NB];
    Event ev_x[NB], ev_c[NB];
    Stream s_copy;
    hipStream_t st = 0;
    // planes handed over per x-stage launch (a multiple of the plane step)
    const int64_t plane_b = N * N * (int64_t) (want_rec ? recsize : 0) + (want_dens ? N * N * 4 : 0);
    // (with a host callback each buffer is mirrored in pinned host memory: 1 GB; the NULL sink takes 8 GB so that an
    // x-stage launch covers several planes even at PPD=4096, where one plane of records is 537 MB)
    const int64_t ring_b = cb ? ((int64_t) 1 << 30) : ((int64_t) 8 << 30);
    int chunk = (int) std::max<int64_t>(1, std::min<int64_t>(Pp, ring_b / std::max<int64_t>(plane_b, 1)));
    chunk     = std::max(pstep, chunk / pstep * pstep);
    const int nbuf = cb ? NB : 1;
    struct Item {
        int slot, pass;
        int64_t first, n, only;  // only >= 0: deliver just that local plane (ZD_qoneslab)
    };
    std::mutex mu;
    std::condition_variable cv;
    std::deque<Item> queue;
    bool slot_busy[NB] = {false, false}, done = false;
    std::atomic<int> cb_failed{0};
    std::thread writer;
    // However the function is left: the writer is joined and the device idle before anything above — all of which the writer or
    // queued work may still read — is released
    struct Quiesce {
        std::function<void()> f;
        ~Quiesce() { f(); }
    } quiesce{[&] {
        if (writer.joinable()) {
            {
                std::lock_guard<std::mutex> lk(mu);
                done = true;
                queue.clear();
            }
            cv.notify_all();
            writer.join();
        }
        hipDeviceSynchronize();
    }};
    if (d_store.store_alloc((size_t) zd_plan_exchange_bytes(pl)) != hipSuccess) {
        fprintf(stderr, "zeldovich_hip: cannot allocate the %.2f GB block store\n", zd_plan_exchange_bytes(pl) / 1e9);
        return 1;
    }
    for (int b2 = 0; b2 < nbuf; b2++) {
        if (want_rec && d_rec[b2].alloc((size_t) chunk * N * N * recsize) != hipSuccess) return 1;
        if (want_dens && d_dens[b2].alloc((size_t) chunk * N * N) != hipSuccess) return 1;
        if (!cb) continue;
        if (want_rec && h_rec[b2].alloc((size_t) chunk * N * N * recsize) != hipSuccess) return 1;
        if (want_dens && h_dens[b2].alloc((size_t) chunk * N * N) != hipSuccess) return 1;
        if (ev_x[b2].create(hipEventDisableTiming) != hipSuccess || ev_c[b2].create(hipEventDisableTiming) != hipSuccess) return 1;
    }
    if (cb && s_copy.create() != hipSuccess) return 1;
    if (hipDeviceSynchronize() != hipSuccess) return 1;
    if (cb) {
        writer = std::thread([&]() {
            for (;;) {
                Item it;
                {
                    std::unique_lock<std::mutex> lk(mu);
                    cv.wait(lk, [&] { return done || !queue.empty(); });
                    if (queue.empty()) return;
                    it = queue.front();
                    queue.pop_front();
                }
                if (hipEventSynchronize(ev_c[it.slot]) != hipSuccess) cb_failed.store(1);
                for (int64_t i = 0; i < it.n && !cb_failed.load(); i++) {
                    if (it.only >= 0 && it.first + i != it.only) continue;
                    const int64_t z = zd_plan_plane_z(pl, it.pass, it.first + i);
                    if (cb(user, z, N * N, want_rec ? h_rec[it.slot] + (size_t) i * N * N * recsize : nullptr,
                           want_dens ? h_dens[it.slot] + (size_t) i * N * N : nullptr))
                        cb_failed.store(1);
                }
                {
                    std::lock_guard<std::mutex> lk(mu);
                    slot_busy[it.slot] = false;
                }
                cv.notify_all();
            }
        });
    }
    const auto t0 = std::chrono::steady_clock::now();
    bool fail = false;
    // ZD_qoneslab (zeldovich.cpp:669): only that slab is wanted -> only its pass and its store plane are finished
    int want_pass = -1;
    int64_t want_plane = -1;
    if (p.qoneslab >= 0) {
        const int r = p.qoneslab % R;
        want_pass   = r % npass;
        want_plane  = (int64_t) (p.qoneslab / R) * pstep + r / npass;
    }
    long long nchunk = 0;
    for (int r = 0; r < npass && !fail; r++) {
        if (want_pass >= 0 && r != want_pass) continue;
        if (zd_plan_stage_z(pl, r, d_store, st) || zd_plan_stage_y(pl, d_store, st)) {
            fail = true;
            break;
        }
        for (int64_t pl0 = 0; pl0 < Pp && !fail; pl0 += chunk) {
            int64_t first = pl0, n = std::min<int64_t>(chunk, Pp - pl0);
            if (want_plane >= 0) {
                if (want_plane < pl0 || want_plane >= pl0 + n) continue;
                first = want_plane / pstep * pstep;
                n     = pstep;
            }
            const int slot = cb ? (int) (nchunk++ % NB) : 0;
            if (cb) {  // the writer has finished with this slot's host buffer (chunk i - 2) — and with it its D2H copy
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return !slot_busy[slot] || cb_failed.load(); });
                if (cb_failed.load()) {
                    fail = true;
                    break;
                }
                slot_busy[slot] = true;
            }
            if (zd_plan_stage_x(pl, r, d_store, first, n, d_rec[slot], d_dens[slot], st)) {
                fail = true;
                break;
            }
            if (cb) {
                if (hipEventRecord(ev_x[slot], st) != hipSuccess || hipStreamWaitEvent(s_copy, ev_x[slot], 0) != hipSuccess) fail = true;
                if (want_rec && hipMemcpyAsync(h_rec[slot], d_rec[slot], (size_t) n * N * N * recsize, hipMemcpyDeviceToHost, s_copy) != hipSuccess) fail = true;
                if (want_dens && hipMemcpyAsync(h_dens[slot], d_dens[slot], (size_t) n * N * N * 4, hipMemcpyDeviceToHost, s_copy) != hipSuccess) fail = true;
                if (hipEventRecord(ev_c[slot], s_copy) != hipSuccess) fail = true;
                {
                    std::lock_guard<std::mutex> lk(mu);
                    queue.push_back(Item{slot, r, first, n, want_plane});
                }
                cv.notify_all();
            }
        }
    }
    if (cb) {  // drain
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return (queue.empty() && !slot_busy[0] && !slot_busy[1]) || cb_failed.load(); });
        }
        if (cb_failed.load()) fail = true;
    }
    if (fail || zd_plan_stats(pl, out)) return 1;
    out->seconds_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return 0;
}
int zd_generate(const zd_params *p_in, const zd_pk *pk, const double *eig, int64_t eig_ppd, zd_slab_cb cb,
                void *user, zd_stats *out) {
    return generate_impl(p_in, pk, eig, eig_ppd, cb, user, out, nullptr);
}
