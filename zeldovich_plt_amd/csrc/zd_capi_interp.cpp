// zd_capi_interp.cpp — off-lattice particle loads: zd_plan_interp and the one-call form zd_displace.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "zd_capi.h"
#include "zd_glass.h"

// ------------------------------------------------------------------------------------------------
// glass and other off-lattice loads (definition, kernels and the consumer object: zd_kernels_glass.hip)

// store, record and density buffers of zd_plan_interp: zd_displace keeps them across its sweeps
struct InterpBuffers {
    DevBuf<void> d_store, d_rec;
    DevBuf<float> d_dens;
    int chunk = 0;  // planes per x-stage call
};

static int64_t interp_record_ring(const zd_plan *pl) {  // bytes of the record (+ density) planes one x-stage call fills: ~1 GB
    const int64_t N = pl->N, Pp = (int64_t) pl->Zq * pl->pstep;
    const int64_t plane_b = N * N * (int64_t) pl->ec.recsize + (pl->p.qdensity ? N * N * 4 : 0);
    int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(Pp, ((int64_t) 1 << 30) / plane_b));
    chunk         = std::max<int64_t>(pl->pstep, chunk / pl->pstep * pl->pstep);
    return chunk * plane_b;
}

static int interp_buffers(zd_plan *pl, InterpBuffers &B) {
    const int64_t N = pl->N;
    const int64_t plane_b = N * N * (int64_t) pl->ec.recsize + (pl->p.qdensity ? N * N * 4 : 0);
    B.chunk = (int) (interp_record_ring(pl) / plane_b);
    if (B.d_store.store_alloc((size_t) zd_plan_exchange_bytes(pl)) != hipSuccess) {
        fprintf(stderr, "zeldovich_hip: cannot allocate the %.2f GB block store\n", zd_plan_exchange_bytes(pl) / 1e9);
        return 1;
    }
    if (B.d_rec.alloc((size_t) B.chunk * N * N * pl->ec.recsize) != hipSuccess || (pl->p.qdensity && B.d_dens.alloc((size_t) B.chunk * N * N) != hipSuccess)) {
        fprintf(stderr, "zeldovich_hip: cannot allocate the record planes of the interpolation\n");
        return 1;
    }
    return 0;
}

// what zd_plan_interp refuses about a plan; NULL: nothing
static const char *interp_plan_refusal(const zd_plan *pl) {
    if (pl->nranks != 1) return "zd_plan_interp runs the passes of a one-rank plan (a plan of several ranks holds a share of every plane)";
    if (pl->p.qdensity == 2 || pl->dens_only || pl->narray < 2) return "ZD_qdensity = 2 delivers no records: nothing to interpolate";
    if (pl->p.qoneslab >= 0) return "ZD_qoneslab delivers one plane: the interpolation needs all of them";
    return nullptr;
}

static int plan_interp_run(zd_plan *pl, zd_interp *it, InterpBuffers &B, hipStream_t st) {
    const int64_t N = pl->N, Pp = zd_plan_local_planes(pl);
    const size_t plane_b = (size_t) N * N * pl->ec.recsize;
    for (int r = 0; r < pl->npass; r++) {
        if (zd_plan_stage_z(pl, r, B.d_store, st) || zd_plan_stage_y(pl, B.d_store, st)) return 1;
        for (int64_t pl0 = 0; pl0 < Pp; pl0 += B.chunk) {
            const int64_t n = std::min<int64_t>(B.chunk, Pp - pl0);
            if (zd_plan_stage_x(pl, r, B.d_store, pl0, n, B.d_rec, B.d_dens, st)) return 1;
            for (int64_t i = 0; i < n; i++)
                if (zd_interp_add_plane(it, zd_plan_plane_z(pl, r, pl0 + i), (const char *) B.d_rec.get() + (size_t) i * plane_b, st)) return 1;
        }
    }
    if (hipStreamSynchronize(st) != hipSuccess) {
        fprintf(stderr, "zeldovich_hip: zd_plan_interp failed: %s\n", hipGetErrorString(hipGetLastError()));
        return 1;
    }
    return 0;
}

int zd_plan_interp(zd_plan *pl, zd_interp *it, void *hip_stream) {
    if (!pl || !it) {
        fprintf(stderr, "zeldovich_hip: zd_plan_interp needs a plan and an interpolation object\n");
        return 1;
    }
    if (const char *why = interp_plan_refusal(pl)) {
        fprintf(stderr, "zeldovich_hip: zd_plan_interp: %s\n", why);
        return 1;
    }
    int64_t ppd = 0;
    int32_t fmt = 0;
    zdglass::shape(it, &ppd, &fmt);
    if (ppd != pl->N || fmt != pl->ec.icformat) {
        fprintf(stderr, "zeldovich_hip: zd_plan_interp: the object was made for ppd = %lld, icformat = %d, the plan delivers ppd = %d, icformat = %d\n",
                (long long) ppd, fmt, pl->N, pl->ec.icformat);
        return 1;
    }
    InterpBuffers B;
    // (however the function is left: the device is idle before the buffers are released)
    struct Idle {
        ~Idle() { hipDeviceSynchronize(); }
    } idle;
    if (interp_buffers(pl, B)) return 1;
    return plan_interp_run(pl, it, B, (hipStream_t) hip_stream);
}

int zd_displace(const zd_params *p_in, const zd_pk *pk, const double *eig, int64_t eig_ppd, int32_t order, int64_t npart, const double *pos_xyz,
                int64_t tile, int64_t max_particles_per_sweep, zd_particle_cb cb, void *user, zd_stats *out) {
    if (!p_in || !pk) {
        fprintf(stderr, "zeldovich_hip: zd_displace needs parameters (p) and a power spectrum (pk)\n");
        return 1;
    }
    if (!cb) {
        fprintf(stderr, "zeldovich_hip: zd_displace: cb is a null pointer: the results are delivered through the callback\n");
        return 1;
    }
    char buf[256];
    if (const char *why = zdglass::load_refusal(p_in->ppd, p_in->icformat, order, npart, pos_xyz, tile, buf, sizeof(buf))) {
        fprintf(stderr, "zeldovich_hip: zd_displace: %s\n", why);
        return 1;
    }
    if (max_particles_per_sweep < 0) {
        fprintf(stderr, "zeldovich_hip: zd_displace: max_particles_per_sweep = %lld must be >= 0 (0: what fits in free HBM)\n", (long long) max_particles_per_sweep);
        return 1;
    }
    if (p_in->qoneslab >= 0) {
        fprintf(stderr, "zeldovich_hip: zd_displace: ZD_qoneslab = %d delivers one plane: the interpolation needs all of them\n", p_in->qoneslab);
        return 1;
    }
    if (p_in->qdensity == 2) {
        fprintf(stderr, "zeldovich_hip: zd_displace: ZD_qdensity = 2 delivers no records: nothing to interpolate\n");
        return 1;
    }
    if (p_in->ngpu > 1) {
        fprintf(stderr, "zeldovich_hip: zd_displace: ngpu = %d: the one-call form drives one GPU (several: zd_interp_* in a driver of its own)\n", p_in->ngpu);
        return 1;
    }
    const auto t0 = std::chrono::steady_clock::now();
    zd_params p = *p_in;
    p.ngpu      = 0;
    const int64_t total = npart * tile * tile * tile;
    const int64_t fixed = 4 * zdglass::hist_bins(p.ppd) + (tile == 1 ? 0 : 24 * npart);  // histogram and base positions beside a sweep
    size_t free_b = 0, total_b = 0;
    HIPCHECK(hipMemGetInfo(&free_b, &total_b));
    if (p.stream_factor <= 0) {  // the plan beside the particles: up to half of free HBM is theirs
        const int64_t want = std::min<int64_t>((int64_t) free_b / 2, fixed + zdglass::BYTES_PER_PARTICLE * std::min<int64_t>(total, zdglass::MAX_SWEEP));
        const int R = zd_choose_stream_factor(&p, 1, (int64_t) free_b - ((int64_t) 16 << 30) - want);
        if (R < 0) {
            fprintf(stderr, "zeldovich_hip: PPD %lld does not fit in %.1f GB of free HBM at any stream factor\n", (long long) p.ppd, free_b / 1e9);
            return 1;
        }
        p.stream_factor = R;
    }
    zd_plan *raw = nullptr;
    if (zd_plan_create(&p, pk, eig, eig_ppd, 0, 1, &raw)) return 1;
    const PlanPtr plan(raw);
    zd_plan *pl = plan.get();
    if (const char *why = interp_plan_refusal(pl)) {
        fprintf(stderr, "zeldovich_hip: zd_displace: %s\n", why);
        return 1;
    }
    InterpBuffers B;
    struct Idle {
        ~Idle() { hipDeviceSynchronize(); }
    } idle;
    if (interp_buffers(pl, B)) return 1;
    int64_t sweep = max_particles_per_sweep;
    if (sweep == 0) {  // what fits beside the plan and its buffers, 2 GB left to the runtime
        HIPCHECK(hipMemGetInfo(&free_b, &total_b));
        sweep = ((int64_t) free_b - ((int64_t) 2 << 30) - fixed) / zdglass::BYTES_PER_PARTICLE;
        if (sweep < 1) {
            fprintf(stderr, "zeldovich_hip: zd_displace: no HBM left for particles beside the plan (%.1f GB free)\n", free_b / 1e9);
            return 1;
        }
    }
    sweep = std::min<int64_t>(std::min<int64_t>(sweep, total), zdglass::MAX_SWEEP);
    std::vector<double> h_out;
    try {
        h_out.resize(6 * (size_t) sweep);
    } catch (const std::bad_alloc &) {
        fprintf(stderr, "zeldovich_hip: zd_displace: no host memory for the %.2f GB of one sweep's results\n", 48.0 * sweep / 1e9);
        return 1;
    }
    zd_stats st;
    memset(&st, 0, sizeof(st));
    for (int64_t first = 0; first < total; first += sweep) {
        const int64_t n = std::min(sweep, total - first);
        zd_interp *raw_it = nullptr;
        if (zdglass::create(p.ppd, p.icformat, order, npart, pos_xyz, tile, first, n, &raw_it)) return 1;
        const std::unique_ptr<zd_interp, void (*)(zd_interp *)> it(raw_it, zd_interp_destroy);
        if (plan_interp_run(pl, it.get(), B, 0) || zd_interp_result(it.get(), h_out.data()) || zd_plan_stats(pl, &st)) return 1;
        if (cb(user, first, n, h_out.data())) {
            fprintf(stderr, "zeldovich_hip: zd_displace: the particle callback failed at particle %lld\n", (long long) first);
            return 1;
        }
    }
    st.seconds_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (out) *out = st;
    return 0;
}
