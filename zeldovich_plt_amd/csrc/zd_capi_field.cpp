// zd_capi_field.cpp — a caller-supplied density or white-noise field: its intake (zd_generate_field, zd_plan_create_field), the second
// order on it (zd_generate_field_lpt, zd_plan_create_field_lpt) and the adjoint of a first-order field run (zd_field_vjp).
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "zd_capi.h"

// ---- a caller-supplied density or white-noise field (definition and kernels: zd_kernels_field.hip) ----
// what a field run refuses, one line that starts "zeldovich_hip: ZD_Field" and names the other option; asked before the GPU is touched
static int field_refused(const zd_params *p, const zd_pk *pk, const FieldSpec &f) {
    char why[256] = "";
    const int64_t N = p->ppd;
    if (!f.field) snprintf(why, sizeof why, "no field given (NULL)");
    else if (f.kind != ZD_FIELD_DENSITY && f.kind != ZD_FIELD_WHITE) snprintf(why, sizeof why, "kind = %d (ZD_FIELD_DENSITY or ZD_FIELD_WHITE expected)", f.kind);
    else if (f.dtype != ZD_FIELD_F32 && f.dtype != ZD_FIELD_F64) snprintf(why, sizeof why, "dtype = %d (ZD_FIELD_F32 or ZD_FIELD_F64 expected)", f.dtype);
    else if (p->f_NL != 0.) snprintf(why, sizeof why, "is not supported together with ZD_f_NL != 0 (the phi round makes PhiK from its own draws)");
    else if (p->q2LPT || p->q3LPT || p->lpt2_dealias)
        snprintf(why, sizeof why, "is not supported together with %s (its final pass keeps S(k) where PhiK goes)", p->q3LPT ? "ZD_q3LPT" : "ZD_q2LPT");
    else if (p->version == 1) snprintf(why, sizeof why, "is not supported together with ZD_Version = 1 (a field run makes no draw; leave ZD_Version at 2)");
    else if (pk->fixed_power) snprintf(why, sizeof why, "is not supported together with ZD_qPk_fix_to_mean (the amplitudes are the field's own)");
    else if (p->ngpu > 1) snprintf(why, sizeof why, "runs on one GPU: ZD_NumGPU = %d", p->ngpu);
    else if (!is_pow2(N) || N < 32 || N > 2048)
        snprintf(why, sizeof why, "needs PPD a power of two in [32, 2048], got PPD = %lld (composite and convolution sizes: not yet)", (long long) N);
    if (!why[0]) return 0;
    fprintf(stderr, "zeldovich_hip: ZD_Field %s\n", why);
    return 1;
}
// ... and what the order argument of zd_generate_field_lpt / zd_plan_create_field_lpt adds (definition: zd_kernels_lpt2_field.hip): the
// parameters come as a first-order field run's (ZD_q2LPT in them keeps its refusal above); with order = 2 whatever ZD_q2LPT refuses
// (zd_route.h lpt2_refusal) is refused here, in a field run's words.  The size comes before the field is looked at.
static int field_order_refused(const zd_params *p, const zd_pk *pk, const FieldSpec &f) {
    char why[256] = "";
    const int64_t N = p->ppd;
    if (f.order == 3) snprintf(why, sizeof why, "order = 3: third order (ZD_q3LPT) on a field is not built");
    else if (f.order != 1 && f.order != 2) snprintf(why, sizeof why, "order = %d (1: Zel'dovich, 2: second order expected)", f.order);
    else if (f.order == 2 && !(p->q2LPT || p->q3LPT || p->lpt2_dealias) && is_pow2(N) && N > 1024 && N <= 2048) {
        zd_params pq = *p;
        pq.q2LPT     = 1;
        snprintf(why, sizeof why, "order = 2 needs PPD a power of two in [32, 1024], got PPD = %lld: the second-order round alone would hold %.0f GB",
                 (long long) N, field_lpt2_round_bytes(&pq) / 1e9);
    }
    if (why[0]) {
        fprintf(stderr, "zeldovich_hip: ZD_Field %s\n", why);
        return 1;
    }
    if (field_refused(p, pk, f)) return 1;
    if (f.order == 1) return 0;
    if (p->qPLT) snprintf(why, sizeof why, "order = 2 is not supported together with ZD_qPLT (the second order rides on the ZA fields)");
    else if (p->qdensity != 0) snprintf(why, sizeof why, "order = 2 is not supported together with a density output (ZD_qdensity = %d)", p->qdensity);
    else if (!zd::nyquist_dead(p))
        snprintf(why, sizeof why, "order = 2 is not supported with live Nyquist planes (ZD_CornerModes with ZD_k_cutoff != 1): the source would not be real");
    else {  // (anything lpt2_refusal learns to refuse later)
        zd_params pq = *p;
        pq.q2LPT     = 1;
        if (const char *r = zd::lpt2_refusal(&pq, 1)) snprintf(why, sizeof why, "order = 2: %s", r);
    }
    if (!why[0]) return 0;
    fprintf(stderr, "zeldovich_hip: ZD_Field %s\n", why);
    return 1;
}
// the second-order round with D(k) resident beside it against the free memory, asked before anything is built (the figure is the message)
int field_lpt2_fits(const zd_params *p, int64_t free_bytes) {
    if (field_lpt2_round_bytes(p) <= free_bytes) return 1;
    fprintf(stderr, "zeldovich_hip: ZD_Field order = 2 needs %.1f GB of HBM at PPD %lld (the second-order round %.1f GB, the modes of the field %.1f GB beside it), %.1f GB are free\n",
            field_lpt2_round_bytes(p) / 1e9, (long long) p->ppd, lpt2_round_bytes(p) / 1e9, fnl_phik_bytes(p->ppd) / 1e9, free_bytes / 1e9);
    return 0;
}
// planes of the intake's workspace (complex x-stage output) and of the staging buffer of a host field: at least 4, at most 256 MB
static int field_ws_planes(int64_t N) { return (int) std::min<int64_t>(N, std::max<int64_t>(4, ((int64_t) 1 << 28) / (N * N * 16))); }
// amp[|k|^2] over the integer |k|^2 the zero rule of g can leave alive: 1 / N^3, or sqrt(power(|k|) / N^3) for white noise (the intake
// and its adjoint, zd_field_vjp)
static std::vector<double> field_amp_table(const zd::GenConst &g, const zd_pk *pk, int32_t kind) {
    const long long all = 3LL * g.half * g.half + 1, n = std::max<long long>(1, g.corner_modes ? all : std::min<long long>(all, g.k2i_cut));
    const double n3 = (double) g.N * (double) g.N * (double) g.N;
    std::vector<double> amp((size_t) n, 1.0 / n3);
    if (kind == ZD_FIELD_WHITE)
        for (long long i = 1; i < n; i++) amp[(size_t) i] = sqrt(zd_pk_power(pk, sqrt((double) i * g.fundamental2)) / n3);
    amp[0] = 0.0;
    return amp;
}
// The field -> d_phik = D(k)[ky][kz][x] for the half-space rows, zero rule and amplitude applied (owned by the caller, untouched on
// failure).  PhiK is the only N^3-sized allocation; x and y stages run chunk by chunk through the workspace, a host field through a
// staging buffer of as many planes; the z lines then run in place on PhiK.
int make_field_phik(const zd_params *p, const zd_pk *pk, const FieldSpec &f, DevBuf<cplx> &d_phik) {
    const int64_t N = p->ppd, P = field_ws_planes(N), esz = f.dtype == ZD_FIELD_F32 ? 4 : 8;
    const int64_t phik_b = fnl_phik_bytes(N), ws_b = P * N * N * 16, stage_b = f.on_device ? 0 : P * N * N * esz;
    size_t free_b = 0, total_b = 0;
    HIPCHECK(hipMemGetInfo(&free_b, &total_b));
    DevBuf<cplx> d_out, d_ws, d_tw;
    DevBuf<char> d_stage;
    DevBuf<double> d_amp;
    if (phik_b + ws_b + stage_b > (int64_t) free_b || d_out.store_alloc((size_t) (N / 2) * N * N) != hipSuccess
        || d_ws.store_alloc((size_t) P * N * N) != hipSuccess || (stage_b && d_stage.alloc((size_t) stage_b) != hipSuccess)) {
        fprintf(stderr, "zeldovich_hip: ZD_Field needs %.2f GB of HBM for the modes of the field at PPD %lld (%.2f GB of them the workspace), %.2f GB are free\n",
                (phik_b + ws_b + stage_b) / 1e9, (long long) N, (ws_b + stage_b) / 1e9, free_b / 1e9);
        return 1;
    }
    zd::GenConst g;
    gen_zero_rule(g, p);
    HIPCHECK(upload(d_amp, field_amp_table(g, pk, f.kind)));
    HIPCHECK(upload(d_tw, make_twiddles((int) N)));
    const hipStream_t st = 0;
    for (int64_t z0 = 0; z0 < N; z0 += P) {
        const int np = (int) std::min<int64_t>(P, N - z0);
        const char *src = (const char *) f.field + (size_t) z0 * N * N * esz;
        if (!f.on_device) {  // (the copy returns when the planes are staged; the kernels of the chunk before are ordered before it)
            HIPCHECK(hipMemcpyAsync(d_stage, src, (size_t) np * N * N * esz, hipMemcpyHostToDevice, st));
            src = d_stage;
        }
        if (zd::launch_field_x((int) N, src, f.dtype == ZD_FIELD_F32, d_tw, d_ws, np, st)) return 1;
        if (zd::launch_field_y((int) N, d_tw, d_ws, (int) z0, np, d_out, st)) return 1;
    }
    if (zd::launch_field_z(g, d_tw, d_amp, d_out, st)) return 1;
    if (hipStreamSynchronize(st) != hipSuccess) {
        fprintf(stderr, "zeldovich_hip: ZD_Field: the intake failed: %s\n", hipGetErrorString(hipGetLastError()));
        return 1;
    }
    d_phik = std::move(d_out);
    return 0;
}

int zd_generate_field(const zd_params *p, const zd_pk *pk, const double *eig, int64_t eig_ppd, int32_t kind, int32_t dtype, const void *field,
                      int32_t field_on_device, zd_slab_cb cb, void *user, zd_stats *out) {
    if (!p || !pk || !out) {
        fprintf(stderr, "zeldovich_hip: ZD_Field: zd_generate_field needs parameters, a power spectrum and a zd_stats\n");
        return 1;
    }
    const FieldSpec fs{kind, dtype, field, field_on_device};
    if (field_refused(p, pk, fs)) return 1;
    return generate_impl(p, pk, eig, eig_ppd, cb, user, out, &fs);
}
int zd_plan_create_field(const zd_params *p, const zd_pk *pk, const double *eig, int64_t eig_ppd, int32_t kind, int32_t dtype, const void *field,
                         int32_t field_on_device, zd_plan **out) {
    if (!p || !pk || !out) {
        fprintf(stderr, "zeldovich_hip: ZD_Field: zd_plan_create_field needs parameters, a power spectrum and a place for the plan\n");
        return 1;
    }
    const FieldSpec fs{kind, dtype, field, field_on_device};
    if (field_refused(p, pk, fs)) return 1;
    DevBuf<cplx> d_phik;
    if (make_field_phik(p, pk, fs, d_phik)) return 1;
    PlanPtr pl;
    if (plan_create_ex(p, pk, eig, eig_ppd, 0, 1, 0, d_phik, pl, true)) return 1;
    pl->d_phik_owned = std::move(d_phik);
    *out             = pl.release();
    return 0;
}

// ---- second order on the field: order 1 is the call above without an eigenmode table; order 2 runs the q2LPT job with D(k) read from
// the field (zd_kernels_lpt2_field.hip).  The plan owns D(k) (d_phik_owned, GenConst::phik) and S(k) (d_lpt2_sk_owned, GenConst::lpt2_sk)
int zd_generate_field_lpt(const zd_params *p, const zd_pk *pk, int32_t kind, int32_t dtype, const void *field, int32_t field_on_device,
                          int32_t order, zd_slab_cb cb, void *user, zd_stats *out) {
    if (!p || !pk || !out) {
        fprintf(stderr, "zeldovich_hip: ZD_Field: zd_generate_field_lpt needs parameters, a power spectrum and a zd_stats\n");
        return 1;
    }
    const FieldSpec fs{kind, dtype, field, field_on_device, order};
    if (field_order_refused(p, pk, fs)) return 1;
    zd_params pq = *p;
    pq.q2LPT     = order == 2;
    return generate_impl(&pq, pk, nullptr, 0, cb, user, out, &fs);
}
int zd_plan_create_field_lpt(const zd_params *p, const zd_pk *pk, int32_t kind, int32_t dtype, const void *field, int32_t field_on_device,
                             int32_t order, zd_plan **out) {
    if (!p || !pk || !out) {
        fprintf(stderr, "zeldovich_hip: ZD_Field: zd_plan_create_field_lpt needs parameters, a power spectrum and a place for the plan\n");
        return 1;
    }
    const FieldSpec fs{kind, dtype, field, field_on_device, order};
    if (field_order_refused(p, pk, fs)) return 1;
    if (order == 1) return zd_plan_create_field(p, pk, nullptr, 0, kind, dtype, field, field_on_device, out);
    zd_params pq = *p;
    pq.q2LPT     = 1;
    size_t free_b = 0, total_b = 0;
    HIPCHECK(hipMemGetInfo(&free_b, &total_b));
    if (lpt2_route_check(&pq, 1, 0) || !field_lpt2_fits(&pq, (int64_t) free_b)) return 1;
    DevBuf<cplx> d_field, d_sk;
    if (make_field_phik(&pq, pk, fs, d_field) || make_lpt2_source(&pq, pk, d_sk, d_field)) return 1;
    PlanPtr pl;
    if (plan_create_ex(&pq, pk, nullptr, 0, 0, 1, 0, d_sk, pl, true, d_field)) return 1;
    pl->d_phik_owned    = std::move(d_field);
    pl->d_lpt2_sk_owned = std::move(d_sk);
    *out                = pl.release();
    return 0;
}

// Adjoint of a field run (definition and kernels: zd_kernels_field_adj.hip).  Stateless: the Jacobian does not depend on the field, so
// neither a plan nor PhiK is built; the GenConst is a field plan's (zero rule, growth constants, eigenmode table) and amp the intake's.
int zd_field_vjp(const zd_params *p, const zd_pk *pk, const double *eig, int64_t eig_ppd, int32_t kind, int32_t dtype, const void *g_q,
                 const void *g_v, const void *g_dens, int32_t cot_on_device, double *out_field, int32_t out_on_device, zd_stats *stats) {
    if (!p || !pk || !out_field) {
        fprintf(stderr, "zeldovich_hip: ZD_Field: zd_field_vjp needs parameters, a power spectrum and a place for the gradient\n");
        return 1;
    }
    const void *any = g_q ? g_q : g_v ? g_v : g_dens;
    if (!any) {
        fprintf(stderr, "zeldovich_hip: ZD_Field: zd_field_vjp needs a cotangent (g_q, g_v and g_dens are all NULL)\n");
        return 1;
    }
    if (field_refused(p, pk, FieldSpec{kind, dtype, any, cot_on_device})) return 1;
    if (p->qPLT && (!eig || eig_ppd <= 0)) {
        fprintf(stderr, "zeldovich_hip: ZD_Field: ZD_qPLT set but no eigenmode table given\n");
        return 1;
    }
    const auto t0 = std::chrono::steady_clock::now();
    const int64_t N = p->ppd, P = field_ws_planes(N), esz = dtype == ZD_FIELD_F32 ? 4 : 8, plane = N * N;
    const bool two = !p->qPLT && g_q && g_v;  // ZA: g_q,j + f g_v,j formed on load, from two arrays
    // T, the half-space array between the y and z lines of a forward pass, is as large as the result and dead before the inverse
    // writes it: a result on the device lends its storage (16-byte aligned, as every allocation is)
    const bool own_T = !(out_on_device && (uintptr_t) out_field % 16 == 0);
    const int64_t h_b = fnl_phik_bytes(N), ws_b = P * plane * 16, arrays_b = (own_T ? 2 : 1) * h_b;
    const int64_t in_b = cot_on_device ? 0 : P * plane * esz * (g_q || g_v ? 3 : 1), out_b = out_on_device ? 0 : P * plane * 8;
    const int64_t stage_b = in_b * (two ? 2 : 1) + out_b;
    size_t free_b = 0, total_b = 0;
    HIPCHECK(hipMemGetInfo(&free_b, &total_b));
    DevBuf<cplx> d_H, d_T, d_ws, d_tw;
    DevBuf<char> d_ina, d_inb;
    DevBuf<double> d_amp, d_eig, d_ostage;
    if (arrays_b + ws_b + stage_b > (int64_t) free_b || d_H.store_alloc((size_t) (N / 2) * plane) != hipSuccess
        || (own_T && d_T.store_alloc((size_t) (N / 2) * plane) != hipSuccess) || d_ws.store_alloc((size_t) P * plane) != hipSuccess
        || (in_b && d_ina.alloc((size_t) in_b) != hipSuccess) || (in_b && two && d_inb.alloc((size_t) in_b) != hipSuccess)
        || (out_b && d_ostage.alloc((size_t) P * plane) != hipSuccess)) {
        fprintf(stderr, "zeldovich_hip: ZD_Field needs %.2f GB of HBM for the adjoint at PPD %lld (%d half-space array%s of %.2f GB, %.2f GB of workspace and staging), %.2f GB are free\n",
                (arrays_b + ws_b + stage_b) / 1e9, (long long) N, own_T ? 2 : 1, own_T ? "s" : "", h_b / 1e9, (ws_b + stage_b) / 1e9, free_b / 1e9);
        return 1;
    }
    zd::GenConst g;
    gen_zero_rule(g, p);
    gen_growth(g, p);
    if (p->qPLT) {
        HIPCHECK(upload(d_eig, eig, (size_t) eig_ppd * eig_ppd * (eig_ppd / 2 + 1) * 4));
        g.eig     = d_eig;
        g.eig_ppd = eig_ppd;
    }
    HIPCHECK(upload(d_amp, field_amp_table(g, pk, kind)));
    HIPCHECK(upload(d_tw, make_twiddles((int) N)));
    // one pass per real component array: fa a + fb b, component comp of nc, coefficient kind of launch_field_adj_z
    struct Pass {
        const void *a, *b;
        double fa, fb;
        int nc, comp, coef;
    };
    std::vector<Pass> passes;
    for (int c = 0; c < 3; c++) {
        if (!p->qPLT) {  // f is one number: the velocities' cotangent joins the displacements' on load
            if (g_q || g_v) passes.push_back(Pass{g_q ? g_q : g_v, two ? g_v : nullptr, g_q ? 1.0 : g.target_f, g.target_f, 3, c, 0});
        } else {
            if (g_q) passes.push_back(Pass{g_q, nullptr, 1.0, 0.0, 3, c, 0});
            if (g_v) passes.push_back(Pass{g_v, nullptr, 1.0, 0.0, 3, c, 1});
        }
    }
    if (g_dens) passes.push_back(Pass{g_dens, nullptr, 1.0, 0.0, 1, 0, 2});
    const hipStream_t st = 0;
    const int is_f32 = dtype == ZD_FIELD_F32;
    cplx *const T = own_T ? d_T.get() : (cplx *) out_field;
    for (size_t i = 0; i < passes.size(); i++) {
        const Pass &ps = passes[i];
        for (int64_t z0 = 0; z0 < N; z0 += P) {
            const int np = (int) std::min<int64_t>(P, N - z0);
            const size_t off = (size_t) z0 * plane * ps.nc * esz, nb = (size_t) np * plane * ps.nc * esz;
            const char *a = (const char *) ps.a + off, *b = ps.b ? (const char *) ps.b + off : nullptr;
            if (!cot_on_device) {  // (the copy returns when the planes are staged; the kernels of the chunk before are ordered before it)
                HIPCHECK(hipMemcpyAsync(d_ina, a, nb, hipMemcpyHostToDevice, st));
                a = d_ina;
                if (b) {
                    HIPCHECK(hipMemcpyAsync(d_inb, b, nb, hipMemcpyHostToDevice, st));
                    b = d_inb;
                }
            }
            if (zd::launch_field_adj_x((int) N, a, b, ps.fa, ps.fb, is_f32, ps.nc, ps.comp, d_tw, d_ws, np, st)) return 1;
            if (zd::launch_field_y((int) N, d_tw, d_ws, (int) z0, np, T, st)) return 1;
        }
        if (zd::launch_field_adj_z(g, d_tw, d_amp, T, d_H, ps.comp, ps.coef, i == 0, st)) return 1;
    }
    if (zd::launch_field_adj_iz((int) N, d_tw, d_H, st)) return 1;
    for (int64_t z0 = 0; z0 < N; z0 += P) {
        const int np = (int) std::min<int64_t>(P, N - z0);
        double *dst = out_field + (size_t) z0 * plane;
        if (zd::launch_field_adj_iy((int) N, d_tw, d_H, (int) z0, np, d_ws, st)) return 1;
        if (zd::launch_field_adj_ix((int) N, d_tw, d_ws, out_on_device ? dst : d_ostage.get(), np, st)) return 1;
        if (!out_on_device) HIPCHECK(hipMemcpyAsync(dst, d_ostage, (size_t) np * plane * 8, hipMemcpyDeviceToHost, st));
    }
    if (hipStreamSynchronize(st) != hipSuccess) {
        fprintf(stderr, "zeldovich_hip: ZD_Field: the adjoint failed: %s\n", hipGetErrorString(hipGetLastError()));
        return 1;
    }
    if (stats) {
        memset(stats, 0, sizeof(*stats));
        stats->stream_factor      = 1;
        stats->bytes_intermediate = arrays_b + ws_b + stage_b;
        stats->seconds_total      = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    return 0;
}
