// zd_capi_diag.cpp — the dispatch report, the allocator of the large device buffers, and the device test hooks (-DZD_TESTING,
// -DZD_TUNING).
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "zd_capi.h"
#include "zd_plt.h"

// ---- dispatch diagnostics (zd_launch.h DispatchSite) and the depth of the table probes on this thread (zd_launch.h TableProbe) ----
namespace zd {
thread_local int table_probe_depth = 0;
static std::atomic<DispatchSite *> g_dispatch_head{nullptr};
DispatchSite::DispatchSite(const char *f, int l) : func(f), line(l) {
    DispatchSite *h = g_dispatch_head.load(std::memory_order_relaxed);
    do {
        next = h;
    } while (!g_dispatch_head.compare_exchange_weak(h, this, std::memory_order_release, std::memory_order_relaxed));
}
}  // namespace zd

int64_t zd_dispatch_report(char *buf, int64_t cap) {
    int64_t need = 0, w = 0;  // bytes the whole report takes / bytes written: whole lines only, nothing after the first that does not fit
    for (zd::DispatchSite *s = zd::g_dispatch_head.load(std::memory_order_acquire); s; s = s->next) {
        char line[1024];
        int n = snprintf(line, sizeof line, "%lld\t%d\t%s\n", s->count.load(std::memory_order_relaxed), s->line, s->func);
        if (n <= 0) continue;
        if (n >= (int) sizeof line) {  // (a launcher name longer than the line: snprintf returns what it WOULD have written)
            n = (int) sizeof line - 1;
            line[n - 1] = '\n';
        }
        if (buf && w == need && w + n < cap) {
            memcpy(buf + w, line, (size_t) n);
            w += n;
        }
        need += n;
    }
    if (buf && cap > 0) buf[w] = 0;  // (w < cap: a C string of at most cap - 1 bytes, every byte of it written)
    return need + 1;
}

// Large device buffers the kernels only partly write (stores, exchange rings, phi fields).  In the -DZD_TESTING library
// zd_test_poison(1) makes every such allocation start out as NaN bytes, so that a kernel reading something no kernel wrote
// shows up in the parity tests instead of depending on what a fresh hipMalloc happens to contain.
#ifdef ZD_TESTING
static std::atomic<int> g_poison{0};
void zd_test_poison(int on) { g_poison.store(on); }
// w = 4: plans of the ZA field store at PPD = 1024 created from now on pair their ring rows in groups of 4 (two pairs per y workgroup,
// the form PPD = 4096 runs) instead of ring_pair_w's 8; 0: back to the table
std::atomic<int> g_ring_pair_w{0};
void zd_test_ring_pair_w(int w) { g_ring_pair_w.store(w); }
#endif
hipError_t zd_store_alloc(void **p, size_t bytes) {
    hipError_t e = hipMalloc(p, bytes);
#ifdef ZD_TESTING
    if (e == hipSuccess && g_poison.load()) e = hipMemset(*p, 0xFF, bytes);
#endif
    return e;
}

#ifdef ZD_TESTING
int zd_test_route(const zd_params *p_in, int32_t R, int32_t nranks, int32_t *out, char *why, int64_t cap) {
    const zd_params pc = zd::canonical(p_in);
    const Route rt = route(&pc, R, nranks, zd::ROLE_MAIN);
    const int32_t v[12] = {rt.family, rt.pack, rt.narray, rt.pstep, rt.npass, rt.R, rt.L, rt.Hq, rt.Zq, rt.dens, rt.dens_only, rt.twr};
    memcpy(out, v, sizeof v);
    if (why && cap > 0) snprintf(why, (size_t) cap, "%s", rt.why);
    return rt.ok() ? 0 : 1;
}
int zd_test_route_kernels(const zd_params *p_in, int32_t R, int32_t nranks, int32_t role, char *text, int64_t cap) {
    if (role < zd::ROLE_MAIN || role > zd::ROLE_LPT2_GRAD) return -3;
    const zd_params pc = zd::canonical(p_in);
    const Route shape = zd::route_shape(&pc, R, nranks, role), rt = route(&pc, R, nranks, role);
    zd::StageList st;
    zd::route_stages(shape, &pc, R, role, nranks, st);
    int missing = 0;
    int64_t w = 0;
    auto put = [&](const char *fmt, ...) {
        if (!text || w >= cap - 1) return;
        va_list ap;
        va_start(ap, fmt);
        const int n = vsnprintf(text + w, (size_t) (cap - w), fmt, ap);
        va_end(ap);
        if (n > 0) w = std::min<int64_t>(cap - 1, w + n);
    };
    if (text && cap > 0) text[0] = 0;
    put("route\t%d\t%s\n", rt.ok() ? 1 : 0, rt.why);
    for (int i = 0; i < st.n; i++) {
        missing += st.s[i].present ? 0 : 1;
        put("%s\t%s\t%s\t%d\n", st.s[i].stage, st.s[i].launcher, st.s[i].key, st.s[i].present ? 1 : 0);
    }
    if (rt.ok()) return missing;
    return shape.ok() ? -2 : -1;
}
void zd_test_lpt2_coefficients(const zd_params *p, double *out) {
    out[0] = zd::lpt2_alpha(p);
    out[1] = zd::lpt2_ratio(p);
    out[2] = zd::lpt2_f2(p);
}
#endif

#ifdef ZD_TESTING
// ------------------------------------------------------------------------------------------------
// device test hooks

int64_t zd_test_live_handles(void) { return (int64_t) zdown::g_live.load(); }

// The three generator hooks: a plan of the job, the mode list up, 16 or 24 bytes per mode down.  which 0: the two uint64 draws,
// 1: Re D, Im D, 2: Re D, Im D, fundamental / |k|^2 through the table arithmetic
static int test_modes_run(const zd_params *p, const zd_pk *pk, int64_t n, const int32_t *kxyz, int which, void *out) {
    zd_params q = *p;
    q.qPLT      = 0;
    q.stream_factor = q.ppd > 4096 ? (int) (q.ppd / 4096) : 1;  // z-FFT kernels exist up to length 4096
    zd_plan *raw = nullptr;
    if (zd_plan_create(&q, pk, nullptr, 0, 0, 1, &raw)) return 1;
    PlanPtr pl(raw);
    const size_t nb = (which == 2 ? 24 : 16) * (size_t) n;
    DevBuf<int> d_k;
    DevBuf<void> d_o;
    if (upload(d_k, kxyz, 3 * (size_t) n) != hipSuccess || d_o.alloc(nb) != hipSuccess) return 1;
    if (which == 2 ? zd::launch_test_modes_table(pl->g, n, d_k, (double *) d_o.get(), 0)
                   : zd::launch_test_modes(pl->g, n, d_k, which == 0 ? (uint64_t *) d_o.get() : nullptr, which == 1 ? (double *) d_o.get() : nullptr, 0))
        return 1;
    return hipMemcpy(out, d_o, nb, hipMemcpyDeviceToHost) != hipSuccess;
}

int zd_test_draws(int64_t seed, int64_t n, const int32_t *kxyz, uint64_t *out) {
    // only the RNG members of GenConst are used by the draw path
    zd_params p;
    memset(&p, 0, sizeof(p));
    p.ppd = 4096;  // row table covers ky < 2048
    p.seed = seed;
    p.boxsize = 1;
    p.fundamental = 1;
    p.nyquist = 1;
    p.k_cutoff = 1;
    p.f_cluster = 1;
    zd_pk pk;
    memset(&pk, 0, sizeof(pk));
    pk.is_powerlaw = 1;
    pk.powerlaw_index = -1;
    pk.normalization = 1;
    return test_modes_run(&p, &pk, n, kxyz, 0, out);
}
int zd_test_modes(const zd_params *p, const zd_pk *pk, int64_t n, const int32_t *kxyz, double *D) { return test_modes_run(p, pk, n, kxyz, 1, D); }
int zd_test_modes_table(const zd_params *p, const zd_pk *pk, int64_t n, const int32_t *kxyz, double *out) {
    return test_modes_run(p, pk, n, kxyz, 2, out);
}

int zd_test_generate_loopback(const zd_params *p, const zd_pk *pk, const double *eig, int64_t eig_ppd, zd_slab_cb cb, void *user,
                              zd_stats *out) {
    if (p->ngpu < 2) return 1;
    return zd_generate_multi(p, pk, eig, eig_ppd, cb, user, out, 2);
}

int zd_test_v1_words(int64_t seed, int32_t nblocks, uint32_t *out) {
    if (nblocks <= 0) return 1;
    DevBuf<zd::V1Stream> d_s;
    DevBuf<uint32_t> d_o;
    if (d_s.alloc(1) != hipSuccess || d_o.alloc(624 * (size_t) nblocks) != hipSuccess) return 1;
    if (zd::launch_v1_seed((unsigned long long) seed, 1, d_s, 0) || zd::launch_test_v1_words(d_s, nblocks, d_o, 0)) return 1;
    return hipMemcpy(out, d_o, sizeof(uint32_t) * 624 * (size_t) nblocks, hipMemcpyDeviceToHost) != hipSuccess;
}

// one batch of `nel` points through a transform: its twiddles and the input up, launch(tw, in, out) — out == in: in place —, the result down
static int test_fft_run(const std::vector<cplx> &tw, size_t nel, bool in_place, const double *in, double *out,
                        const std::function<int(const cplx *, cplx *, cplx *)> &launch) {
    DevBuf<cplx> d_tw, d_in, d_out;
    if (tw.empty() || upload(d_tw, tw) != hipSuccess || upload(d_in, (const cplx *) in, nel) != hipSuccess) return 1;
    if (!in_place && d_out.alloc(nel) != hipSuccess) return 1;
    cplx *res = in_place ? d_in.get() : d_out.get();
    if (launch(d_tw, d_in, res) || hipDeviceSynchronize() != hipSuccess) return 1;
    return hipMemcpy(out, res, sizeof(cplx) * nel, hipMemcpyDeviceToHost) != hipSuccess;
}

// any length through the convolution kernels (zd_kernels_any.hip); axis_kind as in zd_test_fft
static int test_fft_any(int32_t n, int64_t lines, int32_t axis_kind, const double *in, double *out) {
    if (n < 2 || n > 8192) return 1;
    zd::AnyTab tab = {};
    DevBuf<cplx> bufs[3], d;
    const size_t nel = (size_t) n * lines;
    if (any_make_tab(n, &tab, bufs) || upload(d, (const cplx *) in, nel) != hipSuccess) return 1;
    if (axis_kind == 1 ? zd::launch_any_cols(tab, d, 0, lines, (int) lines, 1, -1, 0) : zd::launch_any_lines(tab, d, n, lines, 0)) return 1;
    if (hipDeviceSynchronize() != hipSuccess) return 1;
    return hipMemcpy(out, d, sizeof(cplx) * nel, hipMemcpyDeviceToHost) != hipSuccess;
}

// the y columns of the arrays split over G ranks (k_refq_ycols) on host columns [image][ky][ncols]: the rows go to a chunked store of
// `nimg` planes per chunk (row pitch ncols) by the map of any_chunk_row, are transformed, and come back the same way.  mode 0: ky = N/2
// read as zero, every output written (the main pass, the phi round's first y transform); 1: every input read, outputs ky < N/2 only
// (the phi round's second y transform) — the other rows of `out` keep their input
int zd_test_ycols(int32_t n, int32_t G, int32_t ncols, int32_t nimg, int32_t mode, const double *in, double *out) {
    const size_t nel = (size_t) nimg * n * ncols;
    if (!zd::refq_supported_len(n) || G < 1 || (G & (G - 1)) || (n / 2) % G || ncols < 1 || nimg < 1 || nel > ((size_t) 1 << 26)) return 1;
    zd::AnyChunks C{n, ncols, 1, G, n / (2 * G), nimg, 0};
    C.chunk = (long long) nimg * 2 * C.Hq * ncols;
    const cplx *hin = (const cplx *) in;
    std::vector<cplx> h(nel);
    auto at = [&](int b, int y) -> size_t {
        int c = 0, sl = 0;
        zd::any_chunk_row(C, y, c, sl);
        return (size_t) (c * C.chunk + ((long long) b * 2 * C.Hq + sl) * ncols);
    };
    for (int b = 0; b < nimg; b++)
        for (int y = 0; y < n; y++) std::copy(hin + ((size_t) b * n + y) * ncols, hin + ((size_t) b * n + y + 1) * ncols, h.begin() + at(b, y));
    DevBuf<cplx> d_tw, d;
    if (upload_twq(n, d_tw) || upload(d, h) != hipSuccess) return 1;
    if (zd::launch_refq_ycols(n, d_tw, C, d, ncols, nimg, mode == 0 ? n / 2 : -1, mode == 0 ? n : n / 2, 0)) return 1;
    if (hipDeviceSynchronize() != hipSuccess) return 1;
    if (hipMemcpy(h.data(), d, sizeof(cplx) * nel, hipMemcpyDeviceToHost) != hipSuccess) return 1;
    cplx *hout = (cplx *) out;
    for (int b = 0; b < nimg; b++)
        for (int y = 0; y < n; y++) std::copy(h.begin() + at(b, y), h.begin() + at(b, y) + ncols, hout + ((size_t) b * n + y) * ncols);
    return 0;
}

int zd_test_fft(int32_t n, int64_t lines, int32_t axis_kind, const double *in, double *out) {
    const size_t nel = (size_t) n * lines;
    // the composite transforms of the reference's arrays (zd_kernels_np2_ref.hip), in place, any batch: axis_kind 3 = strided lines
    // (layout [n][lines], k_refq_cols), 4 = contiguous lines ([lines][n], k_refq_lines)
    if (axis_kind == 3 || axis_kind == 4) {
        if (!zd::refq_supported_len(n) || lines < 1 || lines > (1 << 20)) return 1;
        return test_fft_run(make_twq(n), nel, true, in, out, [&](const cplx *tw, cplx *d, cplx *) {
            return axis_kind == 3 ? zd::launch_refq_cols(n, tw, d, 0, lines, (int) lines, 1, -1, 0) : zd::launch_refq_lines(n, tw, d, n, lines, 0);
        });
    }
    if (!is_pow2(n)) {
        int P = 0, Q = 0;
        // composite-length kernels where they exist and the batch is whole tiles; else the convolution kernels (any length,
        // ragged batches)
        if (!(zd::np2_split(n, &P, &Q) && zd::test_fftq_tile_width(n) > 0 && P >= 8 && lines % zd::test_fftq_tile_width(n) == 0))
            return test_fft_any(n, lines, axis_kind, in, out);
        return test_fft_run(make_twq(n), nel, false, in, out, [&](const cplx *tw, cplx *i, cplx *o) {
            return zd::launch_test_fftq(n, axis_kind, tw, tw + P, tw + P + n, i, o, lines, 0);
        });
    }
    const int W = zd::test_fft_tile_width(n);
    if (W == 0 || lines % W) {
        fprintf(stderr, "zd_test_fft: n=%d needs lines %% %d == 0\n", n, W);
        return 1;
    }
    return test_fft_run(make_twiddles(n), nel, false, in, out,
                        [&](const cplx *tw, cplx *i, cplx *o) { return zd::launch_test_fft(n, axis_kind, tw, i, o, lines, 0); });
}

int zd_test_plt_matrix(int64_t n, double alpha, int32_t shells, int64_t nmodes, const int32_t *m_xyz, double *out6) {
    if (n < 1 || n > (1 << 20) || !(alpha > 0.) || shells < 3 || shells > 5 || nmodes < 1 || !m_xyz || !out6) {
        fprintf(stderr, "zd_test_plt_matrix: n in [1, 2^20], alpha > 0, shells 3, 4 or 5, at least one mode\n");
        return 1;
    }
    for (int64_t i = 0; i < 3 * nmodes; i++)
        if (m_xyz[i] < -n || m_xyz[i] > n) {
            fprintf(stderr, "zd_test_plt_matrix: wavenumber %d outside [-n, n]\n", (int) m_xyz[i]);
            return 1;
        }
    DevBuf<double> d_tab, d_o;
    DevBuf<int> d_m;
    if (upload(d_tab, zd::plt_shell_table(alpha, shells)) != hipSuccess || upload(d_m, (const int *) m_xyz, 3 * (size_t) nmodes) != hipSuccess ||
        d_o.alloc(6 * (size_t) nmodes) != hipSuccess)
        return 1;
    if (zd::launch_test_plt_matrix(zd::plt_const((int) n, alpha), shells, d_tab, nmodes, d_m, d_o, 0)) return 1;
    return hipMemcpy(out6, d_o, sizeof(double) * 6 * (size_t) nmodes, hipMemcpyDeviceToHost) != hipSuccess;
}

#endif  // ZD_TESTING

#ifdef ZD_TUNING
// `reps` launches between two events on the null stream -> milliseconds in all; launch() has run once before
static int time_launches(int reps, const std::function<int()> &launch, float *ms) {
    Event e0, e1;
    if (e0.create() != hipSuccess || e1.create() != hipSuccess || launch() || hipEventRecord(e0, 0) != hipSuccess) return 1;
    for (int i = 0; i < reps; i++)
        if (launch()) return 1;
    if (hipEventRecord(e1, 0) != hipSuccess || hipEventSynchronize(e1) != hipSuccess) return 1;
    return hipEventElapsedTime(ms, e0, e1) != hipSuccess;
}

// tuning harness (not part of the product path): time y-pass tile variants on a synthetic store
int zd_test_yfft_variant(int32_t n, int32_t variant, int32_t narray, int32_t nplanes, int32_t tiled, int32_t reps,
                         double *ms_per_launch) {
    zd::StoreLayout S;
    S.N = n; S.half = n / 2; S.Hq = n / 2; S.narray = narray;
    S.lHq = 0;
    while ((1 << S.lHq) < S.Hq) S.lHq++;
    S.lG = 0;
    S.ky_stride = 1;
    int lBk = 0, lBz = 0;
    if (tiled) {
        const long long target = std::max<long long>(1, ((long long) 2 << 20) / ((long long) n * 16));
        int lt = 0;
        while ((1LL << (lt + 1)) <= target) lt++;
        lBk = (lt + 1) / 2; lBz = lt - lBk;
        while ((1 << lBz) > nplanes) lBz--;
    }
    S.lq = 0;
    S.paired = 0;
    S.lBk = lBk; S.lBz = lBz; S.rows_outer = 0; S.one_block = 0; S.pitch = n; S.prune = 0; S.nt = 0; S.kmax = 0; S.fund2 = 0; S.k2_cutoff = 0;
    S.a_rows = (1 << lBk) << lBz;
    S.zb_rows = S.a_rows * narray;
    S.kb_rows = S.zb_rows * (nplanes >> lBz);
    S.chunk_rows = S.kb_rows * (n >> lBk);
    const size_t nel = (size_t) S.chunk_rows * S.pitch;
    DevBuf<cplx> d_tw, d;
    if (upload(d_tw, make_twiddles(n)) != hipSuccess || d.alloc(nel) != hipSuccess || hipMemset(d, 0, nel * sizeof(cplx)) != hipSuccess) return 1;
    float ms = 0;
    if (time_launches(reps, [&] { return zd::launch_yfft_variant(variant, S, nplanes, d_tw, d, 0); }, &ms)) return 1;
    *ms_per_launch = ms / reps;
    return 0;
}

int zd_test_copy_bw(int64_t bytes, int32_t reps, double *gbps) {
    DevBuf<void> a, b;
    if (a.alloc((size_t) bytes) != hipSuccess || b.alloc((size_t) bytes) != hipSuccess || hipMemset(a, 1, (size_t) bytes) != hipSuccess) return 1;
    float ms = 0;
    if (time_launches(reps, [&] { return zd::launch_copy16(a, b, bytes / 16, 0); }, &ms)) return 1;
    *gbps = 2.0 * bytes * reps / (ms * 1e-3) / 1e9;
    return 0;
}

#endif  // ZD_TUNING
