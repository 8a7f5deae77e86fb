// zd_capi.cpp — C ABI (include/zeldovich_hip.h): plan management, the single-GPU driver
// zd_generate (= ZeldovichZ + ZeldovichXY, src/zeldovich.cpp:517-695) and the device test hooks.
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <new>
#include <thread>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/zeldovich_hip.h"
#include "zd_device.h"
#include "zd_launch.h"
#include "zd_plan.h"
#include "zd_glass.h"
#include "zd_route.h"
#include "zd_plt.h"
#ifdef ZD_TUNING
#include "zd_tuning.h"
#endif
#ifdef ZD_TESTING
#include "zd_testing.h"
#endif

using zdfft::cplx;
using zdpcg::u128;
using zd::is_pow2;
using zd::Route;
using zd::route;
using zdown::DevBuf;
using zdown::Event;
using zdown::PinnedBuf;
using zdown::PlanPtr;
using zdown::Stream;
using zdown::upload;

#define HIPCHECK(call)                                                                               \
    do {                                                                                             \
        hipError_t e__ = (call);                                                                     \
        if (e__ != hipSuccess) {                                                                     \
            fprintf(stderr, "zeldovich_hip: %s failed at %s:%d: %s\n", #call, __FILE__, __LINE__,    \
                    hipGetErrorString(e__));                                                         \
            return 1;                                                                                \
        }                                                                                            \
    } while (0)

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
static std::atomic<int> g_ring_pair_w{0};
void zd_test_ring_pair_w(int w) { g_ring_pair_w.store(w); }
#endif
hipError_t zd_store_alloc(void **p, size_t bytes) {
    hipError_t e = hipMalloc(p, bytes);
#ifdef ZD_TESTING
    if (e == hipSuccess && g_poison.load()) e = hipMemset(*p, 0xFF, bytes);
#endif
    return e;
}

namespace {

std::vector<cplx> make_twiddles(int n) {
    std::vector<cplx> tw(n);
    for (int k = 0; k < n; k++) {
        const long double a = 2.0L * 3.14159265358979323846264338327950288L * (long double) k / (long double) n;
        tw[k].x = (double) cosl(a);
        tw[k].y = (double) sinl(a);
    }
    return tw;
}

// Bluestein tables of a length-n transform on the engine of size M = 2^m >= 2n - 1 (zd_kernels_any.hip): c_m = exp(i pi m^2/n)
// with m^2 reduced mod 2n in integers, and the forward DFT_M of b_m = conj(c_m), |m| < n, wrapped (long double radix-2)
int any_make_tab(int n, zd::AnyTab *tab, DevBuf<cplx> *d_bufs) {
    const int M = zd::any_engine_size(n);
    const long double PI = 3.14159265358979323846264338327950288L;
    std::vector<cplx> chirp(n), tw = make_twiddles(M);
    std::vector<long double> br(M, 0.0L), bi(M, 0.0L);
    for (long long m = 0; m < n; m++) {
        const long double a = PI * (long double) ((m * m) % (2LL * n)) / (long double) n;
        const long double c = cosl(a), sn = sinl(a);
        chirp[m] = cplx{(double) c, (double) sn};
        br[m] = c;
        bi[m] = -sn;
        if (m) {
            br[M - m] = c;
            bi[M - m] = -sn;
        }
    }
    // forward DFT (sign -1), iterative radix-2
    for (int i = 1, j = 0; i < M; i++) {
        int bit = M >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) {
            std::swap(br[i], br[j]);
            std::swap(bi[i], bi[j]);
        }
    }
    for (int len = 2; len <= M; len <<= 1) {
        const long double ang = -2.0L * PI / (long double) len;
        for (int i = 0; i < M; i += len)
            for (int k = 0; k < len / 2; k++) {
                const long double wr = cosl(ang * k), wi = sinl(ang * k);
                const long double ur = br[i + k], ui = bi[i + k];
                const long double vr = br[i + k + len / 2] * wr - bi[i + k + len / 2] * wi;
                const long double vi = br[i + k + len / 2] * wi + bi[i + k + len / 2] * wr;
                br[i + k] = ur + vr;
                bi[i + k] = ui + vi;
                br[i + k + len / 2] = ur - vr;
                bi[i + k + len / 2] = ui - vi;
            }
    }
    std::vector<cplx> fb(M);
    for (int i = 0; i < M; i++) fb[i] = cplx{(double) br[i], (double) bi[i]};
    const std::vector<cplx> *src[3] = {&tw, &chirp, &fb};
    for (int i = 0; i < 3; i++)
        if (upload(d_bufs[i], *src[i]) != hipSuccess) return 1;
    tab->n     = n;
    tab->M     = M;
    tab->invM  = 1.0 / (double) M;
    tab->twM   = d_bufs[0];
    tab->chirp = d_bufs[1];
    tab->fb    = d_bufs[2];
    return 0;
}

// LDS image of k_genf; offsets must match GenfTab (zd_kernels.hip): directions {cos, sin}(2 pi j/512) at 0,
// ln bins {c_j, -ln c_j} at 1024, 2^(j/64) at 1392, spline segment records at 1456, uint16 segment LUT after them
std::vector<double> build_genf_table(const zd_pk *pk, int nseg, double *lut_x0, double *lut_inv_dx) {
    constexpr int SC = 0, LG = 1024, EX = 1392, SEG = 1456, GLUT = 1024;
    std::vector<double> T(SEG + 6 * (size_t) nseg + GLUT / 4, 0.0);
    const long double pi = 3.14159265358979323846264338327950288L;
    for (int j = 0; j < 512; j++) {
        T[SC + 2 * j]     = (double) cosl(2.0L * pi * j / 512.0L);
        T[SC + 2 * j + 1] = (double) sinl(2.0L * pi * j / 512.0L);
    }
    for (int j = 0; j < 182; j++) {  // f in [(j+181)/256, (j+182)/256); bins 74, 75 surround f = 1
        double c = 1.0, l = 0.0;
        if (j != 74 && j != 75) {
            c = (double) (1.0L / (((long double) (j + 181) + 0.5L) / 256.0L));
            l = (double) (-logl((long double) c));
        }
        T[LG + 2 * j]     = c;
        T[LG + 2 * j + 1] = l;
    }
    for (int j = 0; j < 64; j++) T[EX + j] = (double) powl(2.0L, (long double) j / 64.0L);
    *lut_x0 = 0.0;
    *lut_inv_dx = 0.0;
    if (nseg > 0) {
        for (int i = 0; i < nseg; i++) {  // SplineFunction::val, include/spline_function.h:153-162
            const double h = pk->x[i + 1] - pk->x[i];
            double *r = &T[SEG + 6 * (size_t) i];
            r[0] = pk->x[i];
            r[1] = 1.0 / h;
            r[2] = pk->y[i];
            r[3] = pk->y[i + 1];
            r[4] = pk->y2[i] * (h * h) / 6.0;
            r[5] = pk->y2[i + 1] * (h * h) / 6.0;
        }
        // segment start table: cell c covers ln k in [x0 + c*dx, x0 + (c+1)*dx); never past the true start
        unsigned short *lut = reinterpret_cast<unsigned short *>(&T[SEG + 6 * (size_t) nseg]);
        const double x0 = pk->x[0], x1 = pk->x[nseg];
        const double dx = (x1 - x0) / GLUT;
        int klo = 0;
        for (int c = 0; c < GLUT; c++) {
            const double cell_start = x0 + c * dx * (1.0 - 1e-12) - 1e-9;
            while (klo < nseg - 1 && pk->x[klo + 1] <= cell_start) klo++;
            lut[c] = (unsigned short) klo;
        }
        *lut_x0     = x0;
        *lut_inv_dx = 1.0 / dx;
    }
    return T;
}

int record_size(int icformat) {  // include/output.h:19-42
    switch (icformat) {
        case ZD_FMT_ZEL: return 32;
        case ZD_FMT_RVZEL: return 32;
        case ZD_FMT_RVDOUBLEZEL: return 56;
        case ZD_FMT_ZELSIMPLE: return 12;
    }
    return 0;
}

}  // namespace

namespace {

void tick(zd_plan *pl, int kind, hipStream_t st, bool begin) {
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
int span_begin(zd_plan *pl, int kind, hipStream_t st) {
    if (!pl->p.profile) return -1;
    EventPair ep;
    hipEventCreate(&ep.a);
    hipEventCreate(&ep.b);
    ep.kind = kind;
    hipEventRecord(ep.a, st);
    pl->events.push_back(ep);
    return (int) pl->events.size() - 1;
}
void span_end(zd_plan *pl, int idx, hipStream_t st) {
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

// Rows of the block store are N*16 B apart: at PPD >= 2048 that is a multiple of 32 KB and the strided accesses of
// the y pass pile onto a few HBM channels (PPD=4096: k_yfft 1.20 s -> 0.92 s with the pad, PPD=2048: 100 -> 93 ms).
// 384 B of padding per row de-aliases them (128 B and 640 B do as well; 256 B does not at PPD=2048) for 0.6-5 % more memory.
int store_row_pad(int64_t N) { return N >= 512 ? 24 : 0; }

bool p_oneslab_off(const zd_plan *pl) { return pl->p.qoneslab < 0; }  // ZD_qoneslab runs finish a single pass

int64_t y_bytes_per_row(const zd_plan *pl) { return (int64_t) pl->jobs.n * pl->L * pl->N * 16; }

// advance by (2*65536*drows - 1) draws, drows may be negative (period 2^128)
zdpcg::Affine row_jump(long long drows) {
    const __int128 d = (__int128) 2 * 65536 * (__int128) drows - 1;
    return zdpcg::jump_map((u128) d);
}
zdpcg::Affine row_jump_full(long long drows) {  // 2*65536*drows draws
    const __int128 d = (__int128) 2 * 65536 * (__int128) drows;
    return zdpcg::jump_map((u128) d);
}

}  // namespace

extern "C" {

// the zero rule of zeldovich.cpp:350-353 as the kernels prune by it (zd_device.h column_is_zero)
static void prune_rule(const zd_params *p, zd::StoreLayout &S) {
    const int half = (int) (p->ppd / 2);
    S.N         = (int) p->ppd;
    S.half      = half;
    S.prune     = 7;
    S.kmax      = (int) ((double) half * (1.0 / p->k_cutoff) + .5);
    S.fund2     = p->fundamental * p->fundamental;
    S.k2_cutoff = p->corner_modes ? 0.0 : p->nyquist * p->nyquist / (p->k_cutoff * p->k_cutoff);  // CornerModes: only |k_i| == kmax prunes
}

// Block table of the field store (zd_device.h FieldLayout) for `nranks` ranks: block b stands for the row slots 8b .. 8b+7
// (rows ky = c + nranks*slot) of every rank c and is sized by the longest of them (ky = nranks*8b).  Returns the elements
// per (plane, field) image.
static int64_t field_rows(const zd_params *p, int nranks, std::vector<zd::FieldRow> *rows) {
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
static int field_ring_planes(int64_t N, int64_t Zq) {
    const int64_t plane_b = 3 * N * (N + store_row_pad(N)) * 16;
    return (int) std::max<int64_t>(1, std::min<int64_t>(Zq, ((int64_t) 6 << 30) / plane_b));
}

const char *zd_fnl_multi_unsupported(const zd_params *p) { return zd::fnl_multi_refusal(p); }
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
static int64_t fnl_phik_bytes(int64_t N) { return (N / 2) * N * N * 16; }
static int64_t fnl_phi_bytes(const zd_params *p) {
    const int64_t N = p->ppd;
    return (route(p, 1, 1, zd::ROLE_PHI).twr ? N / 2 : N) * N * (N + store_row_pad(N)) * 16;
}

// ZD_q2LPT memory: the source S(k) (half-space rows, PhiK's layout) stays beside every pass's store; the second-order round before it
// peaks at its one-array store (every plane, self and twin slots) + the real N^3 accumulator, which S(k) then replaces
static int64_t lpt2_sk_bytes(int64_t N) { return (N / 2) * N * N * 16; }
// ZD_2LPT_dealias: the same round on the lattice of M = 3 N / 2 points per side, (16 + 8) M^3 = 81 N^3 bytes (+ the row pad)
static int64_t lpt2_round_bytes(const zd_params *p) {
    const int64_t M = p->lpt2_dealias ? zd::lpt2_dealias_lattice(p->ppd) : p->ppd;
    return M * M * (M + store_row_pad(M)) * 16 + M * M * M * 8;
}
// ZD_q3LPT memory: P3(k) and C_x,y,z(k) stay beside S(k), 40 N^3 bytes in all; the third-order round before them peaks at its one-array
// store + the twelve real Hessian fields + S(k) = 120 N^3 bytes (+ the row pad), of which the four new spectra then take 32 N^3
static int64_t lpt3_round_bytes(int64_t N) { return N * N * (N + store_row_pad(N)) * 16 + 12 * N * N * N * 8 + lpt2_sk_bytes(N); }
static int64_t lpt_resident_bytes(const zd_params *p) { return p->q2LPT ? (p->q3LPT ? 5 : 1) * lpt2_sk_bytes(p->ppd) : 0; }

using zd::split_routes;  // (zd_route.h)

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

// the line transforms of the reference-array store (pl->any): composite (zd_kernels_np2_ref.hip) where the plan uploaded their
// twiddles, else convolutions (zd_kernels_any.hip).  zlen: lines of length L (the z lines of a pass), else N.
static int any_cols(const zd_plan *pl, bool zlen, void *data, long long batch_stride, long long point_stride, int ncols, int nbatch,
                    int zero_point, hipStream_t st) {
    if (pl->d_twr_n)
        return zd::launch_refq_cols(zlen ? pl->L : pl->N, zlen ? pl->d_twr_l : pl->d_twr_n, data, batch_stride, point_stride, ncols, nbatch,
                                    zero_point, st);
    return zd::launch_any_cols(zlen ? pl->tabL : pl->tabN, data, batch_stride, point_stride, ncols, nbatch, zero_point, st);
}
static int any_lines(const zd_plan *pl, void *data, long long pitch, long long nlines, hipStream_t st) {
    if (pl->d_twr_n) return zd::launch_refq_lines(pl->N, pl->d_twr_n, data, pitch, nlines, st);
    return zd::launch_any_lines(pl->tabN, data, pitch, nlines, st);
}

// phi_mode 1: first f_NL pass (one array holding phi = D/M); phik != NULL: second pass (D = phik * M).  ZD_q2LPT: phi_mode 2 = the
// plan of the second-order round's gradient passes; phik != NULL with phi_mode 0 = the final pass, phik holding the source S(k)
static int plan_create_ex(const zd_params *p, const zd_pk *pk, const double *eig, int64_t eig_ppd, int rank, int nranks,
                          int phi_mode, const cplx *phik, PlanPtr &out, bool field = false);
// a plan that was made goes to a caller of the C ABI; *out is left alone otherwise
static int hand_over(int rc, PlanPtr &pl, zd_plan **out) {
    if (!rc) *out = pl.release();
    return rc;
}

// f_NL: phi field -> local transform phi + f_NL phi^2 -> Fourier space again (zeldovich.cpp:945-960, 699-790): the first
// ZeldovichZ / ZeldovichXY_Phi round of the reference, run once; *d_phik = PhiK[ky][kz][x] for the half-space rows (owned
// by the caller, untouched on failure).  One rank: the forward z transform needs every plane resident.
static int make_phik(const zd_params *p, const zd_pk *pk, DevBuf<cplx> &d_phik) {
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
    ph->phi_half = ph->d_twr_n != nullptr && ph->jobs.n == 1 && ph->R == 1;
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

// ---- a caller-supplied density or white-noise field (definition and kernels: zd_kernels_field.hip) ----
static void gen_zero_rule(zd::GenConst &g, const zd_params *p);
struct FieldSpec {
    int32_t kind, dtype;  // ZD_FIELD_DENSITY / _WHITE, ZD_FIELD_F32 / _F64
    const void *field;    // a[z][y][x], C-contiguous
    int32_t on_device;
};
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
static int make_field_phik(const zd_params *p, const zd_pk *pk, const FieldSpec &f, DevBuf<cplx> &d_phik) {
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

// the round's peak against the free memory, asked before anything is built (the figure is the message)
static int lpt2_round_fits(const zd_params *p, int64_t free_bytes) {
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
static int make_lpt2_source(const zd_params *p, const zd_pk *pk, DevBuf<cplx> &d_sk) {
    const bool dq   = p->lpt2_dealias != 0;
    const int64_t N = p->ppd, M = dq ? zd::lpt2_dealias_lattice(N) : N;  // points per side of the round's lattice
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
    if (plan_create_ex(&pp, pk, nullptr, 0, 0, 1, 2, nullptr, plan)) return 1;
    zd_plan *ph = plan.get();
    if (dq && (!ph->d_twr_n || ph->N != M || ph->g.kmax != (int) ((double) (N / 2) * (1.0 / p->k_cutoff) + .5))) {
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
static int make_lpt3_sources(const zd_params *p, const zd_pk *pk, const cplx *d_sk, DevBuf<cplx> (&d_out)[4]) {
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
static void adopt_lpt3(zd_plan *pl, DevBuf<cplx> (&d_spec)[4]) {
    for (int f = 0; f < 4; f++) pl->d_lpt3_owned[f] = std::move(d_spec[f]);
    pl->g.lpt3_p3 = pl->d_lpt3_owned[0];
    for (int j = 0; j < 3; j++) pl->g.lpt3_c[j] = pl->d_lpt3_owned[1 + j];
}
// a ZD_q2LPT job the route takes for this call (the refusal printed otherwise), asked BEFORE the second-order round is run
static int lpt2_route_check(const zd_params *p, int nranks, int rank) {
    const zd_params pc = zd::canonical(p);
    const Route rt = route(&pc, pc.stream_factor, nranks, zd::ROLE_MAIN, rank, true);
    if (rt.ok()) return 0;
    fprintf(stderr, "zeldovich_hip: %s\n", rt.why);
    return 1;
}

static zd::StoreLayout layout_for_chunks(const zd_plan *pl, int chunk_planes);
static zd::AnyChunks any_chunks(const zd_plan *pl, int chunk_planes);

// twiddles of a composite transform (zd_fft_q.h) of length len = P * Q: exp(2 pi i k / P) | exp(2 pi i k / len) | exp(2 pi i k / Q)
static std::vector<cplx> make_twq(int len) {  // (empty: no such transform)
    int P = 0, Q = 0;
    if (!zd::np2_split(len, &P, &Q)) return {};
    std::vector<cplx> t = make_twiddles(P), b = make_twiddles(len), c = make_twiddles(Q);
    t.insert(t.end(), b.begin(), b.end());
    t.insert(t.end(), c.begin(), c.end());
    return t;
}
static int upload_twq(int len, DevBuf<cplx> &dst) {
    const std::vector<cplx> t = make_twq(len);
    return t.empty() || upload(dst, t) != hipSuccess;
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

int zd_plan_create(const zd_params *p, const zd_pk *pk, const double *eig, int64_t eig_ppd, int rank, int nranks,
                   zd_plan **out) {
    PlanPtr pl;
    DevBuf<cplx> d_phik;  // PhiK or S(k): the round runs here, once; the plan owns the result and its Z stages read it beside their draws
    DevBuf<cplx> d_lpt3[4];  // ZD_q3LPT: P3(k), C_x,y,z(k) of the third-order round, likewise
    if (p->q2LPT || p->q3LPT) {
        if (lpt2_route_check(p, nranks, rank) || make_lpt2_source(p, pk, d_phik)) return 1;
        if (p->q3LPT && make_lpt3_sources(p, pk, d_phik, d_lpt3)) return 1;
    } else if (p->f_NL != 0.) {  // the phi round; the Z stages read D = PhiK * M
        if (nranks != 1) {
            fprintf(stderr, "zeldovich_hip: ZD_f_NL != 0 runs on one rank (the forward z transform of the phi field needs every plane)\n");
            return 1;
        }
        if (make_phik(p, pk, d_phik)) return 1;
        rank = 0;
    }
    if (plan_create_ex(p, pk, eig, eig_ppd, rank, nranks, 0, d_phik, pl)) return 1;
    pl->d_phik_owned = std::move(d_phik);
    if (p->q3LPT) adopt_lpt3(pl.get(), d_lpt3);
    *out             = pl.release();
    return 0;
}

// ---- device tables of the generator and the transforms ----
static int plan_device_tables(zd_plan *pl, const zd_pk *pk, const double *eig, int64_t eig_ppd) {
    const zd_params *p = &pl->p;
    zd::GenConst &g = pl->g;
    if (!pk->is_powerlaw) {
        HIPCHECK(pl->d_pk.alloc(3 * (size_t) pk->n));
        HIPCHECK(hipMemcpy(pl->d_pk, pk->x, sizeof(double) * pk->n, hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(pl->d_pk + pk->n, pk->y, sizeof(double) * pk->n, hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(pl->d_pk + 2 * pk->n, pk->y2, sizeof(double) * pk->n, hipMemcpyHostToDevice));
        g.pk_x  = pl->d_pk;
        g.pk_y  = pl->d_pk + pk->n;
        g.pk_y2 = pl->d_pk + 2 * pk->n;
        // segment start table: cell c covers ln k in [x0 + c*dx, x0 + (c+1)*dx)
        std::vector<int> lut(zd::PK_LUT);
        const double x0 = pk->x[0], x1 = pk->x[pk->n - 1];
        const double dx = (x1 - x0) / zd::PK_LUT;
        int klo = 0;
        for (int c2 = 0; c2 < zd::PK_LUT; c2++) {
            const double cell_start = x0 + c2 * dx * (1.0 - 1e-12) - 1e-9;  // never past the true start
            while (klo < pk->n - 2 && pk->x[klo + 1] <= cell_start) klo++;
            lut[c2] = klo;
        }
        HIPCHECK(upload(pl->d_lut, lut));
        g.pk_lut     = pl->d_lut;
        g.lut_x0     = x0;
        g.lut_inv_dx = 1.0 / dx;
    }
    if (p->qPLT) {
        const size_t n = (size_t) eig_ppd * eig_ppd * (eig_ppd / 2 + 1) * 4;
        HIPCHECK(upload(pl->d_eig, eig, n));
        g.eig = pl->d_eig;
    }
    // per-plane stream heads == v2rng[] of the reference (power_spectrum.cpp:26-37)
    {
        std::vector<u128> rows(pl->half);
        const zdpcg::Affine plane = zdpcg::jump_map((u128) 2 * ZD_MAX_PPD * ZD_MAX_PPD);
        rows[0] = zdpcg::seed_state((uint64_t) p->seed);
        for (int i = 1; i < pl->half; i++) rows[i] = zdpcg::apply(plane, rows[i - 1]);
        HIPCHECK(upload(pl->d_rowstate, rows));
        g.row_state = pl->d_rowstate;
        // (built once; ZD_NumGPU creates its plans from several host threads at a time)
        static const zdpcg::BitTable bt = [] {
            zdpcg::BitTable b;
            zdpcg::make_bit_table(b);
            return b;
        }();
        if (zdk_upload_bit_table(&bt) != 0 || zdk_upload_bit_table_fz(&bt) != 0 || zdk_upload_bit_table_lpt2(&bt) != 0
            || zdk_upload_bit_table_lpt3(&bt) != 0) {
            fprintf(stderr, "zeldovich_hip: uploading the RNG jump table failed\n");
            return 1;
        }
        // z-walk of k_gen (see zd_device.h GenJumps): forward L rows inside a fold, then back to the
        // first term of the next k2; crossing z = N/2 shifts the counter row by +-(65536 - N)
        const long long wrap = 65536 - pl->N, Lr = pl->L, back = -((long long) (pl->R - 1) * Lr - 1);
        pl->J.fwd[0]  = row_jump(Lr);
        pl->J.fwd[1]  = row_jump(Lr + wrap);
        pl->J.back[0] = row_jump(back);
        pl->J.back[1] = row_jump(back > 0 ? back + wrap : back - wrap);
        pl->J.fwd_full[0]  = row_jump_full(Lr);
        pl->J.fwd_full[1]  = row_jump_full(Lr + wrap);
        pl->J.back_full[0] = row_jump_full(back);
        pl->J.back_full[1] = row_jump_full(back > 0 ? back + wrap : back - wrap);
        // the mirrored walker of genf_tile_kz: the same moves negated (crossing z = N/2 in its own direction of motion)
        const long long mf = -Lr, mb = -back;
        pl->J.mfwd[0]       = row_jump(mf);
        pl->J.mfwd[1]       = row_jump(mf - wrap);
        pl->J.mback[0]      = row_jump(mb);
        pl->J.mback[1]      = row_jump(mb > 0 ? mb + wrap : mb - wrap);
        pl->J.mfwd_full[0]  = row_jump_full(mf);
        pl->J.mfwd_full[1]  = row_jump_full(mf - wrap);
        pl->J.mback_full[0] = row_jump_full(mb);
        pl->J.mback_full[1] = row_jump_full(mb > 0 ? mb + wrap : mb - wrap);
    }
    {
        HIPCHECK(upload(pl->d_twN, make_twiddles(pl->N)));
        HIPCHECK(upload(pl->d_twL, make_twiddles(pl->L)));
        if (!is_pow2(pl->N) && !pl->any) {  // composite transforms (zd_fft_q.h): exp(2 pi i k / P) | exp(2 pi i k / len) | exp(2 pi i k / Q) per length
            if (upload_twq(pl->N, pl->d_twq_n) || upload_twq(pl->L, pl->d_twq_l)) {
                fprintf(stderr, "zeldovich_hip: composite twiddle tables failed\n");
                return 1;
            }
        }
        // LDS image of k_genf (layout: GenfTab in zd_kernels.hip).  Spline tables beyond 512 segments do not
        // fit: such runs use the general generator.
        const int nseg = pk->is_powerlaw ? 0 : pk->n - 1;
        if (nseg <= 512 && !tune_env("ZD_GEN_GENERAL")) {
            std::vector<double> T = build_genf_table(pk, nseg, &g.glut_x0, &g.glut_inv_dx);
            HIPCHECK(upload(pl->d_genf, T));
            g.genf_tab  = pl->d_genf;
            g.genf_n    = (int) T.size();
            g.genf_nseg = nseg;
        }
    }
    // {P, 1/k^2} table over the integer |k|^2 that can carry power (zero rule of zeldovich.cpp:350-353)
    if (!tune_env("ZD_NO_PKTAB")) {
        const double half2 = (double) pl->half * pl->half;
        double nmax = p->corner_modes ? 3.0 * half2 : std::min(3.0 * half2, g.k2_cutoff / g.fundamental2 * (1 + 1e-9) + 2);
        const long long n = (long long) nmax + 2;
        if (n <= ((long long) 1 << 26)) {
            HIPCHECK(pl->d_pktab.alloc(2 * (size_t) n));
            if (zd::launch_pk_table(g, (int) n, pl->d_pktab, 0)) return 1;
            HIPCHECK(hipDeviceSynchronize());
            g.pk_tab = (const double2 *) pl->d_pktab.get();
        }
    }
    if (pl->field) {  // a caller-supplied field: PhiK holds D itself, and ph * 1.0 is ph bit for bit
        const std::vector<double> ones((size_t) (3LL * pl->half * pl->half + 2), 1.0);
        HIPCHECK(upload(pl->d_fnlM, ones));
        g.fnl_M = pl->d_fnlM;
    } else if (g.gen_phi || g.phik) {  // M(k) = 2 g c^2 T(k) k^2 / (3 Omega_M H0^2), zeldovich.cpp:377-383
        const double H0 = 100., c = 299792.458, growth = 1. / (1 + p->z_initial);
        g.fnl_pre = 2. * growth * c * c;
        g.fnl_den = 3. * p->Omega_M * H0 * H0;
        g.n_s     = p->n_s;
        // Normalize(): primordial_norm = power(kmin) / primordial_power(kmin) with norm 1 (power_spectrum.cpp:221-222)
        g.primordial_norm = zd_pk_power(pk, pk->kmin) / (1. * exp(log(pk->kmin) * p->n_s));
        const long long n = 3LL * pl->half * pl->half + 2;
        HIPCHECK(pl->d_fnlM.alloc((size_t) n));
        if (zd::launch_fnl_table(g, (int) n, pl->d_fnlM, 0)) return 1;
        HIPCHECK(hipDeviceSynchronize());
        g.fnl_M = pl->d_fnlM;
    }
    HIPCHECK(pl->d_red.alloc(1));
    HIPCHECK(hipMemset(pl->d_red, 0, sizeof(zd::Reduce)));
    g.var_slots = pl->d_red.get()->sumsq;
    return 0;
}

// ---- jobs of the z stage ----
static void plan_zstage_jobs(zd_plan *pl) {
    zd::JobList &jl = pl->jobs;
    memset(&jl, 0, sizeof(jl));
    jl.pack = pl->pack;
    auto add = [&](int kind, int arr, int twin, int res) {
        jl.kind[jl.n] = kind;
        jl.arr[jl.n]  = arr;
        jl.twin[jl.n] = twin;
        jl.res[jl.n]  = res;
        jl.n++;
    };
    if (pl->pack == zd::PACK_PLTFIELD) {  // the six sums (k_zfft_f: job index = field index)
        add(zd::JOB_PX, 0, 0, 0);
        add(zd::JOB_PY, 1, 0, 0);
        add(zd::JOB_PZ, 2, 0, 0);
        add(zd::JOB_PFX, 3, 0, 0);
        add(zd::JOB_PFY, 4, 0, 0);
        add(zd::JOB_PFZ, 5, 0, 0);
    } else if (pl->pack == zd::PACK_ZAFIELD) {  // the potentials E, Z of the two residues (k_zfft_f: job index = field index)
        add(zd::JOB_E, 0, 0, 0);
        add(zd::JOB_Z, 1, 0, 0);
        add(zd::JOB_E, 2, 0, 1);
        add(zd::JOB_Z, 3, 0, 1);
        if (pl->dens) {  // ZD_qdensity = 1: the density sums of the two residues
            add(zd::JOB_DENS, 4, 0, 0);
            add(zd::JOB_DENS, 5, 0, 1);
        }
    } else if (pl->pack == zd::PACK_ZAPAIR) {  // (qy + i qz)_r0 | (qy + i qz)_r1 | qx_r0 + i qx_r1
        add(zd::JOB_B_SELF, 0, 0, 0);
        add(zd::JOB_B_TWIN, 0, 1, 0);
        add(zd::JOB_B_SELF, 1, 0, 1);
        add(zd::JOB_B_TWIN, 1, 1, 1);
        add(zd::JOB_FX, 2, 0, 0);  // generator output slot 4 = X_self, slot 5 = X_twin input (k_gen/k_genf combine F_x(r0), F_x(r1))
        add(zd::JOB_FX, 2, 1, 1);
    } else if (pl->pack == zd::PACK_PLT3) {  // qx + i vx | qy + i qz | vy + i vz
        add(zd::JOB_XV_SELF, 0, 0, 0);
        add(zd::JOB_XV_TWIN, 0, 1, 0);
        add(zd::JOB_B_SELF, 1, 0, 0);
        add(zd::JOB_B_TWIN, 1, 1, 0);
        add(zd::JOB_D_SELF, 2, 0, 0);
        add(zd::JOB_D_TWIN, 2, 1, 0);
    } else if (pl->narray == 1 && pl->g.lpt2) {  // second-order round: two gradient fields as one array (zd_kernels_lpt2.hip)
        add(zd::JOB_G2_SELF, 0, 0, 0);
        add(zd::JOB_G2_TWIN, 0, 1, 0);
    } else if (pl->narray == 1) {
        add(zd::JOB_DENS, 0, 0, 0);
    } else {
        add(zd::JOB_A_SELF, 0, 0, 0);
        add(zd::JOB_A_TWIN, 0, 1, 0);
        add(zd::JOB_B_SELF, 1, 0, 0);
        add(zd::JOB_B_TWIN, 1, 1, 0);
        if (pl->narray == 4) {
            add(zd::JOB_C_BOTH, 2, 0, 0);
            add(zd::JOB_D_SELF, 3, 0, 0);
            add(zd::JOB_D_TWIN, 3, 1, 0);
        }
    }
}

// ---- block store layout (zd_device.h StoreLayout): chunks per peer rank, ~2 MB tiles inside; work items of the fused Z stage ----
static int plan_block_layout(zd_plan *pl, bool v1) {
    const zd_params *p = &pl->p;
    zd::GenConst &g = pl->g;
    const bool main = !g.gen_phi && !g.phik && !(g.lpt2 >= 1 && g.lpt2 <= 4);  // (the second-order round's x lines read every column too)
    zd::StoreLayout &S = pl->S;
    S.N      = pl->N;
    S.half   = pl->half;
    S.Hq     = pl->Hq;
    S.lHq    = 0;
    while ((1 << S.lHq) < pl->Hq) S.lHq++;
    S.lG = 0;
    while ((1 << S.lG) < pl->nranks) S.lG++;
    S.ky_stride = pl->nranks;
    S.narray = pl->narray;
    S.prune     = tune_env("ZD_PRUNE") ? atoi(tune_env("ZD_PRUNE")) : 7;  // bit 0 k_gen, 1 k_zfft, 2 k_yfft
    S.nt = tune_env("ZD_NT") ? atoi(tune_env("ZD_NT")) : 0;
    if (g.phik) S.prune = 0;  // f_NL second pass: every mode carries power (the zero rule is bypassed)
    if (pl->any) S.prune = 0;  // the convolution kernels transform every column: the generator must write every one
    S.kmax      = g.kmax;
    S.fund2     = g.fundamental2;
    S.k2_cutoff = p->corner_modes ? 0.0 : g.k2_cutoff;  // CornerModes: only the |k_i| == kmax rule prunes
    {
        S.rows_outer = 0;
        int lBk = 20, lBz = 0;  // measured best on MI355X (profiles/r01_layout_sweep.txt): rows of one plane together
        if (const char *env = tune_env("ZD_LAYOUT")) {  // experimentation knob: "lBk,lBz,rows_outer"
            int a = lBk, b = lBz, o = 0;
            if (sscanf(env, "%d,%d,%d", &a, &b, &o) >= 2) {
                lBk = a; lBz = b; S.rows_outer = o;
            }
        }
        const int max_lBk = S.lHq + 1;  // self + twin slots of a chunk in ONE block: chunks are plane-major (zd_multi.cpp
                                        // exchanges them in plane groups)
        while (lBk > max_lBk) lBk--;
        while ((1 << lBz) > pl->Zq) lBz--;
        S.lBk = lBk;
        S.lBz = lBz;
        S.one_block = (pl->nranks == 1 && lBk == S.lHq + 1 && lBz == 0 && !S.rows_outer) ? 1 : 0;
        int row_pad = store_row_pad(pl->N);  // in complex elements
        if (const char *env = tune_env("ZD_PAD")) sscanf(env, "%d", &row_pad);
        // Fused Z stage of the packed PLT store (zd_kernels_fz.hip: generator + z FFT in one kernel, the folded inputs stay on the
        // CU): one rank, z lines of 1024 or 512 points (PPD = 512 = BASELINE C2, 1024, or 2048 = BASELINE C3 at R = 2), the table generator's arithmetic,
        // version-2 streams, the whole field; and the kz = N/2 plane must be dead (the kernel never draws it: true unless
        // CornerModes is set together with ZD_k_cutoff != 1).  ZD_StoreMode = packed keeps the two-kernel stage (A/B runs).
        // Its store interleaves 4 planes along x (StoreLayout::lq = 2) so that a lane's 4 neighbours — 4 consecutive planes of
        // ONE column — write a 64-byte run.
        pl->fused_z = pl->pack == zd::PACK_PLT3 && p->store_mode == ZD_STORE_AUTO && S.one_block && zd::genz_plt_supported(pl->N, pl->L)
                      && g.genf_tab && !v1 && p->qoneslab < 0 && main && p->k_cutoff >= 1.0
                      && (g.kmax == pl->half || !p->corner_modes) && (S.prune & 7) == 7 && !tune_env("ZD_NO_FUSED_Z");
        S.lq         = pl->fused_z ? 2 : 0;
        S.paired     = 0;  // (set with the field store's ring, plan_store)
        // (the pad that spreads the y stage's strided rows over the HBM channels: 24 elements per plain row; per plane row of an
        // interleaved row 12 measured best — y stage of PPD=2048 PLT 144.5 ms at 24, 143.2 at 6, 139.7 at 12, 156.7 at 48)
        if (S.lq && !tune_env("ZD_PAD")) row_pad = store_row_pad(pl->N) / 2;
        S.pitch      = (pl->N + row_pad) << S.lq;
        S.a_rows     = (1 << lBk) << lBz;
        S.zb_rows    = S.a_rows * pl->narray;
        S.kb_rows    = S.zb_rows * ((pl->Zq >> S.lq) >> lBz);
        S.chunk_rows = S.kb_rows * ((2 * pl->Hq) >> lBk);
    }

    pl->ec.N        = pl->N;
    pl->ec.narray   = pl->narray;
    pl->ec.icformat = p->icformat;
    pl->ec.recsize  = record_size(p->icformat);
    pl->ec.qPLT     = p->qPLT;
    pl->ec.qdensity = p->qdensity;
    // (ZD_q2LPT: arrays 2, 3 hold the velocity field alpha psi1 + f2 psi2 as PLT's hold its own)
    pl->ec.vnorm    = (p->qPLT || p->q2LPT) ? 1.0 : (sqrt(1. + 24 * p->f_cluster) - 1) * .25;  // output.cpp:78-82
    pl->ec.pack     = pl->pack == zd::PACK_PLTFIELD ? zd::PACK_PLT3 : pl->pack;  // the y stage builds the PLT3 arrays in the ring
    pl->ec.z_pair   = pl->R / 2;
    pl->ec.xdead_lo = 1;  // (none; set below for the field stores' ring)
    pl->ec.xdead_hi = 0;
    pl->store_bytes_ = (int64_t) S.chunk_rows * S.pitch * pl->nranks * 16;
    // columns no row of which survives the zero rule (column_is_zero with ky = 0): never written by the z stage, skipped by the
    // y stage (whole tiles) and taken as zero by the x stage — power-of-two and composite kernels, every store; not the
    // convolution path (it transforms everything) and not the f_NL passes (prune = 0)
    if ((S.prune & 4) && !pl->any && main) {
        int lo = 0;
        while (lo < pl->half && !zd::column_is_zero(S, lo, 0)) lo++;
        bool all = true;  // the rule is an interval in |kx| for every ky: check it rather than assume it
        for (int kx = lo; kx <= pl->half && all; kx++) all = zd::column_is_zero(S, kx, 0) && zd::column_is_zero(S, -kx, 0);
        if (all && lo >= 1) {
            pl->ec.xdead_lo = lo;
            pl->ec.xdead_hi = pl->N - lo;
            S.prune |= zd::PRUNE_YTILE;  // the x kernels take zeros there: the y stage may skip those tiles
        }
    }
    if (pl->fused_z) {
        // work items of k_genz_plt: for every half-space row ky >= 1 the live columns kx in (-w, w) (zero rule: column_is_zero), cut
        // where the draw counter of a row jumps (x = N/2 | N/2 + 1) and into pieces of at most 128 columns (a piece costs its
        // threads one jump from the row's stream head: ~14 steps of the 2^i table against 4 x 128 draws); longest first
        std::vector<zd::FzItem> items;
        const int SEG = 128;
        for (int kyl = (pl->rank == 0 ? 1 : 0); kyl < pl->Hq; kyl++) {
            const int ky = pl->rank + pl->nranks * kyl;
            auto add_range = [&](int xa, int xb) {  // [xa, xb): maximal runs of live columns, in pieces
                int x = xa;
                while (x < xb) {
                    while (x < xb && zd::column_is_zero(S, x > pl->half ? x - pl->N : x, ky)) x++;
                    int e = x;
                    while (e < xb && !zd::column_is_zero(S, e > pl->half ? e - pl->N : e, ky)) e++;
                    for (int q = x; q < e; q += SEG) items.push_back(zd::FzItem{kyl, q, std::min(SEG, e - q), 0});
                    x = e;
                }
            };
            add_range(0, pl->half + 1);
            add_range(pl->half + 1, pl->N);
        }
        std::stable_sort(items.begin(), items.end(), [](const zd::FzItem &a, const zd::FzItem &b) { return a.n > b.n; });
        pl->n_fzitems = (unsigned) items.size();
        if (!items.empty()) HIPCHECK(upload(pl->d_fzitems, items));
        int dev = 0;
        hipGetDevice(&dev);
        hipDeviceGetAttribute(&pl->ncu, hipDeviceAttributeMultiprocessorCount, dev);
        if (pl->ncu < 1) pl->ncu = 256;
    }
    return 0;
}

// ---- the store: the reference arrays as a simple [plane][array][y][x] store with tables for the z lines (length L) and the y / x
// lines (length N) — composite twiddles where the route says so (f_NL on the composite grids), Bluestein tables otherwise; a field
// store and the ring between its y and x stages ----
static int plan_stores(zd_plan *pl, bool twr) {
    if (pl->any) {
        if (twr) {
            if (upload_twq(pl->N, pl->d_twr_n) || upload_twq(pl->L, pl->d_twr_l)) {
                fprintf(stderr, "zeldovich_hip: composite twiddle tables failed\n");
                return 1;
            }
        } else if (any_make_tab(pl->L, &pl->tabL, pl->d_any) || any_make_tab(pl->N, &pl->tabN, pl->d_any + 3)) {
            return 1;
        }
        pl->AL.N         = pl->N;
        pl->AL.pitch     = pl->N + store_row_pad(pl->N);
        pl->AL.narray    = pl->narray;
        pl->store_bytes_ = (int64_t) pl->L * pl->narray * pl->N * pl->AL.pitch * 16;
        if (pl->nranks > 1) {  // [chunk = peer rank][local plane][array][row slot < 2 Hq][x]: 1 / G of the one-rank store
            pl->AC           = zd::AnyChunks{pl->N, pl->AL.pitch, pl->narray, pl->nranks, pl->Hq, pl->Zq, 0};
            pl->AC.chunk     = (long long) pl->Zq * pl->narray * 2 * pl->Hq * pl->AL.pitch;
            pl->store_bytes_ = (int64_t) pl->nranks * pl->AC.chunk * 16;
        }
    }
    if (!zd::pack_is_fields(pl->pack)) return 0;
    zd::StoreLayout &S = pl->S;
    std::vector<zd::FieldRow> rows;
    const int64_t fe = field_rows(&pl->p, pl->nranks, &rows);
    HIPCHECK(upload(pl->d_fieldrows, rows));
    pl->F.lG          = S.lG;
    pl->F.lZq         = 0;
    while ((1 << pl->F.lZq) < pl->Zq) pl->F.lZq++;
    pl->F.Zq          = pl->Zq;
    pl->F.field_elems = fe;
    pl->F.ndens       = pl->dens ? 2 : 0;
    pl->F.nfield      = pl->pack == zd::PACK_PLTFIELD ? 6 : 4 + pl->F.ndens;
    pl->F.chunk_elems = (int64_t) pl->Zq * pl->F.nfield * fe;
    pl->F.rows        = pl->d_fieldrows;
    pl->store_bytes_  = pl->F.chunk_elems * pl->nranks * 16;
    // ring: `ring_planes` store planes of the three arrays, laid out as a single-rank block store (one_block)
    pl->ring_planes = field_ring_planes(pl->N, pl->Zq);
    // the ZA potentials at the sizes whose ring k_xfft_seq consumes: the y stage computes the columns x and N - x from one fetch and
    // writes them side by side (zd_device.h ring_pair_w).  The y launch takes the store's layout, the x launch the ring's: both say so
    S.paired = pl->pack == zd::PACK_ZAFIELD && pl->F.nfield == 4 ? zd::ring_pair_w(pl->N) : 0;
#ifdef ZD_TESTING
    if (S.paired && pl->N == 1024 && g_ring_pair_w.load() == 4) S.paired = 4;  // zd_test_ring_pair_w
#endif
    zd::StoreLayout &Q = pl->SR;
    Q            = S;
    Q.lq         = 0;
    Q.Hq         = pl->half;
    Q.lHq        = 0;
    while ((1 << Q.lHq) < pl->half) Q.lHq++;
    Q.lG         = 0;
    Q.ky_stride  = 1;
    Q.narray     = 3;
    Q.lBk        = Q.lHq + 1;
    Q.lBz        = 0;
    Q.rows_outer = 0;
    Q.one_block  = 1;
    Q.prune      = 0;
    Q.pitch      = pl->N + store_row_pad(pl->N);
    Q.a_rows     = pl->N;
    Q.zb_rows    = 3 * pl->N;
    Q.kb_rows    = Q.zb_rows * pl->ring_planes;
    Q.chunk_rows = Q.kb_rows;
    HIPCHECK(pl->d_ring.store_alloc((size_t) Q.chunk_rows * Q.pitch));
    if (pl->dens)  // the density array delta_r0 + i delta_r1 of the ring's planes: [plane][y][x]
        HIPCHECK(pl->d_ring_dens.store_alloc((size_t) pl->ring_planes * pl->N * Q.pitch));
    return 0;
}

// ---- folded-input slabs (two, for the gen||zfft overlap): enough rows per launch to fill the chip ----
static int plan_slabs(zd_plan *pl, bool v1, int64_t eig_ppd) {
    const zd_params *p = &pl->p;
    zd::GenConst &g = pl->g;
    const int64_t N = pl->N;
    const int64_t row_b = y_bytes_per_row(pl);
    int64_t slab_b = (int64_t) 3 << 29;  // ~1.5 GB per buffer
    if (const char *env = tune_env("ZD_SLAB_MB")) slab_b = (int64_t) atoll(env) << 20;
#ifdef ZD_SLAB_MB_FORCE  // experiment (make variant)
    slab_b = (int64_t) ZD_SLAB_MB_FORCE << 20;
#endif
    int rows = (int) std::max<int64_t>(1, slab_b / row_b);
    rows     = std::min(rows, pl->Hq);
    if (zd::pack_is_fields(pl->pack)) {  // whole row blocks
        rows = std::max(zd::FIELD_RB, rows / zd::FIELD_RB * zd::FIELD_RB);
        while (pl->Hq % rows) rows -= zd::FIELD_RB;
    }
    if (v1) {  // the accepted pairs of a slab: N^2 x 16 B per row, <= ~4 GB
        const int minr = zd::pack_is_fields(pl->pack) ? zd::FIELD_RB : 1;
        rows = std::max<int64_t>(minr, std::min<int64_t>(rows, ((int64_t) 4 << 30) / (N * N * 16)));
        if (zd::pack_is_fields(pl->pack)) rows = rows / zd::FIELD_RB * zd::FIELD_RB;
    }
    while (pl->Hq % rows) rows--;
    pl->slab_rows = rows;
    pl->overlap   = p->serial_z == 0 && !v1 && !pl->any;  // version 1: the streams are sequential in ky
    // PLT with a table that is interpolated (eig_ppd does not divide into PPD): the (x, y) part of the trilinear lookup is
    // done once per column of a slab (k_eig_lines) instead of once per mode; one slab of lines, refilled on the generator's
    // stream in front of every generator launch
    if (g.qPLT && g.genf_tab && !v1 && eig_ppd % N != 0) {
        const size_t n = (size_t) (eig_ppd / 2 + 1) * rows * N * 4;
        if (n * sizeof(double) <= ((size_t) 1 << 30)) {
            HIPCHECK(pl->d_eiglines.alloc(n));
            g.eig_lines = pl->d_eiglines;
            g.eig_rows  = rows;
        }
    }
    if (v1) {
        pl->v1_block = (int) (N / p->numblock);
        HIPCHECK(pl->d_v1streams.alloc((size_t) pl->v1_block));
        HIPCHECK(pl->d_v1dev.alloc((size_t) rows * N * N));
        HIPCHECK(pl->d_v1err.alloc(1));
        HIPCHECK(hipMemset(pl->d_v1err, 0, sizeof(int)));
        g.v1dev = pl->d_v1dev;
    }
    // k_genf is a persistent kernel: a few workgroups per CU pull tiles from a counter (one per launch).  With
    // the second stream active the grid is kept small enough that a k_zfft workgroup (64 KB LDS, 2 waves/SIMD)
    // always fits beside the generator's waves on every CU.
    {
        int dev = 0, ncu = 256;
        hipGetDevice(&dev);
        hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
        int per_cu = pl->overlap ? 3 : 6;
        if (const char *env = tune_env("ZD_GEN_WGS")) per_cu = atoi(env);
#ifdef ZD_GEN_WGS_FORCE  // experiment (make variant)
        if (pl->overlap) per_cu = ZD_GEN_WGS_FORCE;
#endif
        pl->gen_max_wgs = std::max(1, per_cu) * std::max(1, ncu);
        pl->n_tilectr   = 2 * (pl->Hq / rows) + 2;  // per pass parity: the next pass's generator may already run
        HIPCHECK(pl->d_tilectr.alloc((size_t) pl->n_tilectr));
    }
    // ring size: 1 slab without the overlap, else 2 + what the store (allocated by the caller afterwards) leaves
    int K = 1;
    if (pl->overlap) {
        K = 2;
        const int nslab = pl->Hq / rows;
        // Measured (PPD=4096 ZA, 60 slabs ahead): no gain — the generator's resident workgroups take LDS and
        // registers from k_yfft (128 KB LDS per workgroup at PPD=4096), which slows down by what the z stage gains.
        // The larger ring therefore stays an experiment: ZD_Y_AHEAD=1 sizes it from free HBM, ZD_Y_SLABS=n fixes it.
        if (tune_env("ZD_Y_AHEAD") && pl->npass > 1 && nslab > 2) {
            size_t free_b = 0, total_b = 0;
            hipMemGetInfo(&free_b, &total_b);
            const int64_t reserve = zd_plan_exchange_bytes(pl) * (pl->nranks > 1 ? 2 : 1) + ((int64_t) 8 << 30);
            const int64_t spare   = (int64_t) free_b - reserve;
            if (spare > 0) K = (int) std::max<int64_t>(2, std::min<int64_t>(nslab, spare / (row_b * rows)));
        }
        if (const char *env = tune_env("ZD_Y_SLABS")) K = std::max(2, atoi(env));
    }
    pl->d_Y.resize(K);
    for (int i = 0; i < K; i++) HIPCHECK(pl->d_Y[i].alloc((size_t) row_b * rows / sizeof(cplx)));
    if (pl->overlap) {
#ifdef ZD_TUNING
        // A/B (VERDICT r4 #5 i): ZD_CU_SPLIT = n gives the z FFT's stream n CUs of every XCD's 32 and the generator's stream
        // the other 32 - n (hipExtStreamCreateWithCUMask; CU c of the mask = XCD c % 8, CU c / 8 of it on this part)
        if (const char *env = tune_env("ZD_CU_SPLIT")) {
            const int nf = std::max(1, std::min(31, atoi(env)));
            uint32_t mg[8] = {0}, mf[8] = {0};
            for (int c = 0; c < 256; c++) ((c / 8) < nf ? mf : mg)[c / 32] |= 1u << (c % 32);
            hipStream_t sg = nullptr, sf = nullptr;
            HIPCHECK(hipExtStreamCreateWithCUMask(&sg, 8, mg));
            pl->s_gen.reset(sg);
            HIPCHECK(hipExtStreamCreateWithCUMask(&sf, 8, mf));
            pl->s_fft.reset(sf);
        } else
#endif
        {
            HIPCHECK(pl->s_gen.create());
            HIPCHECK(pl->s_fft.create());
        }
        HIPCHECK(pl->ev_fork.create(hipEventDisableTiming));
        pl->ev_gen.resize(K);
        pl->ev_fft.resize(K);
        for (int i = 0; i < K; i++) {
            HIPCHECK(pl->ev_gen[i].create(hipEventDisableTiming));
            HIPCHECK(pl->ev_fft[i].create(hipEventDisableTiming));
        }
    }
    return 0;
}

// a zeroed GenConst with the constants of the zero rule (zeldovich.cpp:299-320, 350; zd_device.h mode_is_zero): what every plan starts
// from, and all that the intake of a caller-supplied field (make_field_phik) needs of it
static void gen_zero_rule(zd::GenConst &g, const zd_params *p) {
    memset(&g, 0, sizeof(g));
    g.N            = (int) p->ppd;
    g.half         = g.N / 2;
    g.kmax         = (int) ((double) g.half * (1.0 / p->k_cutoff) + .5);
    g.corner_modes = p->corner_modes;
    g.qonemode     = p->qonemode;
    for (int i = 0; i < 3; i++) g.one_mode[i] = p->one_mode[i];
    g.fundamental  = p->fundamental;
    g.fundamental2 = p->fundamental * p->fundamental;
    g.k2_cutoff    = p->nyquist * p->nyquist / (p->k_cutoff * p->k_cutoff);
    {  // the comparison `k2 >= k2_cutoff` of zeldovich.cpp:353 is monotonic in the integer |k|^2
        long long c = (long long) floor(g.k2_cutoff / g.fundamental2);
        while (c > 0 && (double) c * g.fundamental2 >= g.k2_cutoff) c--;
        while ((double) c * g.fundamental2 < g.k2_cutoff) c++;
        g.k2i_cut = (int) std::min<long long>(c, 0x7fffffffLL);
    }
}

// the growth constants of the per-mode coefficients (zeldovich.cpp:403-434): every plan's, and those of zd_field_vjp
static void gen_growth(zd::GenConst &g, const zd_params *p) {
    g.qPLT         = p->qPLT;
    g.qPLTrescale  = p->qPLTrescale;
    g.f_cluster    = p->f_cluster;
    g.target_f     = (sqrt(1. + 24 * p->f_cluster) - 1) / 4.;
    double a_NL = 1.0, a0 = 1.0;
    if (p->qPLTrescale) {
        a_NL = 1. / (1 + p->PLT_target_z);
        a0   = 1. / (1 + p->z_initial);
    }
    g.ln_growth_ratio = log(a_NL / a0);
}

// a plan of the shape an accepted route gives; each part above fills its own members; a plan that fails half-way releases what it has
static int plan_create_one(const zd_params *p, const Route &rt, const zd_pk *pk, const double *eig, int64_t eig_ppd, int rank, int nranks,
                           int role, const cplx *phik, bool field, PlanPtr &out) {
    PlanPtr plan(new zd_plan);
    zd_plan *pl   = plan.get();
    pl->p         = *p;
    pl->field     = field;
    pl->rank      = rank;
    pl->nranks    = nranks;
    pl->N         = (int) p->ppd;
    pl->half      = pl->N / 2;
    pl->any       = rt.family >= zd::FAM_REF_COMPOSITE;
    pl->pack      = rt.pack;
    pl->narray    = rt.narray;
    pl->dens      = rt.dens;
    pl->dens_only = rt.dens_only;
    pl->pstep     = rt.pstep;
    pl->npass     = rt.npass;
    pl->R         = rt.R;
    pl->L         = rt.L;
    pl->Hq        = rt.Hq;
    pl->Zq        = rt.Zq;
    const bool v1 = p->version == 1 && phik == nullptr && !p->q2LPT;  // (the second f_NL pass takes D from PhiK and draws nothing)
    // ---- generator constants (zeldovich.cpp:299-320, 350) ----
    zd::GenConst &g = pl->g;
    gen_zero_rule(g, p);
    g.ablate       = tune_env("ZD_ABLATE") ? atoi(tune_env("ZD_ABLATE")) : 0;
    g.pk_n         = pk->n;
    g.fixed_power  = pk->fixed_power;
    g.is_powerlaw  = pk->is_powerlaw;
    g.pk_norm      = pk->normalization;
    g.pk_smooth2   = pk->Pk_smooth2;
    g.powerlaw_index = pk->powerlaw_index;
    gen_growth(g, p);
    g.eig_ppd = eig_ppd;
    g.gen_phi = role == zd::ROLE_PHI;
    g.phik    = p->q2LPT ? nullptr : phik;
    if (role == zd::ROLE_LPT2_GRAD) g.lpt2 = 1;  // (make_lpt2_source sets the pass in front of every Z stage)
    if (role == zd::ROLE_MAIN && p->q2LPT) {     // final pass: positions from D + gamma S, velocities from alpha D + f2 gamma S
        g.lpt2       = 5;
        g.lpt2_sk    = phik;
        g.lpt2_gamma = -zd::lpt2_ratio(p);
        g.lpt2_alpha = zd::lpt2_alpha(p);
        g.lpt2_f2g   = zd::lpt2_f2(p) * g.lpt2_gamma;
        if (p->q3LPT) {  // ... plus the third order (the spectra: adopt_lpt3)
            g.lpt3     = 7;
            g.lpt3_g3c = zd::lpt3_g3c(p);
            g.lpt3_f3  = zd::lpt3_f3(p);
        }
    }
    if (role == zd::ROLE_PHI) g.qPLT = 0;  // the phi pass stops before the displacement algebra (zeldovich.cpp:385-391)
    plan_zstage_jobs(pl);
    if (plan_device_tables(pl, pk, eig, eig_ppd) || plan_block_layout(pl, v1) || plan_stores(pl, rt.twr) || plan_slabs(pl, v1, eig_ppd)) return 1;
    out = std::move(plan);
    return 0;
}

static int plan_create_ex(const zd_params *p_in, const zd_pk *pk, const double *eig, int64_t eig_ppd, int rank, int nranks,
                          int phi_mode, const cplx *phik, PlanPtr &out, bool field) {
    const zd_params pc = zd::canonical(p_in);
    const int role = phi_mode == 1 ? zd::ROLE_PHI : phi_mode == 2 ? zd::ROLE_LPT2_GRAD : (phik && !pc.q2LPT) ? zd::ROLE_PHIK : zd::ROLE_MAIN;
    if (pc.q2LPT && role == zd::ROLE_MAIN && !phik) {  // (zd_plan_create and zd_generate run the second-order round first)
        fprintf(stderr, "zeldovich_hip: a ZD_q2LPT plan needs the second-order source\n");
        return 1;
    }
    const bool have_eig = eig != nullptr && eig_ppd > 0;
    zd_params pa, pb;
    Route ra, rb;
    if (role == zd::ROLE_MAIN && zd::plt_dens_split(&pc, nranks) && have_eig && split_routes(&pc, pc.stream_factor, &pa, &pb, &ra, &rb) && ra.ok()
        && rb.ok()) {
        PlanPtr A, B;
        if (plan_create_one(&pa, ra, pk, eig, eig_ppd, rank, nranks, role, nullptr, false, A) == 0
            && plan_create_one(&pb, rb, pk, nullptr, 0, rank, nranks, role, nullptr, false, B) == 0
            && A->d_dens_pass.store_alloc((size_t) A->Zq * pc.ppd * pc.ppd) == hipSuccess) {
            A->p            = pc;  // (what the callers read back: ZD_qdensity = 1)
            A->store_bytes_ = std::max(A->store_bytes_, B->store_bytes_);
            A->dens_sub     = std::move(B);
            out             = std::move(A);
            return 0;
        }
        // (A and B go away here) the run falls back to the reference arrays (convolution path)
    }
    const Route rt = route(&pc, pc.stream_factor, nranks, role, rank, have_eig);
    if (!rt.ok()) {
        fprintf(stderr, "zeldovich_hip: %s\n", rt.why);
        return 1;
    }
    return plan_create_one(&pc, rt, pk, eig, eig_ppd, rank, nranks, role, phik, field, out);
}

zd_plan::~zd_plan() {  // the members release themselves afterwards
    collect_events(this);
    zdown::live(-1);
}
void zd_plan_destroy(zd_plan *pl) { delete pl; }

int32_t zd_plan_narray(const zd_plan *pl) { return pl->narray; }
int32_t zd_plan_store_mode(const zd_plan *pl) {
    return pl->pack == zd::PACK_NONE ? ZD_STORE_REFERENCE : zd::pack_is_fields(pl->pack) ? ZD_STORE_FIELDS : ZD_STORE_PACKED;
}
int32_t zd_plan_stream_factor(const zd_plan *pl) { return pl->R; }
int32_t zd_plan_record_size(const zd_plan *pl) { return pl->ec.recsize; }
int64_t zd_plan_exchange_bytes(const zd_plan *pl) { return pl->store_bytes_; }
int32_t zd_plan_passes(const zd_plan *pl) { return pl->npass; }
int32_t zd_plan_plane_step(const zd_plan *pl) { return pl->pstep; }
int64_t zd_plan_local_planes(const zd_plan *pl) { return (int64_t) pl->Zq * pl->pstep; }
int64_t zd_plan_plane_z(const zd_plan *pl, int pass, int64_t local_plane) {
    // PACK_ZAPAIR: store plane zl of pass p carries z-residues p (delivered plane 2 zl) and p + R/2 (plane 2 zl + 1)
    const int64_t zl = local_plane / pl->pstep, which = local_plane % pl->pstep;
    return (pass + which * (pl->R / 2)) + (int64_t) pl->R * ((int64_t) pl->rank * pl->Zq + zl);
}

// z FFT of one slab of generated rows into the block store (reference / packed arrays with Hermitian twins, or the
// potentials of the field store)
static int launch_zstage_fft(zd_plan *pl, int ky0, int kyloc0, int nky, const void *Y, void *d_send, hipStream_t st) {
    if (pl->d_twq_l) return zd::launch_zfft_fields_np2(pl->L, pl->F, pl->S, ky0, kyloc0, nky, Y, pl->d_twq_l, d_send, st);
    if (zd::pack_is_fields(pl->pack)) return zd::launch_zfft_fields(pl->L, pl->F, pl->S, ky0, kyloc0, nky, Y, pl->d_twL, d_send, st);
    return zd::launch_zfft(pl->L, pl->jobs, pl->S, ky0, kyloc0, nky, pl->Zq, Y, pl->d_twL, d_send, st);
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
        tick(pl, ZD_K_GEN, st, true);
        if (pl->v1_block) {  // ZD_Version = 1: rows that share a stream are drawn by successive launches (zd_plan_stage_z)
            const int group = pl->v1_block / G;
            for (int i0 = 0; i0 < nky; i0 += group)
                if (zd::launch_v1_draw(pl->g, pl->v1_block, ky_first + G * (r0 + i0), G, std::min(group, nky - i0), pl->d_v1streams,
                                       pl->d_v1dev + (size_t) i0 * pl->N * pl->N, pl->d_v1err, st))
                    return 1;
        }
        // (k_genf with walks of 16 / 4 / 2 z rows where the kernel exists, else the general generator)
        if (pl->d_eiglines && zd::launch_eig_lines(pl->g, ky_first + G * r0, G, nky, pl->d_eiglines, st)) return 1;
        if (zd::launch_gen(pl->g, pl->J, pl->jobs, pl->S, ky_first + G * r0, nky, pl->L, residue, residue, pl->d_twN, pl->d_Y[0],
                           pl->d_tilectr + slab, pl->gen_max_wgs, st))
            return 1;
        tick(pl, ZD_K_GEN, st, false);
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
            tick(pl, ZD_K_GEN, st, true);
            if (pl->v1_block) {
                const int group = pl->v1_block / G;
                for (int i0 = 0; i0 < nky; i0 += group)
                    if (zd::launch_v1_draw(pl->g, pl->v1_block, ky_first + G * (r0 + i0), G, std::min(group, nky - i0), pl->d_v1streams,
                                           pl->d_v1dev + (size_t) i0 * pl->N * pl->N, pl->d_v1err, st))
                        return 1;
            }
            if (pl->d_eiglines && zd::launch_eig_lines(pl->g, ky_first + G * r0, G, nky, pl->d_eiglines, st)) return 1;
            if (zd::launch_gen(pl->g, pl->J, pl->jobs, pl->S, ky_first + G * r0, nky, pl->L, residue, residue2, pl->d_twN, pl->d_Y[0],
                               pl->d_tilectr + slab, pl->gen_max_wgs, st))
                return 1;
            tick(pl, ZD_K_GEN, st, false);
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
        tick(pl, ZD_K_GEN, pl->s_gen, true);
        if (pl->d_eiglines && zd::launch_eig_lines(pl->g, ky_first + G * r0, G, pl->slab_rows, pl->d_eiglines, pl->s_gen)) return 1;
        if (zd::launch_gen(pl->g, pl->J, pl->jobs, pl->S, ky_first + G * r0, pl->slab_rows, pl->L, pass,
                           pl->pstep == 2 ? pass + pl->R / 2 : pass, pl->d_twN, pl->d_Y[slot], ctr + slab,
                           pl->gen_max_wgs, pl->s_gen))
            return 1;
        tick(pl, ZD_K_GEN, pl->s_gen, false);
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
static zd::StoreLayout layout_for_chunks(const zd_plan *pl, int chunk_planes) {
    zd::StoreLayout S = pl->S;
    if (chunk_planes != pl->Zq) {
        S.kb_rows    = S.zb_rows * (chunk_planes >> S.lBz);
        S.chunk_rows = S.kb_rows * ((2 * pl->Hq) >> S.lBk);
    }
    return S;
}
static zd::AnyChunks any_chunks(const zd_plan *pl, int chunk_planes) {
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
        for (int g0 = 0; g0 < np; g0 += pl->ring_planes) {
            const int ng = std::min(pl->ring_planes, np - g0);
            char *rec_g = d_records ? (char *) d_records + (size_t) g0 * ps * pl->N * pl->N * pl->ec.recsize : nullptr;
            const int z_first = (int) zd_plan_plane_z(pl, residue, gplane0 + (int64_t) g0 * ps);
            tick(pl, ZD_K_YFFT, st, true);
            if (!pl->dens_only
                && (pl->d_twq_n ? zd::launch_yfft_fields_np2(F, pl->S, pl->d_twq_n, d_recv, p0 + g0, ng, pl->SR.pitch, pl->d_ring, 0, st)
                                : zd::launch_yfft_fields(F, pl->S, pl->d_twN, d_recv, p0 + g0, ng, pl->SR.pitch, pl->d_ring, st)))
                return 1;
            if (pl->dens && d_density
                && zd::launch_yfft_fields_np2(F, pl->S, pl->d_twq_n, d_recv, p0 + g0, ng, pl->SR.pitch, pl->d_ring_dens, 1, st))
                return 1;
            tick(pl, ZD_K_YFFT, st, false);
            tick(pl, ZD_K_XFFT, st, true);
            if (!pl->dens_only
                && (pl->d_twq_n ? zd::launch_xfft_np2(pl->N, pl->ec, pl->d_twq_n, pl->d_ring, pl->SR.pitch, ng, z_first, pl->R, rec_g, pl->d_red, st)
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

// ------------------------------------------------------------------------------------------------
// zd_generate, and zd_generate_field (fs != NULL: the modes come from the caller's field; its refusals have been asked)
static int generate_impl(const zd_params *p_in, const zd_pk *pk, const double *eig, int64_t eig_ppd, zd_slab_cb cb, void *user, zd_stats *out,
                         const FieldSpec *fs);
int zd_generate(const zd_params *p_in, const zd_pk *pk, const double *eig, int64_t eig_ppd, zd_slab_cb cb,
                void *user, zd_stats *out) {
    return generate_impl(p_in, pk, eig, eig_ppd, cb, user, out, nullptr);
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

static int generate_impl(const zd_params *p_in, const zd_pk *pk, const double *eig, int64_t eig_ppd, zd_slab_cb cb, void *user, zd_stats *out,
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
    // ---- ZD_q2LPT: the second-order round (zd_kernels_lpt2.hip); the chooser has counted S(k) beside the passes' stores ----
    if (p.q2LPT && make_lpt2_source(&p, pk, d_phik)) return 1;
    // ---- ZD_q3LPT: the third-order round (zd_kernels_lpt3.hip); P3(k) and C_x,y,z(k) stay beside S(k), counted likewise ----
    DevBuf<cplx> d_lpt3[4];
    if (p.q3LPT && make_lpt3_sources(&p, pk, d_phik, d_lpt3)) return 1;
    // ---- a caller-supplied field (zd_kernels_field.hip): PhiK = its modes; no draw is made ----
    if (fs && make_field_phik(&p, pk, *fs, d_phik)) return 1;
    PlanPtr plan;
    if (plan_create_ex(&p, pk, eig, eig_ppd, 0, 1, 0, d_phik, plan, fs != nullptr)) return 1;
    zd_plan *pl      = plan.get();
    pl->d_phik_owned = std::move(d_phik);
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

// ------------------------------------------------------------------------------------------------
// the PLT eigenmode table (definition and kernels: zd_kernels_plt.hip)

// what zd_make_eigenmodes (and the parameter reader, zd_host.cpp) refuses; NULL: nothing
static const char *plt_table_refusal(int64_t n, char *buf, size_t cap) {
    if (n >= 4 && n <= ZD_PLT_MAX_PPD && n % 2 == 0) return nullptr;
    snprintf(buf, cap, "an eigenmode table has an even number of points per side in [4, %d] (got %lld)", ZD_PLT_MAX_PPD, (long long) n);
    return buf;
}

int zd_make_eigenmodes(int64_t n, double *eig) {
    char buf[160];
    if (const char *why = plt_table_refusal(n, buf, sizeof(buf))) {
        fprintf(stderr, "zeldovich_hip: zd_make_eigenmodes: %s\n", why);
        return 1;
    }
    if (!eig) {
        fprintf(stderr, "zeldovich_hip: zd_make_eigenmodes needs an output array\n");
        return 1;
    }
    const zd::PltConst c = zd::plt_const((int) n, zd::PLT_ALPHA);
    const size_t plane = (size_t) n * (n / 2 + 1) * 4;  // doubles of one kx plane
    // chunks of kx planes of at most 2^21 wavevectors (64 MB): a table of 512 points is 2.2 GB and 7e7 threads
    const int chunk = (int) std::max<int64_t>(1, std::min<int64_t>(n, ((int64_t) 1 << 23) / (int64_t) plane));
    DevBuf<double> d_tab, d_out;
    if (upload(d_tab, zd::plt_shell_table(zd::PLT_ALPHA, zd::PLT_SHELLS)) != hipSuccess || d_out.alloc(plane * chunk) != hipSuccess) {
        fprintf(stderr, "zeldovich_hip: zd_make_eigenmodes: no device memory for %zu bytes (is there a GPU?)\n", plane * chunk * sizeof(double));
        return 1;
    }
    for (int kx0 = 0; kx0 < n; kx0 += chunk) {
        const int nkx = std::min<int>(chunk, (int) n - kx0);
        if (zd::launch_plt_modes(c, d_tab, kx0, nkx, d_out, 0)) return 1;
        HIPCHECK(hipMemcpy(eig + plane * kx0, d_out, plane * nkx * sizeof(double), hipMemcpyDeviceToHost));
    }
    return 0;
}

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

}  // extern "C"
