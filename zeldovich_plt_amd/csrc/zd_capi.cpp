// zd_capi.cpp — C ABI (include/zeldovich_hip.h): plan management — the device tables of the generator and the transforms, the jobs
// of the Z stage, the layouts of the stores, the slabs; zd_plan_create, zd_plan_destroy, the plan's accessors — and the PLT eigenmode
// table.  The other jobs of the C ABI have a unit each (zd_capi*.cpp); zd_capi.h holds what they share.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "zd_capi.h"
#include "zd_plt.h"

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
static std::vector<double> build_genf_table(const zd_pk *pk, int nseg, double *lut_x0, double *lut_inv_dx) {
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

static int record_size(int icformat) {  // include/output.h:19-42
    switch (icformat) {
        case ZD_FMT_ZEL: return 32;
        case ZD_FMT_RVZEL: return 32;
        case ZD_FMT_RVDOUBLEZEL: return 56;
        case ZD_FMT_ZELSIMPLE: return 12;
    }
    return 0;
}

static int64_t y_bytes_per_row(const zd_plan *pl) { return (int64_t) pl->jobs.n * pl->L * pl->N * 16; }

// advance by (2*65536*drows - 1) draws, drows may be negative (period 2^128)
static zdpcg::Affine row_jump(long long drows) {
    const __int128 d = (__int128) 2 * 65536 * (__int128) drows - 1;
    return zdpcg::jump_map((u128) d);
}
static zdpcg::Affine row_jump_full(long long drows) {  // 2*65536*drows draws
    const __int128 d = (__int128) 2 * 65536 * (__int128) drows;
    return zdpcg::jump_map((u128) d);
}

// a plan that was made goes to a caller of the C ABI; *out is left alone otherwise
int hand_over(int rc, PlanPtr &pl, zd_plan **out) {
    if (!rc) *out = pl.release();
    return rc;
}

// twiddles of a composite transform (zd_fft_q.h) of length len = P * Q: exp(2 pi i k / P) | exp(2 pi i k / len) | exp(2 pi i k / Q)
std::vector<cplx> make_twq(int len) {  // (empty: no such transform)
    int P = 0, Q = 0;
    if (!zd::np2_split(len, &P, &Q)) return {};
    std::vector<cplx> t = make_twiddles(P), b = make_twiddles(len), c = make_twiddles(Q);
    t.insert(t.end(), b.begin(), b.end());
    t.insert(t.end(), c.begin(), c.end());
    return t;
}
int upload_twq(int len, DevBuf<cplx> &dst) {
    const std::vector<cplx> t = make_twq(len);
    return t.empty() || upload(dst, t) != hipSuccess;
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
static int plan_block_layout(zd_plan *pl, int role) {
    const zd_params *p = &pl->p;
    zd::GenConst &g = pl->g;
    // (a second-order plan on a caller-supplied field reads D from PhiK where the seeded one draws it: same zero rule, same pruning)
    const bool every_mode = g.phik && !g.lpt2;
    const bool main = !g.gen_phi && !every_mode && !(g.lpt2 >= 1 && g.lpt2 <= 4);  // (the second-order round's x lines read every column too)
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
    if (every_mode) S.prune = 0;  // f_NL second pass: every mode carries power (the zero rule is bypassed)
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
        pl->fused_z = zd::fused_z_route(p, pl->pack, pl->N, pl->L, role, S.one_block != 0) && g.genf_tab && (S.prune & 7) == 7;
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
static int plan_stores(zd_plan *pl) {
    if (pl->any) {
        if (pl->twr) {
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
void gen_zero_rule(zd::GenConst &g, const zd_params *p) {
    memset(&g, 0, sizeof(g));
    g.N            = (int) p->ppd;
    g.half         = g.N / 2;
    g.kmax         = zd::kmax(g.half, p->k_cutoff);
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
void gen_growth(zd::GenConst &g, const zd_params *p) {
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
                           int role, const cplx *phik, bool field, const cplx *field_d, PlanPtr &out) {
    PlanPtr plan(new zd_plan);
    zd_plan *pl   = plan.get();
    pl->p         = *p;
    pl->field     = field;
    pl->rank      = rank;
    pl->nranks    = nranks;
    pl->N         = (int) p->ppd;
    pl->half      = pl->N / 2;
    pl->family    = rt.family;
    pl->twr       = rt.twr;
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
    g.phik    = p->q2LPT ? field_d : phik;  // (ZD_q2LPT: phik is S(k), below; PhiK is there only as the modes of a caller-supplied field)
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
    if (plan_device_tables(pl, pk, eig, eig_ppd) || plan_block_layout(pl, role) || plan_stores(pl) || plan_slabs(pl, v1, eig_ppd)) return 1;
    out = std::move(plan);
    return 0;
}

int plan_create_ex(const zd_params *p_in, const zd_pk *pk, const double *eig, int64_t eig_ppd, int rank, int nranks, int phi_mode,
                   const cplx *phik, PlanPtr &out, bool field, const cplx *field_d) {
    const zd_params pc = zd::canonical(p_in);
    if (field_d && (!pc.q2LPT || !field || nranks != 1)) {  // (the first order of a field run takes its modes as phik)
        fprintf(stderr, "zeldovich_hip: ZD_Field: the modes of a field beside S(k) belong to a second-order plan on one rank\n");
        return 1;
    }
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
        if (plan_create_one(&pa, ra, pk, eig, eig_ppd, rank, nranks, role, nullptr, false, nullptr, A) == 0
            && plan_create_one(&pb, rb, pk, nullptr, 0, rank, nranks, role, nullptr, false, nullptr, B) == 0
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
    return plan_create_one(&pc, rt, pk, eig, eig_ppd, rank, nranks, role, phik, field, field_d, out);
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
