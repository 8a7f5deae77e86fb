// zd_sweep.h — the walk over the modes a plan realises, without transform or store, shared by the band-power sweep
// (zd_kernels_pk.hip), the site sums (zd_kernels_ds.hip) and the sums of the LPT plans (zd_kernels_lpt_ds.hip).  Moved out of
// k_pk_sweep unchanged; what a sweep does with a mode is the functor it hands to sweep_modes.
//
// One thread owns one x and walks the z indices [z0, z1) of the half-space row ky with ONE RNG state (the z-major walk of k_gen at
// stream factor 1).  FAST = the table arithmetic of k_genf (zd_genmath.h: ln / exp / sincos / sqrt and P(k) from the LDS image T,
// waves of zeroed modes only move the RNG) for the rows ky >= 1; the general form = the per-mode arithmetic of k_gen, position by
// position (ky = 0 with the conjugate "loser" rule of zeldovich.cpp:485-503, ZD_f_NL, the one-mode filter, splines too large for
// the LDS image).  every_mode (general form only): the zero rule is not applied — what k_gen does on a ZD_f_NL plan, whose second pass
// forms D = PhiK M for every mode but k = 0 (zeldovich.cpp:393-400).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "zd_genmath.h"

struct zd_plan;

namespace zdsweep {
using zd::GenConst;
using zdpcg::u128;

constexpr int SW_NBIT = 34;  // the first mode of a thread lies < 2^33 + 1 draws into its row

struct SweepJumps {
    zdpcg::Affine bit[SW_NBIT];  // 2^i draws
    // z -> z + 1 with the state one draw ahead and two draws consumed (2 * 65536 * rows - 1 draws); index 1: the step crosses the
    // z = N/2 wrap of the counter (rows N/2 + 1 .. live at 65536 - N + z, zeldovich.cpp:335); _full: no draw consumed
    zdpcg::Affine next[2], next_full[2];
};

// Site sums (zd_kernels_ds.hip, zd_kernels_lpt_ds.hip): what the two sweeps over sample sites share
constexpr int DS_BX = 256;        // threads (consecutive x) per workgroup; a thread walks every z of its row
constexpr int DS_NS = 8;          // sites per launch
constexpr int DS_RESEED = 32;     // FAST rows: z steps between two table look-ups of a site's phase
constexpr int DS_MAX_SITES = 64;

template <int NS>
struct DsSites {
    int z[NS], y[NS], x[NS];
    double wr[NS], wi[NS];  // e^{2 pi i z_s / N}: the rotation of the site's phase per z step
};

// the sites of launch group grp of a call; a short last group sums its first site again (those sums are dropped)
DsSites<DS_NS> make_ds_sites(int N, int64_t nsites, const int64_t *sites_zyx, int grp);
// out[o] = sum of partial[i * nv + o] over the nwg partials of a launch group, o < nv, in an order that depends on nothing but nwg
int launch_ds_reduce(const double *partial, long long nwg, int nv, double *out, hipStream_t st);
// k_ds_sweep over this rank's rows of a plan's GenConst for sites already checked, with the ZA velocity factor vnorm, into
// out7[nsites][7]: what zd_plan_direct_sum does once it has accepted the plan, and the first order of zd_plan_lpt_direct_sum
// (a ZD_q2LPT plan's first-order velocity factor is lpt2_alpha; its EpiConst::vnorm is 1)
int ds_sweep_sites(zd_plan *pl, int64_t nsites, const int64_t *sites_zyx, double vnorm, double *out7, hipStream_t st);

inline SweepJumps make_sweep_jumps(int N) {
    SweepJumps J;
    for (int i = 0; i < SW_NBIT; i++) J.bit[i] = zdpcg::jump_map(((u128) 1) << i);
    const u128 row = (u128) 2 * 65536, wrap = (u128) (65536 - N);
    J.next[0]      = zdpcg::jump_map(row - 1);
    J.next[1]      = zdpcg::jump_map(row * (1 + wrap) - 1);
    J.next_full[0] = zdpcg::jump_map(row);
    J.next_full[1] = zdpcg::jump_map(row * (1 + wrap));
    return J;
}

#if defined(__HIPCC__)
__device__ __forceinline__ u128 sweep_advance(const SweepJumps &J, u128 s, uint64_t delta) {
    for (int i = 0; i < SW_NBIT; i++) {
        if ((delta >> i) == 0) break;
        if ((delta >> i) & 1ULL) s = zdpcg::apply(J.bit[i], s);
    }
    return s;
}

// One visited position.  (kx, ky, kz) is the mode that was GENERATED for it: the position's own wavevector, or — cj, losers of
// the plane ky = 0 — its mirror image, whose conjugate the position holds.  FAST visits every position of a wave that has a live
// one and marks the zeroed ones (live = false, dr = di = 0 exactly); the general form visits live positions only.
struct SweepMode {
    int z;           // the position's z index
    int kx, kz, k2i; // generated mode (signed), kx^2 + ky^2 + kz^2
    bool cj, live;
    double P, ik2;   // PowerSpectrum::power(|k|), 1 / |k|^2 (physical units)
    double dr, di;   // D(k) of the generated mode
};

template <bool PLAW, bool FAST, class F>
__device__ __forceinline__ void sweep_modes(const GenConst &g, const SweepJumps &J, const double *T, int ky, int lG, int x, bool act, int z0,
                                            int z1, bool every_mode, F &&visit) {
    using namespace zdgen;
    const int N = g.N, half = g.half;
    const int kx = x > half ? x - N : x;
    u128 s = 0;
    if (ky != 0 && act && !g.phik) {  // state one step ahead of the first mode's counter
        const int kz0 = z0 > half ? z0 - N : z0;
        s = sweep_advance(J, g.row_state[ky], 2ULL * ((uint64_t) (kz0 & 65535) * 65536ULL + (uint64_t) (kx & 65535)) + 1ULL);
    }
    if constexpr (FAST) {  // rows ky >= 1, the arithmetic of genf_tile
        const int kxy2  = kx * kx + ky * ky;
        const bool dead = !act || (kx < 0 ? -kx : kx) == g.kmax || ky == g.kmax;  // zeldovich.cpp:350
#pragma unroll 1
        for (int z = z0; z < z1; z++) {
            const int kz  = z > half ? z - N : z;
            const int k2i = kxy2 + kz * kz;
            const bool live = !dead && (kz < 0 ? -kz : kz) != g.kmax && (g.corner_modes || k2i < g.k2i_cut);
            const int sel   = z == half;
            if (!__any(live)) {  // all 64 modes zeroed: only the walk moves on
                s = zdpcg::apply(J.next_full[sel], s);
                continue;
            }
            const uint64_t r1 = zdpcg::output(s);
            const u128 s2     = zdpcg::step(s);
            const uint64_t r2 = zdpcg::output(s2);
            s = zdpcg::apply(J.next[sel], s2);
            // ---- cgauss<2> (power_spectrum.cpp:338-359) as in genf_tile ----
            const double k2v = (double) k2i * g.fundamental2;
            const double P   = genf_power<PLAW>(g, T, k2v);
            const double ik2 = frcp(k2v);
            const uint64_t m1 = r1 + 1ULL;
            double v = P;
            if (!g.fixed_power) v = -P * flog(u64_to_double(m1), 64, T);
            v = (m1 == 0 && !g.fixed_power) || !live ? 0.0 : v;
            const double amp = sqrt_pos(v);
            double sn, cs;
            sincos_u01(u64_to_double(r2 + 1ULL), T, sn, cs);
            visit(SweepMode{z, kx, kz, k2i, false, live, P, ik2, amp * cs, amp * sn});
        }
    } else {  // the arithmetic of k_gen, position by position
#pragma unroll 1
        for (int z = z0; z < z1 && act; z++) {
            int zs = z, xs = x;
            bool cj = false, zero = false;
            uint64_t r1 = 0, r2 = 0;
            if (ky != 0) {
                if (!g.phik) {
                    r1 = zdpcg::output(s);
                    const u128 s2 = zdpcg::step(s);
                    r2 = zdpcg::output(s2);
                    s  = zdpcg::apply(J.next[z == half], s2);
                }
            } else {  // "loser" positions take the conjugate of the winner's mode (zeldovich.cpp:485-503)
                if (z > half) {
                    zs = N - z;
                    xs = x ? N - x : 0;
                    cj = true;
                } else if (z == 0) {
                    if (x == 0)
                        zero = true;
                    else if (x > half) {
                        xs = N - x;
                        cj = true;
                    }
                }
            }
            const int kxm = xs > half ? xs - N : xs, kzm = zs > half ? zs - N : zs;  // generated mode
            const int k2i = kxm * kxm + ky * ky + kzm * kzm;
            const double k2v = (double) k2i * g.fundamental2;
            if (zero || k2i == 0 || (!every_mode && zd::mode_is_zero(g, kxm, ky, kzm, k2v))) continue;
            double P, ik2;
            if (g.pk_tab && !every_mode) {  // {P(k), 1/k^2} by integer k^2; the table ends where the zero rule does
                const double2 pv = g.pk_tab[k2i];
                P   = pv.x;
                ik2 = pv.y;
            } else {
                P   = pk_power<PLAW>(g, k2v);
                ik2 = 1.0 / k2v;
            }
            double dr, di;
            if (g.phik) {  // f_NL: D = phi_NG(k) M(k) (zeldovich.cpp:393-400); PhiK rows are this rank's row slots
                const zdfft::cplx ph = g.phik[((long long) (ky >> lG) * N + zs) * N + xs];
                const double M = g.fnl_M[k2i];
                dr = ph.x * M;
                di = ph.y * M;
            } else {
                if (ky == 0) {
                    const u128 t = sweep_advance(J, g.row_state[0], 2ULL * ((uint64_t) (kzm & 65535) * 65536ULL + (uint64_t) (kxm & 65535)) + 1ULL);
                    r1 = zdpcg::output(t);
                    r2 = zdpcg::output(zdpcg::step(t));
                }
                gauss_from_pk(g, P, r1, r2, dr, di);
            }
            visit(SweepMode{z, kxm, kzm, k2i, cj, true, P, ik2, dr, di});
        }
    }
}
#endif

}  // namespace zdsweep
