// zd_tables.h — one predicate per dispatch table: "is there a kernel for this key".  Each runs the launcher itself under a
// TableProbe (zd_launch.h): the launcher's own case list and the run-time refusals of the instantiation answer, nothing is launched
// and no HIP call is made.  zd::route (zd_route.h) asks them for every stage of a job it would otherwise accept.  Host only.
#pragma once
#include "zd_device.h"
#include "zd_launch.h"

namespace zd {

// ---- the power-of-two engine (zd_kernels.hip) ----
// z lines of the reference's / packed arrays (k_zfft)
inline bool has_zfft(int L) {
    TableProbe probe;
    const JobList jobs{};
    const StoreLayout S{};
    return launch_zfft(L, jobs, S, 0, 0, 1, 1, nullptr, nullptr, nullptr, nullptr) == 0;
}
// z lines of the field stores (k_zfft_f): slabs of nky rows, whole row blocks
inline bool has_zfft_fields(int L, int nky) {
    TableProbe probe;
    const FieldLayout F{};
    const StoreLayout S{};
    return launch_zfft_fields(L, F, S, 0, 0, nky, nullptr, nullptr, nullptr, nullptr) == 0;
}
// y columns of the arrays (k_yfft); lq: plane-interleaved rows of the fused Z stage, which need the single-rank store and whole plane groups
inline bool has_yfft(int N, int lq, int one_block, int nplanes) {
    TableProbe probe;
    StoreLayout S{};
    S.N         = N;
    S.lq        = lq;
    S.one_block = one_block;
    S.pitch     = (N + (lq ? (N >= 512 ? 12 : 0) : (N >= 512 ? 24 : 0))) << lq;  // (the row pad of plan_block_layout)
    return launch_yfft(S, nplanes, nullptr, nullptr, nullptr) == 0;
}
// y stage of the field stores (k_yfft_f): the row-block table of Hq row slots sits in LDS beside the transform
inline bool has_yfft_fields(int N, int Hq) {
    TableProbe probe;
    const FieldLayout F{};
    StoreLayout S{};
    S.N  = N;
    S.Hq = Hq;
    return launch_yfft_fields(F, S, nullptr, nullptr, 0, 1, 0, nullptr, nullptr) == 0;
}
// x lines + epilogue (k_xfft and its one-row forms); pack as the epilogue sees it (EpiConst::pack)
inline bool has_xfft(int N, int narray, int pack, int lq, int one_block) {
    TableProbe probe;
    StoreLayout S{};
    S.N         = N;
    S.narray    = narray;
    S.lq        = lq;
    S.one_block = one_block;
    S.paired    = pack == PACK_ZAFIELD && narray == 3 ? ring_pair_w(N) : 0;  // (the ring of the ZA potentials, as plan_store lays it out)
    EpiConst ec{};
    ec.N      = N;
    ec.narray = narray;
    ec.pack   = pack;
    return launch_xfft(S, ec, nullptr, nullptr, 0, 1, 0, 1, nullptr, nullptr, nullptr, nullptr) == 0;
}
// the f_NL phi round's x / y / z kernels (one table), also the forward chains of the second- and third-order rounds
inline bool has_fnl_stage(int N) {
    TableProbe probe;
    StoreLayout S{};
    S.N = N;
    return launch_fnl_stage(0, S, 0., nullptr, nullptr, nullptr, 1, 0, nullptr) == 0;
}
// ---- the second- and third-order rounds (zd_kernels_lpt2.hip, _lpt2q.hip, _lpt3.hip) ----
inline bool has_lpt2_xsrc(int N) {
    TableProbe probe;
    StoreLayout S{};
    S.N      = N;
    S.narray = 1;
    return launch_lpt2_xsrc(S, 1, nullptr, nullptr, nullptr, 1, nullptr) == 0;
}
inline bool has_lpt2q_xsrc(int M) {
    TableProbe probe;
    return launch_lpt2q_xsrc(M, nullptr, 1, nullptr, M, 1, nullptr, nullptr) == 0;
}
inline bool has_lpt2q_zsrc(int M, int N) {
    TableProbe probe;
    return launch_lpt2q_zsrc(M, N, nullptr, nullptr, M, nullptr, nullptr) == 0;
}
inline bool has_lpt3_xpair(int N) {
    TableProbe probe;
    StoreLayout S{};
    S.N      = N;
    S.narray = 1;
    return launch_lpt3_xpair(S, nullptr, nullptr, nullptr, nullptr, 1, nullptr) == 0;
}
inline bool has_lpt3_xfwd(int N) {
    TableProbe probe;
    StoreLayout S{};
    S.N      = N;
    S.narray = 1;
    return launch_lpt3_xfwd(S, nullptr, nullptr, nullptr, 1, nullptr) == 0;
}
// ---- the composite-transform kernels of the field stores (zd_kernels_np2.hip) ----
inline bool has_zfft_fields_np2(int L, int nky) {
    TableProbe probe;
    const FieldLayout F{};
    const StoreLayout S{};
    return launch_zfft_fields_np2(L, F, S, 0, 0, nky, nullptr, nullptr, nullptr, nullptr) == 0;
}
inline bool has_yfft_fields_np2(int N) {
    TableProbe probe;
    const FieldLayout F{};
    StoreLayout S{};
    S.N = N;
    return launch_yfft_fields_np2(F, S, nullptr, nullptr, 0, 1, 0, nullptr, 0, nullptr) == 0;
}
inline bool has_xfft_np2(int N, int pack) {
    TableProbe probe;
    EpiConst ec{};
    ec.N    = N;
    ec.pack = pack;
    return launch_xfft_np2(N, ec, nullptr, nullptr, 0, 1, 0, 1, nullptr, nullptr, nullptr) == 0;
}
inline bool has_xdens_np2(int N) {
    TableProbe probe;
    return launch_xdens_np2(N, nullptr, nullptr, 0, 1, nullptr, nullptr) == 0;
}
// ---- composite transforms of the reference's arrays (zd_kernels_np2_ref.hip) ----
inline bool has_refq_cols(int n) {
    TableProbe probe;
    return launch_refq_cols(n, nullptr, nullptr, 0, 0, 1, 1, -1, nullptr) == 0;
}
inline bool has_refq_cols_oop(int n) {
    TableProbe probe;
    return launch_refq_cols_oop(n, nullptr, nullptr, 0, 0, nullptr, 0, 0, 1, 1, false, nullptr) == 0;
}
inline bool has_refq_lines(int n) {
    TableProbe probe;
    return launch_refq_lines(n, nullptr, nullptr, n, 1, nullptr) == 0;
}
inline bool has_refq_yphi(int n) {
    TableProbe probe;
    return launch_refq_yphi(n, nullptr, nullptr, n, 1, 0., nullptr) == 0;
}
inline bool has_refq_ycols(int n) {
    TableProbe probe;
    AnyChunks C{};
    C.N = n;
    return launch_refq_ycols(n, nullptr, C, nullptr, 1, 1, -1, n, nullptr) == 0;
}
inline bool has_refq_xphi(int n) {
    TableProbe probe;
    return launch_refq_xphi(n, nullptr, nullptr, n, 1, 0., nullptr) == 0;
}
// ---- lines as convolutions on the power-of-two engine (zd_kernels_any.hip): the engine of a line of n points ----
inline bool has_any_cols(int n) {
    TableProbe probe;
    AnyTab tb{};
    tb.M = any_engine_size(n);
    return launch_any_cols(tb, nullptr, 0, 0, 1, 1, -1, nullptr) == 0;
}
inline bool has_any_lines(int n) {
    TableProbe probe;
    AnyTab tb{};
    tb.M = any_engine_size(n);
    return launch_any_lines(tb, nullptr, n, 1, nullptr) == 0;
}

}  // namespace zd
