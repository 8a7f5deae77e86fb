// zd_launch.h — host-callable launchers implemented in zd_kernels.hip
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include "zd_device.h"

// Dispatch diagnostics (zd_dispatch_report, include/zeldovich_hip.h): every launch site counts its launches under the name of
// the launcher instantiation it sits in (template arguments included) — which kernel variant a configuration really took.
// One relaxed atomic increment per launch; a site registers itself in a lock-free list the first time it is reached.
#include <atomic>
namespace zd {
struct DispatchSite {
    const char *func;
    int line;
    std::atomic<long long> count{0};
    DispatchSite *next = nullptr;
    DispatchSite(const char *f, int l);
};
}  // namespace zd

#define ZD_LAUNCH_CHECK()                                                                       \
    do {                                                                                        \
        static zd::DispatchSite site__(__PRETTY_FUNCTION__, __LINE__);                          \
        site__.count.fetch_add(1, std::memory_order_relaxed);                                   \
        hipError_t e__ = hipGetLastError();                                                     \
        if (e__ != hipSuccess) {                                                                \
            fprintf(stderr, "zeldovich_hip: launch failed at %s:%d: %s\n", __FILE__, __LINE__,  \
                    hipGetErrorString(e__));                                                    \
            return 1;                                                                           \
        }                                                                                       \
    } while (0)

// Table probes (zd_tables.h): while a TableProbe is alive on the calling thread, a launcher runs its own dispatch — the case list and
// the run-time refusals inside the instantiation (threads, LDS, row blocks, plane groups) — and returns 0 where it would launch,
// before any HIP call; a key without a case returns non-zero without a message.  So "is there a kernel for this key" is answered by
// the launcher's own code, not by a second list of sizes.  ZD_PROBE_RETURN() stands in every instantiation behind its refusals
// and in front of set_dyn_lds; ZD_TABLE_MISS is the message of a launcher that found no case.
namespace zd {
extern thread_local int table_probe_depth;
struct TableProbe {
    TableProbe() { table_probe_depth++; }
    ~TableProbe() { table_probe_depth--; }
    TableProbe(const TableProbe &) = delete;
    TableProbe &operator=(const TableProbe &) = delete;
};
inline bool table_probe() { return table_probe_depth > 0; }
}  // namespace zd
#define ZD_PROBE_RETURN() \
    do {                  \
        if (zd::table_probe()) return 0; \
    } while (0)
#define ZD_TABLE_MISS(...)                                    \
    do {                                                      \
        if (!zd::table_probe()) fprintf(stderr, __VA_ARGS__); \
    } while (0)

// hipFuncAttributeMaxDynamicSharedMemorySize belongs to (kernel, device): ZD_NumGPU runs one host thread per device through
// the same launchers, so what has been set is kept per device — a process-wide flag would leave
// every device but the first with the 64 KB default and the launches of the large-LDS kernels would fail there.
#if defined(__HIPCC__)
#include <atomic>
template <auto Kernel>
static inline void set_dyn_lds(size_t bytes) {
    // largest size set so far per device: a kernel whose dynamic LDS depends on run-time arguments gets the attribute raised when
    // a later launch needs more than the first one did
    static std::atomic<size_t> have[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    std::atomic<size_t> &h = have[dev & 63];
    if (bytes == 0 || h.load(std::memory_order_acquire) >= bytes) return;
    hipFuncSetAttribute((const void *) Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) bytes);
    size_t cur = h.load(std::memory_order_relaxed);
    while (cur < bytes && !h.compare_exchange_weak(cur, bytes, std::memory_order_release, std::memory_order_relaxed)) {
    }
}
#endif

namespace zd {
constexpr int GEN_BX = 256;  // threads (consecutive x) per generator workgroup
constexpr int GEN_ZR = 16;   // z rows walked by one generator thread

// tile_ctr: zeroed device counter for this launch (k_genf pulls its tiles from it; NULL -> general kernel only);
// max_wgs: size of k_genf's persistent grid
// residue2: second z-residue of the pass (PACK_ZAPAIR only)
int launch_gen(const GenConst &g, const GenJumps &J, const JobList &jobs, const StoreLayout &S, int ky0, int nky, int L,
               int residue, int residue2, const void *twN, void *Y, unsigned *tile_ctr, int max_wgs, hipStream_t st);
int launch_pk_table(const GenConst &g, int n, void *tab, hipStream_t st);
int launch_eig_lines(const GenConst &g, int ky0, int ky_stride, int nrows, void *lines, hipStream_t st);
int launch_test_modes(const GenConst &g, long long n, const int *kxyz, uint64_t *draws, double *D, hipStream_t st);
int launch_test_modes_table(const GenConst &g, long long n, const int *kxyz, double *out, hipStream_t st);
int launch_zfft(int L, const JobList &jobs, const StoreLayout &S, int ky0, int kyloc0, int nky, int Zq, const void *Y,
                const void *twL, void *out, hipStream_t st);
int zfft_tile_width(int L);
int zfft_fields_tile_columns(int L);
int launch_zfft_fields(int L, const FieldLayout &F, const StoreLayout &S, int ky0, int kyloc0, int nky, const void *Y,
                       const void *twL, void *out, hipStream_t st);
int launch_yfft_fields(const FieldLayout &F, const StoreLayout &S, const void *tw, const void *store, int plane0,
                       int nplanes, int ring_pitch, void *ring, hipStream_t st);
int launch_yfft(const StoreLayout &S, int nplanes, const void *tw, void *data, hipStream_t st);
int launch_xfft(const StoreLayout &S, const EpiConst &ec, const void *tw, const void *data, int plane0, int nplanes,
                int z_first, int z_step, void *records, float *density, Reduce *red, hipStream_t st);
int launch_yfft_variant(int variant, const StoreLayout &S, int nplanes, const void *tw, void *data, hipStream_t st);
int launch_fnl_table(const GenConst &g, int n, void *tab, hipStream_t st);
int launch_fnl_stage(int which, const StoreLayout &S, double f_NL, const void *tw, void *data, void *phik, int nplanes, int lZq,
                     hipStream_t st);
int launch_test_fft(int n, int kind, const void *tw, const void *in, void *out, long long lines, hipStream_t st);
int test_fft_tile_width(int n);
// ---- fused generator + z FFT of the packed PLT store (zd_kernels_fz.hip) ----
bool genz_plt_supported(int N, int L);
int launch_genz_plt(const GenConst &g, const StoreLayout &S, int ky0, int L, int residue, unsigned nitems, const FzItem *items,
                    const void *twN, const void *twL, void *out, unsigned *ctr, int ncu, hipStream_t st);
// ---- PPD = 2^a 3^b (zd_kernels_np2.hip) ----
bool np2_split(int n, int *P, int *Q);
int test_fftq_tile_width(int n);
bool np2_supported_ppd(int N);
bool np2_supported_zlen(int L);
int zfft_fields_np2_columns(int L);
int launch_zfft_fields_np2(int L, const FieldLayout &F, const StoreLayout &S, int ky0, int kyloc0, int nky, const void *Y,
                           const void *tw, void *out, hipStream_t st);
int launch_yfft_fields_np2(const FieldLayout &F, const StoreLayout &S, const void *tw, const void *store, int plane0, int nplanes,
                           int ring_pitch, void *ring, int dens, hipStream_t st);
int launch_xdens_np2(int N, const void *tw, const void *dring, int ring_pitch, int nplanes, float *density, hipStream_t st);
int launch_xfft_np2(int N, const EpiConst &ec, const void *tw, const void *ring, int ring_pitch, int nplanes, int z_first, int z_step,
                    void *records, Reduce *red, hipStream_t st);
int launch_test_fftq(int n, int kind, const void *twP, const void *twN, const void *twQ, const void *in, void *out, long long lines,
                     hipStream_t st);
// ---- any even PPD (zd_kernels_any.hip) ----
int any_engine_size(int n);
int launch_any_cols(const AnyTab &tb, void *data, long long batch_stride, long long point_stride, int ncols, int nbatch, int zero_point,
                    hipStream_t st);
int launch_any_lines(const AnyTab &tb, void *data, long long pitch, long long nlines, hipStream_t st);
int launch_any_scatter(const JobList &jobs, const AnyLayout &A, int ky0, int nky, int L, const void *Y, void *store, hipStream_t st);
int launch_any_emit(const AnyLayout &A, const EpiConst &ec, const void *store, int plane0, int nplanes, int z_first, int z_step, void *records,
                    float *density, Reduce *red, hipStream_t st);
int launch_any_phi_nl(const AnyLayout &A, double f_NL, void *store, hipStream_t st);
int launch_any_phik(const AnyLayout &A, const void *store, void *phik, hipStream_t st);
// ---- composite-length transforms of the reference's arrays (zd_kernels_np2_ref.hip): ZD_f_NL on the composite grids ----
// tw: exp(2 pi i k / P) | exp(2 pi i k / n) | exp(2 pi i k / Q) for n = P * Q (zd_fft_q.h); the arguments of launch_any_cols / _lines
bool refq_supported_len(int n);
int launch_refq_cols(int n, const void *tw, void *data, long long batch_stride, long long point_stride, int ncols, int nbatch, int zero_point,
                     hipStream_t st);
int launch_refq_lines(int n, const void *tw, void *data, long long pitch, long long nlines, hipStream_t st);
int launch_refq_cols_oop(int n, const void *tw, const void *in, long long in_bs, long long in_ps, void *out, long long out_bs, long long out_ps,
                         int ncols, int nbatch, bool conj, hipStream_t st);
// ZD_f_NL phi round, half-space planes [z][ky < n/2][x] of pitch `pitch`: y inverse, phi + f_NL phi^2, y again (k_refq_yphi)
int launch_refq_yphi(int n, const void *tw, void *store, long long pitch, int nplanes, double f_NL, hipStream_t st);
// several ranks (AnyChunks store): z lines into the send store, y columns over the chunks (point ky = zero_point read as zero, outputs
// k >= out_limit not written), the phi round's x lines (inverse, phi + f_NL phi^2, again), the particle epilogue
int launch_refq_scatter(const JobList &jobs, const AnyChunks &C, int ky_first, int r0, int nky, int L, const void *Y, void *store, hipStream_t st);
int launch_refq_ycols(int n, const void *tw, const AnyChunks &C, void *data, int ncols, int nbatch, int zero_point, int out_limit,
                      hipStream_t st);
int launch_refq_xphi(int n, const void *tw, void *data, long long pitch, long long nlines, double f_NL, hipStream_t st);
int launch_refq_emit(const AnyChunks &C, const EpiConst &ec, const void *store, int plane0, int nplanes, int z_first, int z_step, void *records,
                     float *density, Reduce *red, hipStream_t st);
// ---- second-order displacements (zd_kernels_lpt2.hip) ----
// the generator of a plan with GenConst::lpt2 != 0 (launch_gen hands such plans over): gradient pairs or the final pass
int launch_gen_lpt2(const GenConst &g, const GenJumps &J, const JobList &jobs, const StoreLayout &S, int ky0, int nky, int L, int residue,
                    const void *twN, void *Y, hipStream_t st);
// x lines of the planes [0, nplanes) of a one-array store in gradient pass `pass` (1 .. 4): inverse transform, the pass's term of
// the source into acc[z][y][x] (N^3 doubles); pass 4 goes on to acc / N^3 and the forward x transform, in place
int launch_lpt2_xsrc(const StoreLayout &S, int pass, const void *tw, void *data, double *acc, int nplanes, hipStream_t st);
// ---- second order on a caller-supplied field (zd_kernels_lpt2_field.hip) ----
// the generator of a second-order plan that carries field modes (GenConst::lpt2 != 0 and GenConst::phik = D(k); launch_gen hands such
// plans over): launch_gen_lpt2's jobs with D loaded from phik instead of drawn
int launch_gen_lpt2_field(const GenConst &g, const JobList &jobs, const StoreLayout &S, int ky0, int nky, int L, int residue, const void *twN,
                          void *Y, hipStream_t st);
// ---- the de-aliased second-order round on the lattice of m = 3 n / 2 points per side (zd_kernels_lpt2q.hip); tw as for launch_refq_* ----
// x lines l < nlines at data[l * pitch] in gradient pass `pass` (1 .. 4): launch_lpt2_xsrc's contract with acc[l * m + x] (m^3 doubles)
int launch_lpt2q_xsrc(int m, const void *tw, int pass, void *data, long long pitch, long long nlines, double *acc, hipStream_t st);
// the last z lines of the store [z][y][x] (row pitch `pitch`): columns |kx| < n/2, rows 0 <= ky < n/2, outputs |kz| < n/2, conjugated,
// into sk[ky][kz][x] of the n layout (zeros on its Nyquist planes)
int launch_lpt2q_zsrc(int m, int n, const void *tw, const void *store, long long pitch, void *sk, hipStream_t st);
// ---- third-order displacements (zd_kernels_lpt3.hip) ----
// the generator of a plan with GenConst::lpt3 != 0 (launch_gen hands such plans over): Hessian pairs or the final pass
int launch_gen_lpt3(const GenConst &g, const GenJumps &J, const JobList &jobs, const StoreLayout &S, int ky0, int nky, int L, int residue,
                    const void *twN, void *Y, hipStream_t st);
// x lines of the planes [0, nplanes) of a one-array store in a pair pass: inverse transform, Re -> td[z][y][x], Im -> ts[z][y][x]
int launch_lpt3_xpair(const StoreLayout &S, const void *tw, const void *data, double *td, double *ts, int nplanes, hipStream_t st);
// the sources of the third order at `nsites` lattice sites, written over F.d[0 .. 3]: g3a S3a + g3b S3b, C_x, C_y, C_z
int launch_lpt3_point(const Lpt3Fields &F, double g3a, double g3b, long long nsites, hipStream_t st);
// rows of the real field src[z][y][x] / N^3 through the forward x transform into the one-array store (launch_fnl_stage 1, 2 go on)
int launch_lpt3_xfwd(const StoreLayout &S, const void *tw, const double *src, void *data, int nplanes, hipStream_t st);
// ---- intake of a caller-supplied real field (zd_kernels_field.hip): a[z][y][x] -> PhiK[ky < N/2][kz][x] ----
// rows of the planes [0, nplanes) of src (float32 or float64, [plane][y][x]) through the x lines into work[plane][y][x] (complex)
int launch_field_x(int N, const void *src, int is_f32, const void *tw, void *work, int nplanes, hipStream_t st);
// y lines of those planes; the outputs ky < N/2 into phik[ky][z0 + plane][x]
int launch_field_y(int N, const void *tw, const void *work, int z0, int nplanes, void *phik, hipStream_t st);
// z lines of phik in place; the store conjugates, applies the zero rule of g and multiplies by amp[kx^2 + ky^2 + kz^2]
int launch_field_z(const GenConst &g, const void *tw, const double *amp, void *phik, hipStream_t st);
// ---- adjoint of a field run (zd_kernels_field_adj.hip): cotangents -> H[ky < N/2][kz][x] -> abar[z][y][x] ----
// rows of the planes [0, nplanes) of the cotangents a, b (b may be NULL; float32 or float64, [plane][y][x][nc]), component comp:
// fa a + fb b through the x lines into work[plane][y][x]; launch_field_y then takes the columns into T[ky][z][x]
int launch_field_adj_x(int N, const void *a, const void *b, double fa, double fb, int is_f32, int nc, int comp, const void *tw, void *work,
                       int nplanes, hipStream_t st);
// z lines of T; the store conjugates and puts this pass's term into H (first != 0: written, otherwise added): coef 0 = alive A conj(i s_comp),
// 1 = the same times f (PLT velocities), 2 = alive A (density)
int launch_field_adj_z(const GenConst &g, const void *tw, const double *amp, const void *T, void *H, int comp, int coef, int first, hipStream_t st);
// the inverse: z lines of H in place (weight 1 on ky = 0, 2 on the other rows), columns of the planes [z0, z0 + nplanes) into
// work[plane][y][x], rows of the workspace with the real part into out[plane][y][x]
int launch_field_adj_iz(int N, const void *tw, void *H, hipStream_t st);
int launch_field_adj_iy(int N, const void *tw, const void *H, int z0, int nplanes, void *work, hipStream_t st);
int launch_field_adj_ix(int N, const void *tw, const void *work, double *out, int nplanes, hipStream_t st);
// ---- ZD_Version = 1 streams (zd_kernels_v1.hip) ----
int launch_v1_seed(unsigned long long seed, int block, V1Stream *streams, hipStream_t st);
int launch_v1_draw(const GenConst &g, int block, int ky0, int ky_stride, int nrows, V1Stream *streams, void *dev, int *err,
                   hipStream_t st);
int launch_test_v1_words(V1Stream *streams, int nblocks, uint32_t *out, hipStream_t st);
int launch_copy16(const void *in, void *out, long long n16, hipStream_t st);
}  // namespace zd

extern "C" int zdk_upload_bit_table(const zdpcg::BitTable *host);
extern "C" int zdk_upload_bit_table_fz(const zdpcg::BitTable *host);
extern "C" int zdk_upload_bit_table_lpt2(const zdpcg::BitTable *host);
extern "C" int zdk_upload_bit_table_lpt3(const zdpcg::BitTable *host);
