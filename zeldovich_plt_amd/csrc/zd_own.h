// zd_own.h — move-only owners of the HIP resources of the host layer (zd_capi*.cpp, zd_multi.cpp, the host launchers of
// zd_kernels_pk.hip / zd_kernels_ds.hip): device and pinned buffers, events, streams, plans.  A handle converts to the raw
// pointer / handle it owns, so launch call sites read as before; the structs passed to kernels keep raw pointers (.get()).
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <vector>
#ifdef ZD_TESTING
#include <atomic>
#endif

struct zd_plan;
extern "C" void zd_plan_destroy(zd_plan *pl);
hipError_t zd_store_alloc(void **p, size_t bytes);  // zd_capi_diag.cpp: hipMalloc, NaN-filled under zd_test_poison

namespace zdown {

// live handles + plans, counted in the -DZD_TESTING library only (zd_test_live_handles); the product carries no counter
#ifdef ZD_TESTING
inline std::atomic<long long> g_live{0};
inline void live(int d) { g_live.fetch_add(d, std::memory_order_relaxed); }
#else
inline void live(int) {}
#endif

struct DevFree    { void operator()(void *p) const { hipFree(p); } };
struct HostFree   { void operator()(void *p) const { hipHostFree(p); } };
struct EventFree  { void operator()(hipEvent_t e) const { hipEventDestroy(e); } };
struct StreamFree { void operator()(hipStream_t s) const { hipStreamDestroy(s); } };

template <class H, class Free>
class Owned {
    H h_ = H{};

public:
    Owned() = default;
    Owned(Owned &&o) noexcept { reset(o.release()); }
    Owned &operator=(Owned &&o) noexcept { return reset(o.release()), *this; }
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    ~Owned() { reset(); }
    H get() const { return h_; }
    operator H() const { return h_; }
    H release() {
        H h = h_;
        h_  = H{};
        if (h) live(-1);
        return h;
    }
    void reset(H h = H{}) {  // frees what it owns, adopts h
        if (h_) Free{}(h_), live(-1);
        if ((h_ = h)) live(+1);
    }
};

template <class T> inline constexpr size_t elem_size = sizeof(T);
template <> inline constexpr size_t elem_size<void> = 1;

template <class T, class Free, hipError_t (*Alloc)(void **, size_t)>
struct Buf : Owned<T *, Free> {
    hipError_t alloc(size_t n) { return alloc_by(Alloc, n); }
    hipError_t store_alloc(size_t n) { return alloc_by(zd_store_alloc, n); }  // (device buffers)
    hipError_t alloc_by(hipError_t (*f)(void **, size_t), size_t n) {
        void *p            = nullptr;
        const hipError_t e = f(&p, n * elem_size<T>);
        this->reset(e == hipSuccess ? (T *) p : nullptr);
        return e;
    }
};
inline hipError_t dev_malloc(void **p, size_t nb) { return hipMalloc(p, nb); }
inline hipError_t host_malloc(void **p, size_t nb) { return hipHostMalloc(p, nb); }
template <class T> using DevBuf    = Buf<T, DevFree, dev_malloc>;
template <class T> using PinnedBuf = Buf<T, HostFree, host_malloc>;

struct Event : Owned<hipEvent_t, EventFree> {
    hipError_t create(unsigned flags = hipEventDefault) {
        hipEvent_t e       = nullptr;
        const hipError_t r = hipEventCreateWithFlags(&e, flags);
        reset(r == hipSuccess ? e : nullptr);
        return r;
    }
};
struct Stream : Owned<hipStream_t, StreamFree> {
    hipError_t create(unsigned flags = hipStreamNonBlocking) {
        hipStream_t s      = nullptr;
        const hipError_t r = hipStreamCreateWithFlags(&s, flags);
        reset(r == hipSuccess ? s : nullptr);
        return r;
    }
};

struct PlanFree { void operator()(zd_plan *pl) const { zd_plan_destroy(pl); } };
using PlanPtr = std::unique_ptr<zd_plan, PlanFree>;

// allocate-and-copy of a host table
template <class T> hipError_t upload(DevBuf<T> &b, const T *src, size_t n) {
    const hipError_t e = b.alloc(n);
    return e != hipSuccess ? e : hipMemcpy(b.get(), src, n * sizeof(T), hipMemcpyHostToDevice);
}
template <class T> hipError_t upload(DevBuf<T> &b, const std::vector<T> &v) { return upload(b, v.data(), v.size()); }

}  // namespace zdown
