// zd_multi.cpp — the N > 1 data path inside the library: one rank per GPU, the block exchange between the Z stage and
// the XY stage (the reference's StoreBlock / LoadBlock "transpose", src/block_array.cpp:387-414,466-504, called per
// block from src/zeldovich.cpp:583-587,634-637) pipelined against the XY compute, and a thread-per-GPU driver behind
// zd_generate / `zeldovich <param_file>` (ZD_NumGPU).
//
// Design.  Rank g generates and z-transforms its half-space rows into a SEND store laid out [destination rank d]
// [plane][array|field][row slot][x] (zd_device.h).  Inside a chunk the planes are the outer index, so the planes
// [j0, j1) of chunk d are ONE contiguous range: the exchange is cut into plane groups.  Group j of every peer's chunk
// <me> is received into one of two ring slots ([source rank s][planes of the group]...) on a communication stream while
// the y and x stages of group j-1 run on the compute stream.  No second full-size store exists (round 1 doubled it),
// so on 8 GPUs the stream factor is set by ONE store per rank.  Transports:
//   * RCCL: grouped ncclSend / ncclRecv per plane group (all 7 xGMI links of a GPU busy at once); the communicator
//     comes from ncclCommInitRank (one process per GPU: bench.py under torch.distributed.run) or ncclCommInitAll
//     (one thread per GPU: zd_generate).  librccl is opened lazily so that the library loads on hosts without it.
//   * local: all ranks are threads of this process and PULL their slices with hipMemcpyAsync (peer copies over xGMI when
//     the ranks sit on different GPUs).  It is also what lets the multi-rank pipeline run — with the real kernels — on
//     a one-GPU test box (several ranks share the device).
#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

#include "zd_launch.h"
#include "zd_plan.h"
#ifdef ZD_TESTING
#include "zd_testing.h"  // (default visibility of the test hooks defined here)
#endif

using zdfft::cplx;
using zdown::DevBuf;
using zdown::Event;
using zdown::PinnedBuf;
using zdown::PlanPtr;
using zdown::Stream;

#define MHIP(call)                                                                                  \
    do {                                                                                            \
        hipError_t e__ = (call);                                                                    \
        if (e__ != hipSuccess) {                                                                    \
            fprintf(stderr, "zeldovich_hip: %s failed at %s:%d: %s\n", #call, __FILE__, __LINE__,   \
                    hipGetErrorString(e__));                                                        \
            return 1;                                                                               \
        }                                                                                           \
    } while (0)

namespace {

// ---- lazily bound RCCL entry points --------------------------------------------------------------
struct RcclApi {
    void *h = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *)                                            = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int)                     = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *)                            = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t)                                                = nullptr;
    ncclResult_t (*CommAbort)(ncclComm_t)                                                  = nullptr;
    ncclResult_t (*CommGetAsyncError)(ncclComm_t, ncclResult_t *)                          = nullptr;
    ncclResult_t (*GroupStart)()                                                           = nullptr;
    ncclResult_t (*GroupEnd)()                                                             = nullptr;
    ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t)     = nullptr;
    const char *(*GetErrorString)(ncclResult_t)                                            = nullptr;
};
#ifdef ZD_TESTING
RcclApi *g_rccl_override = nullptr;  // test transport (loopback emulation below): stands in for librccl
#endif
RcclApi *rccl() {
#ifdef ZD_TESTING
    if (g_rccl_override) return g_rccl_override;
#endif
    static RcclApi api;
    static std::once_flag once;
    std::call_once(once, [] {
        // a process that already carries an RCCL (PyTorch ships one) must keep using that copy
        for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            api.h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (api.h) break;
        }
        if (!api.h) return;
#define BIND(f) api.f = reinterpret_cast<decltype(api.f)>(dlsym(api.h, "nccl" #f))
        BIND(GetUniqueId);
        BIND(CommInitRank);
        BIND(CommInitAll);
        BIND(CommDestroy);
        BIND(CommAbort);
        BIND(CommGetAsyncError);
        BIND(GroupStart);
        BIND(GroupEnd);
        BIND(Send);
        BIND(Recv);
        BIND(GetErrorString);
#undef BIND
        if (!api.GetUniqueId || !api.CommInitRank || !api.CommInitAll || !api.GroupStart || !api.GroupEnd || !api.Send || !api.Recv)
            api.h = nullptr;
    });
    return api.h ? &api : nullptr;
}
#define MNCCL(call)                                                                                          \
    do {                                                                                                     \
        ncclResult_t r__ = (call);                                                                           \
        if (r__ != ncclSuccess) {                                                                            \
            fprintf(stderr, "zeldovich_hip: %s failed at %s:%d: %s\n", #call, __FILE__, __LINE__,            \
                    rccl()->GetErrorString ? rccl()->GetErrorString(r__) : "?");                             \
            return 1;                                                                                        \
        }                                                                                                    \
    } while (0)

#ifdef ZD_TESTING
// ---- loopback emulation of the RCCL calls (tests only: zd_test_generate_loopback) --------------------------------------------
// Lets the RCCL branch of the exchange code — buffer offsets, grouped send / receive order, stream and event ordering — run
// with several ranks as threads on ONE GPU, where real RCCL refuses duplicate devices.  Semantics kept: Send / Recv inside a
// group are matched per (source, destination) pair in posting order; data moves on the receiver's stream after the sender's
// stream has reached the send; the sender's stream does not run past the group before its buffers have been read.
struct LoopComm {
    int rank = 0, n = 1;
};
struct LoopMsg {
    const void *ptr;
    size_t nb;
    hipEvent_t ready, done;
    bool has_done;
};
struct LoopState {
    std::mutex mu;
    std::condition_variable cv;
    std::vector<std::vector<LoopMsg>> box;  // box[src * n + dst]: messages in posting order
    std::vector<size_t> taken;              // next message the receiver takes
    int n = 0;
    std::atomic<bool> aborted{false};       // the emulated ncclCommAbort: a rank blocked in loop_group_end comes out with an error
} g_loop;
std::atomic<int> g_test_fail_rank{-1};      // zd_test_fail_rank: this rank of the thread-per-GPU driver fails before its first pass
struct LoopOp {
    bool send;
    void *ptr;
    size_t nb;
    int peer;
    hipStream_t st;
};
thread_local std::vector<LoopOp> t_loop_ops;
thread_local LoopComm *t_loop_comm = nullptr;

ncclResult_t loop_group_start() {
    t_loop_ops.clear();
    return ncclSuccess;
}
ncclResult_t loop_send(const void *p, size_t nb, ncclDataType_t, int peer, ncclComm_t c, hipStream_t st) {
    t_loop_comm = reinterpret_cast<LoopComm *>(c);
    t_loop_ops.push_back(LoopOp{true, const_cast<void *>(p), nb, peer, st});
    return ncclSuccess;
}
ncclResult_t loop_recv(void *p, size_t nb, ncclDataType_t, int peer, ncclComm_t c, hipStream_t st) {
    t_loop_comm = reinterpret_cast<LoopComm *>(c);
    t_loop_ops.push_back(LoopOp{false, p, nb, peer, st});
    return ncclSuccess;
}
ncclResult_t loop_group_end() {
    if (t_loop_ops.empty()) return ncclSuccess;
    const int me = t_loop_comm->rank, n = g_loop.n;
    std::vector<std::pair<int, size_t>> mine;  // (peer, index) of the messages this group posted
    {
        std::lock_guard<std::mutex> lk(g_loop.mu);
        for (const LoopOp &op : t_loop_ops)
            if (op.send) {
                LoopMsg m{op.ptr, op.nb, nullptr, nullptr, false};
                if (hipEventCreateWithFlags(&m.ready, hipEventDisableTiming) != hipSuccess) return ncclInternalError;
                if (hipEventRecord(m.ready, op.st) != hipSuccess) return ncclInternalError;
                auto &q = g_loop.box[(size_t) me * n + op.peer];
                q.push_back(m);
                mine.emplace_back(op.peer, q.size() - 1);
            }
    }
    g_loop.cv.notify_all();
    for (const LoopOp &op : t_loop_ops)
        if (!op.send) {
            std::unique_lock<std::mutex> lk(g_loop.mu);
            const size_t key = (size_t) op.peer * n + me;
            // (bounded: a rank that failed never posts, and a test must not hang the box)
            if (!g_loop.cv.wait_for(lk, std::chrono::seconds(30), [&] { return g_loop.aborted.load() || g_loop.box[key].size() > g_loop.taken[key]; })
                || g_loop.aborted.load())
                return ncclInternalError;
            LoopMsg &m = g_loop.box[key][g_loop.taken[key]++];
            if (m.nb != op.nb) return ncclInvalidArgument;
            if (hipStreamWaitEvent(op.st, m.ready, 0) != hipSuccess) return ncclInternalError;
            if (hipMemcpyAsync(op.ptr, m.ptr, op.nb, hipMemcpyDeviceToDevice, op.st) != hipSuccess) return ncclInternalError;
            if (hipEventCreateWithFlags(&m.done, hipEventDisableTiming) != hipSuccess) return ncclInternalError;
            if (hipEventRecord(m.done, op.st) != hipSuccess) return ncclInternalError;
            m.has_done = true;
            lk.unlock();
            g_loop.cv.notify_all();
        }
    hipStream_t st = t_loop_ops[0].st;
    for (auto &pi : mine) {  // the send buffers may be reused only after the receivers have read them
        std::unique_lock<std::mutex> lk(g_loop.mu);
        const size_t key = (size_t) me * n + pi.first;
        if (!g_loop.cv.wait_for(lk, std::chrono::seconds(30), [&] { return g_loop.aborted.load() || g_loop.box[key][pi.second].has_done; })
            || g_loop.aborted.load())
            return ncclInternalError;
        if (hipStreamWaitEvent(st, g_loop.box[key][pi.second].done, 0) != hipSuccess) return ncclInternalError;
    }
    t_loop_ops.clear();
    return ncclSuccess;
}
// like ncclCommAbort for a blocking communicator: whoever is inside a blocking call of the job comes out with an error
ncclResult_t loop_comm_abort(ncclComm_t) {
    g_loop.aborted.store(true);
    std::lock_guard<std::mutex> lk(g_loop.mu);
    g_loop.cv.notify_all();
    return ncclSuccess;
}
const char *loop_error_string(ncclResult_t) { return "loopback transport"; }
RcclApi g_loop_api;

#endif  // ZD_TESTING

// in-process rendezvous of the local transport
struct LocalGroup {
    int n = 0;
    std::vector<const char *> send_base;  // each rank's send store of the current pass
    std::vector<const char *> ring_base;  // each rank's exchange ring (phi round: the reverse exchange pulls from the peers' slots)
    std::atomic<int> failed{0};
    // barrier that a failed rank can break (a plain pthread barrier would hang the survivors)
    std::mutex mu;
    std::condition_variable cv;
    int waiting = 0;
    long long generation = 0;
    int wait() {  // 0: everybody arrived; 1: some rank failed
        std::unique_lock<std::mutex> lk(mu);
        const long long gen = generation;
        if (++waiting == n) {
            waiting = 0;
            generation++;
            cv.notify_all();
            return failed.load() ? 1 : 0;
        }
        while (generation == gen && !failed.load()) cv.wait_for(lk, std::chrono::milliseconds(50));
        return failed.load() ? 1 : 0;
    }
    void fail() {
        failed.store(1);
        std::lock_guard<std::mutex> lk(mu);
        cv.notify_all();
    }
};

}  // namespace

struct zd_comm {
    int rank = 0, nranks = 1;
    int kind = 0;  // 0 RCCL, 1 local
    ncclComm_t nccl = nullptr;
    // `nccl` against an abort from another thread (thread-per-GPU driver: whichever rank thread fails aborts EVERY communicator of
    // the process).  The mutex is held only to publish / fetch / clear the handle and to count the rank into a block of RCCL host
    // calls (`in_rccl`) — NEVER across the calls themselves: ncclGroupEnd may block (lazy p2p connection set-up waits for the
    // peer), and CommAbort exists to unblock exactly such a call when the peer has failed (round 4 held the mutex across the
    // block: a rank stuck in its first GroupEnd kept the aborter waiting for the lock).  The aborter takes the handle
    // away under the lock (no NEW block starts), gives a rank that is inside a block a moment to come out (the common case: the
    // calls only enqueue), and aborts — which frees the communicator — whether or not it did (comm_abort_handle).
    std::mutex nccl_mu;
    std::atomic<int> in_rccl{0};
    bool owns_nccl = false;  // zd_comm_create: this object aborts / destroys the communicator; thread-per-GPU driver: the driver does
    LocalGroup *grp = nullptr;
    Stream s_comm;
    Event ev_z, ev_x[2], ev_r[2];
    DevBuf<char> ring;  // two slots of [source rank][planes of a group]...
    int64_t ring_bytes = 0;  // bytes allocated at `ring`
    int64_t slot_bytes = 0;
    int group_planes = 0;
    // Set when ANY rank of the job has failed (thread-per-GPU driver: shared by the ranks; one process per GPU: this rank's
    // own).  A rank that fails aborts the communicators it can reach (ncclCommAbort) so that send / receive kernels already
    // queued — which would spin for ever on the missing rank — drain, and every rank returns non-zero from its next check.
    std::atomic<int> *failed = nullptr;
    std::atomic<int> own_failed{0};
    // per-rank accounting of the exchange (zd_comm_stats)
    int64_t bytes_sent = 0, bytes_received = 0;
    // pipelined passes (zd_plan_run_passes with two send stores): Z stage of a store complete / its sends complete
    Event ev_zd[2], ev_free[2];
    bool slot_used[2] = {false, false};  // an XY stage has been recorded on ev_x[slot] since the ring was (re)allocated
};

namespace {

int comm_prepare(zd_comm *c) {
    MHIP(c->s_comm.create());
    MHIP(c->ev_z.create(hipEventDisableTiming));
    for (int i = 0; i < 2; i++) {
        MHIP(c->ev_x[i].create(hipEventDisableTiming));
        MHIP(c->ev_r[i].create(hipEventDisableTiming));
        MHIP(c->ev_zd[i].create(hipEventDisableTiming));
        MHIP(c->ev_free[i].create(hipEventDisableTiming));
    }
    return 0;
}

// bytes of ONE store plane inside one chunk (chunks are plane-major)
int64_t chunk_plane_bytes(const zd_plan *pl) { return zd_plan_exchange_bytes(pl) / pl->nranks / pl->Zq; }

// The exchange ring belongs to the communicator and is sized by the plan that uses it: a later plan on the same
// communicator (another PPD, stream factor, store or exchange_planes) may need a larger one.  `st` and the communication
// stream are drained before the old ring goes away.
int comm_ring(zd_comm *c, int64_t ring_b, int gp, hipStream_t st) {
    if (c->ring && c->ring_bytes >= ring_b) {
        c->slot_bytes   = ring_b / 2;
        c->group_planes = gp;
        return 0;
    }
    if (c->ring) {
        MHIP(hipStreamSynchronize(st));
        MHIP(hipStreamSynchronize(c->s_comm));
        c->ring.reset();
        c->ring_bytes = 0;
    }
    MHIP(c->ring.store_alloc((size_t) ring_b));
    c->slot_used[0] = c->slot_used[1] = false;
    c->ring_bytes   = ring_b;
    c->slot_bytes   = ring_b / 2;
    c->group_planes = gp;
    return 0;
}

bool comm_failed(const zd_comm *c) { return c->failed && c->failed->load(std::memory_order_acquire) != 0; }

}  // namespace

extern "C" {

int zd_comm_unique_id(void *id128) {
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
    RcclApi *R = rccl();
    if (!R) {
        fprintf(stderr, "zeldovich_hip: librccl.so not found: multi-process runs need RCCL\n");
        return 1;
    }
    ncclUniqueId id;
    MNCCL(R->GetUniqueId(&id));
    memcpy(id128, &id, sizeof(id));
    return 0;
}

// one process per GPU: the caller has made `id128` (from rank 0's zd_comm_unique_id) known to every rank and has
// selected this rank's device (hipSetDevice / torch.cuda.set_device)
int zd_comm_create(int rank, int nranks, const void *id128, zd_comm **out) {
    RcclApi *R = rccl();
    if (!R) {
        fprintf(stderr, "zeldovich_hip: librccl.so not found: multi-process runs need RCCL\n");
        return 1;
    }
    zd_comm *c = new zd_comm;
    c->rank    = rank;
    c->nranks  = nranks;
    c->kind    = 0;
    c->failed  = &c->own_failed;
    c->owns_nccl = true;
    ncclUniqueId id;
    memcpy(&id, id128, sizeof(id));
    ncclResult_t r = R->CommInitRank(&c->nccl, nranks, id, rank);
    if (r != ncclSuccess || comm_prepare(c)) {
        fprintf(stderr, "zeldovich_hip: ncclCommInitRank failed (rank %d of %d)\n", rank, nranks);
        delete c;
        return 1;
    }
    // Handshake: 1 MB to the next rank, 1 MB from the previous one, as ONE grouped send / receive on the communication stream —
    // the call pattern of the exchange.  A communicator that is wired wrongly (ranks on the wrong devices, an id that did not
    // reach everybody, a transport that cannot reach a peer) fails or times out HERE, in well under a minute, instead of
    // inside pass 0 with 200 GB of stores allocated.
    if (nranks > 1) {
        const size_t nb = (size_t) 1 << 20;
        DevBuf<char> buf;
        bool ok = buf.alloc(2 * nb) == hipSuccess && hipMemsetAsync(buf, 0x5a, nb, c->s_comm) == hipSuccess;
        if (ok) {
            ok = R->GroupStart() == ncclSuccess;
            ok = ok && R->Send(buf, nb, ncclChar, (rank + 1) % nranks, c->nccl, c->s_comm) == ncclSuccess;
            ok = ok && R->Recv(buf + nb, nb, ncclChar, (rank + nranks - 1) % nranks, c->nccl, c->s_comm) == ncclSuccess;
            ok = (R->GroupEnd() == ncclSuccess) && ok;
        }
        const auto t0 = std::chrono::steady_clock::now();
        while (ok) {
            const hipError_t q = hipStreamQuery(c->s_comm);
            if (q == hipSuccess) break;
            if (q != hipErrorNotReady || std::chrono::steady_clock::now() - t0 > std::chrono::seconds(60)) ok = false;
            else std::this_thread::sleep_for(std::chrono::milliseconds(2));
        }
        unsigned char probe[2] = {0, 0};
        if (ok) ok = hipMemcpy(probe, buf + nb, 1, hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(probe + 1, buf + 2 * nb - 1, 1, hipMemcpyDeviceToHost) == hipSuccess
                     && probe[0] == 0x5a && probe[1] == 0x5a;
        if (!ok) {
            fprintf(stderr, "zeldovich_hip: rank %d of %d: the 1 MB send / receive handshake with the neighbouring ranks failed or timed out: "
                            "the communicator is not usable\n", rank, nranks);
            zd_comm_abort(c);  // queued send / receive kernels drain
            buf.reset();
            zd_comm_destroy(c);
            return 1;
        }
        c->bytes_sent = c->bytes_received = 0;
    }
    *out = c;
    return 0;
}

namespace {
bool comm_failed(const zd_comm *c);
// A block of RCCL host calls of the rank that owns `c`: the handle is fetched and the rank counted in under the lock, the calls
// run WITHOUT it (zd_comm::nccl_mu); h == nullptr: a peer failed (and may have taken the communicator away)
struct RcclBlock {
    zd_comm *c;
    ncclComm_t h = nullptr;
    explicit RcclBlock(zd_comm *c_) : c(c_) {
        std::lock_guard<std::mutex> lk(c->nccl_mu);
        if (!comm_failed(c) && c->nccl) {
            h = c->nccl;
            c->in_rccl.fetch_add(1, std::memory_order_acq_rel);
        }
    }
    ~RcclBlock() {
        if (h) c->in_rccl.fetch_sub(1, std::memory_order_acq_rel);
    }
    RcclBlock(const RcclBlock &) = delete;
    RcclBlock &operator=(const RcclBlock &) = delete;
};
// take the communicator away from its rank and abort it (= free it: never destroyed again).  Not under the lock: a rank blocked
// inside RCCL is what the abort is for.  A rank that is merely between two enqueueing calls gets up to `grace_ms` to leave its block
// first.  Returns the handle it aborted (nullptr: there was none)
ncclComm_t comm_abort_handle(zd_comm *c, int grace_ms = 500) {
    ncclComm_t h = nullptr;
    {
        std::lock_guard<std::mutex> lk(c->nccl_mu);
        h       = c->nccl;
        c->nccl = nullptr;
    }
    if (!h) return nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    while (c->in_rccl.load(std::memory_order_acquire) > 0
           && std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(grace_ms))
        std::this_thread::sleep_for(std::chrono::milliseconds(1));
    if (rccl() && rccl()->CommAbort) rccl()->CommAbort(h);
    return h;
}
}  // namespace

#ifdef ZD_TESTING
void zd_test_fail_rank(int rank) { g_test_fail_rank.store(rank); }
#endif

void zd_comm_abort(zd_comm *c) {
    if (!c) return;
    c->own_failed.store(1);
    if (c->failed) c->failed->store(1, std::memory_order_release);
    if (c->kind == 0 && c->owns_nccl) comm_abort_handle(c);
}

// Timed probe of the links (VERDICT r4 #3b): `bytes_per_peer` to and from EVERY peer at once — the pattern of the exchange, every
// link of the rank busy — as grouped send / receive calls on the communication stream, one warm-up and `reps` timed repetitions
// between two hipEvents.  *GBps_per_peer = bytes_per_peer * reps / time: what ONE link of this rank carries per direction while
// all of them work (the figure zd_choose_pass_groups_measured prices the all-to-all with).  0 for a communicator without peers or
// with the local transport.  Every rank of the communicator must call it.
int zd_comm_probe(zd_comm *c, int64_t bytes_per_peer, int32_t reps, double *GBps_per_peer) {
    if (GBps_per_peer) *GBps_per_peer = 0.0;
    if (!c || !GBps_per_peer || bytes_per_peer < 1 || reps < 1) return 1;
    if (c->nranks < 2 || c->kind != 0) return 0;
    RcclApi *R = rccl();
    if (!R) return 1;
    const int G = c->nranks, me = c->rank;
    const size_t nb = (size_t) bytes_per_peer;
    DevBuf<char> sbuf, rbuf;
    Event e0, e1;
    if (sbuf.alloc(nb * (size_t) (G - 1)) != hipSuccess || rbuf.alloc(nb * (size_t) (G - 1)) != hipSuccess) return 1;
    if (hipMemsetAsync(sbuf, 0x3c, nb * (size_t) (G - 1), c->s_comm) != hipSuccess) return 1;
    if (e0.create() != hipSuccess || e1.create() != hipSuccess) return 1;
    bool ok = true;
    for (int it = 0; it <= reps && ok; it++) {
        if (it == 1) ok = hipEventRecord(e0, c->s_comm) == hipSuccess;  // (repetition 0 = warm-up: connection set-up)
        RcclBlock blk(c);
        if (!blk.h) {
            ok = false;
            break;
        }
        ok = ok && R->GroupStart() == ncclSuccess;
        int slot = 0;
        for (int p = 0; p < G && ok; p++) {
            if (p == me) continue;
            ok = R->Send(sbuf + nb * (size_t) slot, nb, ncclChar, p, blk.h, c->s_comm) == ncclSuccess
                 && R->Recv(rbuf + nb * (size_t) slot, nb, ncclChar, p, blk.h, c->s_comm) == ncclSuccess;
            slot++;
        }
        ok = (R->GroupEnd() == ncclSuccess) && ok;
    }
    ok = ok && hipEventRecord(e1, c->s_comm) == hipSuccess;
    const auto t0 = std::chrono::steady_clock::now();
    while (ok) {  // (bounded like the handshake: a link that does not come up must not hang the job)
        const hipError_t q = hipStreamQuery(c->s_comm);
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady || comm_failed(c) || std::chrono::steady_clock::now() - t0 > std::chrono::seconds(120)) ok = false;
        else std::this_thread::sleep_for(std::chrono::milliseconds(2));
    }
    if (!ok) {
        fprintf(stderr, "zeldovich_hip: rank %d of %d: the link probe (%lld bytes to every peer) failed or timed out\n", me, G, (long long) bytes_per_peer);
        zd_comm_abort(c);
        return 1;
    }
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e0, e1) != hipSuccess || ms <= 0.f) return 1;
    *GBps_per_peer = (double) nb * reps / (ms * 1e-3) / 1e9;
    return 0;
}

void zd_comm_traffic(zd_comm *c, int64_t *bytes_sent, int64_t *bytes_received, int reset) {
    if (bytes_sent) *bytes_sent = c ? c->bytes_sent : 0;
    if (bytes_received) *bytes_received = c ? c->bytes_received : 0;
    if (c && reset) c->bytes_sent = c->bytes_received = 0;
}

void zd_comm_destroy(zd_comm *c) {
    if (!c) return;
    if (c->nccl && c->owns_nccl && rccl() && rccl()->CommDestroy) rccl()->CommDestroy(c->nccl);
    delete c;  // (stream, events and ring release themselves)
}

// planes per exchange group and bytes of the two-slot ring that zd_plan_run_pass allocates on first use
int64_t zd_plan_ring_bytes(const zd_plan *pl, int32_t *group_planes) {
    if (pl->nranks <= 1) {
        if (group_planes) *group_planes = pl->Zq;
        return 0;
    }
    const int64_t per_plane = chunk_plane_bytes(pl) * pl->nranks;  // one store plane from every source rank
    int gp = (int) std::max<int64_t>(1, std::min<int64_t>(pl->Zq, ((int64_t) 4 << 30) / per_plane));  // ~4 GB per slot
    // field store: whole y->x ring loads per group
    if (zd::pack_is_fields(pl->pack) && gp > pl->ring_planes) gp = gp / pl->ring_planes * pl->ring_planes;
    if (pl->p.exchange_planes > 0) gp = std::min<int>(pl->Zq, pl->p.exchange_planes);
    if (group_planes) *group_planes = gp;
    return 2 * per_plane * gp;
}

// One residue pass of one rank: Z stage into d_store, exchange + XY stages plane group by plane group.
//   comm       NULL (or nranks == 1): no exchange, the XY stages read d_store directly
//   d_records  room for `rec_planes` delivered planes (a multiple of zd_plan_plane_step); every time it has been filled
//              (or the pass ends) `cb(user, first_local_plane, nplanes, d_records, stream)` is called with the work
//              still queued on `stream` — the consumer orders itself after it (or syncs); cb may be NULL (benchmark sink)
typedef int (*zd_group_cb)(void *user, int64_t first_local_plane, int64_t nplanes, const void *d_records, void *hip_stream);

static int run_passes_impl(zd_plan *pl, zd_comm *c, int first, int step, void *d_store, void *d_store2, void *d_records, float *d_density,
                           int64_t rec_planes, zd_pass_cb cb, void *user, void *hip_stream);
// d_density: room for rec_planes planes of float32 (stores with a density field only) or NULL
static int run_pass_impl(zd_plan *pl, zd_comm *c, int pass, void *d_store, void *d_records, float *d_density, int64_t rec_planes,
                         zd_group_cb cb, void *user, void *hip_stream);

int zd_plan_run_pass(zd_plan *pl, zd_comm *c, int pass, void *d_store, void *d_records, int64_t rec_planes, zd_group_cb cb,
                     void *user, void *hip_stream) {
    return run_pass_impl(pl, c, pass, d_store, d_records, nullptr, rec_planes, cb, user, hip_stream);
}

// z_done: NULL = run the Z stage here, joined to the stream (one store); else the Z stage of this pass has been issued
// detached (zd_plan_stage_z_detached) and z_done is recorded behind it.  sends_done (with z_done): recorded on the
// communication stream behind the last send of the pass instead of holding the compute stream back.
static int run_pass_body(zd_plan *pl, zd_comm *c, int pass, void *d_store, void *d_records, float *d_density, int64_t rec_planes,
                         zd_group_cb cb, void *user, void *hip_stream, hipEvent_t z_done = nullptr, hipEvent_t sends_done = nullptr);

// A rank that fails (allocation, launch, RCCL error, consumer returning non-zero) must not leave its peers spinning in the
// send / receive kernels they have already queued for it: the failure is published (zd_comm::failed) and this rank's
// communicator is aborted before the error is returned.  Peers notice at their next check and return 1 as well.
static int run_pass_impl(zd_plan *pl, zd_comm *c, int pass, void *d_store, void *d_records, float *d_density, int64_t rec_planes,
                         zd_group_cb cb, void *user, void *hip_stream) {
    if (c && comm_failed(c)) return 1;
    const int rc = run_pass_body(pl, c, pass, d_store, d_records, d_density, rec_planes, cb, user, hip_stream);
    if (rc && c && pl->nranks > 1) {
        if (c->failed) c->failed->store(1, std::memory_order_release);
        if (c->kind == 0) zd_comm_abort(c);
        if (c->kind == 1 && c->grp) c->grp->fail();
    }
    return rc;
}

static int run_pass_body(zd_plan *pl, zd_comm *c, int pass, void *d_store, void *d_records, float *d_density, int64_t rec_planes,
                         zd_group_cb cb, void *user, void *hip_stream, hipEvent_t z_done, hipEvent_t sends_done) {
    hipStream_t st = (hipStream_t) hip_stream;
    const int ps = pl->pstep;
    const int64_t Pp = zd_plan_local_planes(pl);
    if (rec_planes < ps || rec_planes % ps) {
        fprintf(stderr, "zeldovich_hip: record buffer of %lld planes (multiples of %d needed)\n", (long long) rec_planes, ps);
        return 1;
    }
    if (!z_done && zd_plan_stage_z(pl, pass, d_store, st)) return 1;
    if (!c || pl->nranks <= 1) {
        if (z_done) MHIP(hipStreamWaitEvent(st, z_done, 0));
        if (zd_plan_stage_y(pl, d_store, st)) return 1;
        for (int64_t q0 = 0; q0 < Pp; q0 += rec_planes) {
            const int64_t n = std::min<int64_t>(rec_planes, Pp - q0);
            if (zd_plan_stage_x_group(pl, pass, d_store, pl->Zq, q0, q0, n, d_records, d_density, st)) return 1;
            if (cb && cb(user, q0, n, d_records, st)) return 1;
        }
        if (sends_done) MHIP(hipEventRecord(sends_done, st));  // (one rank, two stores: the XY stages have left d_store)
        return 0;
    }
    if (c->nranks != pl->nranks || c->rank != pl->rank) {
        fprintf(stderr, "zeldovich_hip: communicator (rank %d of %d) does not match the plan (rank %d of %d)\n", c->rank,
                c->nranks, pl->rank, pl->nranks);
        return 1;
    }
    // ---- ring ----
    int gp = 0;
    const int64_t ring_b = zd_plan_ring_bytes(pl, &gp);
    if (comm_ring(c, ring_b, gp, st)) return 1;
    const int G = pl->nranks, me = pl->rank;
    const int64_t cpb = chunk_plane_bytes(pl), chunk_b = cpb * pl->Zq;
    const int ngroups = (pl->Zq + gp - 1) / gp;
    // the Z stage must be complete before anything leaves the send store
    if (z_done) {
        MHIP(hipStreamWaitEvent(c->s_comm, z_done, 0));
    } else {
        MHIP(hipEventRecord(c->ev_z, st));
        MHIP(hipStreamWaitEvent(c->s_comm, c->ev_z, 0));
    }
    if (c->kind == 1) {  // local: every rank's send store must be complete before anybody pulls from it
        MHIP(hipStreamSynchronize(st));
        c->grp->send_base[me] = (const char *) d_store;
        if (c->grp->wait()) return 1;
    }
    auto exchange = [&](int j) -> int {
        const int slot = j & 1;
        const int64_t p0 = (int64_t) j * gp, np = std::min<int64_t>(gp, pl->Zq - p0);
        const size_t nb = (size_t) (cpb * np);
        char *dst = c->ring + (size_t) slot * c->slot_bytes;
        // the XY stages of the group that used the slot before (group j-2, or the last groups of the previous pass when the
        // passes are pipelined and the communication stream no longer waits for the compute stream in between) have left it
        if (j >= 2 || c->slot_used[slot]) MHIP(hipStreamWaitEvent(c->s_comm, c->ev_x[slot], 0));
        if (c->kind == 1) {
            for (int s = 0; s < G; s++)  // pull: chunk <me> of rank s's send store, planes of the group
                MHIP(hipMemcpyAsync(dst + (size_t) s * cpb * gp, c->grp->send_base[s] + (size_t) me * chunk_b + (size_t) p0 * cpb, nb,
                                    hipMemcpyDeviceToDevice, c->s_comm));
        } else {
            RcclApi *R = rccl();
            RcclBlock blk(c);
            if (!blk.h) return 1;  // a peer failed (and may have aborted this communicator)
            MNCCL(R->GroupStart());
            for (int p = 0; p < G; p++) {
                const char *sb = (const char *) d_store + (size_t) p * chunk_b + (size_t) p0 * cpb;
                char *rb       = dst + (size_t) p * cpb * gp;
                if (p == me) continue;
                MNCCL(R->Send(sb, nb, ncclChar, p, blk.h, c->s_comm));
                MNCCL(R->Recv(rb, nb, ncclChar, p, blk.h, c->s_comm));
            }
            MNCCL(R->GroupEnd());
            MHIP(hipMemcpyAsync(dst + (size_t) me * cpb * gp, (const char *) d_store + (size_t) me * chunk_b + (size_t) p0 * cpb, nb,
                                hipMemcpyDeviceToDevice, c->s_comm));
        }
        const int64_t moved = (int64_t) nb * (G - 1);
        c->bytes_sent += moved;
        c->bytes_received += moved;
        pl->bytes_sent += moved;
        MHIP(hipEventRecord(c->ev_r[slot], c->s_comm));
        return 0;
    };
    if (exchange(0)) return 1;
    for (int j = 0; j < ngroups; j++) {
        if (j + 1 < ngroups && exchange(j + 1)) return 1;  // next group travels while this one is transformed
        const int slot = j & 1;
        const int64_t p0 = (int64_t) j * gp, np = std::min<int64_t>(gp, pl->Zq - p0);
        if (comm_failed(c)) return 1;
        zd_plan_tick(pl, ZD_K_XWAIT, st, 1);  // two events around the wait: their distance = the time the compute stream stood
        MHIP(hipStreamWaitEvent(st, c->ev_r[slot], 0));
        zd_plan_tick(pl, ZD_K_XWAIT, st, 0);
        const void *src = c->ring + (size_t) slot * c->slot_bytes;
        if (zd_plan_stage_y_group(pl, const_cast<void *>(src), gp, (int) np, st)) return 1;
        // XY on the slot: chunks are gp planes long there
        for (int64_t q0 = 0; q0 < np * ps; q0 += rec_planes) {
            const int64_t n = std::min<int64_t>(rec_planes, np * ps - q0);
            if (zd_plan_stage_x_group(pl, pass, src, gp, q0, p0 * ps + q0, n, d_records, d_density, st)) return 1;
            if (cb && cb(user, p0 * ps + q0, n, d_records, st)) return 1;
        }
        MHIP(hipEventRecord(c->ev_x[slot], st));
        c->slot_used[slot] = true;
    }
    if (c->kind == 1) {  // nobody may start the next Z stage (overwriting its send store) while a peer still pulls
        MHIP(hipStreamSynchronize(c->s_comm));
        MHIP(hipStreamSynchronize(st));
        if (c->grp->wait()) return 1;
    } else if (sends_done) {
        MHIP(hipEventRecord(sends_done, c->s_comm));  // (pipelined: the Z stage that reuses this store waits for it)
    } else {
        // the sends of this pass must have left d_store before the caller's next Z stage overwrites it
        MHIP(hipEventRecord(c->ev_z, c->s_comm));
        MHIP(hipStreamWaitEvent(st, c->ev_z, 0));
    }
    return 0;
}

// Passes first, first + step, ... of this rank.  With a second send store (d_store2, same size), several ranks and the RCCL
// transport the passes are PIPELINED: the Z stage of the next pass is issued detached from the compute stream into the other
// store before this pass's planes are exchanged and transformed, so generator and z FFT of pass p+1 run while the exchange
// of pass p occupies the links (the reference's per-block StoreBlock inside the generation loop, src/zeldovich.cpp:558-587,
// in units of passes); a store is rewritten only after its sends have completed.  Otherwise the passes run one after the
// other on d_store.
int zd_plan_run_passes(zd_plan *pl, zd_comm *c, int first, int step, void *d_store, void *d_store2, void *d_records, int64_t rec_planes,
                       zd_pass_cb cb, void *user, void *hip_stream) {
    return run_passes_impl(pl, c, first, step, d_store, d_store2, d_records, nullptr, rec_planes, cb, user, hip_stream);
}

namespace {
struct PassCb {
    zd_pass_cb cb;
    void *user;
    int pass;
};
int pass_cb_adaptor(void *u, int64_t first_local_plane, int64_t nplanes, const void *d_records, void *hip_stream) {
    PassCb *p = (PassCb *) u;
    return p->cb ? p->cb(p->user, p->pass, first_local_plane, nplanes, d_records, hip_stream) : 0;
}
}  // namespace

static int run_passes_impl(zd_plan *pl, zd_comm *c, int first, int step, void *d_store, void *d_store2, void *d_records, float *d_density,
                           int64_t rec_planes, zd_pass_cb cb, void *user, void *hip_stream) {
    hipStream_t st = (hipStream_t) hip_stream;
    if (first < 0 || step < 1) return 1;
    // the generator's run-ahead (stage_z_impl) needs this rank's NEXT pass while these passes run — and only then: left on the plan,
    // a later zd_plan_stage_z / zd_plan_run_pass of consecutive residues would generate ahead into residue + step and throw it away
    struct StepScope {
        zd_plan *pl;
        ~StepScope() { pl->pass_step = 1; }
    } step_scope{pl};
    pl->pass_step = step;
    PassCb pc{cb, user, 0};
    const bool pipelined = c && pl->nranks > 1 && c->kind == 0 && d_store2 != nullptr && first + step < pl->npass;
    // ONE rank with a second store: the Z stage of pass p + 1 — vector-bound — is issued detached into the other
    // store while the y / x stages of pass p — HBM-bound — run on the caller's stream; its z FFT waits until the XY stages of pass
    // p - 1 have left that store.  Two stores of half the size mean twice the passes (twice the generations), so whether this
    // pays is a measurement: bench.py --two-stores (profiles/r04_tuning_notes.md).
    if (!pipelined && pl->nranks == 1 && d_store2 != nullptr && first + step < pl->npass && pl->overlap && !pl->any && !pl->dens_sub) {
        for (Event &e : pl->ev_pipe)
            if (!e) MHIP(e.create(hipEventDisableTiming));
        const hipEvent_t ev_start = pl->ev_pipe[0], ev_zd[2] = {pl->ev_pipe[1], pl->ev_pipe[2]}, ev_xy[2] = {pl->ev_pipe[3], pl->ev_pipe[4]};
        void *stores[2] = {d_store, d_store2};
        MHIP(hipEventRecord(ev_start, st));
        if (zd_plan_stage_z_detached(pl, first, stores[0], st, ev_start, ev_zd[0])) return 1;
        int i = 0;
        for (int pass = first; pass < pl->npass; pass += step, i++) {
            const int b = i & 1, nxt = pass + step;
            if (nxt < pl->npass && zd_plan_stage_z_detached(pl, nxt, stores[1 - b], st, i >= 1 ? ev_xy[1 - b] : ev_start, ev_zd[1 - b])) return 1;
            pc.pass = pass;
            if (run_pass_body(pl, nullptr, pass, stores[b], d_records, d_density, rec_planes, pass_cb_adaptor, &pc, st, ev_zd[b], ev_xy[b])) return 1;
        }
        return 0;
    }
    if (!pipelined) {
        for (int pass = first; pass < pl->npass; pass += step) {
            pc.pass = pass;
            if (run_pass_impl(pl, c, pass, d_store, d_records, d_density, rec_planes, pass_cb_adaptor, &pc, st)) return 1;
        }
        return 0;
    }
    if (comm_failed(c)) return 1;
    void *stores[2] = {d_store, d_store2};
    // (every failure in here must reach the abort epilogue below, or the peers spin in their queued send / receive kernels)
    const int rc = [&]() -> int {
        // the first Z stage starts after whatever the caller queued on its stream (the stores' previous users)
        if (hipEventRecord(c->ev_z, st) != hipSuccess) return 1;
        if (zd_plan_stage_z_detached(pl, first, stores[0], st, c->ev_z, c->ev_zd[0])) return 1;
        int i = 0;
        for (int pass = first; pass < pl->npass; pass += step, i++) {
            const int b = i & 1, nxt = pass + step;
            // store 1-b was last read by the sends of pass i-1 (ev_free); the very first use is free
            if (nxt < pl->npass && zd_plan_stage_z_detached(pl, nxt, stores[1 - b], st, i >= 1 ? c->ev_free[1 - b] : c->ev_z, c->ev_zd[1 - b])) return 1;
            pc.pass = pass;
            if (run_pass_body(pl, c, pass, stores[b], d_records, d_density, rec_planes, pass_cb_adaptor, &pc, st, c->ev_zd[b], c->ev_free[b])) return 1;
        }
        // the caller's stream ends behind the last sends (the stores may be freed or rewritten by the caller afterwards)
        return hipEventRecord(c->ev_z, c->s_comm) != hipSuccess || hipStreamWaitEvent(st, c->ev_z, 0) != hipSuccess;
    }();
    if (rc) {
        if (c->failed) c->failed->store(1, std::memory_order_release);
        zd_comm_abort(c);
    }
    return rc;
}

// The phi round of ZD_f_NL on several ranks (zeldovich.cpp:945-960: ZeldovichZ(gen_phi) + ZeldovichXY_Phi, then the forward z
// transform that LoadBlockForward / ForwardFFT_Yonly do for the second ZeldovichZ).  `ph` is the plan of zd_plan_create_phi
// (one array, R = 1).  Rank g generates phi = D / M for its rows into d_store; plane groups travel to their XY ranks exactly
// as in zd_plan_run_pass, are transformed there (inverse y, x with phi + f_NL phi^2, forward y) and travel BACK into the same
// places of d_store — the reverse exchange, on the same communication stream, so that a ring slot is reused only after its
// return trip; finally every rank transforms its own rows along z into d_phik[row slot][kz][x].
static int phi_round(zd_plan *ph, zd_comm *c, void *d_store, void *d_phik, double f_NL, hipStream_t st) {
    if (zd_plan_stage_z(ph, 0, d_store, st)) return 1;
    int gp = 0;
    const int64_t ring_b = zd_plan_ring_bytes(ph, &gp);
    if (comm_ring(c, ring_b, gp, st)) return 1;
    const int G = ph->nranks, me = ph->rank;
    const int64_t cpb = chunk_plane_bytes(ph), chunk_b = cpb * ph->Zq;
    const int ngroups = (ph->Zq + gp - 1) / gp;
    MHIP(hipEventRecord(c->ev_z, st));
    MHIP(hipStreamWaitEvent(c->s_comm, c->ev_z, 0));
    if (c->kind == 1) {
        MHIP(hipStreamSynchronize(st));
        c->grp->send_base[me] = (const char *) d_store;
        c->grp->ring_base[me] = c->ring;
        if (c->grp->wait()) return 1;
    }
    // forward: chunk <me> of every peer's store -> slot[source rank]; reverse: slot[rank s] -> chunk <me> of rank s's store
    auto travel = [&](int j, bool reverse) -> int {
        const int slot = j & 1;
        const int64_t p0 = (int64_t) j * gp, np = std::min<int64_t>(gp, ph->Zq - p0);
        const size_t nb = (size_t) (cpb * np);
        char *ring = c->ring + (size_t) slot * c->slot_bytes;
        if (c->kind == 1) {
            for (int s = 0; s < G; s++) {
                if (!reverse)
                    MHIP(hipMemcpyAsync(ring + (size_t) s * cpb * gp, c->grp->send_base[s] + (size_t) me * chunk_b + (size_t) p0 * cpb, nb,
                                        hipMemcpyDeviceToDevice, c->s_comm));
                else  // pull what rank s finished of MY rows: its slot[me] -> my chunk s
                    MHIP(hipMemcpyAsync((char *) d_store + (size_t) s * chunk_b + (size_t) p0 * cpb,
                                        c->grp->ring_base[s] + (size_t) slot * c->slot_bytes + (size_t) me * cpb * gp, nb, hipMemcpyDeviceToDevice,
                                        c->s_comm));
            }
        } else {
            RcclApi *R = rccl();
            RcclBlock blk(c);
            if (!blk.h) return 1;  // (see run_pass_body)
            MNCCL(R->GroupStart());
            for (int p = 0; p < G; p++) {
                char *sb = (char *) d_store + (size_t) p * chunk_b + (size_t) p0 * cpb;  // my rows, planes of rank p
                char *rb = ring + (size_t) p * cpb * gp;                                 // rank p's rows, my planes
                if (p == me) continue;
                MNCCL(R->Send(reverse ? rb : sb, nb, ncclChar, p, blk.h, c->s_comm));
                MNCCL(R->Recv(reverse ? sb : rb, nb, ncclChar, p, blk.h, c->s_comm));
            }
            MNCCL(R->GroupEnd());
            char *own_s = (char *) d_store + (size_t) me * chunk_b + (size_t) p0 * cpb, *own_r = ring + (size_t) me * cpb * gp;
            MHIP(hipMemcpyAsync(reverse ? own_s : own_r, reverse ? own_r : own_s, nb, hipMemcpyDeviceToDevice, c->s_comm));
        }
        if (!reverse) MHIP(hipEventRecord(c->ev_r[slot], c->s_comm));
        return 0;
    };
    if (c->kind == 1) {  // local transport (test boxes): one group at a time, rendezvous around every step
        for (int j = 0; j < ngroups; j++) {
            const int64_t np = std::min<int64_t>(gp, ph->Zq - (int64_t) j * gp);
            if (travel(j, false)) return 1;
            MHIP(hipStreamSynchronize(c->s_comm));
            if (zd_plan_phi_xy_group(ph, c->ring + (size_t) (j & 1) * c->slot_bytes, gp, (int) np, f_NL, st)) return 1;
            MHIP(hipStreamSynchronize(st));
            if (c->grp->wait()) return 1;  // every rank's slot is finished before anybody pulls from it
            if (travel(j, true)) return 1;
            MHIP(hipStreamSynchronize(c->s_comm));
            if (c->grp->wait()) return 1;  // ... and pulled before it is overwritten
        }
    } else {
        if (travel(0, false)) return 1;
        if (ngroups > 1 && travel(1, false)) return 1;
        for (int j = 0; j < ngroups; j++) {
            const int slot = j & 1;
            const int64_t np = std::min<int64_t>(gp, ph->Zq - (int64_t) j * gp);
            MHIP(hipStreamWaitEvent(st, c->ev_r[slot], 0));
            if (zd_plan_phi_xy_group(ph, c->ring + (size_t) slot * c->slot_bytes, gp, (int) np, f_NL, st)) return 1;
            MHIP(hipEventRecord(c->ev_x[slot], st));
            MHIP(hipStreamWaitEvent(c->s_comm, c->ev_x[slot], 0));
            if (travel(j, true)) return 1;                           // the group goes home ...
            if (j + 2 < ngroups && travel(j + 2, false)) return 1;   // ... and only then is its slot filled again
        }
        MHIP(hipEventRecord(c->ev_z, c->s_comm));
        MHIP(hipStreamWaitEvent(st, c->ev_z, 0));
    }
    if (zd_plan_phi_zfwd(ph, d_store, d_phik, st)) return 1;
    MHIP(hipStreamSynchronize(st));
    return 0;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// thread-per-GPU driver behind zd_generate (ngpu > 1)

namespace {

struct RankCtx {
    int rank = 0, device = 0;
    zd_comm *comm = nullptr;
    int rc = 0;
    zd_stats stats;
};

struct Delivery {  // serialises the per-plane callback over the rank threads (WriteParticlesSlab is not re-entrant,
                   // src/output.cpp:28-39)
    std::mutex mu;
    zd_slab_cb cb = nullptr;
    void *user    = nullptr;
};

struct GroupSink {
    zd_plan *pl;
    int pass;
    Delivery *dl;
    char *h_rec;
    size_t plane_rec_b;
    const float *d_dens;  // device density planes of the group (ZD_qdensity) or NULL
    float *h_dens;
    int64_t only_z;       // ZD_qoneslab: deliver just this z (-1: every plane)
    const std::atomic<int> *failed = nullptr;  // the job's failure flag
    std::atomic<int> *failed_w = nullptr;      // (the same, to set it when this rank's consumer fails)
};

int sink_cb(void *user, int pass, int64_t first_local_plane, int64_t nplanes, const void *d_records, void *hip_stream) {
    GroupSink *s = (GroupSink *) user;
    s->pass = pass;
    if (!s->dl->cb) return 0;
    hipStream_t st = (hipStream_t) hip_stream;
    const size_t nn = (size_t) s->pl->N * s->pl->N;
    if (s->plane_rec_b && hipMemcpyAsync(s->h_rec, d_records, s->plane_rec_b * (size_t) nplanes, hipMemcpyDeviceToHost, st) != hipSuccess) return 1;
    if (s->d_dens && hipMemcpyAsync(s->h_dens, s->d_dens, nn * 4 * (size_t) nplanes, hipMemcpyDeviceToHost, st) != hipSuccess) return 1;
    if (hipStreamSynchronize(st) != hipSuccess) return 1;
    if (s->failed && s->failed->load(std::memory_order_acquire)) return 1;  // a peer failed: what arrived may be incomplete
    std::lock_guard<std::mutex> lock(s->dl->mu);
    for (int64_t i = 0; i < nplanes; i++) {
        const int64_t z = zd_plan_plane_z(s->pl, s->pass, first_local_plane + i);
        if (s->only_z >= 0 && z != s->only_z) continue;
        if (s->failed && s->failed->load(std::memory_order_acquire)) return 1;  // (another rank's consumer failed meanwhile)
        if (s->dl->cb(s->dl->user, z, (int64_t) nn, s->plane_rec_b ? s->h_rec + (size_t) i * s->plane_rec_b : nullptr,
                      s->d_dens ? s->h_dens + (size_t) i * nn : nullptr))
        {
            if (s->failed_w) s->failed_w->store(1, std::memory_order_release);  // published before the mutex is released
            return 1;
        }
    }
    return 0;
}

}  // namespace

// ZeldovichZ + ZeldovichXY on `ngpu` GPUs of this node, one host thread per GPU (called by zd_generate).
// transport: 0 = RCCL (ncclCommInitAll), 1 = local pulls; ranks are placed on devices rank % device_count, so with the
// local transport a one-GPU box can run several ranks (tests).
int zd_generate_multi(const zd_params *p_in, const zd_pk *pk, const double *eig, int64_t eig_ppd, zd_slab_cb cb, void *user,
                      zd_stats *out, int transport) {
    const int G = p_in->ngpu;
    int ndev = 0;
    MHIP(hipGetDeviceCount(&ndev));
    if (ndev < 1) {
        fprintf(stderr, "zeldovich_hip: no GPU\n");
        return 1;
    }
    if (p_in->f_NL != 0.) {  // powers of two up to 4096 and the composite grids with composite transforms (the arrays split over the ranks)
        if (const char *why = zd_fnl_multi_unsupported(p_in)) {
            fprintf(stderr, "zeldovich_hip: %s\n", why);
            return 1;
        }
    }
    if (transport == 0 && ndev < G) {
        fprintf(stderr, "zeldovich_hip: ZD_NumGPU = %d but only %d GPU(s) are visible\n", G, ndev);
        return 1;
    }
    // How the GPUs share the job (zd_choose_pass_groups): `groups` independent groups of gsz ranks.  Group j runs the residue
    // passes j, j + groups, ...; the rows / planes of a pass are sharded over the gsz ranks of a group with the exchange of
    // run_pass_impl.  gsz = 1: no exchange at all.
    zd_params p = *p_in;
    int groups = 1;
    {
        size_t free_b = 0, total_b = 0;
        MHIP(hipMemGetInfo(&free_b, &total_b));
        const int ranks_per_dev = (G + ndev - 1) / ndev;
        // (ZD_f_NL on the powers of two: every rank also keeps PhiK of its rows, N^3 / (2 G) complex; on the composite grids the
        // chooser counts it itself, with the phi round's peak)
        const bool pow2 = (p.ppd & (p.ppd - 1)) == 0;
        const int64_t phik_b = p.f_NL != 0. && pow2 ? (p.ppd / 2 / G) * p.ppd * p.ppd * 16 : 0;
        int32_t g = 1, R = 0;
        if (zd_choose_pass_groups(&p, G, ((int64_t) free_b - ((int64_t) 16 << 30)) / ranks_per_dev - phik_b, &g, &R)) {
            fprintf(stderr, "zeldovich_hip: PPD %lld does not fit %d GPU(s)\n", (long long) p.ppd, G);
            return 1;
        }
        groups          = g;
        p.stream_factor = R;
    }
    const int gsz = G / groups;
    if (transport == 2 && groups > 1) {
        fprintf(stderr, "zeldovich_hip: the test transport runs one group of ranks\n");
        return 1;
    }
    std::vector<RankCtx> ctx(G);
    std::vector<LocalGroup> grps(groups);  // rendezvous of the local transport, one per group
    std::vector<ncclComm_t> nccls(G, nullptr);
#ifdef ZD_TESTING
    std::vector<LoopComm> loops(G);
#endif
    if (transport == 2) {  // tests: the RCCL branch of the exchange on an in-process emulation of its calls
#ifdef ZD_TESTING
        g_loop.n = G;
        g_loop.box.assign((size_t) G * G, {});
        g_loop.taken.assign((size_t) G * G, 0);
        g_loop_api             = RcclApi{};
        g_loop_api.h           = &g_loop_api;
        g_loop_api.GroupStart  = loop_group_start;
        g_loop_api.GroupEnd    = loop_group_end;
        g_loop_api.Send        = loop_send;
        g_loop_api.Recv        = loop_recv;
        g_loop_api.GetErrorString = loop_error_string;
        g_loop_api.CommAbort   = loop_comm_abort;
        g_loop.aborted.store(false);
        g_rccl_override        = &g_loop_api;
        for (int g = 0; g < G; g++) {
            loops[g].rank = g;
            loops[g].n    = G;
            nccls[g]      = reinterpret_cast<ncclComm_t>(&loops[g]);
        }
#else
        fprintf(stderr, "zeldovich_hip: transport 2 is test scaffolding (-DZD_TESTING build only)\n");
        return 1;
#endif
    } else if (transport == 1) {
        for (LocalGroup &grp : grps) {
            grp.n = gsz;
            grp.send_base.assign(gsz, nullptr);
            grp.ring_base.assign(gsz, nullptr);
        }
    } else if (gsz > 1) {  // one communicator per group (ranks j * gsz ... of the devices in order)
        RcclApi *R = rccl();
        if (!R) {
            fprintf(stderr, "zeldovich_hip: librccl.so not found\n");
            return 1;
        }
        for (int j = 0; j < groups; j++) {
            std::vector<int> devs(gsz);
            for (int i = 0; i < gsz; i++) devs[i] = j * gsz + i;
            MNCCL(R->CommInitAll(nccls.data() + (size_t) j * gsz, gsz, devs.data()));
        }
    }
    Delivery dl;
    dl.cb   = cb;
    dl.user = user;
    // One failure flag for the job.  The rank that fails sets it and aborts EVERY communicator of the process (they are all
    // here): the send / receive kernels its peers have queued for it drain instead of spinning, the peers' stream syncs
    // return, they see the flag and leave.  Aborted communicators are freed by the abort, not destroyed again.
    // (the abort FREES a communicator, and a healthy rank thread may be about to enter RCCL with the same handle —
    // every rank's zd_comm lives for the whole job, owned by this driver; its `nccl_mu` is held only to publish, fetch or take
    // away the handle and to count the rank into a block of RCCL host calls (RcclBlock), never across the calls or the abort
    // themselves (zd_comm::nccl_mu); after the abort the handle is gone from the zd_comm and the rank's next exchange returns
    // 1 before touching RCCL.)
    std::atomic<int> job_failed{0};
    std::mutex abort_mu;
    bool aborted = false;
    std::vector<zd_comm *> comms(G, nullptr);
    for (int g = 0; g < G; g++) comms[g] = new zd_comm;
    auto abort_all = [&]() {
        job_failed.store(1, std::memory_order_release);
        for (LocalGroup &grp : grps) grp.fail();
        std::lock_guard<std::mutex> lk(abort_mu);
        if (aborted || transport == 1) return;  // (RCCL, or its emulation in the testing library)
        aborted = true;
        RcclApi *R = rccl();
        (void) R;
        // first every handle is taken away (no rank starts a new block of RCCL calls), then the communicators are aborted — none
        // of it under a rank's lock: a rank may sit in a blocking RCCL call that only the abort ends
        for (int g = 0; g < G; g++) {
            {
                // a communicator its rank thread has not taken yet (the thread publishes nccls[g] into its zd_comm under this
                // lock): nobody can be inside RCCL with it — aborted here, and the thread will find nullptr
                std::lock_guard<std::mutex> lc(comms[g]->nccl_mu);
                if (!comms[g]->nccl) {
                    if (nccls[g] && rccl() && rccl()->CommAbort) rccl()->CommAbort(nccls[g]);
                    nccls[g] = nullptr;
                    continue;
                }
            }
            comm_abort_handle(comms[g]);
            nccls[g] = nullptr;
        }
    };
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<std::thread> threads;
    for (int g = 0; g < G; g++) {
        ctx[g].rank   = g;
        ctx[g].device = g % ndev;
        threads.emplace_back([&, g]() {
            RankCtx &me = ctx[g];
            zd_comm *c  = comms[g];
            // what this rank holds: released at the end of this function — on the rank's thread, its device current, and after
            // abort_all() below has let the peers go — the stream first and the plan last
            PlanPtr plan;
            DevBuf<cplx> d_phik;  // f_NL: PhiK of this rank's rows, until the main plan exists and owns it
            PinnedBuf<float> h_dens;
            PinnedBuf<char> h_rec;
            DevBuf<float> d_dens;
            DevBuf<void> d_rec, d_store2, d_store;
            Stream st;
            me.rc = [&]() -> int {
                if (hipSetDevice(me.device) != hipSuccess || st.create() != hipSuccess) return 1;
                const int grp_id = g / gsz, rk = g % gsz;  // group, rank inside it
                c->rank   = rk;
                c->nranks = gsz;
                c->kind   = transport == 2 ? 0 : transport;  // the loopback emulation runs the RCCL branch
                {
                    std::lock_guard<std::mutex> lc(c->nccl_mu);
                    c->nccl = nccls[g];
                }
                c->grp    = &grps[grp_id];
                c->failed = &job_failed;
                if (comm_prepare(c)) return 1;
#ifdef ZD_TESTING
                if (g_test_fail_rank.load() == g) {  // a rank that fails BEFORE its first exchange (store allocation, plan error):
                    fprintf(stderr, "zeldovich_hip: (test) rank %d fails before pass 0\n", g);  // its peers sit in their first GroupEnd
                    return 1;
                }
#endif
                zd_plan *pl = nullptr;
                if (p.f_NL != 0.) {  // the phi round first (its own plan, store and ring), then the main plan reads PhiK
                    {
                        zd_plan *ph = nullptr;
                        if (zd_plan_create_phi(&p, pk, rk, gsz, &ph)) return 1;
                        PlanPtr phi_plan(ph);
                        DevBuf<void> d_phi;
                        if (d_phi.store_alloc((size_t) zd_plan_exchange_bytes(ph)) != hipSuccess
                            || d_phik.store_alloc((size_t) ph->Hq * ph->N * ph->N) != hipSuccess) {
                            fprintf(stderr, "zeldovich_hip: rank %d: f_NL needs %.1f GB of HBM for the phi field\n", g,
                                    (zd_plan_exchange_bytes(ph) + (double) ph->Hq * ph->N * ph->N * 16) / 1e9);
                            return 1;
                        }
                        if (g == 0) fprintf(stderr, "Generating phi field\n");
                        if (phi_round(ph, c, d_phi, d_phik, p.f_NL, st)) return 1;
                    }
                    if (zd_plan_create_phik(&p, pk, eig, eig_ppd, rk, gsz, d_phik, &pl)) return 1;
                    plan.reset(pl);
                    pl->d_phik_owned = std::move(d_phik);
                } else {
                    if (zd_plan_create(&p, pk, eig, eig_ppd, rk, gsz, &pl)) return 1;
                    plan.reset(pl);
                }
                const int ps = pl->pstep;
                const bool want_rec = pl->narray >= 2 && !pl->dens_only, want_dens = p.qdensity != 0;  // ZD_qdensity = 2: density only
                const size_t nn = (size_t) pl->N * pl->N;
                const size_t plane_rec_b = want_rec ? nn * pl->ec.recsize : 0;
                const int64_t ring_b = cb ? ((int64_t) 1 << 30) : ((int64_t) 4 << 30);
                int64_t rec_planes = std::max<int64_t>(ps, std::min<int64_t>(zd_plan_local_planes(pl),
                                                                             ring_b / (int64_t) (plane_rec_b + (want_dens ? nn * 4 : 0))) / ps * ps);
                if (d_store.store_alloc((size_t) zd_plan_exchange_bytes(pl)) != hipSuccess) {
                    fprintf(stderr, "zeldovich_hip: rank %d cannot allocate the %.2f GB block store\n", g, zd_plan_exchange_bytes(pl) / 1e9);
                    return 1;
                }
                if (want_rec && d_rec.alloc(plane_rec_b * (size_t) rec_planes) != hipSuccess) return 1;
                if (want_rec && cb && h_rec.alloc(plane_rec_b * (size_t) rec_planes) != hipSuccess) return 1;
                if (want_dens && d_dens.alloc(nn * (size_t) rec_planes) != hipSuccess) return 1;
                if (want_dens && cb && h_dens.alloc(nn * (size_t) rec_planes) != hipSuccess) return 1;
                if (pl->npass % groups) {
                    fprintf(stderr, "zeldovich_hip: %d passes do not deal out over %d pass groups\n", pl->npass, groups);
                    return 1;
                }
                // sum |D|^2 of the packed stores comes from the generator, once per run and rank: every group sees every
                // mode, so only group 0 accumulates it (its ranks cover all rows between them)
                if (grp_id != 0) pl->var_pending = false;
                // a second send store (several ranks exchanging over RCCL, more than one pass for this group, memory to spare):
                // the passes are pipelined — Z stage of pass p+1 beside the exchange of pass p (run_passes_impl)
                if (gsz > 1 && c->kind == 0 && grp_id + groups < pl->npass) {
                    size_t free_b = 0, total_b = 0;
                    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess
                        && free_b > (size_t) zd_plan_exchange_bytes(pl) * ((G + ndev - 1) / ndev) + ((size_t) 12 << 30))
                        d_store2.store_alloc((size_t) zd_plan_exchange_bytes(pl));  // (no second store: the passes run one after the other)
                }
                GroupSink sink{pl, grp_id, &dl, h_rec, plane_rec_b, cb ? d_dens.get() : nullptr, h_dens, -1, &job_failed, &job_failed};
                if (run_passes_impl(pl, c, grp_id, groups, d_store, d_store2, d_rec, d_dens, rec_planes, sink_cb, &sink, st)) return 1;
                if (zd_plan_stats(pl, &me.stats)) return 1;
                return job_failed.load(std::memory_order_acquire) != 0;  // a peer failed: this rank's planes are not a result
            }();
            if (me.rc) abort_all();
        });
    }
    for (auto &t : threads) t.join();
    for (int g = 0; g < G; g++) {  // the communicators themselves are destroyed (or were aborted) by this driver, below / above
        hipSetDevice(ctx[g].device);
        comms[g]->nccl = nullptr;
        zd_comm_destroy(comms[g]);
    }
    if (transport == 2) {
#ifdef ZD_TESTING
        g_rccl_override = nullptr;
        for (auto &q : g_loop.box)
            for (LoopMsg &m : q) {
                if (m.ready) hipEventDestroy(m.ready);
                if (m.done) hipEventDestroy(m.done);
            }
        g_loop.box.clear();
#endif
    } else if (transport != 1)
        for (int g = 0; g < G; g++)
            if (nccls[g] && rccl()->CommDestroy) rccl()->CommDestroy(nccls[g]);
    int rc = 0;
    for (int g = 0; g < G; g++) rc |= ctx[g].rc;
    if (rc) return 1;
    // reductions over the ranks (output.cpp:28-30,190-197): signed value of the largest |displacement|, sum of dens^2
    memset(out, 0, sizeof(*out));
    *out = ctx[0].stats;
    for (int g = 1; g < G; g++) {
        out->density_variance += ctx[g].stats.density_variance;
        for (int j = 0; j < 3; j++) {  // largest |v|; on a tie the record met first in (z, y, x) order (output.cpp:190-193)
            const double a = std::abs(ctx[g].stats.max_disp[j]), b = std::abs(out->max_disp[j]);
            const int64_t ia = ctx[g].stats.max_disp_index[j], ib = out->max_disp_index[j];
            if (a > b || (a == b && a > 0 && ia >= 0 && (ib < 0 || ia < ib))) {
                out->max_disp[j]       = ctx[g].stats.max_disp[j];
                out->max_disp_index[j] = ia;
            }
        }
        for (int k = 0; k < ZD_K_COUNT; k++) {
            out->kernel_ms[k] = std::max(out->kernel_ms[k], ctx[g].stats.kernel_ms[k]);
            out->kernel_launches[k] += ctx[g].stats.kernel_launches[k];
        }
        out->bytes_sent += ctx[g].stats.bytes_sent;
    }
    out->seconds_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return 0;
}
