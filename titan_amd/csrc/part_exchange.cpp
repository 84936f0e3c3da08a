// part_exchange.cpp — the two forms of the exchange object (part_exchange.hpp) that the native
// partitioned loops and the partitioned row load issue their collectives through:
//   * tgo_exchange_rccl_*  : RCCL over xGMI on the ctx stream (production, one process per GPU);
//   * tgo_exchange_local_group : ranks as threads of one process on one device (tests: the
//     same loops at world 2 / 4 on a one-GPU box), collectives as device-to-device copies
//     between the ranks' buffers at a barrier.
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include "part_exchange.hpp"

namespace {

// ------------------------------------------------------------------ RCCL (production)
struct RcclExchange : tgo_exchange {
    ncclComm_t comm = nullptr;
    bool aborted = false;
    ~RcclExchange() override {
        if (comm) (void)ncclCommDestroy(comm);
        release_pinned();
    }
    // A rank that fails between collectives (a local step's error, a HIP error) aborts its own
    // communicator and refuses further use here, so it returns the error at once instead of
    // entering another collective.  ncclCommAbort does NOT notify the peers: a peer already
    // in, or about to enter, a collective with this rank waits until its launcher ends it.
    // One process per GPU under torch.distributed.run provides that: the failed rank exits
    // with an error and the launcher terminates the rest of the group.
    void abort() override {
        if (comm) (void)ncclCommAbort(comm);
        comm = nullptr;
        aborted = true;
    }
    int check(ncclResult_t r, const char* what) {
        if (r == ncclSuccess) return TGO_OK;
        err = std::string(what) + ": " + ncclGetErrorString(r);
        return TGO_E_HIP;
    }
    bool usable() {
        if (!aborted) return true;
        err = "RCCL exchange aborted by an earlier failure";
        return false;
    }
    int all_gather(void* buf, size_t bytes, hipStream_t s) override {
        if (!usable()) return TGO_E_COMM;
        if (world == 1) return TGO_OK;
        char* b = static_cast<char*>(buf);
        return check(ncclAllGather(b + rank * bytes, b, bytes, ncclChar, comm, s), "ncclAllGather");
    }
    int all_to_all(const void* send, void* recv, size_t bytes, hipStream_t s) override {
        if (!usable()) return TGO_E_COMM;
        if (world == 1) return copy(recv, send, bytes, s);
        return check(ncclAllToAll(send, recv, bytes, ncclChar, comm, s), "ncclAllToAll");
    }
    int all_to_allv(const void* send, const size_t* sb, const size_t* so, void* recv, const size_t* rb,
                    const size_t* ro, hipStream_t s) override {
        if (!usable()) return TGO_E_COMM;
        if (world == 1) return copy(static_cast<char*>(recv) + ro[0], static_cast<const char*>(send) + so[0], sb[0], s);
        int rc = check(ncclGroupStart(), "ncclGroupStart");
        for (int p = 0; !rc && p < world; ++p) {
            if (sb[p]) rc = check(ncclSend(static_cast<const char*>(send) + so[p], sb[p], ncclChar, p, comm, s), "ncclSend");
            if (!rc && rb[p]) rc = check(ncclRecv(static_cast<char*>(recv) + ro[p], rb[p], ncclChar, p, comm, s), "ncclRecv");
        }
        const int rc2 = check(ncclGroupEnd(), "ncclGroupEnd");
        return rc ? rc : rc2;
    }
    int all_reduce(int64_t* buf, size_t count, int op, hipStream_t s) override {
        if (!usable()) return TGO_E_COMM;
        if (world == 1) return TGO_OK;
        const ncclRedOp_t o = op == kRedMin ? ncclMin : op == kRedMax ? ncclMax : ncclSum;
        return check(ncclAllReduce(buf, buf, count, ncclInt64, o, comm, s), "ncclAllReduce");
    }
};

// ------------------------------------------------------------------ in-process group (tests)
// Ranks are threads of one process; a collective is: finish the own stream, publish the
// buffer pointers, barrier, copy what this rank needs from the peers' buffers (device to
// device, own stream), finish, barrier (the peers' buffers may be reused afterwards).
struct LocalGroup {
    int world;
    std::mutex mu;
    std::condition_variable cv;
    int arrived = 0;
    long generation = 0;
    bool broken = false;
    struct Slot { const void* send; void* recv; const size_t* sb; const size_t* so; std::vector<int64_t> red; };
    std::vector<Slot> slot;
    explicit LocalGroup(int w) : world(w), slot(w) {}
    bool barrier() {
        std::unique_lock<std::mutex> lk(mu);
        if (broken) return false;
        const long gen = generation;
        if (++arrived == world) {
            arrived = 0;
            ++generation;
            cv.notify_all();
            return true;
        }
        const bool ok = cv.wait_for(lk, std::chrono::seconds(60), [&] { return generation != gen || broken; });
        if (!ok || broken) { broken = true; cv.notify_all(); return false; }
        return true;
    }
};

struct LocalExchange : tgo_exchange {
    std::shared_ptr<LocalGroup> g;
    ~LocalExchange() override { release_pinned(); }
    void abort() override {
        std::lock_guard<std::mutex> lk(g->mu);
        g->broken = true;
        g->cv.notify_all();
    }
    int fail_msg(const char* m) { err = m; return TGO_E_STATE; }
    int sync(hipStream_t s) {
        const hipError_t e = hipStreamSynchronize(s);
        if (e == hipSuccess) return TGO_OK;
        err = hipGetErrorString(e);
        return TGO_E_HIP;
    }
    template <class F>
    int collective(hipStream_t s, const LocalGroup::Slot& mine, F&& body) {
        int rc = sync(s);
        g->slot[rank] = mine;
        if (!g->barrier()) return fail_msg("local exchange: a rank failed or timed out");
        if (!rc) rc = body();
        if (!rc) rc = sync(s);
        if (!g->barrier()) return fail_msg("local exchange: a rank failed or timed out");
        return rc;
    }
    int all_gather(void* buf, size_t bytes, hipStream_t s) override {
        if (world == 1) return TGO_OK;                      // one rank: nothing to exchange (as RCCL)
        return collective(s, {buf, buf, nullptr, nullptr, {}}, [&]() -> int {
            for (int p = 0; p < world; ++p)
                if (p != rank) {
                    const char* src = static_cast<const char*>(g->slot[p].recv) + p * bytes;
                    if (int rc = copy(static_cast<char*>(buf) + p * bytes, src, bytes, s)) return rc;
                }
            return TGO_OK;
        });
    }
    int all_to_all(const void* send, void* recv, size_t bytes, hipStream_t s) override {
        if (world == 1) return copy(recv, send, bytes, s);
        return collective(s, {send, recv, nullptr, nullptr, {}}, [&]() -> int {
            for (int p = 0; p < world; ++p) {
                const char* src = static_cast<const char*>(g->slot[p].send) + rank * bytes;
                if (int rc = copy(static_cast<char*>(recv) + p * bytes, src, bytes, s)) return rc;
            }
            return TGO_OK;
        });
    }
    int all_to_allv(const void* send, const size_t* sb, const size_t* so, void* recv, const size_t* rb,
                    const size_t* ro, hipStream_t s) override {
        if (world == 1) {
            if (sb[0] != rb[0]) return fail_msg("local exchange: all_to_allv sizes do not match");
            return copy(static_cast<char*>(recv) + ro[0], static_cast<const char*>(send) + so[0], rb[0], s);
        }
        return collective(s, {send, recv, sb, so, {}}, [&]() -> int {
            for (int p = 0; p < world; ++p) {
                const LocalGroup::Slot& q = g->slot[p];
                if (q.sb[rank] != rb[p]) return fail_msg("local exchange: all_to_allv sizes do not match");
                const char* src = static_cast<const char*>(q.send) + q.so[rank];
                if (int rc = copy(static_cast<char*>(recv) + ro[p], src, rb[p], s)) return rc;
            }
            return TGO_OK;
        });
    }
    int all_reduce(int64_t* buf, size_t count, int op, hipStream_t s) override {
        if (world == 1) return TGO_OK;
        std::vector<int64_t> mine(count);
        int rc = sync(s);
        if (!rc) {
            const hipError_t e = hipMemcpy(mine.data(), buf, count * sizeof(int64_t), hipMemcpyDeviceToHost);
            if (e != hipSuccess) { err = hipGetErrorString(e); rc = TGO_E_HIP; }
        }
        g->slot[rank] = {nullptr, nullptr, nullptr, nullptr, mine};
        if (!g->barrier()) return fail_msg("local exchange: a rank failed or timed out");
        std::vector<int64_t> sum(mine);
        for (int p = 0; p < world; ++p) {
            if (p == rank) continue;
            for (size_t i = 0; i < count && i < g->slot[p].red.size(); ++i) {
                const int64_t v = g->slot[p].red[i];
                sum[i] = op == kRedMin ? std::min(sum[i], v) : op == kRedMax ? std::max(sum[i], v) : sum[i] + v;
            }
        }
        if (!g->barrier()) return fail_msg("local exchange: a rank failed or timed out");
        if (rc) return rc;
        const hipError_t e = hipMemcpyAsync(buf, sum.data(), count * sizeof(int64_t), hipMemcpyHostToDevice, s);
        if (e != hipSuccess) { err = hipGetErrorString(e); return TGO_E_HIP; }
        return sync(s);          // sum is a local: the copy must finish before it goes away
    }
};

}  // namespace

extern "C" {

int tgo_exchange_rccl_id(uint8_t* id_out) {
    if (!id_out) return TGO_E_INVALID;
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return TGO_E_HIP;
    std::memcpy(id_out, &id, sizeof(id));
    return TGO_OK;
}

int tgo_exchange_rccl_create(int32_t world, int32_t rank, const uint8_t* id, int32_t device, tgo_exchange** out) {
    if (!id || !out || world < 1 || rank < 0 || rank >= world) return TGO_E_INVALID;
    *out = nullptr;
    if (hipSetDevice(device) != hipSuccess) return TGO_E_HIP;
    auto x = std::make_unique<RcclExchange>();
    x->world = world;
    x->rank = rank;
    ncclUniqueId uid;
    std::memcpy(&uid, id, sizeof(uid));
    if (ncclCommInitRank(&x->comm, world, uid, rank) != ncclSuccess) return TGO_E_HIP;
    *out = x.release();
    return TGO_OK;
}

int tgo_exchange_local_group(int32_t world, tgo_exchange** ranks_out) {
    if (!ranks_out || world < 1 || world > 64) return TGO_E_INVALID;
    auto g = std::make_shared<LocalGroup>(world);
    for (int r = 0; r < world; ++r) {
        auto* x = new LocalExchange();
        x->world = world;
        x->rank = r;
        x->g = g;
        ranks_out[r] = x;
    }
    return TGO_OK;
}

void tgo_exchange_destroy(tgo_exchange* x) { delete x; }

const char* tgo_exchange_last_error(const tgo_exchange* x) { return x ? x->err.c_str() : "null exchange"; }

}  // extern "C"
