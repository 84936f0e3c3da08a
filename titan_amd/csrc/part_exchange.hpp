// part_exchange.hpp — the exchange object behind the C-ABI's opaque tgo_exchange (part_exchange.cpp
// holds its two forms), and the host-side helpers that the native loops (part_driver.cpp) and the
// partitioned row load (part_load.cpp) share over it.  Private.
#pragma once
#include <string>
#include <vector>

#include "ctx.hpp"

// Exchange: the four collectives the loops need, all on device buffers, ordered on `s`.
struct tgo_exchange {
    int world = 1, rank = 0;
    virtual ~tgo_exchange() = default;
    // buf holds `world` slices of `bytes` (this rank's at rank * bytes); every rank's slice
    // ends up in every buffer
    virtual int all_gather(void* buf, size_t bytes, hipStream_t s) = 0;
    // send / recv hold `world` blocks of `bytes`: block r of send goes to rank r, block p of
    // recv comes from rank p
    virtual int all_to_all(const void* send, void* recv, size_t bytes, hipStream_t s) = 0;
    // per-peer byte counts and offsets (host arrays of `world`)
    virtual int all_to_allv(const void* send, const size_t* sb, const size_t* so, void* recv, const size_t* rb,
                            const size_t* ro, hipStream_t s) = 0;
    // element-wise reduction over the ranks, in place (op: kRedSum / kRedMin / kRedMax)
    enum { kRedSum = 0, kRedMin = 1, kRedMax = 2 };
    virtual int all_reduce(int64_t* buf, size_t count, int op, hipStream_t s) = 0;
    int all_reduce_sum(int64_t* buf, size_t count, hipStream_t s) { return all_reduce(buf, count, kRedSum, s); }
    // a rank leaving the protocol early releases the peers waiting on it (in-process group)
    virtual void abort() {}
    std::string err;
    // a device-to-device copy on s (what one rank's collective comes to)
    int copy(void* dst, const void* src, size_t bytes, hipStream_t s) {
        if (!bytes || dst == src) return TGO_OK;
        const hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) return TGO_OK;
        err = hipGetErrorString(e);
        return TGO_E_HIP;
    }
    int64_t* pinned = nullptr;      // host counts of the driver (pinned once per exchange)
    int64_t* host_counts() {
        if (!pinned && hipHostMalloc(reinterpret_cast<void**>(&pinned), 8 * sizeof(int64_t), hipHostMallocDefault) != hipSuccess)
            pinned = nullptr;
        return pinned;
    }
    void release_pinned() {
        if (pinned) (void)hipHostFree(pinned);
        pinned = nullptr;
    }
};

namespace tgo {

// One rank's view of a loop: its context, its exchange, and the small transfers and global
// reductions every loop is made of.  An exchange failure never aborts here (the loops abort
// after a failed level); a HIP failure aborts only where hip_aborts says so (the row load).
struct Driver {
    tgo_ctx* ctx = nullptr;
    tgo_exchange* x = nullptr;
    hipStream_t st = nullptr;
    int64_t* dbuf = nullptr;        // device scalars (driver_open's `words`)
    int64_t* hc = nullptr;          // pinned host view (8 words)
    std::string prefix;             // of the HIP failures' messages
    bool hip_aborts = false;
    int xfail(int code) { return fail(ctx, code, "exchange: " + x->err); }
    int hip(const std::string& what) {
        if (hip_aborts) x->abort();
        return fail(ctx, TGO_E_HIP, prefix + what);
    }
    int upload(void* dst, const void* src, size_t bytes, const std::string& what) {
        return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) == hipSuccess ? TGO_OK : hip(what);
    }
    // device to host, and the wait for it (and for everything queued before it)
    int download(void* dst, const void* src, size_t bytes, const std::string& what) {
        if ((bytes && hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st) != hipSuccess) ||
            hipStreamSynchronize(st) != hipSuccess)
            return hip(what);
        return TGO_OK;
    }
    int reduce_device(int64_t* buf, size_t count, int op = tgo_exchange::kRedSum) {
        if (int r = x->all_reduce(buf, count, op, st)) return xfail(r);
        return TGO_OK;
    }
    // out[i] = op over the ranks of vals[i], i < k <= 8, read back through the counter page
    // (one round trip, no stream wait)
    int reduce(const int64_t* vals, int k, int op, int64_t* out) {
        for (int i = 0; i < k; ++i) hc[i] = vals[i];
        if (int rc = upload(dbuf, hc, k * sizeof(int64_t), "reduce upload")) return rc;
        if (int rc = reduce_device(dbuf, static_cast<size_t>(k), op)) return rc;
        return part_read_words(ctx, dbuf, k, out);
    }
    // vals[0, k) reduced in place through the device words buf, copied up and down (one stream
    // wait): any k, and a context that holds no graph yet
    int reduce_copy(int64_t* buf, int64_t* vals, size_t k, int op, const std::string& what) {
        if (int rc = upload(buf, vals, k * sizeof(int64_t), what + " upload")) return rc;
        if (int rc = reduce_device(buf, k, op)) return rc;
        return download(vals, buf, k * sizeof(int64_t), what + " read");
    }
};

// Per-peer byte counts and offsets of an all_to_allv from the peers' element counts; the total bytes.
inline size_t peer_splits(const int64_t* counts, int world, size_t elem_bytes, std::vector<size_t>& sb,
                          std::vector<size_t>& so) {
    sb.resize(world);
    so.resize(world);
    size_t at = 0;
    for (int p = 0; p < world; ++p) {
        sb[p] = static_cast<size_t>(counts[p]) * elem_bytes;
        so[p] = at;
        at += sb[p];
    }
    return at;
}

}  // namespace tgo
