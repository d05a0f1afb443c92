// Host pieces every batched entry point is written against (the batched MSM, the KZG / IPA audit, prove and verify batches, the
// update batch) and the older per-device workspaces share: the workspace registry, the argument refusals, the dynamic-LDS attribute
// set once per device, the block -> owner lists of a work list, the fenced call, and a commitment pass with its follow-up kernel
// under the table's lock.
#pragma once
#include "engine.hpp"
#include <initializer_list>

namespace porla {

// One workspace per device, created on first use and kept for the life of the process.  Ws has a default constructor and an
// `int device`.  The lock is the registry's only: what serialises the use of a workspace is the owner's business.
template <class Ws>
struct PerDevice {
    std::mutex mu;
    std::vector<Ws*> all;
    int get(Ws** out) {
        int dev = 0;
        PORLA_HIP(hipGetDevice(&dev));
        std::lock_guard<std::mutex> lk(mu);
        for (Ws* w : all) if (w->device == dev) { *out = w; return PORLA_OK; }
        Ws* w = new Ws();
        w->device = dev;
        all.push_back(w);
        *out = w;
        return PORLA_OK;
    }
    // every workspace made so far: a walk over all devices works on the copy, outside the registry's lock
    std::vector<Ws*> snapshot() {
        std::lock_guard<std::mutex> lk(mu);
        return all;
    }
};

static inline bool mul_ok(size_t a, size_t b, size_t* out) { return !__builtin_mul_overflow(a, b, out); }

// the refusal of an argument by the entry point `who`
static inline int bad_arg(const char* who, const std::string& what) {
    set_last_error(std::string(who) + ": " + what);
    return PORLA_ERR_ARG;
}

// "n_total must be a power of two, 2 .. 2^max_log": the refusal every batched call over levels of n_total rows makes first
static inline int check_n_total(const char* who, size_t n_total, int max_log) {
    if (n_total >= 2 && (n_total & (n_total - 1)) == 0 && n_total <= ((size_t)1 << max_log)) return PORLA_OK;
    return bad_arg(who, "n_total must be a power of two, 2 .. 2^" + std::to_string(max_log));
}

// "more than 65535 requests in one call": the request is a launch's grid.y, which stops there
static inline int check_request_count(const char* who, size_t k) {
    return k > 0xffffu ? bad_arg(who, "more than 65535 requests in one call") : PORLA_OK;
}

// Dynamic LDS above 64 KiB: a kernel must be told once per device before its first launch.  One static LdsOnce per group of
// kernels that are launched together; set() does its work the first time it is called on a device.
struct LdsKernel { const void* f; size_t bytes; };
template <class F>
static inline LdsKernel lds_kernel(F* kernel, size_t bytes) { return LdsKernel{reinterpret_cast<const void*>(kernel), bytes}; }
struct LdsOnce {
    std::mutex mu;
    std::vector<int> done;
    void set(std::initializer_list<LdsKernel> kernels) {
        int dev = 0;
        const bool known = hipGetDevice(&dev) == hipSuccess;               // (unknown: set them anyway, remember nothing)
        std::lock_guard<std::mutex> lk(mu);
        for (int d : done) if (known && d == dev) return;
        for (const LdsKernel& k : kernels) (void)hipFuncSetAttribute(k.f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.bytes);
        if (known) done.push_back(dev);
    }
};

// block -> owner list of a work list: blocks_of(a) times a, for a = 0 .. k - 1; returns the list's end
template <class BlocksOf>
static inline uint32_t* fill_owner_list(uint32_t* dst, size_t k, BlocksOf blocks_of) {
    for (size_t a = 0; a < k; a++)
        for (uint64_t b = blocks_of(a); b; b--) *dst++ = (uint32_t)a;
    return dst;
}

// One call's use of a workspace (Ws: `mu`, `fence`) whose buffers later calls reuse, possibly on another stream.  The mutex is held
// for the object's life; run() enters the fence on the call's stream BEFORE the enqueue sizes or touches any buffer, and the buffers
// of the call are behind the fence on every exit, a failing one included.
struct FencedCall {
    std::unique_lock<std::mutex> lk;
    UseFence& fence;
    hipStream_t stream;
    template <class Ws>
    FencedCall(Ws* ws, hipStream_t s) : lk(ws->mu), fence(ws->fence), stream(s) {}
    template <class Enqueue>
    int run(Enqueue enqueue) {
        int rc = fence.enter(stream);
        if (rc) return rc;
        rc = enqueue();
        const int rf = fence.leave(stream);
        return rc ? rc : rf;
    }
};

// one commitment pass over n_rows contiguous rows of n_coeffs coefficients, sums left projective in the table's partials, and
// `then(sums, S)` (row r at sums[r S]) enqueued under the table's lock before its fence is recorded again: the partials hold only the
// LAST pass's sums, and another caller's pass may follow as soon as the lock is let go.  The _locked form is for a caller that holds
// fb.mu already (the resident SRS table behind its guard, kzg_state.hpp).
template <class C, class Then>
static int commit_then_locked(FixedBase<C>& fb, const uint8_t* d_rows, size_t n_rows, size_t n_coeffs, hipStream_t stream, Then then) {
    int rc;
    if ((rc = fb.commit_device(d_rows, n_rows, n_coeffs, 32 * n_coeffs, nullptr, stream))) return rc;
    // the table's fence was recorded behind the commit; `then` reads the partials after it, so the fence moves behind `then`
    if ((rc = then((const XYZZ<typename C::Fp>*)fb.partial, fb.last_S))) return rc;
    return fb.fence.leave(stream);
}
template <class C, class Then>
static int commit_then(FixedBase<C>& fb, const uint8_t* d_rows, size_t n_rows, size_t n_coeffs, hipStream_t stream, Then then) {
    std::lock_guard<std::mutex> lk(fb.mu);
    return commit_then_locked(fb, d_rows, n_rows, n_coeffs, stream, then);
}

}  // namespace porla
