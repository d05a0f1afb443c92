// Client::audit's check (KZG build) of K replies in ONE call (include/porla_gpu.h:porla_kzg_verify_batch_device): the auditor that
// checks the replies porla_kzg_audit_batch_device produced (porla/Client/Client.hpp:633-880).  Per reply the reference runs an MSM
// over the challenged MAC complements, two variable-base multiplications by alpha, two additions and a compare (the MAC check), and
// verify_proof's host pairing (the opening).  Here each MAC check is one batched-MSM entry that sums to infinity iff it holds,
//   sum_j coef_j comp[idx_j] + alpha C - alpha A - M = O          (the complements, then the 3-pair entry)
// and the K openings are weighted with secret random 128-bit scalars w_k and folded into ONE check of verify_proof's form,
//   e(P, G2) * e(-Q, tau G2) = 1,   P = sum w_k (C_k - y_k G + z_k H_k),   Q = sum w_k H_k.
// One fixed sequence of launches per call on the caller's stream:
//
//   upload               one copy of the host-built work list (reply descriptors, G, gather blocks) from pinned memory
//   k_kzg_verify_prep    a lane per reply: validate its four points, z and y mod r, w z and -w y; its 3-pair entry
//                        (alpha, C), (r - alpha, A), (r - 1, M) and its pairs of P: (w, C), (w z, H), (-w y, G) and of Q: (w, H)
//   k_kzg_verify_gather  the complement entries (coef_j, comp[idx_j]) (kzg_batch.hip.h, as the audit batch gathers its MACs)
//   batch_*              the batched MSM over the 2K + 2 entries (msm_batch_impl.hip.h), projective sums kept
//   k_kzg_verify_join    a lane per reply: complement sum + 3-pair sum = O ? -> FULL; one more lane: P and Q to affine with one inversion
//   copy back            P | Q | K flag bytes, then ONE host pairing; only when it fails, verify_proof's predicate per reply
#include "kzg_state.hpp"
#include "icc.hip.h"
#include "kzg_batch.hip.h"
#include "../../include/porla_gpu.h"

#include <sys/random.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstddef>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

namespace porla {

constexpr size_t KZG_VERIFY_RECORD = PORLA_KZG_AUDIT_RECORD_BYTES;
constexpr uint32_t KZG_VERIFY_MAX_N = 32768;          // the batched MSM's entry limit (SMALL_MAX_N)
constexpr uint32_t KZG_VERIFY_THREADS = 16;           // host threads of the per-reply fallback

// One reply as the device kernels see it: the client's arrays, its complement entry at pairs [pair0, pair0 + n) with its 3-pair MAC
// entry right behind, alpha mod r and r - alpha, and its weight (plain little-endian limbs, w < 2^128).
struct KzgVerifyDesc {
    const uint8_t* comp_store; const uint64_t* idx; const uint32_t* coef;
    uint32_t n, gat0;                 // gat0: the reply's first block of the gather
    unsigned long long pair0;
    uint32_t alpha[8], nalpha[8], w[8];
};
static_assert(sizeof(KzgVerifyDesc) == 136, "KzgVerifyDesc: 24 bytes of pointers, 8 of counts, pair0, three scalars");

// a 64-byte big-endian affine G1 point: both coordinates < p, and on y^2 = x^3 + 3 or 64 zero bytes (infinity); the cofactor is 1
__device__ __forceinline__ bool g1_well_formed(const uint8_t* b) {
    using M = Bn254Fp;
    Fe<M> x, y;
    load_be256(x.v, b);
    load_be256(y.v, b + 32);
    uint32_t s[8];
    if (!sub_p<M>(s, x.v) || !sub_p<M>(s, y.v)) return false;           // sub_p borrows iff the coordinate is < p
    if (fe_is_zero<M>(x) && fe_is_zero<M>(y)) return true;
    const Fe<M> xm = fe_to_mont<M>(x), ym = fe_to_mont<M>(y);
    const Fe<M> three = fe_add<M>(fe_dbl<M>(fe_one<M>()), fe_one<M>());
    return fe_eq<M>(fe_mul_call<M>(ym, ym), fe_add<M>(fe_mul_call<M>(fe_mul_call<M>(xm, xm), xm), three));
}

// ---- a lane per reply.  The scalars are plain residues mod r (IccBn254Fr: q = r): z and y reduced as verify_proof's SetBytes does,
// w z and -w y as Montgomery products of w R with a plain value.  A malformed record gets zero scalars and points at infinity in all
// its pairs, so that it adds nothing to any sum, and its flag MALFORMED (the join leaves it so).
__global__ void __launch_bounds__(64)
k_kzg_verify_prep(const KzgVerifyDesc* __restrict__ desc, uint32_t k, const uint8_t* __restrict__ records, const uint8_t* __restrict__ g_be,
                  unsigned long long p0, unsigned long long q0, uint8_t* __restrict__ scalars, uint8_t* __restrict__ points,
                  uint8_t* __restrict__ flags) {
    using Q = IccBn254Fr;
    const uint32_t a = blockIdx.x * 64 + threadIdx.x;
    if (a >= k) return;
    const KzgVerifyDesc& D = desc[a];
    const uint8_t* rec = records + (size_t)a * KZG_VERIFY_RECORD;
    const bool ok = g1_well_formed(rec) && g1_well_formed(rec + 64) && g1_well_formed(rec + 192) && g1_well_formed(rec + 256);
    Fe<Q> z, y, w, m1;
    load_be256(z.v, rec + 128);
    load_be256(y.v, rec + 160);
    fe_reduce_plain<Q>(z.v, Q::MAX_Q_IN);
    fe_reduce_plain<Q>(y.v, Q::MAX_Q_IN);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        w.v[i] = D.w[i];
        m1.v[i] = Q::P[i];
    }
    m1.v[0] -= 1;                                                       // r - 1
    const Fe<Q> wM = fe_to_mont<Q>(w);
    const Fe<Q> wz = fe_mul<Q>(wM, z), nwy = fe_neg<Q>(fe_mul<Q>(wM, y));
    auto pair = [&](unsigned long long i, const uint32_t* s, const uint8_t* pt) {
        const uint4 zero = make_uint4(0, 0, 0, 0);
        uint4* pd = reinterpret_cast<uint4*>(points + 64 * i);
        if (ok) {
            store_be256(scalars + 32 * i, s);
            const uint4* ps = reinterpret_cast<const uint4*>(pt);
            pd[0] = ps[0]; pd[1] = ps[1]; pd[2] = ps[2]; pd[3] = ps[3];
        } else {
            uint4* sd = reinterpret_cast<uint4*>(scalars + 32 * i);
            sd[0] = zero; sd[1] = zero;
            pd[0] = zero; pd[1] = zero; pd[2] = zero; pd[3] = zero;
        }
    };
    const unsigned long long t = D.pair0 + D.n;
    pair(t, D.alpha, rec);                                              // (alpha, C)
    pair(t + 1, D.nalpha, rec + 256);                                   // (r - alpha, A)
    pair(t + 2, m1.v, rec + 192);                                       // (r - 1, M)
    pair(p0 + 3ull * a, w.v, rec);                                      // (w, C)
    pair(p0 + 3ull * a + 1, wz.v, rec + 64);                            // (w z, H)
    pair(p0 + 3ull * a + 2, nwy.v, g_be);                               // (-w y, G)
    pair(q0 + a, w.v, rec + 64);                                        // (w, H)
    flags[a] = ok ? 0 : PORLA_KZG_VERIFY_MALFORMED;
}

// ---- the complement entries.  Block b covers pairs [64 (b - gat0), ...) of reply gat_reply[b].
__global__ void __launch_bounds__(4 * KZG_GATHER_PAIRS)
k_kzg_verify_gather(const KzgVerifyDesc* __restrict__ desc, const uint32_t* __restrict__ gat_reply, uint8_t* __restrict__ scalars,
                    uint8_t* __restrict__ points) {
    const KzgVerifyDesc& D = desc[gat_reply[blockIdx.x]];
    kzg_gather_pairs<false>(D.comp_store, nullptr, D.idx, D.coef, D.n, D.pair0, blockIdx.x - D.gat0, scalars, points);
}

// ---- lane a < k: the reply's MAC check, sums[2a] + sums[2a + 1] = O, into its flag (out[128 + a]) unless it is malformed; lane k:
// P = sums[2k] and Q = sums[2k + 1] to 64-byte big-endian affine at out[0, 128) with one inversion.
__global__ void __launch_bounds__(64)
k_kzg_verify_join(const XYZZ<Bn254Fp>* __restrict__ sums, uint32_t k, uint8_t* __restrict__ out) {
    using C = Bn254G1;
    using M = Bn254Fp;
    const uint32_t a = blockIdx.x * 64 + threadIdx.x;
    if (a < k) {
        XYZZ<M> s = load_xyzz<M>(sums + 2 * (size_t)a);
        const XYZZ<M> t = load_xyzz<M>(sums + 2 * (size_t)a + 1);
        xyzz_add_cold<M>(&s, &t);
        uint8_t* f = out + 128 + a;
        if (*f == 0) *f = fe_is_zero<M>(s.zzz) ? PORLA_KZG_VERIFY_FULL : 0;
    } else if (a == k) {
        const XYZZ<M> pq[2] = {load_xyzz<M>(sums + 2 * (size_t)k), load_xyzz<M>(sums + 2 * (size_t)k + 1)};
        constexpr uint32_t at[2] = {0, 64};
        xyzz_to_be_one_inv<C, 2>(pq, out, at);
    }
}

// ---- per-device workspace: the work list (pinned staging + device copy), the MSM entries and sums, the results (device + pinned).
// One call at a time enqueues and waits for its results (mu); `fence` orders the buffers between calls on different streams.  The
// call waits for its own copy back, so the staging buffer's upload is done whenever mu is free.
struct KzgVerifyBatchWs {
    std::mutex mu;
    int device = -1;
    Buf list, msm_sc, msm_pt, msm_sums, out;
    PinnedList h_list;
    void* h_out = nullptr;
    size_t h_out_cap = 0;
    hipEvent_t done = nullptr;
    UseFence fence;
};
static PerDevice<KzgVerifyBatchWs> g_kvb_ws;

// ws->mu held, ws->fence entered: everything up to the copy back of P | Q | flags into ws->h_out, then ws->done recorded
static int verify_batch_enqueue(KzgVerifyBatchWs* ws, const porla_kzg_verify_req* reqs, size_t k, const uint8_t* d_records,
                                const uint8_t* weights, const uint8_t g_be[64], hipStream_t stream) {
    int rc;
    // ---- the plan: entry 2a = reply a's complements, 2a + 1 = its 3-pair MAC entry, 2k = P (3 pairs per reply), 2k + 1 = Q
    std::vector<KzgVerifyDesc> desc(k);
    std::vector<uint64_t> offsets(2 * k + 3);
    uint64_t gblocks = 0, pairs = 0;
    for (size_t a = 0; a < k; a++) {
        const porla_kzg_verify_req& R = reqs[a];
        KzgVerifyDesc& D = desc[a];
        D.comp_store = (const uint8_t*)R.d_comp_store; D.idx = R.d_idx; D.coef = R.d_coef;
        D.n = (uint32_t)R.n;
        D.gat0 = (uint32_t)gblocks;
        D.pair0 = pairs;
        const Fe<Bn254Fr> al = h_fe_from_be_var<Bn254Fr>(R.alpha, 32);  // mult_point's reduction of the scalar
        h_fe_to_plain<Bn254Fr>(D.alpha, al);
        h_fe_to_plain<Bn254Fr>(D.nalpha, fe_neg<Bn254Fr>(al));
        uint8_t wb[32] = {0};
        memcpy(wb + 16, weights + 16 * a, 16);
        h_load_be(D.w, wb);
        offsets[2 * a] = pairs;
        offsets[2 * a + 1] = pairs + R.n;
        pairs += R.n + 3;
        gblocks += gather_blocks(R.n);
    }
    const uint64_t p0 = pairs, q0 = p0 + 3 * (uint64_t)k;
    offsets[2 * k] = p0;
    offsets[2 * k + 1] = q0;
    offsets[2 * k + 2] = q0 + k;
    pairs = q0 + k;
    // ---- the work list: descriptors | G | gather block -> reply, one pinned buffer, one copy
    const size_t desc_b = (k * sizeof(KzgVerifyDesc) + 63) & ~(size_t)63;    // G 16-byte aligned for its uint4 loads
    const size_t list_b = desc_b + 64 + 4 * (size_t)gblocks;
    const size_t out_b = 128 + k;
    if ((rc = ws->h_list.stage(list_b))) return rc;
    if (ws->h_out_cap < out_b) {           // read only after this call's own `done`
        if (ws->h_out) PORLA_HIP(hipHostFree(ws->h_out));
        ws->h_out = nullptr;
        ws->h_out_cap = 0;
        PORLA_HIP(hipHostMalloc(&ws->h_out, out_b + out_b / 4 + 4096, hipHostMallocDefault));
        ws->h_out_cap = out_b + out_b / 4 + 4096;
    }
    {
        uint8_t* h = (uint8_t*)ws->h_list.h;
        memcpy(h, desc.data(), k * sizeof(KzgVerifyDesc));
        memcpy(h + desc_b, g_be, 64);
        fill_owner_list((uint32_t*)(h + desc_b + 64), k, [&](size_t a) { return gather_blocks(desc[a].n); });
    }
    if ((rc = ws->list.ensure(list_b))) return rc;
    if ((rc = ws->msm_sc.ensure((size_t)pairs * 32 + 64))) return rc;
    if ((rc = ws->msm_pt.ensure((size_t)pairs * 64 + 64))) return rc;
    if ((rc = ws->msm_sums.ensure((2 * k + 2) * sizeof(XYZZ<Bn254Fp>)))) return rc;
    if ((rc = ws->out.ensure(out_b))) return rc;
    if (!ws->done) PORLA_HIP(hipEventCreateWithFlags(&ws->done, hipEventDisableTiming));
    if ((rc = ws->h_list.send(ws->list.p, list_b, stream))) return rc;
    const KzgVerifyDesc* d_desc = (const KzgVerifyDesc*)ws->list.p;
    const uint8_t* d_g = (const uint8_t*)ws->list.p + desc_b;
    const uint32_t* d_gat = (const uint32_t*)(d_g + 64);
    uint8_t* sc = (uint8_t*)ws->msm_sc.p;
    uint8_t* pt = (uint8_t*)ws->msm_pt.p;
    uint8_t* d_out = (uint8_t*)ws->out.p;
    {
        ProfScope ps("kzg_verify_prep", stream);
        hipLaunchKernelGGL(k_kzg_verify_prep, dim3((unsigned)((k + 63) / 64)), dim3(64), 0, stream, d_desc, (uint32_t)k, d_records, d_g,
                           (unsigned long long)p0, (unsigned long long)q0, sc, pt, d_out + 128);
        PORLA_HIP(hipGetLastError());
    }
    if (gblocks) {
        ProfScope ps("kzg_verify_gather", stream);
        hipLaunchKernelGGL(k_kzg_verify_gather, dim3((unsigned)gblocks), dim3(4 * KZG_GATHER_PAIRS), 0, stream, d_desc, d_gat, sc, pt);
        PORLA_HIP(hipGetLastError());
    }
    XYZZ<Bn254Fp>* sums = (XYZZ<Bn254Fp>*)ws->msm_sums.p;
    if ((rc = msm_batch_sums_device<Bn254G1>(sc, pt, offsets.data(), 2 * k + 2, sums, stream))) return rc;
    {
        ProfScope ps("kzg_verify_join", stream);
        hipLaunchKernelGGL(k_kzg_verify_join, dim3((unsigned)((k + 1 + 63) / 64)), dim3(64), 0, stream, (const XYZZ<Bn254Fp>*)sums,
                           (uint32_t)k, d_out);
        PORLA_HIP(hipGetLastError());
    }
    PORLA_HIP(hipMemcpyAsync(ws->h_out, d_out, out_b, hipMemcpyDeviceToHost, stream));
    PORLA_HIP(hipEventRecord(ws->done, stream));
    return PORLA_OK;
}

// k x 16 bytes from the operating system's random source, every weight nonzero
static int draw_weights(uint8_t* w, size_t k) {
    size_t got = 0;
    while (got < 16 * k) {
        const ssize_t r = getrandom(w + got, 16 * k - got, 0);
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) { set_last_error("porla_kzg_verify_batch_device: getrandom failed"); return PORLA_ERR_STATE; }
        got += (size_t)r;
    }
    for (size_t a = 0; a < k; a++) {
        uint8_t* x = w + 16 * a;
        while (std::all_of(x, x + 16, [](uint8_t b) { return b == 0; }))
            if (getrandom(x, 16, 0) != 16) { set_last_error("porla_kzg_verify_batch_device: getrandom failed"); return PORLA_ERR_STATE; }
    }
    return PORLA_OK;
}

}  // namespace porla

using namespace porla;

static_assert(sizeof(porla_kzg_verify_req) == PORLA_KZG_VERIFY_REQ_BYTES, "porla_kzg_verify_req size");
static_assert(offsetof(porla_kzg_verify_req, d_comp_store) == 0 && offsetof(porla_kzg_verify_req, d_idx) == 8 &&
              offsetof(porla_kzg_verify_req, d_coef) == 16 && offsetof(porla_kzg_verify_req, n) == 24 &&
              offsetof(porla_kzg_verify_req, alpha) == 32,
              "porla_kzg_verify_req offsets (include/porla_gpu.h)");
static_assert(3 * PORLA_KZG_VERIFY_MAX_K <= KZG_VERIFY_MAX_N && 3 * (PORLA_KZG_VERIFY_MAX_K + 1) > KZG_VERIFY_MAX_N,
              "PORLA_KZG_VERIFY_MAX_K: the folded entry P holds 3 pairs per reply");

extern "C" int porla_kzg_verify_batch_device(const porla_kzg_verify_req* reqs, size_t k, const void* d_records, const uint8_t* weights,
                                             uint8_t* status, void* hip_stream) {
    static const char* who = "porla_kzg_verify_batch_device";
    if (k && (!reqs || !d_records || !status)) return bad_arg(who, "reqs, d_records or status is NULL");
    if (k > PORLA_KZG_VERIFY_MAX_K) return bad_arg(who, "k > 10922 (the folded entry P holds 3 pairs per reply, at most 32768): split the batch");
    uint64_t pairs = 4 * (uint64_t)k;
    for (size_t a = 0; a < k; a++) {
        const porla_kzg_verify_req& R = reqs[a];
        if (R.n && (!R.d_comp_store || !R.d_idx || !R.d_coef)) return bad_arg(who, "a NULL complement or challenge array with n > 0");
        if (R.n > KZG_VERIFY_MAX_N) return bad_arg(who, "n > 32768 (the batched MSM's entry limit)");
        pairs += R.n + 3;
        if (weights && std::all_of(weights + 16 * a, weights + 16 * a + 16, [](uint8_t b) { return b == 0; }))
            return bad_arg(who, "an all-zero weight");
    }
    size_t bytes;
    if (!mul_ok((size_t)pairs, 96, &bytes) || !mul_ok(k, KZG_VERIFY_RECORD, &bytes)) return bad_arg(who, "the batch's byte size overflows");
    if (k == 0) return PORLA_OK;
    int rc = ensure_device();
    if (rc) return rc;
    uint8_t g_be[64];
    if ((rc = kzg_verify_base(g_be))) return rc;
    std::vector<uint8_t> drawn;
    if (!weights) {
        drawn.resize(16 * k);
        if ((rc = draw_weights(drawn.data(), k))) return rc;
        weights = drawn.data();
    }
    KzgVerifyBatchWs* ws = nullptr;
    if ((rc = g_kvb_ws.get(&ws))) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    uint8_t pq[128];
    {
        FencedCall call(ws, stream);       // mu stays held for the wait: h_out and `done` are the workspace's
        if ((rc = call.run([&] { return verify_batch_enqueue(ws, reqs, k, (const uint8_t*)d_records, weights, g_be, stream); }))) return rc;
        PORLA_HIP(hipEventSynchronize(ws->done));
        memcpy(pq, ws->h_out, 128);
        memcpy(status, (const uint8_t*)ws->h_out + 128, k);
    }
    if (kzg_folded_opening_holds(pq, pq + 64)) {
        for (size_t a = 0; a < k; a++)
            if (!(status[a] & PORLA_KZG_VERIFY_MALFORMED)) status[a] |= PORLA_KZG_VERIFY_PROOF;
        return PORLA_OK;
    }
    // ---- the folded check failed: verify_proof's predicate on every well-formed reply, on up to 16 host threads
    std::vector<uint8_t> recs(k * KZG_VERIFY_RECORD);
    PORLA_HIP(hipMemcpyAsync(recs.data(), d_records, recs.size(), hipMemcpyDeviceToHost, stream));
    PORLA_HIP(hipStreamSynchronize(stream));
    std::vector<size_t> todo;
    for (size_t a = 0; a < k; a++)
        if (!(status[a] & PORLA_KZG_VERIFY_MALFORMED)) todo.push_back(a);
    std::atomic<size_t> next{0};
    auto work = [&] {
        for (size_t i; (i = next.fetch_add(1)) < todo.size();)
            if (kzg_opening_holds(recs.data() + todo[i] * KZG_VERIFY_RECORD)) status[todo[i]] |= PORLA_KZG_VERIFY_PROOF;
    };
    const size_t hw = std::max<size_t>(1, std::thread::hardware_concurrency());
    const size_t nt = std::min<size_t>({(size_t)KZG_VERIFY_THREADS, hw, todo.size()});
    std::vector<std::thread> pool;
    for (size_t t = 1; t < nt; t++) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
    return PORLA_OK;
}
