// Pieces the batched audits (kzg_audit_batch.hip, ipa_audit_batch.hip) and the batched verifiers (kzg_verify_batch.hip,
// ipa_verify_batch.hip) share.  Device: the gather of challenged store entries into batched-MSM pairs, and the conversion of a lane's
// projective points to affine with one inversion.  Host: the plan of an audit batch.
#pragma once
#include "batch_host.hpp"
#include "fixed_base.hip.h"
#include <cstring>

namespace porla {

constexpr uint32_t KZG_GATHER_PAIRS = 64;          // pairs per block of a gather kernel (four lanes per pair)
constexpr uint32_t AUDIT_BATCH_MAX_MACS = 32768;   // the batched MSM's entry limit (SMALL_MAX_N)
static inline uint64_t gather_blocks(uint64_t n) { return (n + KZG_GATHER_PAIRS - 1) / KZG_GATHER_PAIRS; }

// ---- the host plan of an audit batch (Req: porla_kzg_audit_req or porla_ipa_audit_req, alike in their first 104 bytes)
// The per-request checks of the entry point `who` (`single`: the call that takes what a batch does not); the batch's MSM pairs to *pairs.
template <class Req>
static int audit_batch_check(const char* who, const char* single, const Req* reqs, size_t k, uint64_t* pairs) {
    *pairs = 0;
    for (size_t a = 0; a < k; a++) {
        const Req& R = reqs[a];
        if (R.n64 && (!R.d_rows64 || !R.d_idx64 || !R.d_coef64)) return bad_arg(who, "a NULL 64-byte-row array with n64 > 0");
        if (R.n32 && (!R.d_rows32 || !R.d_idx32 || !R.d_coef32)) return bad_arg(who, "a NULL 32-byte-row array with n32 > 0");
        if (R.n_macs && (!R.d_mac_store || !R.d_align_store || !R.d_mac_idx || !R.d_mac_coef)) return bad_arg(who, "a NULL MAC array with n_macs > 0");
        if (R.n_macs > AUDIT_BATCH_MAX_MACS)
            return bad_arg(who, std::string("n_macs > 32768 (the batched MSM's entry limit; use ") + single + ")");
        if (R.n64 >= (1ull << 32) || R.n32 >= (1ull << 32) || R.n64 + R.n32 >= (1ull << 32)) return bad_arg(who, "n64 + n32 >= 2^32");
        *pairs += 2 * (uint64_t)R.n_macs;
    }
    return PORLA_OK;
}

// The audits as the kernels see them, their share of the row combine (the single call's rule over the batch's total rows) and of the
// MSM gather, and the batched MSM's 2k entries: 2a = audit a's MAC entry, 2a + 1 = its alignment entry.
struct AuditPlan {
    uint32_t per_slice = 0;
    std::vector<KzgAuditDesc> desc;
    std::vector<uint64_t> offsets;
    uint64_t blocks = 0, gblocks = 0, pairs = 0;
    size_t desc_bytes() const { return desc.size() * sizeof(KzgAuditDesc); }
    size_t list_bytes() const { return desc_bytes() + 4 * (size_t)(blocks + gblocks); }
    // descriptors | combine block -> audit | gather block -> audit
    void write(uint8_t* h) const {
        memcpy(h, desc.data(), desc_bytes());
        uint32_t* gl = fill_owner_list((uint32_t*)(h + desc_bytes()), desc.size(), [&](size_t a) { return desc[a].nblk; });
        fill_owner_list(gl, desc.size(), [&](size_t a) { return gather_blocks(desc[a].n_macs); });
    }
};
// z_of(a): the descriptor's z (the KZG opening's point)
template <class Req, class ZOf>
static int audit_batch_plan(const Req* reqs, size_t k, ZOf z_of, AuditPlan* plan) {
    AuditPlan& P = *plan;
    uint64_t rows_total = 0;
    for (size_t a = 0; a < k; a++) rows_total += reqs[a].n64 + reqs[a].n32;
    const uint64_t spb = (uint64_t)AUDIT_BATCH_SLICES * 512;
    uint64_t per_slice64 = (rows_total + spb - 1) / spb;
    if (per_slice64 < 4) per_slice64 = 4;
    if (per_slice64 > 0xffffffffull / AUDIT_BATCH_SLICES) per_slice64 = 0xffffffffull / AUDIT_BATCH_SLICES;
    P.per_slice = (uint32_t)per_slice64;
    const uint32_t per_block = P.per_slice * AUDIT_BATCH_SLICES;
    P.desc.resize(k);
    P.offsets.resize(2 * k + 1);
    for (size_t a = 0; a < k; a++) {
        const Req& R = reqs[a];
        KzgAuditDesc& D = P.desc[a];
        D.rows64 = (const uint8_t*)R.d_rows64; D.idx64 = R.d_idx64; D.coef64 = R.d_coef64;
        D.rows32 = (const uint8_t*)R.d_rows32; D.idx32 = R.d_idx32; D.coef32 = R.d_coef32;
        D.mac_store = (const uint8_t*)R.d_mac_store; D.align_store = (const uint8_t*)R.d_align_store;
        D.mac_idx = R.d_mac_idx; D.mac_coef = R.d_mac_coef;
        D.n64 = (uint32_t)R.n64; D.n32 = (uint32_t)R.n32; D.n_macs = (uint32_t)R.n_macs;
        const uint64_t total = R.n64 + R.n32;
        const uint64_t nb = total ? (total + per_block - 1) / per_block : 1;   // an empty challenge still writes B = 0
        D.blk0 = (uint32_t)P.blocks; D.nblk = (uint32_t)nb;
        D.gat0 = (uint32_t)P.gblocks;
        D.z = z_of(a);
        D.pair0 = P.pairs;
        P.blocks += nb;
        P.gblocks += gather_blocks(R.n_macs);
        P.offsets[2 * a] = P.pairs;
        P.offsets[2 * a + 1] = P.pairs + R.n_macs;
        P.pairs += 2 * (uint64_t)R.n_macs;
    }
    P.offsets[2 * k] = P.pairs;
    if (P.blocks > 0xffffffffull || P.gblocks > 0xffffffffull) { set_last_error("porla: audit batch too large for one call"); return PORLA_ERR_ARG; }
    size_t pt_b;
    if (!mul_ok((size_t)P.pairs, 64, &pt_b)) { set_last_error("porla: audit batch byte size overflows"); return PORLA_ERR_ARG; }
    return PORLA_OK;
}

// The pairs (coef_i, store_a[idx_i]) at pair0 + i and, when TWO, (coef_i, store_b[idx_i]) at pair0 + n + i, for the pairs
// i = 64 blk + threadIdx.x / 4 < n of the calling block; four lanes per pair as k_audit_gather (msm_impl.hip.h), the scalar a 32-byte
// big-endian integer (bn254_scalar_set_int).
template <bool TWO>
__device__ __forceinline__ void kzg_gather_pairs(const uint8_t* store_a, const uint8_t* store_b, const uint64_t* idx, const uint32_t* coef,
                                                 uint32_t n, uint64_t pair0, uint32_t blk, uint8_t* scalars, uint8_t* points) {
    const uint32_t i = blk * KZG_GATHER_PAIRS + (threadIdx.x >> 2), q = threadIdx.x & 3u;
    if (i >= n) return;
    const uint64_t src = idx[i];
    const size_t pa = pair0 + i, pb = pair0 + n + i;
    reinterpret_cast<uint4*>(points + 64 * pa)[q] = reinterpret_cast<const uint4*>(store_a + 64 * src)[q];
    if (TWO) reinterpret_cast<uint4*>(points + 64 * pb)[q] = reinterpret_cast<const uint4*>(store_b + 64 * src)[q];
    if (q < 2) {
        uint4 z = make_uint4(0, 0, 0, 0);
        if (q == 1) z.w = __builtin_bswap32(coef[i]);         // bytes 28..31 of the big-endian scalar
        reinterpret_cast<uint4*>(scalars + 32 * pa)[q] = z;
        if (TWO) reinterpret_cast<uint4*>(scalars + 32 * pb)[q] = z;
    }
}

// N projective points to affine with ONE inversion: Montgomery's trick over their ZZZ, as k_fb_finish does for a lane's rows.
// emit(j, live, x, y) for j = N - 1 .. 0: the plain (non-Montgomery) coordinates of point j, or live = false for infinity
template <class C, int N, class Emit>
__device__ __forceinline__ void xyzz_each_affine_one_inv(const XYZZ<typename C::Fp> (&p)[N], Emit emit) {
    using M = typename C::Fp;
    Fe<M> zzz[N], pre[N];
    bool live[N];
    Fe<M> acc = fe_one<M>();
#pragma unroll
    for (int j = 0; j < N; j++) {
        live[j] = !fe_is_zero<M>(p[j].zzz);
        zzz[j] = live[j] ? p[j].zzz : fe_one<M>();
        pre[j] = acc;
        acc = fe_mul_call<M>(acc, zzz[j]);
    }
    Fe<M> inv;
    if constexpr (C::F30_BUCKETS) inv = fe_inv_safegcd<M>(acc);
    else inv = fe_inv_dev<M>(acc);
    Fe<M> one = fe_zero<M>();
    one.v[0] = 1;
#pragma unroll
    for (int j = N - 1; j >= 0; j--) {
        const Fe<M> inv_j = fe_mul_call<M>(inv, pre[j]);
        inv = fe_mul_call<M>(inv, zzz[j]);
        if (!live[j]) {
            emit(j, false, one, one);
            continue;
        }
        const Affine<M> af = xyzz_to_affine_with_inv<M>(p[j], inv_j);
        const Fe<M> x = fe_mul_call<M>(af.x, one), y = fe_mul_call<M>(af.y, one);   // out of Montgomery form
        emit(j, true, x, y);
    }
}

// ... to 64-byte big-endian affine at base + at[j] (64 zero bytes = infinity)
template <class C, int N>
__device__ __forceinline__ void xyzz_to_be_one_inv(const XYZZ<typename C::Fp> (&p)[N], uint8_t* base, const uint32_t (&at)[N]) {
    using M = typename C::Fp;
    xyzz_each_affine_one_inv<C, N>(p, [&](int j, bool live, const Fe<M>& x, const Fe<M>& y) {
        uint8_t* dst = base + at[j];
        if (!live) {
            const uint4 z = make_uint4(0, 0, 0, 0);
            uint4* q = reinterpret_cast<uint4*>(dst);
            q[0] = z; q[1] = z; q[2] = z; q[3] = z;
            return;
        }
        store_be256(dst, x.v);
        store_be256(dst + 32, y.v);
    });
}

}  // namespace porla
