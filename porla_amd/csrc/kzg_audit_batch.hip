// Server::audit (KZG build) for K independent audits in ONE asynchronous call (include/porla_gpu.h:porla_kzg_audit_batch_device):
// the server that audits many files or clients, each audit an MSM pair over its challenged MACs plus a row combine and a proof
// (porla/Server/Server.hpp:564-931).  porla_kzg_audit_device runs one audit at a time and waits on the host twice; here every step
// of every audit is on the device and on the caller's stream, one fixed sequence of launches per call:
//
//   upload                one copy of the host-built work list (audit descriptors, combine blocks, gather blocks) from pinned memory
//   audit_batch_*         the row combine of all K audits (audit.hip: the blocks of k_audit_accumulate / k_audit_finish from a work
//                         list): alignment scalars c_k and B_k (big-endian, mod p_icc) into the commit rows [c_k, B_k, h_k]
//   k_kzg_open            a wave per audit: y = B(z) and the quotient h (create_proof's Horner pass and synthetic division,
//                         kzg_abi.hip:kzg_open_rows) into the commit row h_k; point and claim into the record
//   k_kzg_audit_gather    the 2K MSM entries (coef_i, MAC[idx_i]) and (coef_i, align[idx_i])
//   batch_*               the batched MSM over the 2K entries (msm_batch_impl.hip.h), projective sums kept
//   fb_commit / fb_fold   ONE commitment pass over the 3K rows against the resident SRS table, projective sums kept
//   k_kzg_audit_join      per audit: align_value + MSM(align) (align_MAC, Server.hpp:903), the four points of the record to affine
//                         with one inversion, the 320-byte record
#include "kzg_state.hpp"
#include "icc.hip.h"
#include "kzg_batch.hip.h"
#include "../../include/porla_gpu.h"

#include <cstddef>
#include <mutex>
#include <vector>

namespace porla {

constexpr size_t KZG_AUDIT_RECORD = PORLA_KZG_AUDIT_RECORD_BYTES;
constexpr uint32_t KZG_OPEN_WAVES = 4;             // audits per block of k_kzg_open

// ---- the KZG opening, a wave per audit.  f = B_k reduced mod r (fr.SetBytes), n >= 1 coefficients.  C_j = sum_{i >= j} f_i z^(i-j)
// (C_n = 0) gives every output: h[j - 1] = C_j for 1 <= j < n, h[n - 1] = 0, y = C_0.  Lane l owns the run [s, e) of m = ceil(n / 64)
// coefficients: its Horner value a = sum_{s <= i < e} f_i z^(i-s) and z^(e-s) make C_s = a + z^(e-s) C_e, an affine map; a suffix scan
// of these maps across the wave (operator (a1, m1) o (a2, m2) = (a1 + m1 a2, m1 m2), lane l + d above lane l) gives every lane its
// C_s, the lane above's C_s is its C_e, and a second Horner pass over the run writes its h values.  Values stay plain residues and only
// the powers of z are in the Montgomery form (a Montgomery product of a plain value with z R is the plain product).
__global__ void __launch_bounds__(64 * KZG_OPEN_WAVES)
k_kzg_open(const KzgAuditDesc* __restrict__ desc, uint32_t k, uint32_t n, uint8_t* __restrict__ rows3, uint8_t* __restrict__ out,
           uint8_t* __restrict__ b_out) {
    using Q = IccBn254Fr;
    const uint32_t a = blockIdx.x * KZG_OPEN_WAVES + (threadIdx.x >> 6);
    if (a >= k) return;                                       // wave-uniform
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t m = (n + 63) / 64;
    const uint32_t s = lane * m < n ? lane * m : n, e = s + m < n ? s + m : n;
    const uint8_t* f = rows3 + ((size_t)3 * a + 1) * 32 * n;
    uint8_t* h = rows3 + ((size_t)3 * a + 2) * 32 * n;
    Fe<Q> z = fe_zero<Q>();
    const unsigned long long zz = desc[a].z;
    z.v[0] = (uint32_t)zz;
    z.v[1] = (uint32_t)(zz >> 32);                            // z < 2^64 < r
    const Fe<Q> zM = fe_to_mont<Q>(z);
    auto coef = [&](uint32_t i) {
        Fe<Q> c;
        load_be256(c.v, f + (size_t)i * 32);
        fe_reduce_plain<Q>(c.v, Q::MAX_Q_P + 1);               // B < p_icc: fr.SetBytes' reduction
        return c;
    };
    Fe<Q> acc = fe_zero<Q>(), zm = fe_one<Q>();
    for (uint32_t i = e; i-- > s;) {
        acc = fe_add<Q>(fe_mul<Q>(acc, zM), coef(i));
        zm = fe_mul<Q>(zm, zM);
        if (b_out) {
            const uint4* src = reinterpret_cast<const uint4*>(f + (size_t)i * 32);
            uint4* dst = reinterpret_cast<uint4*>(b_out + ((size_t)a * n + i) * 32);
            dst[0] = src[0]; dst[1] = src[1];
        }
    }
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        Fe<Q> oa, om;
#pragma unroll
        for (int w = 0; w < 8; w++) {
            oa.v[w] = (uint32_t)__shfl_down((int)acc.v[w], d, 64);
            om.v[w] = (uint32_t)__shfl_down((int)zm.v[w], d, 64);
        }
        if (lane + d < 64) {
            acc = fe_add<Q>(acc, fe_mul<Q>(oa, zm));
            zm = fe_mul<Q>(zm, om);
        }
    }
    Fe<Q> carry;                                              // C_e: the lane above's C_s (0 above the top lane)
#pragma unroll
    for (int w = 0; w < 8; w++) carry.v[w] = (uint32_t)__shfl_down((int)acc.v[w], 1, 64);
    if (lane == 63) carry = fe_zero<Q>();
    for (uint32_t i = e; i-- > s;) {
        carry = fe_add<Q>(fe_mul<Q>(carry, zM), coef(i));
        if (i >= 1) store_be256(h + (size_t)(i - 1) * 32, carry.v);
    }
    if (s <= n - 1 && n - 1 < e) {
        const uint4 zero = make_uint4(0, 0, 0, 0);
        uint4* d = reinterpret_cast<uint4*>(h + (size_t)(n - 1) * 32);
        d[0] = zero; d[1] = zero;
    }
    if (lane == 0) {                                          // acc = C_0 = y
        uint8_t* rec = out + (size_t)a * KZG_AUDIT_RECORD;
        store_be256(rec + 128, z.v);
        store_be256(rec + 160, acc.v);
    }
}

// ---- the MSM entries of every audit: entry 2a = (coef_i, mac_store[idx_i]), entry 2a + 1 = (coef_i, align_store[idx_i]), i < n_macs,
// at pairs [pair0, pair0 + n) and [pair0 + n, pair0 + 2n).  Block b covers pairs [64 (b - gat0), ...) of audit gat_audit[b].
__global__ void __launch_bounds__(4 * KZG_GATHER_PAIRS)
k_kzg_audit_gather(const KzgAuditDesc* __restrict__ desc, const uint32_t* __restrict__ gat_audit, uint8_t* __restrict__ scalars,
                   uint8_t* __restrict__ points) {
    const KzgAuditDesc& D = desc[gat_audit[blockIdx.x]];
    kzg_gather_pairs<true>(D.mac_store, D.align_store, D.mac_idx, D.mac_coef, D.n_macs, D.pair0, blockIdx.x - D.gat0, scalars, points);
}

// ---- the records: a lane per audit.  Its commit rows' sums (c_k, B_k, h_k at commit[(3a + j) S]) and MSM sums (msm[2a], msm[2a + 1]);
// combined_align = MSM(align) + Commit(c) (align_MAC); then commitment, proof_h, combined_mac and combined_align to affine with ONE
// inversion, big-endian, 64 zero bytes = infinity.
__global__ void __launch_bounds__(64)
k_kzg_audit_join(const XYZZ<Bn254Fp>* __restrict__ commit, uint32_t S, const XYZZ<Bn254Fp>* __restrict__ msm, uint32_t k,
                 uint8_t* __restrict__ out) {
    using C = Bn254G1;
    using M = Bn254Fp;
    const uint32_t a = blockIdx.x * 64 + threadIdx.x;
    if (a >= k) return;
    XYZZ<M> p[4];
    p[0] = load_xyzz<M>(commit + ((size_t)3 * a + 1) * S);
    p[1] = load_xyzz<M>(commit + ((size_t)3 * a + 2) * S);
    p[2] = load_xyzz<M>(msm + 2 * (size_t)a);
    p[3] = load_xyzz<M>(msm + 2 * (size_t)a + 1);
    {
        const XYZZ<M> av = load_xyzz<M>(commit + (size_t)3 * a * S);
        xyzz_add_cold<M>(&p[3], &av);
    }
    constexpr uint32_t at[4] = {0, 64, 192, 256};
    xyzz_to_be_one_inv<C, 4>(p, out + (size_t)a * KZG_AUDIT_RECORD, at);
}

// ---- per-device workspace: the work list (pinned staging + device copy), the combine's partials, the commit rows, the MSM entries and
// sums.  One call at a time enqueues (mu); `fence` orders the buffers between calls on different streams.
struct KzgAuditBatchWs {
    std::mutex mu;
    int device = -1;
    Buf list, partial, rows3, msm_sc, msm_pt, msm_sums;
    PinnedList h_list;
    UseFence fence;
};
static PerDevice<KzgAuditBatchWs> g_kab_ws;

// ws->mu held, ws->fence entered
static int audit_batch_enqueue(KzgAuditBatchWs* ws, const porla_kzg_audit_req* reqs, size_t k, size_t n, uint8_t* d_out, uint8_t* d_b_out,
                               hipStream_t stream) {
    int rc;
    AuditPlan P;
    if ((rc = audit_batch_plan(reqs, k, [&](size_t a) { return reqs[a].random_point; }, &P))) return rc;
    size_t rows3_b;
    if (!mul_ok(3 * k, 32 * n, &rows3_b)) { set_last_error("porla: audit batch byte size overflows"); return PORLA_ERR_ARG; }
    const uint64_t blocks = P.blocks, gblocks = P.gblocks;
    // ---- the work list: descriptors | combine block -> audit | gather block -> audit, one pinned buffer, one copy
    const size_t list_b = P.list_bytes();
    if ((rc = ws->h_list.stage(list_b))) return rc;
    P.write((uint8_t*)ws->h_list.h);
    if ((rc = ws->list.ensure(list_b))) return rc;
    if ((rc = ws->partial.ensure(audit_combine_partial_bytes((uint32_t)blocks, (uint32_t)n)))) return rc;
    if ((rc = ws->rows3.ensure(rows3_b))) return rc;
    if ((rc = ws->msm_sc.ensure((size_t)P.pairs * 32 + 64))) return rc;
    if ((rc = ws->msm_pt.ensure((size_t)P.pairs * 64 + 64))) return rc;
    if ((rc = ws->msm_sums.ensure(2 * k * sizeof(XYZZ<Bn254Fp>)))) return rc;
    if ((rc = ws->h_list.send(ws->list.p, list_b, stream))) return rc;
    const KzgAuditDesc* d_desc = (const KzgAuditDesc*)ws->list.p;
    const uint32_t* d_blk = (const uint32_t*)((const uint8_t*)ws->list.p + P.desc_bytes());
    const uint32_t* d_gat = d_blk + blocks;
    uint8_t* rows3 = (uint8_t*)ws->rows3.p;
    // ---- 1. the row combine: c_k and B_k into the commit rows
    if ((rc = audit_combine_batch_launch(d_desc, d_blk, (uint32_t)blocks, (uint32_t)k, (uint32_t)n, P.per_slice, ws->partial.p, 0, rows3,
                                         rows3 + 32 * n, 3 * 32 * n, stream)))
        return rc;
    // ---- 2. the opening: h_k, point, claim (and B into d_b_out)
    {
        ProfScope ps("kzg_open", stream);
        hipLaunchKernelGGL(k_kzg_open, dim3((unsigned)((k + KZG_OPEN_WAVES - 1) / KZG_OPEN_WAVES)), dim3(64 * KZG_OPEN_WAVES), 0, stream, d_desc,
                           (uint32_t)k, (uint32_t)n, rows3, d_out, d_b_out);
        PORLA_HIP(hipGetLastError());
    }
    // ---- 3. the MSM pairs: gather, then the batched MSM over the 2K entries, sums left projective
    if (gblocks) {
        ProfScope ps("kzg_audit_gather", stream);
        hipLaunchKernelGGL(k_kzg_audit_gather, dim3((unsigned)gblocks), dim3(4 * KZG_GATHER_PAIRS), 0, stream, d_desc, d_gat,
                           (uint8_t*)ws->msm_sc.p, (uint8_t*)ws->msm_pt.p);
        PORLA_HIP(hipGetLastError());
    }
    XYZZ<Bn254Fp>* msm_sums = (XYZZ<Bn254Fp>*)ws->msm_sums.p;
    if ((rc = msm_batch_sums_device<Bn254G1>((const uint8_t*)ws->msm_sc.p, (const uint8_t*)ws->msm_pt.p, P.offsets.data(), 2 * k, msm_sums, stream)))
        return rc;
    // ---- 4. the 3K commitments, then 5. the join into the records
    return kzg_commit_rows_raw(rows3, 3 * k, stream, [&](const XYZZ<Bn254Fp>* sums, uint32_t S) {
        ProfScope ps("kzg_audit_join", stream);
        hipLaunchKernelGGL(k_kzg_audit_join, dim3((unsigned)((k + 63) / 64)), dim3(64), 0, stream, sums, S, msm_sums, (uint32_t)k, d_out);
        PORLA_HIP(hipGetLastError());
        return PORLA_OK;
    });
}

}  // namespace porla

using namespace porla;

static_assert(sizeof(porla_kzg_audit_req) == PORLA_KZG_AUDIT_REQ_BYTES, "porla_kzg_audit_req size");
static_assert(offsetof(porla_kzg_audit_req, d_rows64) == 0 && offsetof(porla_kzg_audit_req, d_idx64) == 8 &&
              offsetof(porla_kzg_audit_req, d_coef64) == 16 && offsetof(porla_kzg_audit_req, n64) == 24 &&
              offsetof(porla_kzg_audit_req, d_rows32) == 32 && offsetof(porla_kzg_audit_req, d_idx32) == 40 &&
              offsetof(porla_kzg_audit_req, d_coef32) == 48 && offsetof(porla_kzg_audit_req, n32) == 56 &&
              offsetof(porla_kzg_audit_req, d_mac_store) == 64 && offsetof(porla_kzg_audit_req, d_align_store) == 72 &&
              offsetof(porla_kzg_audit_req, d_mac_idx) == 80 && offsetof(porla_kzg_audit_req, d_mac_coef) == 88 &&
              offsetof(porla_kzg_audit_req, n_macs) == 96 && offsetof(porla_kzg_audit_req, random_point) == 104,
              "porla_kzg_audit_req offsets (include/porla_gpu.h)");

extern "C" int porla_kzg_audit_batch_device(const porla_kzg_audit_req* reqs, size_t k, void* d_out, void* d_b_out, void* hip_stream) {
    static const char* who = "porla_kzg_audit_batch_device";
    if (k && (!reqs || !d_out)) return bad_arg(who, "reqs or d_out is NULL");
    size_t out_b;
    if (!mul_ok(k, KZG_AUDIT_RECORD, &out_b)) return bad_arg(who, "k records overflow a byte size");
    uint64_t pairs = 0;
    int rc = audit_batch_check(who, "porla_kzg_audit_device", reqs, k, &pairs);
    if (rc) return rc;
    size_t pt_b;
    if (!mul_ok(k, 3 * 32 * 65536, &pt_b) || !mul_ok((size_t)pairs, 96, &pt_b)) return bad_arg(who, "the batch's byte size overflows");
    if (k == 0) return PORLA_OK;
    if ((rc = ensure_device())) return rc;
    size_t n;
    if ((rc = kzg_row_width(&n))) return rc;
    KzgAuditBatchWs* ws = nullptr;
    if ((rc = g_kab_ws.get(&ws))) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    return FencedCall(ws, stream).run([&] { return audit_batch_enqueue(ws, reqs, k, n, (uint8_t*)d_out, (uint8_t*)d_b_out, stream); });
}
