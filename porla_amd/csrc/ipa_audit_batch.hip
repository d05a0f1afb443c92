// Server::audit (IPA build) for K independent audits in ONE asynchronous call, inner-product proofs included
// (include/porla_gpu.h: porla_ipa_audit_batch_device, porla_ipa_prove_batch_device).  porla_ipa_audit_device stops before the proof and
// leaves Server::inner_product_prove (porla/Server/Server.hpp:2279-2452) to the caller: six blocking two-row commitments per audit with
// the folding and the transcript hash on the host between them.  For K audits the rounds stay sequential, but each round is ONE
// fixed-base pass over 2K rows, and everything between the passes runs on the device, on the caller's stream:
//
//   upload                one copy of the host-built work list (a_values, audit descriptors, combine blocks, gather blocks)
//   audit_batch_*         the row combine of all K audits (audit.hip): alignment scalars c_k (mod n) and B_k into the rows [c_k, B_k]
//   k_ipa_audit_gather    the 2K MSM entries (coef_i, MAC[idx_i]) and (coef_i, align[idx_i]); batch_*: the batched MSM over them
//   fb_commit / fb_fold   ONE pass over the 2K rows [c_k, B_k] (128 coefficients), then
//   k_ipa_audit_join      per audit: Commit(B), MSM(MAC), MSM(align) + Commit(c) (align_MAC) to affine with one inversion, compressed
//   k_ipa_open            a block per audit: a = B_k, b = (v, v^2, v^4, ...) by repeated squaring (Server.hpp:863-867), x_values = 1,
//                         c = <a, b> mod n into the proof, the first transcript hash
//   six times:
//   k_ipa_round_rows      a block per audit: x, 1/x from the hash, cL, cR, the L row and the R row (129 coefficients: the
//                         generators' and u's), the x_values updates
//   fb_commit / fb_fold   ONE pass over the 2K rows [L_k, R_k]
//   k_ipa_round_close     a block per audit: L, R to affine with one inversion, compressed into the proof; the next hash; the fold of
//                         a and b; after the last round a0 b0 a1 b1
//
// The transcript (Server.hpp:2306-2310, :2381-2382, :2431-2432) is ONE secp256k1_sha256 object that is written to again after
// every finalize.  finalize (secp256k1_lib/hash_impl.h:151-165) pads, emits the state and sets the eight state words to ZERO while the
// byte counter keeps counting, padding included.  So h0 = SHA-256(tag | c), and every later hash is one compression from the all-zero
// state over a 33-byte point padded with the cumulative length: 128 + 64 (i - 1) + 33 bytes for the i-th of them.  The hash over L
// is overwritten before anything reads it and leaves no trace in the state, so only R's is computed: the challenge of round r + 1.
#include "ipa_batch.hip.h"

#include <cstddef>
#include <mutex>
#include <vector>

namespace porla {

// the prover's state of one audit between kernels, 32-bit words: a, b, x_values (Montgomery residues mod n), then the transcript's last
// hash (the eight state words), x and 1 / x of the current round (Montgomery)
constexpr uint32_t ST_A = 0, ST_B = 8 * IPA_N, ST_XV = 16 * IPA_N, ST_H = 24 * IPA_N, ST_X = ST_H + 8, ST_XI = ST_X + 8;
constexpr uint32_t ST_WORDS = ST_XI + 8;

// 32 bytes little-endian (convert_ZZ_to_arr, utils.h:353-364) of a plain residue at any address
__device__ __forceinline__ void store_le256_bytes(uint8_t* dst, const uint32_t v[8]) {
#pragma unroll
    for (int i = 0; i < 32; i++) dst[i] = (uint8_t)(v[i >> 2] >> (8 * (i & 3)));
}
// a point in libsecp256k1's compressed form at any address: 0x02 | (y & 1), X big-endian; infinity (which the reference cannot
// serialise) as 33 zero bytes
__device__ __forceinline__ void store_compressed(uint8_t* dst, bool live, const uint32_t x[8], const uint32_t y[8]) {
    dst[0] = live ? (uint8_t)(2u | (y[0] & 1u)) : (uint8_t)0;
#pragma unroll
    for (int i = 0; i < 32; i++) dst[1 + i] = live ? (uint8_t)(x[7 - (i >> 2)] >> (24 - 8 * (i & 3))) : (uint8_t)0;
}

__device__ __forceinline__ Fe<Fn> st_load(const uint32_t* st, uint32_t at) { return ld_fe<Fn>(st + at); }
__device__ __forceinline__ void st_store(uint32_t* st, uint32_t at, const Fe<Fn>& f) { st_fe<Fn>(st + at, f); }

// ---- the opening of the proof, a block of 128 lanes per audit, lane j = element j.  a from a_src (128 x 32 bytes big-endian per audit);
// b from b_src likewise, or, with a_values, b_j = v^(2^j): A[i] = A_value, A_value = A_value^2 (Server.hpp:863-867).  c = <a, b> mod n
// (Server.hpp:2286) goes to the proof's first 32 bytes, h0 = SHA-256(tag | c) to the state.  b_out: the audit's copy of B.
__global__ void __launch_bounds__(IPA_N)
k_ipa_open(const uint8_t* __restrict__ a_src, size_t a_stride, const uint8_t* __restrict__ b_src, const uint8_t* __restrict__ a_values,
           uint32_t* __restrict__ state, uint8_t* __restrict__ proofs, size_t proof_stride, uint8_t* __restrict__ b_out) {
    __shared__ uint32_t red[IPA_N][8];
    const uint32_t k = blockIdx.x, j = threadIdx.x;
    uint32_t* st = state + (size_t)k * ST_WORDS;
    const uint8_t* ap = a_src + k * a_stride + 32 * (size_t)j;
    const Fe<Fn> a = load_scalar_mont(ap);
    if (b_out) {
        const uint4* s4 = reinterpret_cast<const uint4*>(ap);
        uint4* d4 = reinterpret_cast<uint4*>(b_out + ((size_t)k * IPA_N + j) * 32);
        d4[0] = s4[0]; d4[1] = s4[1];
    }
    Fe<Fn> b;
    if (a_values) {
        b = load_scalar_mont(a_values + 32 * (size_t)k);
#pragma unroll 1
        for (uint32_t i = 0; i + 1 < IPA_N; i++) {
            const Fe<Fn> sq = fe_mul<Fn>(b, b);
            if (i < j) b = sq;
        }
    } else {
        b = load_scalar_mont(b_src + ((size_t)k * IPA_N + j) * 32);
    }
    st_store(st, ST_A + 8 * j, a);
    st_store(st, ST_B + 8 * j, b);
    st_store(st, ST_XV + 8 * j, fe_one<Fn>());
    const Fe<Fn> c = fe_from_mont<Fn>(block_sum(fe_mul<Fn>(a, b), red));
    if (j != 0) return;
    store_le256_bytes(proofs + k * proof_stride, c.v);
    uint32_t s[8], w[16];
#pragma unroll
    for (int i = 0; i < 8; i++) { s[i] = Sha256K::IV[i]; w[i] = Sha256K::TAG[i]; w[8 + i] = __builtin_bswap32(c.v[i]); }
    sha256_compress(s, w);
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = 0;
    w[0] = 0x80000000u;
    w[15] = 512;
    sha256_compress(s, w);
    uint4* h4 = reinterpret_cast<uint4*>(st + ST_H);
    h4[0] = make_uint4(s[0], s[1], s[2], s[3]);
    h4[1] = make_uint4(s[4], s[5], s[6], s[7]);
}

// ---- the rows of one round (Server.hpp:2320-2349, :2388-2399), a block per audit, lane j = generator j.  x = the last hash read as a
// little-endian integer mod n (convert_arr_to_ZZ_p, utils.h:384-393), 1 / x by Fermat: every lane runs the same chain, which costs
// the block no more time than one lane running it and saves the broadcast.  A hash that is 0 mod n has no inverse (NTL raises an error
// there; probability 2^-256): the chain then gives 0 and the kernel goes on.  cL = <a_lo, b_hi>, cR = <a_hi, b_lo> as block sums.
// With blk = j / half, q = j % half: the L row takes a[q] x_values[j] on odd blk (then x_values[j] *= x), the R row a[half + q]
// x_values[j] on even blk (then x_values[j] *= 1 / x), 0 elsewhere; coefficient 128 (u's) is cL and cR.  The R row does not depend on
// L's hash, so both rows go into one commitment pass: rows 2k and 2k + 1 of `rows`, 129 x 32 bytes big-endian each.
__global__ void __launch_bounds__(IPA_N)
k_ipa_round_rows(uint32_t* __restrict__ state, uint8_t* __restrict__ rows, uint32_t half) {
    __shared__ uint32_t red[IPA_N][8];
    const uint32_t k = blockIdx.x, j = threadIdx.x;
    uint32_t* st = state + (size_t)k * ST_WORDS;
    Fe<Fn> x;
    {
        const Fe<Fn> h = st_load(st, ST_H);
#pragma unroll
        for (int i = 0; i < 8; i++) x.v[i] = __builtin_bswap32(h.v[i]);
        fe_reduce_plain<Fn>(x.v, Fn::MAX_Q_IN);
        x = fe_to_mont<Fn>(x);
    }
    const Fe<Fn> xi = fe_inv_dev<Fn>(x);
    Fe<Fn> tl = fe_zero<Fn>(), tr = fe_zero<Fn>();
    if (j < half) {
        tl = fe_mul<Fn>(st_load(st, ST_A + 8 * j), st_load(st, ST_B + 8 * (half + j)));
        tr = fe_mul<Fn>(st_load(st, ST_A + 8 * (half + j)), st_load(st, ST_B + 8 * j));
    }
    const Fe<Fn> cl = block_sum(tl, red), cr = block_sum(tr, red);
    const uint32_t q = j & (half - 1);
    const bool odd = (j / half) & 1u;
    Fe<Fn> xv = st_load(st, ST_XV + 8 * j);
    const Fe<Fn> coef = fe_from_mont<Fn>(fe_mul<Fn>(st_load(st, ST_A + 8 * (odd ? q : half + q)), xv));
    st_store(st, ST_XV + 8 * j, fe_mul<Fn>(xv, odd ? x : xi));
    uint8_t* lrow = rows + (size_t)2 * k * IPA_ROW_COEFFS * 32;
    uint8_t* rrow = lrow + IPA_ROW_COEFFS * 32;
    const Fe<Fn> zero = fe_zero<Fn>();
    store_be256(lrow + 32 * j, odd ? coef.v : zero.v);
    store_be256(rrow + 32 * j, odd ? zero.v : coef.v);
    if (j == 0) {
        const Fe<Fn> pl = fe_from_mont<Fn>(cl), pr = fe_from_mont<Fn>(cr);
        store_be256(lrow + 32 * IPA_N, pl.v);
        store_be256(rrow + 32 * IPA_N, pr.v);
        st_store(st, ST_X, x);
        st_store(st, ST_XI, xi);
    }
}

// ---- the end of round r, a block per audit.  Wave 1's first lane: L and R (the pass's sums, row i at sums[i S]) to affine with ONE
// inversion, compressed into the proof, and the hash over R: the next round's challenge.  Lanes j < half: the fold
// a'[j] = a[j] x + a[j + half] / x, b'[j] = b[j] / x + b[j + half] x (Server.hpp:2436-2442): a lane writes element j < half only and
// reads, of the elements below half, only its own.  After the last round lanes 0 and 1 write a0 b0 a1 b1 (Server.hpp:2445-2451).
__global__ void __launch_bounds__(IPA_N)
k_ipa_round_close(uint32_t* __restrict__ state, const XYZZ<Secp256k1Fp>* __restrict__ sums, uint32_t S, uint8_t* __restrict__ proofs,
                  size_t proof_stride, uint32_t round, uint32_t half) {
    using M = Secp256k1Fp;
    const uint32_t k = blockIdx.x, j = threadIdx.x;
    uint32_t* st = state + (size_t)k * ST_WORDS;
    uint8_t* proof = proofs + k * proof_stride;
    if (j == 64) {
        XYZZ<M> p[2];
        p[0] = load_xyzz<M>(sums + (size_t)2 * k * S);
        p[1] = load_xyzz<M>(sums + ((size_t)2 * k + 1) * S);
        uint8_t* dst = proof + 32 + 66 * round;
        uint32_t w[16];
#pragma unroll
        for (int i = 0; i < 16; i++) w[i] = 0;
        xyzz_each_affine_one_inv<Secp256k1G, 2>(p, [&](int i, bool live, const Fe<M>& x, const Fe<M>& y) {
            store_compressed(dst + 33 * i, live, x.v, y.v);
            if (i == 1 && live) {          // the 33 bytes of R as big-endian words
                w[0] = ((2u | (y.v[0] & 1u)) << 24) | (x.v[7] >> 8);
#pragma unroll
                for (int t = 1; t < 8; t++) w[t] = (x.v[8 - t] << 24) | (x.v[7 - t] >> 8);
                w[8] = x.v[0] << 24;
            }
        });
        w[8] |= 0x00800000u;
        w[15] = 8u * (225u + 128u * round);        // the object's byte count so far: 128 + 64 (2 round + 1) + 33
        uint32_t s[8];
#pragma unroll
        for (int i = 0; i < 8; i++) s[i] = 0;
        sha256_compress(s, w);
        uint4* h4 = reinterpret_cast<uint4*>(st + ST_H);
        h4[0] = make_uint4(s[0], s[1], s[2], s[3]);
        h4[1] = make_uint4(s[4], s[5], s[6], s[7]);
    }
    if (j >= half) return;
    const Fe<Fn> x = st_load(st, ST_X), xi = st_load(st, ST_XI);
    const Fe<Fn> a = fe_add<Fn>(fe_mul<Fn>(st_load(st, ST_A + 8 * j), x), fe_mul<Fn>(st_load(st, ST_A + 8 * (j + half)), xi));
    const Fe<Fn> b = fe_add<Fn>(fe_mul<Fn>(st_load(st, ST_B + 8 * j), xi), fe_mul<Fn>(st_load(st, ST_B + 8 * (j + half)), x));
    st_store(st, ST_A + 8 * j, a);
    st_store(st, ST_B + 8 * j, b);
    if (half == 2) {
        const Fe<Fn> pa = fe_from_mont<Fn>(a), pb = fe_from_mont<Fn>(b);
        uint8_t* tail = proof + 32 + 66 * IPA_ROUNDS + 64 * j;
        store_le256_bytes(tail, pa.v);
        store_le256_bytes(tail + 32, pb.v);
    }
}

// ---- the MSM entries of every audit, as the batched KZG audit's: entry 2a = (coef_i, mac_store[idx_i]), entry 2a + 1 = (coef_i,
// align_store[idx_i]); the stores are 64-byte big-endian affine points on both curves
__global__ void __launch_bounds__(4 * KZG_GATHER_PAIRS)
k_ipa_audit_gather(const KzgAuditDesc* __restrict__ desc, const uint32_t* __restrict__ gat_audit, uint8_t* __restrict__ scalars,
                   uint8_t* __restrict__ points) {
    const KzgAuditDesc& D = desc[gat_audit[blockIdx.x]];
    kzg_gather_pairs<true>(D.mac_store, D.align_store, D.mac_idx, D.mac_coef, D.n_macs, D.pair0, blockIdx.x - D.gat0, scalars, points);
}

// ---- the three points of the record, a lane per audit: commitment = Commit(B) (row 2a + 1 of the pass), combined_MAC = msm[2a],
// combined_align = msm[2a + 1] + Commit(c) (align_MAC, Server.hpp:495-529; row 2a), to affine with ONE inversion, compressed
__global__ void __launch_bounds__(64)
k_ipa_audit_join(const XYZZ<Secp256k1Fp>* __restrict__ commit, uint32_t S, const XYZZ<Secp256k1Fp>* __restrict__ msm, uint32_t k,
                 uint8_t* __restrict__ out) {
    using M = Secp256k1Fp;
    const uint32_t a = blockIdx.x * 64 + threadIdx.x;
    if (a >= k) return;
    XYZZ<M> p[3];
    p[0] = load_xyzz<M>(commit + ((size_t)2 * a + 1) * S);
    p[1] = load_xyzz<M>(msm + 2 * (size_t)a);
    p[2] = load_xyzz<M>(msm + 2 * (size_t)a + 1);
    {
        const XYZZ<M> av = load_xyzz<M>(commit + (size_t)2 * a * S);
        xyzz_add_cold<M>(&p[2], &av);
    }
    uint8_t* rec = out + (size_t)a * IPA_RECORD;
    xyzz_each_affine_one_inv<Secp256k1G, 3>(p, [&](int i, bool live, const Fe<M>& x, const Fe<M>& y) {
        store_compressed(rec + 33 * i, live, x.v, y.v);
    });
}

// ---- per-device workspace: the work list (pinned staging + device copy), the combine's partials, the rows [c_k, B_k], the MSM
// entries and sums, the prover's state and round rows.  One call at a time enqueues (mu); `fence` orders the buffers between calls on
// different streams.
struct IpaBatchWs {
    std::mutex mu;
    int device = -1;
    Buf list, partial, rows2, msm_sc, msm_pt, msm_sums, state, rows;
    PinnedList h_list;
    UseFence fence;
};
static PerDevice<IpaBatchWs> g_ipa_ws;

// ws->mu held, ws->fence entered.  The k proofs of (a, b): a_src as k_ipa_open takes it, b from b_src or from a_values.
static int prove_enqueue(IpaBatchWs* ws, FixedBase<Secp256k1G>& fb, size_t k, const uint8_t* a_src, size_t a_stride, const uint8_t* b_src,
                         const uint8_t* a_values, uint8_t* proofs, size_t proof_stride, uint8_t* b_out, hipStream_t stream) {
    int rc;
    if ((rc = ws->state.ensure(k * ST_WORDS * 4))) return rc;
    if ((rc = ws->rows.ensure(2 * k * IPA_ROW_COEFFS * 32))) return rc;
    uint32_t* state = (uint32_t*)ws->state.p;
    uint8_t* rows = (uint8_t*)ws->rows.p;
    {
        ProfScope ps("ipa_open", stream);
        hipLaunchKernelGGL(k_ipa_open, dim3((unsigned)k), dim3(IPA_N), 0, stream, a_src, a_stride, b_src, a_values, state, proofs, proof_stride,
                           b_out);
        PORLA_HIP(hipGetLastError());
    }
    for (uint32_t r = 0, half = IPA_N / 2; r < IPA_ROUNDS; r++, half >>= 1) {
        {
            ProfScope ps("ipa_round_rows", stream);
            hipLaunchKernelGGL(k_ipa_round_rows, dim3((unsigned)k), dim3(IPA_N), 0, stream, state, rows, half);
            PORLA_HIP(hipGetLastError());
        }
        rc = commit_then(fb, rows, 2 * k, IPA_ROW_COEFFS, stream, [&](const XYZZ<Secp256k1Fp>* sums, uint32_t S) {
            ProfScope ps("ipa_round_close", stream);
            hipLaunchKernelGGL(k_ipa_round_close, dim3((unsigned)k), dim3(IPA_N), 0, stream, state, sums, S, proofs, proof_stride, r, half);
            PORLA_HIP(hipGetLastError());
            return (int)PORLA_OK;
        });
        if (rc) return rc;
    }
    return PORLA_OK;
}

// ws->mu held, ws->fence entered
static int audit_enqueue(IpaBatchWs* ws, FixedBase<Secp256k1G>& fb, const porla_ipa_audit_req* reqs, size_t k, uint8_t* d_out,
                         uint8_t* d_b_out, hipStream_t stream) {
    int rc;
    const size_t n = IPA_N;
    AuditPlan P;
    if ((rc = audit_batch_plan(reqs, k, [](size_t) { return 0ull; }, &P))) return rc;
    const uint64_t blocks = P.blocks, gblocks = P.gblocks;
    // ---- the work list: a_values | descriptors | combine block -> audit | gather block -> audit, one pinned buffer, one copy
    const size_t av_b = 32 * k, list_b = av_b + P.list_bytes();
    if ((rc = ws->h_list.stage(list_b))) return rc;
    {
        uint8_t* h = (uint8_t*)ws->h_list.h;
        for (size_t a = 0; a < k; a++) memcpy(h + 32 * a, reqs[a].a_value, 32);
        P.write(h + av_b);
    }
    if ((rc = ws->list.ensure(list_b))) return rc;
    if ((rc = ws->partial.ensure(audit_combine_partial_bytes((uint32_t)blocks, (uint32_t)n)))) return rc;
    if ((rc = ws->rows2.ensure(2 * k * 32 * n))) return rc;
    if ((rc = ws->msm_sc.ensure((size_t)P.pairs * 32 + 64))) return rc;
    if ((rc = ws->msm_pt.ensure((size_t)P.pairs * 64 + 64))) return rc;
    if ((rc = ws->msm_sums.ensure(2 * k * sizeof(XYZZ<Secp256k1Fp>)))) return rc;
    if ((rc = ws->h_list.send(ws->list.p, list_b, stream))) return rc;
    const uint8_t* d_av = (const uint8_t*)ws->list.p;
    const KzgAuditDesc* d_desc = (const KzgAuditDesc*)(d_av + av_b);
    const uint32_t* d_blk = (const uint32_t*)(d_av + av_b + P.desc_bytes());
    const uint32_t* d_gat = d_blk + blocks;
    uint8_t* rows2 = (uint8_t*)ws->rows2.p;
    // ---- 1. the row combine: c_k (mod n) and B_k into the rows [c_k, B_k]
    if ((rc = audit_combine_batch_launch(d_desc, d_blk, (uint32_t)blocks, (uint32_t)k, (uint32_t)n, P.per_slice, ws->partial.p, 1, rows2,
                                         rows2 + 32 * n, 2 * 32 * n, stream)))
        return rc;
    // ---- 2. the MSM pairs: gather, then the batched MSM over the 2K entries, sums left projective
    if (gblocks) {
        ProfScope ps("ipa_audit_gather", stream);
        hipLaunchKernelGGL(k_ipa_audit_gather, dim3((unsigned)gblocks), dim3(4 * KZG_GATHER_PAIRS), 0, stream, d_desc, d_gat,
                           (uint8_t*)ws->msm_sc.p, (uint8_t*)ws->msm_pt.p);
        PORLA_HIP(hipGetLastError());
    }
    XYZZ<Secp256k1Fp>* msm_sums = (XYZZ<Secp256k1Fp>*)ws->msm_sums.p;
    if ((rc = msm_batch_sums_device<Secp256k1G>((const uint8_t*)ws->msm_sc.p, (const uint8_t*)ws->msm_pt.p, P.offsets.data(), 2 * k, msm_sums,
                                                stream)))
        return rc;
    // ---- 3. the 2K Pedersen commitments and the record's points: the prover's first pass overwrites these sums
    rc = commit_then(fb, rows2, 2 * k, n, stream, [&](const XYZZ<Secp256k1Fp>* sums, uint32_t S) {
        ProfScope ps("ipa_audit_join", stream);
        hipLaunchKernelGGL(k_ipa_audit_join, dim3((unsigned)((k + 63) / 64)), dim3(64), 0, stream, sums, S, msm_sums, (uint32_t)k, d_out);
        PORLA_HIP(hipGetLastError());
        return (int)PORLA_OK;
    });
    if (rc) return rc;
    // ---- 4. the proofs of (B_k, powers of a_value): B < p_icc < n, so the reduction mod n leaves it as it is
    return prove_enqueue(ws, fb, k, rows2 + 32 * n, 2 * 32 * n, nullptr, d_av, d_out + 99, IPA_RECORD, d_b_out, stream);
}

}  // namespace porla

using namespace porla;

static_assert(sizeof(porla_ipa_audit_req) == PORLA_IPA_AUDIT_REQ_BYTES, "porla_ipa_audit_req size");
static_assert(offsetof(porla_ipa_audit_req, d_rows64) == 0 && offsetof(porla_ipa_audit_req, d_idx64) == 8 &&
              offsetof(porla_ipa_audit_req, d_coef64) == 16 && offsetof(porla_ipa_audit_req, n64) == 24 &&
              offsetof(porla_ipa_audit_req, d_rows32) == 32 && offsetof(porla_ipa_audit_req, d_idx32) == 40 &&
              offsetof(porla_ipa_audit_req, d_coef32) == 48 && offsetof(porla_ipa_audit_req, n32) == 56 &&
              offsetof(porla_ipa_audit_req, d_mac_store) == 64 && offsetof(porla_ipa_audit_req, d_align_store) == 72 &&
              offsetof(porla_ipa_audit_req, d_mac_idx) == 80 && offsetof(porla_ipa_audit_req, d_mac_coef) == 88 &&
              offsetof(porla_ipa_audit_req, n_macs) == 96 && offsetof(porla_ipa_audit_req, a_value) == 104,
              "porla_ipa_audit_req offsets (include/porla_gpu.h)");

extern "C" int porla_ipa_audit_batch_device(porla_fixed_base* gens_u_fb, const porla_ipa_audit_req* reqs, size_t k, void* d_out,
                                            void* d_b_out, void* hip_stream) {
    static const char* who = "porla_ipa_audit_batch_device";
    if (k && (!reqs || !d_out || !gens_u_fb)) return bad_arg(who, "reqs, d_out or gens_u_fb is NULL");
    size_t out_b;
    if (!mul_ok(k, IPA_RECORD, &out_b)) return bad_arg(who, "k records overflow a byte size");
    uint64_t pairs = 0;
    int rc = audit_batch_check(who, "porla_ipa_audit_device", reqs, k, &pairs);
    if (rc) return rc;
    size_t b;
    if (!mul_ok(k, (size_t)ST_WORDS * 4 + 2 * IPA_ROW_COEFFS * 32 + 3 * 32 * IPA_N, &b) || !mul_ok((size_t)pairs, 96, &b))
        return bad_arg(who, "the batch's byte size overflows");
    if (k == 0) return PORLA_OK;
    if ((rc = ensure_device())) return rc;
    if ((rc = ipa_check_base(gens_u_fb, who))) return rc;
    IpaBatchWs* ws = nullptr;
    if ((rc = g_ipa_ws.get(&ws))) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    return FencedCall(ws, stream).run(
        [&] { return audit_enqueue(ws, gens_u_fb->secp, reqs, k, (uint8_t*)d_out, (uint8_t*)d_b_out, stream); });
}

extern "C" int porla_ipa_prove_batch_device(porla_fixed_base* gens_u_fb, const void* d_a, const void* d_b, size_t k, void* d_proofs,
                                            void* hip_stream) {
    static const char* who = "porla_ipa_prove_batch_device";
    if (k && (!gens_u_fb || !d_a || !d_b || !d_proofs)) return bad_arg(who, "gens_u_fb, d_a, d_b or d_proofs is NULL");
    size_t b;
    if (!mul_ok(k, (size_t)ST_WORDS * 4 + 2 * IPA_ROW_COEFFS * 32, &b)) return bad_arg(who, "k proofs overflow a byte size");
    if (k > 0x7fffffffu) return bad_arg(who, "more than 2^31 - 1 proofs in one call");
    if (k == 0) return PORLA_OK;
    int rc = ensure_device();
    if (rc) return rc;
    if ((rc = ipa_check_base(gens_u_fb, who))) return rc;
    IpaBatchWs* ws = nullptr;
    if ((rc = g_ipa_ws.get(&ws))) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    return FencedCall(ws, stream).run([&] {
        return prove_enqueue(ws, gens_u_fb->secp, k, (const uint8_t*)d_a, 32 * IPA_N, (const uint8_t*)d_b, nullptr, (uint8_t*)d_proofs, IPA_PROOF,
                             nullptr, stream);
    });
}
