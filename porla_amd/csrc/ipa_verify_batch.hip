// Client::audit's check (IPA build) of K replies in ONE asynchronous call (include/porla_gpu.h: porla_ipa_verify_batch_device): the
// auditor that checks the records porla_ipa_audit_batch_device wrote (porla/Client/Client.hpp:633-880, the proof by
// Client::inner_product_verify, Client.hpp:1465-1633).  Nothing here needs a pairing, so every verdict is computed on the device,
// exactly per reply, and the status bytes stay in HBM.  Per reply, with C, M, A the record's three points:
//   FULL    sum_j coef_j comp[idx_j] + alpha C - alpha A - M = O          (the complements, then a 3-pair entry)
//   PROOF   C + sum_r (x_r^2 L_r + x_r^-2 R_r) - sum_j s_j G_j - (a0 b0 + a1 b1 - c) u = O,   s_j = a_(j & 1) x_values[j]
//           (a 13-pair entry minus one row of 129 coefficients on the generators' fixed base)
//   BVEC    b_i = sum_(j = i mod 2) v^(2^j) x_values[j] for i = 0, 1: the proof's b0, b1 are the fold of b = (v, v^2, v^4, ...)
// One fixed sequence of launches per call on the caller's stream:
//
//   upload               one copy of the host-built work list (reply descriptors, gather blocks) from pinned memory
//   k_ipa_verify_prep    a block of 128 lanes per reply: the six challenges, their inverses with ONE inversion mod n, x_values, the
//                        row of 129 coefficients, the 3-pair and 13-pair entries, the fifteen decompressions, BVEC
//   k_ipa_verify_gather  the complement entries (coef_j, comp[idx_j]) (kzg_batch.hip.h, as the KZG verifier gathers its own)
//   batch_*              the batched MSM over the 3K entries (msm_batch_impl.hip.h), projective sums kept
//   fb_commit / fb_fold  ONE pass of the generators' fixed base over the K rows, then under the table's lock
//   k_ipa_verify_join    a lane per reply: the two sums against infinity, the flags of the prep, the status byte
//
// The transcript: every hashed byte is in the record, so the challenges do not wait for any group arithmetic.  x_0 comes from
// h0 = SHA-256(tag | c) (two compressions), x_(r+1) from one compression of R_r from the all-zero state (ipa_audit_batch.hip's note
// on secp256k1_sha256's finalize): six independent hashes on six lanes.
#include "ipa_batch.hip.h"
#include "fe30.hip.h"

#include <cstddef>
#include <cstring>
#include <mutex>
#include <vector>

namespace porla {

constexpr uint32_t IPA_VERIFY_MAX_N = 32768;          // the batched MSM's entry limit (SMALL_MAX_N)
constexpr uint32_t IPA_VERIFY_POINTS = 3 + 2 * IPA_ROUNDS;    // C, M, A, then L_r, R_r
constexpr uint32_t IPA_VERIFY_PAIRS = 3 + 1 + 2 * IPA_ROUNDS; // the 3-pair entry, then (1, C), (x_r^2, L_r), (x_r^-2, R_r)

// One reply as the device kernels see it: the client's arrays, its complement entry at pairs [pair0, pair0 + n) with its 3-pair and
// its 13-pair entry right behind, and alpha, n - alpha and a_value reduced mod n (plain little-endian limbs).
struct IpaVerifyDesc {
    const uint8_t* comp_store; const uint64_t* idx; const uint32_t* coef;
    uint32_t n, gat0;                 // gat0: the reply's first block of the gather
    unsigned long long pair0;
    uint32_t alpha[8], nalpha[8], a_value[8];
};
static_assert(sizeof(IpaVerifyDesc) == 136, "IpaVerifyDesc: 24 bytes of pointers, 8 of counts, pair0, three scalars");

// 32 bytes at any address as eight words: big-endian words in memory order (a hash block's), or the little-endian integer's limbs
__device__ __forceinline__ uint32_t load_be32_bytes(const uint8_t* p) {
    return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
}
// 32 little-endian bytes (convert_arr_to_ZZ_p's order) at any address taken mod n, in the Montgomery form
__device__ __forceinline__ Fe<Fn> load_le_scalar_mont(const uint8_t* p) {
    Fe<Fn> f;
#pragma unroll
    for (int i = 0; i < 8; i++) f.v[i] = __builtin_bswap32(load_be32_bytes(p + 4 * i));
    fe_reduce_plain<Fn>(f.v, Fn::MAX_Q_IN);
    return fe_to_mont<Fn>(f);
}

using Fp = Secp256k1Fp;
// a^(2^n) in the 9 x 30-bit form, out of line: one body for the eleven runs of the square root's chain
__device__ __noinline__ F30<Fp> f30_sqr_n(F30<Fp> a, int n) {
#pragma unroll 1
    for (int i = 0; i < n; i++) a = f30_sqr<Fp>(a);
    return a;
}
// a^((p + 1) / 4): the square root of a where it has one (p = 3 mod 4).  (p + 1) / 4 = 2^254 - 2^30 - 244 is 223 ones, a zero, 22
// ones, 0000, 11, 00 in binary: the runs of ones built by doubling their length (2, 3, 6, 9, 11, 22, 44, 88, 176, 220, 223), 253
// squarings and 13 products.
__device__ __forceinline__ F30<Fp> f30_sqrt_candidate(const F30<Fp>& a) {
    const F30<Fp> x2 = f30_mul<Fp>(f30_sqr_n(a, 1), a);
    const F30<Fp> x3 = f30_mul<Fp>(f30_sqr_n(x2, 1), a);
    const F30<Fp> x6 = f30_mul<Fp>(f30_sqr_n(x3, 3), x3);
    const F30<Fp> x9 = f30_mul<Fp>(f30_sqr_n(x6, 3), x3);
    const F30<Fp> x11 = f30_mul<Fp>(f30_sqr_n(x9, 2), x2);
    const F30<Fp> x22 = f30_mul<Fp>(f30_sqr_n(x11, 11), x11);
    const F30<Fp> x44 = f30_mul<Fp>(f30_sqr_n(x22, 22), x22);
    const F30<Fp> x88 = f30_mul<Fp>(f30_sqr_n(x44, 44), x44);
    const F30<Fp> x176 = f30_mul<Fp>(f30_sqr_n(x88, 88), x88);
    const F30<Fp> x220 = f30_mul<Fp>(f30_sqr_n(x176, 44), x44);
    const F30<Fp> x223 = f30_mul<Fp>(f30_sqr_n(x220, 3), x3);
    F30<Fp> t = f30_mul<Fp>(f30_sqr_n(x223, 23), x22);
    t = f30_mul<Fp>(f30_sqr_n(t, 6), x2);
    return f30_sqr_n(t, 2);
}

// secp256k1_eckey_pubkey_parse's rules on 33 bytes at any address: first byte 2 or 3, X < p, X^3 + 7 a square; y takes the first
// byte's parity.  33 zero bytes are this library's infinity: well-formed, x = y = 0.  Plain coordinates, little-endian limbs.
__device__ __forceinline__ bool ipa_decompress(const uint8_t* c, Fe<Fp>& x, Fe<Fp>& y) {
    const uint32_t prefix = c[0];
    uint32_t any = prefix;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        x.v[7 - i] = load_be32_bytes(c + 1 + 4 * i);
        any |= x.v[7 - i];
    }
    y = fe_zero<Fp>();
    if (any == 0) return true;
    uint32_t s[8];
    if ((prefix != 2 && prefix != 3) || !sub_p<Fp>(s, x.v)) return false;      // sub_p borrows iff X < p
    const F30<Fp> xf = f30_from_fe<Fp>(x);
    Fe<Fp> seven = fe_zero<Fp>();
    seven.v[0] = 7;
    const Fe<Fp> rhs = fe_add<Fp>(f30_to_fe_canonical<Fp>(f30_mul<Fp>(f30_sqr_n(xf, 1), xf)), seven);
    const Fe<Fp> r = f30_to_fe_canonical<Fp>(f30_sqrt_candidate(f30_from_fe<Fp>(rhs)));
    if (!fe_eq<Fp>(f30_to_fe_canonical<Fp>(f30_sqr_n(f30_from_fe<Fp>(r), 1)), rhs)) return false;
    y = fe_neg_if<Fp>(r, (r.v[0] & 1u) != (prefix & 1u));
    return true;
}

// ---- a block of 128 lanes per reply.
//   lanes 0..5     the challenges x_0 .. x_5 (above), Montgomery residues mod n into LDS
//   wave 0         1 / x_r by Montgomery's trick from ONE Fermat inversion of the product (every lane runs the chain, as
//                  k_ipa_round_rows does).  A challenge that is 0 mod n makes the product 0: every inverse is then taken as 0.
//   wave 1         beside it, lanes 64..78: the fifteen decompressions (C, M, A, L_0, R_0, ...), coordinates into LDS
//   lane j         x_values[j] = prod_r (bit 6 - r of j ? x_r : 1 / x_r): the verifier's array after the six rounds
//                  (Client.hpp:1508-1524: round r, half = 64 >> r, multiplies odd blocks of `half` by x_r and even ones by 1 / x_r);
//                  s_j = a_(j & 1) x_values[j], coefficient j of the row; v^(2^j) by repeated squaring and the two BVEC sums
//   lane 0         the row's coefficient of u, a0 b0 + a1 b1 - c; the flags
//   lanes 0..15    the reply's 16 pairs: (alpha, C), (n - alpha, A), (n - 1, M); (1, C), (x_r^2, L_r), (x_r^-2, R_r)
// A malformed record gets zero scalars and points at infinity in all its pairs and a zero row, so that nothing is computed on its
// bytes, and the flag MALFORMED (the join leaves it so).
__global__ void __launch_bounds__(IPA_N)
k_ipa_verify_prep(const IpaVerifyDesc* __restrict__ desc, const uint8_t* __restrict__ records, uint8_t* __restrict__ scalars,
                  uint8_t* __restrict__ points, uint8_t* __restrict__ rows, uint8_t* __restrict__ flags) {
    __shared__ uint32_t red[IPA_N][8];
    __shared__ uint32_t ch[2 * IPA_ROUNDS][8];            // x_r, then 1 / x_r
    __shared__ uint32_t pts[IPA_VERIFY_POINTS][16];       // x, y
    __shared__ uint32_t bad;
    const uint32_t k = blockIdx.x, j = threadIdx.x;
    const IpaVerifyDesc& D = desc[k];
    const uint8_t* rec = records + (size_t)k * IPA_RECORD;
    const uint8_t* proof = rec + 99;
    const uint8_t* tail = proof + 32 + 66 * IPA_ROUNDS;   // a0 b0 a1 b1
    if (j == 0) bad = 0;
    if (j < IPA_ROUNDS) {
        uint32_t s[8], w[16];
        if (j == 0) {
#pragma unroll
            for (int i = 0; i < 8; i++) { s[i] = Sha256K::IV[i]; w[i] = Sha256K::TAG[i]; w[8 + i] = load_be32_bytes(proof + 4 * i); }
            sha256_compress(s, w);
#pragma unroll
            for (int i = 0; i < 16; i++) w[i] = 0;
            w[0] = 0x80000000u;
            w[15] = 512;
            sha256_compress(s, w);
        } else {
            const uint8_t* R = proof + 32 + 66 * (j - 1) + 33;
#pragma unroll
            for (int i = 0; i < 8; i++) { s[i] = 0; w[i] = load_be32_bytes(R + 4 * i); w[8 + i] = 0; }
            w[8] = ((uint32_t)R[32] << 24) | 0x00800000u;
            w[15] = 8u * (225u + 128u * (j - 1));          // the object's byte count so far: 128 + 64 (2 (j - 1) + 1) + 33
            sha256_compress(s, w);
        }
        Fe<Fn> x;
#pragma unroll
        for (int i = 0; i < 8; i++) x.v[i] = __builtin_bswap32(s[i]);
        fe_reduce_plain<Fn>(x.v, Fn::MAX_Q_IN);
        x = fe_to_mont<Fn>(x);
#pragma unroll
        for (int i = 0; i < 8; i++) ch[j][i] = x.v[i];
    }
    __syncthreads();
    if (j < 64) {
        Fe<Fn> acc = fe_one<Fn>();
#pragma unroll 1
        for (uint32_t r = 0; r < IPA_ROUNDS; r++) {
            Fe<Fn> x;
#pragma unroll
            for (int i = 0; i < 8; i++) { x.v[i] = ch[r][i]; red[r][i] = acc.v[i]; }     // red[r]: x_0 .. x_(r-1); every lane writes the same
            acc = fe_mul<Fn>(acc, x);
        }
        Fe<Fn> inv = fe_inv_dev<Fn>(acc);
#pragma unroll 1
        for (int r = IPA_ROUNDS - 1; r >= 0; r--) {
            Fe<Fn> x, pre;
#pragma unroll
            for (int i = 0; i < 8; i++) { x.v[i] = ch[r][i]; pre.v[i] = red[r][i]; }
            const Fe<Fn> xi = fe_mul<Fn>(inv, pre);
            inv = fe_mul<Fn>(inv, x);
#pragma unroll
            for (int i = 0; i < 8; i++) ch[IPA_ROUNDS + r][i] = xi.v[i];
        }
    } else if (j < 64 + IPA_VERIFY_POINTS) {
        const uint32_t i = j - 64;
        const uint8_t* c = i < 3 ? rec + 33 * i : proof + 32 + 33 * (i - 3);
        Fe<Fp> x, y;
        if (!ipa_decompress(c, x, y)) atomicOr(&bad, 1u);
#pragma unroll
        for (int t = 0; t < 8; t++) { pts[i][t] = x.v[t]; pts[i][8 + t] = y.v[t]; }
    }
    __syncthreads();
    Fe<Fn> xv = fe_one<Fn>();
#pragma unroll 1
    for (uint32_t r = 0; r < IPA_ROUNDS; r++) {
        const uint32_t at = ((j >> (6 - r)) & 1u) ? r : IPA_ROUNDS + r;
        Fe<Fn> f;
#pragma unroll
        for (int i = 0; i < 8; i++) f.v[i] = ch[at][i];
        xv = fe_mul<Fn>(xv, f);
    }
    const Fe<Fn> a_own = load_le_scalar_mont(tail + 64 * (j & 1u));
    const Fe<Fn> s_j = fe_from_mont<Fn>(fe_mul<Fn>(a_own, xv));
    Fe<Fn> vp;
#pragma unroll
    for (int i = 0; i < 8; i++) vp.v[i] = D.a_value[i];
    vp = fe_to_mont<Fn>(vp);
#pragma unroll 1
    for (uint32_t i = 0; i + 1 < IPA_N; i++) {
        const Fe<Fn> sq = fe_mul<Fn>(vp, vp);
        if (i < j) vp = sq;
    }
    const Fe<Fn> term = fe_mul<Fn>(vp, xv), zero = fe_zero<Fn>();
    const Fe<Fn> even = block_sum((j & 1u) ? zero : term, red), odd = block_sum((j & 1u) ? term : zero, red);
    const bool ok = bad == 0;
    store_be256(rows + ((size_t)k * IPA_ROW_COEFFS + j) * 32, ok ? s_j.v : zero.v);
    if (j == 0) {
        const Fe<Fn> a0 = load_le_scalar_mont(tail), b0 = load_le_scalar_mont(tail + 32), a1 = load_le_scalar_mont(tail + 64),
                     b1 = load_le_scalar_mont(tail + 96), c = load_le_scalar_mont(proof);
        const Fe<Fn> cu = fe_from_mont<Fn>(fe_sub<Fn>(fe_add<Fn>(fe_mul<Fn>(a0, b0), fe_mul<Fn>(a1, b1)), c));
        store_be256(rows + ((size_t)k * IPA_ROW_COEFFS + IPA_N) * 32, ok ? cu.v : zero.v);
        const bool bvec = fe_eq<Fn>(even, b0) && fe_eq<Fn>(odd, b1);
        flags[k] = ok ? (bvec ? PORLA_IPA_VERIFY_BVEC : 0) : PORLA_IPA_VERIFY_MALFORMED;
    }
    if (j < IPA_VERIFY_PAIRS) {
        Fe<Fn> sc = fe_zero<Fn>();
        uint32_t pt;
        if (j < 3) {
            pt = j == 0 ? 0u : (j == 1 ? 2u : 1u);
#pragma unroll
            for (int i = 0; i < 8; i++) sc.v[i] = j == 0 ? D.alpha[i] : (j == 1 ? D.nalpha[i] : Fn::P[i]);
            if (j == 2) sc.v[0] -= 1;                                    // n - 1
        } else if (j == 3) {
            pt = 0;
            sc.v[0] = 1;
        } else {
            const uint32_t q = j - 4, r = q >> 1;
            pt = 3 + q;
            Fe<Fn> f;
#pragma unroll
            for (int i = 0; i < 8; i++) f.v[i] = ch[(q & 1u) ? IPA_ROUNDS + r : r][i];
            sc = fe_from_mont<Fn>(fe_mul<Fn>(f, f));
        }
        const size_t at = (size_t)D.pair0 + D.n + j;
        uint32_t x[8], y[8];
#pragma unroll
        for (int i = 0; i < 8; i++) { x[i] = ok ? pts[pt][i] : 0u; y[i] = ok ? pts[pt][8 + i] : 0u; }
        store_be256(scalars + 32 * at, ok ? sc.v : zero.v);
        store_be256(points + 64 * at, x);
        store_be256(points + 64 * at + 32, y);
    }
}

// ---- the complement entries.  Block b covers pairs [64 (b - gat0), ...) of reply gat_reply[b].
__global__ void __launch_bounds__(4 * KZG_GATHER_PAIRS)
k_ipa_verify_gather(const IpaVerifyDesc* __restrict__ desc, const uint32_t* __restrict__ gat_reply, uint8_t* __restrict__ scalars,
                    uint8_t* __restrict__ points) {
    const IpaVerifyDesc& D = desc[gat_reply[blockIdx.x]];
    kzg_gather_pairs<false>(D.comp_store, nullptr, D.idx, D.coef, D.n, D.pair0, blockIdx.x - D.gat0, scalars, points);
}

// ---- a lane per reply: msm[3a] + msm[3a + 1] = O -> FULL; msm[3a + 2] - row a (of the pass, at rows[a S]) = O -> PROOF; with the
// prep's BVEC; a malformed reply keeps MALFORMED alone.  Sums of projective points against infinity: no inversion.
__global__ void __launch_bounds__(64)
k_ipa_verify_join(const XYZZ<Secp256k1Fp>* __restrict__ msm, const XYZZ<Secp256k1Fp>* __restrict__ rows, uint32_t S, uint32_t k,
                  const uint8_t* __restrict__ flags, uint8_t* __restrict__ status) {
    using M = Secp256k1Fp;
    const uint32_t a = blockIdx.x * 64 + threadIdx.x;
    if (a >= k) return;
    uint8_t f = flags[a];
    if (!(f & PORLA_IPA_VERIFY_MALFORMED)) {
        XYZZ<M> s = load_xyzz<M>(msm + 3 * (size_t)a);
        const XYZZ<M> t = load_xyzz<M>(msm + 3 * (size_t)a + 1);
        xyzz_add_cold<M>(&s, &t);
        if (xyzz_is_inf<M>(s)) f |= PORLA_IPA_VERIFY_FULL;
        XYZZ<M> p = load_xyzz<M>(msm + 3 * (size_t)a + 2);
        XYZZ<M> r = load_xyzz<M>(rows + (size_t)a * S);
        r.y = fe_neg<M>(r.y);
        xyzz_add_cold<M>(&p, &r);
        if (xyzz_is_inf<M>(p)) f |= PORLA_IPA_VERIFY_PROOF;
    }
    status[a] = f;
}

// ---- per-device workspace: the work list (pinned staging + device copy), the MSM entries and sums, the rows, the prep's flags.  One
// call at a time enqueues (mu); `fence` orders the buffers between calls on different streams.
struct IpaVerifyWs {
    std::mutex mu;
    int device = -1;
    Buf list, msm_sc, msm_pt, msm_sums, rows, flags;
    PinnedList h_list;
    UseFence fence;
};
static PerDevice<IpaVerifyWs> g_ivb_ws;

// ws->mu held, ws->fence entered.  Every buffer is sized before the first launch, so a k whose buffers cannot exist fails there.
static int verify_enqueue(IpaVerifyWs* ws, FixedBase<Secp256k1G>& fb, const porla_ipa_verify_req* reqs, size_t k, const uint8_t* d_records,
                          uint8_t* d_status, hipStream_t stream) {
    int rc;
    // ---- the plan: entry 3a = reply a's complements, 3a + 1 = its 3-pair entry, 3a + 2 = its 13-pair entry
    std::vector<IpaVerifyDesc> desc(k);
    std::vector<uint64_t> offsets(3 * k + 1);
    uint64_t gblocks = 0, pairs = 0;
    auto mod_n = [](uint32_t out[8], const uint8_t be[32]) {
        h_load_be(out, be);
        fe_reduce_plain<Fn>(out, Fn::MAX_Q_IN);
    };
    for (size_t a = 0; a < k; a++) {
        const porla_ipa_verify_req& R = reqs[a];
        IpaVerifyDesc& D = desc[a];
        D.comp_store = (const uint8_t*)R.d_comp_store; D.idx = R.d_idx; D.coef = R.d_coef;
        D.n = (uint32_t)R.n;
        D.gat0 = (uint32_t)gblocks;
        D.pair0 = pairs;
        Fe<Fn> al;
        mod_n(al.v, R.alpha);
        const Fe<Fn> nal = fe_neg<Fn>(al);
        memcpy(D.alpha, al.v, 32);
        memcpy(D.nalpha, nal.v, 32);
        mod_n(D.a_value, R.a_value);
        offsets[3 * a] = pairs;
        offsets[3 * a + 1] = pairs + R.n;
        offsets[3 * a + 2] = pairs + R.n + 3;
        pairs += R.n + IPA_VERIFY_PAIRS;
        gblocks += gather_blocks(R.n);
    }
    offsets[3 * k] = pairs;
    if (gblocks > 0xffffffffull) { set_last_error("porla: verify batch too large for one call"); return PORLA_ERR_ARG; }
    // ---- the work list: descriptors | gather block -> reply, one pinned buffer, one copy
    const size_t desc_b = k * sizeof(IpaVerifyDesc);
    const size_t list_b = desc_b + 4 * (size_t)gblocks;
    if ((rc = ws->h_list.stage(list_b))) return rc;
    {
        uint8_t* h = (uint8_t*)ws->h_list.h;
        memcpy(h, desc.data(), desc_b);
        fill_owner_list((uint32_t*)(h + desc_b), k, [&](size_t a) { return gather_blocks(desc[a].n); });
    }
    if ((rc = ws->list.ensure(list_b))) return rc;
    if ((rc = ws->msm_sc.ensure((size_t)pairs * 32 + 64))) return rc;
    if ((rc = ws->msm_pt.ensure((size_t)pairs * 64 + 64))) return rc;
    if ((rc = ws->msm_sums.ensure(3 * k * sizeof(XYZZ<Secp256k1Fp>)))) return rc;
    if ((rc = ws->rows.ensure(k * IPA_ROW_COEFFS * 32))) return rc;
    if ((rc = ws->flags.ensure(k))) return rc;
    if ((rc = ws->h_list.send(ws->list.p, list_b, stream))) return rc;
    const IpaVerifyDesc* d_desc = (const IpaVerifyDesc*)ws->list.p;
    const uint32_t* d_gat = (const uint32_t*)((const uint8_t*)ws->list.p + desc_b);
    uint8_t* sc = (uint8_t*)ws->msm_sc.p;
    uint8_t* pt = (uint8_t*)ws->msm_pt.p;
    uint8_t* rows = (uint8_t*)ws->rows.p;
    uint8_t* flags = (uint8_t*)ws->flags.p;
    {
        ProfScope ps("ipa_verify_prep", stream);
        hipLaunchKernelGGL(k_ipa_verify_prep, dim3((unsigned)k), dim3(IPA_N), 0, stream, d_desc, d_records, sc, pt, rows, flags);
        PORLA_HIP(hipGetLastError());
    }
    if (gblocks) {
        ProfScope ps("ipa_verify_gather", stream);
        hipLaunchKernelGGL(k_ipa_verify_gather, dim3((unsigned)gblocks), dim3(4 * KZG_GATHER_PAIRS), 0, stream, d_desc, d_gat, sc, pt);
        PORLA_HIP(hipGetLastError());
    }
    XYZZ<Secp256k1Fp>* msm_sums = (XYZZ<Secp256k1Fp>*)ws->msm_sums.p;
    if ((rc = msm_batch_sums_device<Secp256k1G>(sc, pt, offsets.data(), 3 * k, msm_sums, stream))) return rc;
    return commit_then(fb, rows, k, IPA_ROW_COEFFS, stream, [&](const XYZZ<Secp256k1Fp>* sums, uint32_t S) {
        ProfScope ps("ipa_verify_join", stream);
        hipLaunchKernelGGL(k_ipa_verify_join, dim3((unsigned)((k + 63) / 64)), dim3(64), 0, stream, (const XYZZ<Secp256k1Fp>*)msm_sums, sums, S,
                           (uint32_t)k, (const uint8_t*)flags, d_status);
        PORLA_HIP(hipGetLastError());
        return (int)PORLA_OK;
    });
}

}  // namespace porla

using namespace porla;

static_assert(sizeof(porla_ipa_verify_req) == PORLA_IPA_VERIFY_REQ_BYTES, "porla_ipa_verify_req size");
static_assert(offsetof(porla_ipa_verify_req, d_comp_store) == 0 && offsetof(porla_ipa_verify_req, d_idx) == 8 &&
              offsetof(porla_ipa_verify_req, d_coef) == 16 && offsetof(porla_ipa_verify_req, n) == 24 &&
              offsetof(porla_ipa_verify_req, alpha) == 32 && offsetof(porla_ipa_verify_req, a_value) == 64,
              "porla_ipa_verify_req offsets (include/porla_gpu.h)");

extern "C" int porla_ipa_verify_batch_device(porla_fixed_base* gens_u_fb, const porla_ipa_verify_req* reqs, size_t k, const void* d_records,
                                             uint8_t* d_status, void* hip_stream) {
    static const char* who = "porla_ipa_verify_batch_device";
    if (k && (!reqs || !d_records || !d_status || !gens_u_fb)) return bad_arg(who, "reqs, d_records, d_status or gens_u_fb is NULL");
    size_t bytes;
    if (!mul_ok(k, IPA_RECORD + (size_t)IPA_ROW_COEFFS * 32 + 3 * sizeof(XYZZ<Secp256k1Fp>) + sizeof(IpaVerifyDesc) + 96 * IPA_VERIFY_PAIRS,
                &bytes))
        return bad_arg(who, "k replies overflow a byte size");
    uint64_t pairs = 0;
    for (size_t a = 0; a < k; a++) {
        const porla_ipa_verify_req& R = reqs[a];
        if (R.n && (!R.d_comp_store || !R.d_idx || !R.d_coef)) return bad_arg(who, "a NULL complement or challenge array with n > 0");
        if (R.n > IPA_VERIFY_MAX_N) return bad_arg(who, "n > 32768 (the batched MSM's entry limit)");
        pairs += R.n + IPA_VERIFY_PAIRS;
    }
    if (!mul_ok((size_t)pairs, 96, &bytes)) return bad_arg(who, "the batch's byte size overflows");
    if (k == 0) return PORLA_OK;
    int rc = ensure_device();
    if (rc) return rc;
    if ((rc = ipa_check_base(gens_u_fb, who))) return rc;
    IpaVerifyWs* ws = nullptr;
    if ((rc = g_ivb_ws.get(&ws))) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    return FencedCall(ws, stream).run(
        [&] { return verify_enqueue(ws, gens_u_fb->secp, reqs, k, (const uint8_t*)d_records, d_status, stream); });
}
