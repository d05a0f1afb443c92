// The ICC decode: the data network of icc30_split.hip.h run BACKWARDS, for K independent levels in one call (include/porla_gpu.h:
// porla_icc_decode_batch_device).  The reference never wrote this step (its icc/*.m toy demonstrates it); it is the inverse of
// Server::CRebuild_Cached's X part (porla/Server/Server.hpp:1548-1687) and of the chain of Server::mix calls that builds a level.
//
// WHAT: stage s of the encode is (a, b) <- (a + vi b, a - vi b) on the rows k, k + 2^(s-1); its inverse is (a, b) <- ((a + b) / 2,
// (a - b) / (2 vi)).  The stages run from log2 n_rows down to 1 as (a, b) <- (a + b, (a - b) vi^-1) and the 2^-1 of every stage is
// collected into ONE factor n_rows^-1 per plane, which the finish multiplies by (in the 2^270 form it is the integer 2^(270 - log2
// n_rows) mod the modulus: the host reduces it, IcdScale).  Z/LCM = Z/p_icc x Z/q, so the two residues are inverted separately and
// joined at the end.
//
// Twiddles: vi = w^e mod p_icc, e = j N / 2^(s-1) with N = n_total (root_w(n)^(n / m2) does not depend on n, so the table of n_total
// serves every n_rows <= n_total).  Mod p_icc w has order N: vi^-1 = w^(N - e), entry (N - e) mod N of the encode's tw30p.  Mod q the
// encode multiplies by the INTEGER (w^e mod p_icc) mod q, which is no power of anything: its inverse is a true inversion mod q, one
// table per (n_total, curve) built by k_icd_twiddles_qinv with the division steps of inv30.hip.h (none of the residues is 0 mod q).
//
// HOW: the encode's tiles and passes (icc_pass_plan, icc30_block_tile, icc30_symbol_index) with the passes in reverse order and,
// inside a pass, the rounds in reverse order: a radix-2 round first when the stage count is odd, then radix-4 rounds -- stage d + 1
// on the pairs (0, 2), (1, 3), then stage d on (0, 1), (2, 3) -- one plane through the LDS region at a time.  The first round of a
// plane reads from memory (the 64-byte symbols, the 32-byte rows of the aligned store, or the plane's work array), the last one
// (d = 0: four neighbouring rows) leaves its symbols in registers for the work array or the finish.
//
// BOUNDS: in the encode a sum adds a fresh product, so a symbol gains 2 p per stage.  Here a + b adds two unreduced symbols and row
// 0 of a tile is never multiplied: left alone it doubles per stage.  So EVERY symbol of the stream is below 2 p, at every stage:
//   * the load step: a 64-byte symbol is hi C526 + lo < (p + 2^242) + 2^256 < 2^258, then icc30_reduce_top: < 2 p; a 32-byte row is
//     any 256-bit value, < 2 p_icc as it is;
//   * a butterfly: a + b < 4 p goes through icc30_reduce_top: < 2 p; a - b + 3 p < 5 p (icc30_sub<3>: b < 2 p) is multiplied by the
//     inverse twiddle (< p + 2^250 < 2^257 as an operand): the product is below p + 2^250 < 2 p;
//   * the finish: products again, then icc30_reduce_top + icc30_canonical.
// 4 p and 5 p are far below the 2^263 a product and icc30_reduce_top take; tools/check_fe30_bounds.py:check_icc_decode_chain walks
// this chain for the three moduli.  The cost of the bound is one short reduction per butterfly (9 multiply-adds; for p_icc, whose
// limbs 1..7 are zero, almost nothing) beside the butterfly's product.
#pragma once
#include "icc30_split.hip.h"
#include "inv30.hip.h"

namespace porla {

// a request as the kernels see it: the layout of porla_icc_decode_req, uploaded as it is
struct IcdDesc {
    const uint8_t* rows;
    uint8_t* out;
    const unsigned long long* steps;
    uint32_t* bad;
};
static_assert(sizeof(IcdDesc) == 32, "IcdDesc is porla_icc_decode_req");

// n_rows^-1 in the 2^270 form, per plane: the plain integer 2^(270 - log2 n_rows) mod the modulus
struct IcdScale { uint32_t p[8], q[8]; };

// where the first round of a pass finds its symbols
enum IcdSrc { ICD_WORK = 0, ICD_ROWS64 = 1, ICD_ROWS32 = 2, ICD_LDS = 3 };

// the q plane's inverse twiddles: entry e = ((w^e mod p_icc) mod q)^-1 in the 2^270 form, 40-byte slots like tw30q.  tw: the
// twiddle table of icc.hip.h (2^256 Montgomery form).  The division steps vote across the wave, so no lane leaves early.
// The raw inverse is v^-1 plus a multiple of q that depends on the rounds the lane's WAVE ran (inv30.hip.h), so a slot of twqi is a
// representative of its residue below q + 2^250, not canonical bytes: the same entry may hold another representative in a table
// of another size or launch shape.  The butterflies take any representative in that range.
template <class Q>
__global__ void __launch_bounds__(256)
k_icd_twiddles_qinv(const IccElem<Q>* __restrict__ tw, uint32_t n, uint32_t* __restrict__ twqi) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    const Fe<Q> v = fe_from_mont<Q>(ld_elem<Q>(tw + (e < n ? e : 0)).q);          // the plain residue, non-zero
    const F30<Q> r = f30_inv_safegcd_raw<Q>(v);                                   // v^-1 + k q, below 4 q
    const F30<Q> t = icc30_mul<Q>(r, f30_const<Q>(Icc30Const<Q>::C540));          // -> the 2^270 form, below q + 2^250
    if (e < n) icc30_st_pslot<Q>(twqi + (size_t)e * ICC30_PSLOT_WORDS, t);
}

// the inverse of the twiddle with exponent idx < N: mod p_icc entry (N - idx) mod N of tw30p, mod q entry idx of the inverse table
template <class M>
__device__ __forceinline__ F30<M> icd_tw(const uint32_t* __restrict__ tw, uint32_t tw_n, uint32_t idx) {
    const uint32_t at = std::is_same<M, IccFp>::value ? ((tw_n - idx) & (tw_n - 1u)) : idx;
    return icc30_ld_pslot<M>(tw + (size_t)at * ICC30_PSLOT_WORDS);
}

// one inverse butterfly on one plane: (a, b) <- (a + b reduced below 2 p, (a - b + 3 p) w); a, b < 2 p in, < 2 p out
template <class M>
__device__ __forceinline__ void icd_bfly(F30<M>& a, F30<M>& b, const F30<M>& w) {
    const F30<M> d = icc30_sub<M, 3>(a, b);
    a = icc30_reduce_top<M>(icc30_add<M>(a, b));
    b = icc30_mul<M>(w, d);
}

// a 64-byte little-endian symbol mod the modulus of M, below 2 p (the load step of BOUNDS)
template <class M>
__device__ __forceinline__ F30<M> icd_load64(const uint8_t* __restrict__ sym) {
    const Fe<IccFp> lo = ld_fe<IccFp>(reinterpret_cast<const uint32_t*>(sym));
    const Fe<IccFp> hi = ld_fe<IccFp>(reinterpret_cast<const uint32_t*>(sym + 32));
    return icc30_reduce_top<M>(icc30_add<M>(icc30_mul<M>(f30_unpack<M>(hi.v), f30_const<M>(Icc30Const<M>::C526)), f30_unpack<M>(lo.v)));
}

// a tile symbol from where the pass finds it, below 2 p
template <class M, int SRC>
__device__ __forceinline__ F30<M> icd_fetch(const IccTile& T, uint32_t e, const uint8_t* __restrict__ rows, const uint32_t* __restrict__ work) {
    const size_t gi = icc30_symbol_index(T, e);
    if (SRC == ICD_ROWS64) return icd_load64<M>(rows + 64 * gi);
    if (SRC == ICD_ROWS32) return f30_unpack<M>(ld_fe<IccFp>(reinterpret_cast<const uint32_t*>(rows + 32 * gi)).v);
    return icc30_ld_work<M>(work + gi * ICC30_PLANE_WORDS);
}

// One round of a plane, the inverse of icc30_round: stages s + 1 and then s = s0 + d (RADIX4), or stage s alone, on the lane's
// symbols.  SRC: ICD_LDS or where the pass's first round reads; keep: the pass's last round leaves them in res[] / slot[].
template <class M, int SRC, bool RADIX4>
__device__ __forceinline__ void icd_round(uint32_t* lds, const IccTile& T, int d, bool keep, const uint8_t* __restrict__ rows,
                                          const uint32_t* __restrict__ work, const uint32_t* __restrict__ tw, uint32_t tw_n,
                                          F30<M> (&res)[4], uint32_t (&slot)[4]) {
    const uint32_t tid = threadIdx.x;
    const uint32_t Cc = 1u << T.cc_log;
    const int s = T.s0 + d;
    if (RADIX4) {
        const uint32_t col = tid & (Cc - 1), qq = tid >> T.cc_log;
        if (tid < (T.elems >> 2) && T.c0 + col < T.ncols) {
            const uint32_t low = qq & ((1u << d) - 1u);
            const uint32_t m0 = ((qq >> d) << (d + 2)) | low;
            uint32_t e[4];
            F30<M> a[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                e[i] = ((m0 | ((uint32_t)i << d)) << T.cc_log) + col;
                a[i] = SRC == ICD_LDS ? icc30_ld_pslot<M>(lds + (size_t)e[i] * ICC30_PSLOT_WORDS) : icd_fetch<M, SRC>(T, e[i], rows, work);
            }
            const uint32_t j = (low << T.lo_bits) + T.lo;                        // row index mod 2^(s-1)
            // stage s + 1: pair (0, 2) has j' = j, pair (1, 3) j' = j + 2^(s-1) -> exponent + N / 2
            const uint32_t i2 = j * (tw_n >> s);
            icd_bfly<M>(a[0], a[2], icd_tw<M>(tw, tw_n, i2));
            icd_bfly<M>(a[1], a[3], icd_tw<M>(tw, tw_n, i2 + (tw_n >> 1)));
            const F30<M> w1 = icd_tw<M>(tw, tw_n, j * (tw_n >> (s - 1)));
            icd_bfly<M>(a[0], a[1], w1);
            icd_bfly<M>(a[2], a[3], w1);
            if (keep) {
#pragma unroll
                for (int i = 0; i < 4; i++) { res[i] = a[i]; slot[i] = e[i]; }
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++) icc30_st_pslot<M>(lds + (size_t)e[i] * ICC30_PSLOT_WORDS, a[i]);
            }
        }
    } else {
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const uint32_t bf = tid + h * ICC30_SPLIT_THREADS;
            const uint32_t col = bf & (Cc - 1), qq = bf >> T.cc_log;
            if (bf < (T.elems >> 1) && T.c0 + col < T.ncols) {
                const uint32_t low = qq & ((1u << d) - 1u);
                const uint32_t m0 = ((qq >> d) << (d + 1)) | low;
                const uint32_t e0 = (m0 << T.cc_log) + col, e1 = ((m0 | (1u << d)) << T.cc_log) + col;
                F30<M> a = SRC == ICD_LDS ? icc30_ld_pslot<M>(lds + (size_t)e0 * ICC30_PSLOT_WORDS) : icd_fetch<M, SRC>(T, e0, rows, work);
                F30<M> b = SRC == ICD_LDS ? icc30_ld_pslot<M>(lds + (size_t)e1 * ICC30_PSLOT_WORDS) : icd_fetch<M, SRC>(T, e1, rows, work);
                const uint32_t j = (low << T.lo_bits) + T.lo;
                icd_bfly<M>(a, b, icd_tw<M>(tw, tw_n, j * (tw_n >> (s - 1))));
                if (keep) {
                    res[2 * h] = a; slot[2 * h] = e0;
                    res[2 * h + 1] = b; slot[2 * h + 1] = e1;
                } else {
                    icc30_st_pslot<M>(lds + (size_t)e0 * ICC30_PSLOT_WORDS, a);
                    icc30_st_pslot<M>(lds + (size_t)e1 * ICC30_PSLOT_WORDS, b);
                }
            }
        }
    }
}

// the ns stages of ONE plane of the block's tile, highest first: a radix-2 round when ns is odd, then radix-4 rounds down to d = 0.
// Out: the lane's (up to) four symbols of the last round in res[], their tile slots in slot[] (0xffffffff: none).  The caller syncs
// before the LDS region is used again.
template <class M, int SRC>
__device__ __forceinline__ void icd_plane(uint32_t* lds, const IccTile& T, const uint8_t* __restrict__ rows, const uint32_t* __restrict__ work,
                                          const uint32_t* __restrict__ tw, uint32_t tw_n, F30<M> (&res)[4], uint32_t (&slot)[4]) {
#pragma unroll
    for (int i = 0; i < 4; i++) slot[i] = 0xffffffffu;
    if (T.ns == 1) {
        icd_round<M, SRC, false>(lds, T, 0, true, rows, work, tw, tw_n, res, slot);
        return;
    }
    int d;
    if (T.ns & 1) {
        d = T.ns - 1;
        icd_round<M, SRC, false>(lds, T, d, false, rows, work, tw, tw_n, res, slot);
    } else {
        d = T.ns - 2;
        icd_round<M, SRC, true>(lds, T, d, d == 0, rows, work, tw, tw_n, res, slot);
    }
    while (d >= 2) {
        d -= 2;
        __syncthreads();
        icd_round<M, ICD_LDS, true>(lds, T, d, d == 0, rows, work, tw, tw_n, res, slot);
    }
}

// the row of the level a tile slot belongs to
__device__ __forceinline__ uint32_t icd_row(const IccTile& T, uint32_t e) { return T.row_base + ((e >> T.cc_log) << T.lo_bits); }

// ---- PORLA_ICC_DECODE_EXACT: one pass of request blockIdx.y, both planes.  FIRST reads the 64-byte symbols, LAST runs stages
// .. 1 and the finish: the p_icc plane stores r_p = chunk mod p_icc (canonical) in the symbol's 32 bytes of the output -- where the
// lane reads it back after the q plane, and what a bad symbol keeps -- then t = (r_q - r_p) p_icc^-1 mod q, the value is r_p + p_icc t:
// below 2^256 only for t = 0, or t = 1 with r_p + p_icc < 2^256.  Anything else cannot be a chunk: it is counted in the request's
// counter (an ordinary atomic add; k_icd_clear zeroed it) and keeps r_p.
template <class Q, bool FIRST, bool LAST>
__global__ void __launch_bounds__(ICC30_SPLIT_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4)))
k_icd_exact(const IcdDesc* __restrict__ desc, uint32_t* __restrict__ work, size_t plane_words, const uint32_t* __restrict__ twp,
            const uint32_t* __restrict__ twqi, uint32_t tw_n, uint32_t n, uint32_t ncols, int s0, int ns, int cc_log, IcdScale sc) {
    __shared__ uint2 lds2[ICC_TILE_ELEMS * ICC30_PSLOT_WORDS / 2];
    uint32_t* lds = reinterpret_cast<uint32_t*>(lds2);
    constexpr int SRC = FIRST ? ICD_ROWS64 : ICD_WORK;
    const IcdDesc D = desc[blockIdx.y];
    uint32_t* work_p = work + (size_t)blockIdx.y * 2 * plane_words;
    uint32_t* work_q = work_p + plane_words;
    const IccTile T = icc30_block_tile(n, ncols, s0, ns, cc_log, false);
    uint32_t slot[4];
    {
        F30<IccFp> rp[4];
        icd_plane<IccFp, SRC>(lds, T, D.rows, work_p, twp, tw_n, rp, slot);
        const F30<IccFp> K = f30_unpack<IccFp>(sc.p);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (slot[i] != 0xffffffffu) {
                const size_t gi = icc30_symbol_index(T, slot[i]);
                if (LAST) st_fe<IccFp>(reinterpret_cast<uint32_t*>(D.out + 32 * gi), icc30_finish_p(icc30_mul<IccFp>(K, rp[i])));
                else icc30_st_work<IccFp>(work_p + gi * ICC30_PLANE_WORDS, rp[i]);
            }
        }
        __syncthreads();                                 // every lane has read its last round's symbols: the region is free
    }
    {
        F30<Q> rq[4];
        icd_plane<Q, SRC>(lds, T, D.rows, work_q, twqi, tw_n, rq, slot);
        const F30<Q> K = f30_unpack<Q>(sc.q);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (slot[i] != 0xffffffffu) {
                const size_t gi = icc30_symbol_index(T, slot[i]);
                if (LAST) {
                    uint32_t* const o = reinterpret_cast<uint32_t*>(D.out + 32 * gi);
                    const Fe<IccFp> P = ld_fe<IccFp>(o);                   // what this lane stored after the p_icc plane
                    const Fe<Q> aq = icc30_canonical<Q>(icc30_reduce_top<Q>(icc30_mul<Q>(K, rq[i])));
                    Fe<Q> pq;
#pragma unroll
                    for (int k = 0; k < 8; k++) pq.v[k] = P.v[k];
                    fe_reduce_small<Q, Q::MAX_Q_P>(pq.v);                  // P < p_icc <= (MAX_Q_P + 1) q
                    const Fe<Q> df = fe_sub<Q>(aq, pq);
                    const Fe<Q> t = icc30_canonical<Q>(icc30_mul<Q>(f30_unpack<Q>(df.v), f30_const<Q>(Icc30Const<Q>::PINV270)));
                    uint32_t hi = 0;
#pragma unroll
                    for (int k = 1; k < 8; k++) hi |= t.v[k];
                    if (hi != 0 || t.v[0] > 1u) {
                        if (D.bad) atomicAdd(D.bad, 1u);
                    } else if (t.v[0] == 1u) {
                        Fe<IccFp> S;
                        uint32_t c = 0;
#pragma unroll
                        for (int k = 0; k < 8; k++) S.v[k] = adc32(P.v[k], IccFp::P[k], c);
                        if (c) { if (D.bad) atomicAdd(D.bad, 1u); }
                        else st_fe<IccFp>(o, S);
                    }
                } else {
                    icc30_st_work<Q>(work_q + gi * ICC30_PLANE_WORDS, rq[i]);
                }
            }
        }
    }
}

// ---- PORLA_ICC_DECODE_RESIDUE64 / _RESIDUE32: one pass of request blockIdx.y, the p_icc plane alone (a 64-byte symbol reduces on
// load).  LAST: output position i = chunk mod p_icc, canonical; with write steps it is first multiplied by wt_i^-1 = w^(N - e_i),
// e_i = reverse_bits(step_i % N, log2 N): entry (N - e_i) mod N of tw30p.
template <int SRC, bool LAST>
__global__ void __launch_bounds__(ICC30_SPLIT_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4)))
k_icd_residue(const IcdDesc* __restrict__ desc, uint32_t* __restrict__ work, size_t plane_words, const uint32_t* __restrict__ twp,
              uint32_t tw_n, int tw_log, uint32_t n, uint32_t ncols, int s0, int ns, int cc_log, IcdScale sc) {
    __shared__ uint2 lds2[ICC_TILE_ELEMS * ICC30_PSLOT_WORDS / 2];
    uint32_t* lds = reinterpret_cast<uint32_t*>(lds2);
    const IcdDesc D = desc[blockIdx.y];
    uint32_t* work_p = work + (size_t)blockIdx.y * plane_words;
    const IccTile T = icc30_block_tile(n, ncols, s0, ns, cc_log, false);
    uint32_t slot[4];
    F30<IccFp> rp[4];
    icd_plane<IccFp, SRC>(lds, T, D.rows, work_p, twp, tw_n, rp, slot);
    const F30<IccFp> K = f30_unpack<IccFp>(sc.p);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        if (slot[i] != 0xffffffffu) {
            const size_t gi = icc30_symbol_index(T, slot[i]);
            if (LAST) {
                F30<IccFp> r = icc30_mul<IccFp>(K, rp[i]);
                if (D.steps) {
                    const uint32_t e = __brev((uint32_t)D.steps[icd_row(T, slot[i])] & (tw_n - 1u)) >> (32 - tw_log);
                    r = icc30_mul<IccFp>(icd_tw<IccFp>(twp, tw_n, e), r);
                }
                st_fe<IccFp>(reinterpret_cast<uint32_t*>(D.out + 32 * gi), icc30_finish_p(r));
            } else {
                icc30_st_work<IccFp>(work_p + gi * ICC30_PLANE_WORDS, rp[i]);
            }
        }
    }
}

// ---- a level of ONE row in the form RESIDUE64 (level 0's Y row): no stage runs, the symbol is chunk * wt mod p_icc and the decode is
// the unscale alone, a lane per symbol of request blockIdx.y: wt^-1 = w^(N - e), e = reverse_bits(step % N, log2 N), as in the finish
// of k_icd_residue.  The symbol enters below 2 p (icd_load64), the product with the twiddle is below p + 2^250; out: canonical.
// steps: the one write step of the row (never nullptr here)
static __global__ void __launch_bounds__(256)
k_icd_row0(const IcdDesc* __restrict__ desc, const uint32_t* __restrict__ twp, uint32_t tw_n, int tw_log, uint32_t ncols) {
    const IcdDesc D = desc[blockIdx.y];
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncols) return;
    const uint32_t e = tw_log ? __brev((uint32_t)D.steps[0] & (tw_n - 1u)) >> (32 - tw_log) : 0u;
    const F30<IccFp> r = icc30_mul<IccFp>(icd_tw<IccFp>(twp, tw_n, e), icd_load64<IccFp>(D.rows + 64 * (size_t)c));
    st_fe<IccFp>(reinterpret_cast<uint32_t*>(D.out + 32 * (size_t)c), icc30_finish_p(r));
}

// the counters of the requests that have one, zeroed in front of the passes
static __global__ void __launch_bounds__(256)
k_icd_clear(const IcdDesc* __restrict__ desc, uint32_t k) {
    const uint32_t a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a < k && desc[a].bad) *desc[a].bad = 0u;
}

}  // namespace porla
