// Kernels of the top-level repair (repair_batch.hip: porla_{kzg,ipa}_repair_top_batch_device): the damaged rows of a top level are
// written back in place from the other half.  The rebuild that wrote the top level scaled every chunk of the Y part by ONE wt = w^e,
// e = reverse_bits(top_step % n_total), and the network is linear, so row by row Y_j = wt X_j mod LCM (mod p_icc in the RESIDUE32
// form): a row that fails its check while its sibling passes is a function of the sibling.
//
// The row check is the aligned retrieval's under RtMapStarts (retrieve_batch.hip.h), the two halves of every file as two requests of
// one pass.  k_rp_patch then writes the data rows, both directions and all files in one launch; the check's expected-MAC stages run
// once more over the rows as repaired and their last kernel writes the MAC rows (RtActWrite, retrieve_batch.hip.h).  The action bytes
// are written in that order: zero (k_rp_clear), LOST or the data bit (k_rp_patch: a lost row has no data bit, so no two values meet in
// one byte), the MAC bit (the write kernel, a lane per row, which also counts the rewritten rows of both kinds).
#pragma once
#include "retrieve_batch.hip.h"
#include "icc_decode.hip.h"
#include "../../include/porla_gpu.h"

namespace porla {

// one file as the kernels see it; half 0 = X, 1 = Y
struct RpFile {
    uint8_t* rows[2];          // d_rows_x, d_rows_y
    const uint8_t* status[2];  // d_status_x, d_status_y: written by the check pass
    uint8_t* action[2];        // d_action_x, d_action_y
    uint32_t* counts;          // d_counts or nullptr
    uint32_t e;                // reverse_bits(top_step % n_total, log2 n_total): wt = w^e
    uint32_t pad;
};
static_assert(sizeof(RpFile) == 64, "RpFile: seven pointers and two words");

// the action bytes of both halves and the eight counters: zero
__global__ void __launch_bounds__(256)
k_rp_clear(const RpFile* __restrict__ files, uint32_t n_total) {
    const RpFile& F = files[blockIdx.y];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_total) { F.action[0][i] = 0; F.action[1][i] = 0; }
    if (i < 8u && F.counts) F.counts[i] = 0;
}

// wt^-1 v (INVERSE) or wt v of the stored symbol at src, canonical in FORM's modulus, as SYMB / 16 16-byte words.  FORM:
// PORLA_ICC_DECODE_EXACT (64-byte symbols, both planes, joined below LCM as the encode's finish joins them) or
// PORLA_ICC_DECODE_RESIDUE32 (32-byte symbols, the p_icc plane alone; Q and the q tables are unused).  tp, tq: the factor's two planes
// in the 2^270 form.  Any input bytes are defined: the symbol enters below 2 p by the decode's load step (icd_load64; a 256-bit value
// is below 2 p_icc as it is), the product with a table entry is below p + 2^250, the finish makes it canonical -- k_ex_top_patch's chain
template <int FORM, class Q>
__device__ __forceinline__ void rp_scale_symbol(const uint8_t* __restrict__ src, const F30<IccFp>& tp, const F30<Q>& tq, uint4* c) {
    if (FORM == PORLA_ICC_DECODE_EXACT) {
        const F30<IccFp> rp = icc30_mul<IccFp>(tp, icd_load64<IccFp>(src));
        const F30<Q> rq = icc30_mul<Q>(tq, icd_load64<Q>(src));
        IccOut o;
        o.x = reinterpret_cast<uint8_t*>(c); o.al = nullptr; o.sc = nullptr; o.qres = nullptr; o.scalar_le = 0;
        icc30_finish_q<Q>(icc30_finish_p(rp), rq, 0, o);
    } else {
        const F30<IccFp> y = f30_unpack<IccFp>(ld_fe<IccFp>(reinterpret_cast<const uint32_t*>(src)).v);
        const Fe<IccFp> r = icc30_finish_p(icc30_mul<IccFp>(tp, y));
        c[0] = make_uint4(r.v[0], r.v[1], r.v[2], r.v[3]);
        c[1] = make_uint4(r.v[4], r.v[5], r.v[6], r.v[7]);
    }
}

// ---- the data rows: a lane per symbol of both halves of file blockIdx.y, the X half's symbols first.  A symbol of a row that is not
// repairable is left alone (the first lane of a lost row says LOST, the X side counts the index).  A repairable row's candidate is
// wt^-1 times the sibling symbol for an X row -- the p_icc plane by entry (N - e) mod N of the encode's tw30p, the q plane by entry e of
// the decode's table of inverses -- and wt times it for a Y row: entry e of tw30p and entry e of the encode's q-plane table tw30q.  With
// e == 0 the sibling symbol is copied as it lies.  The sibling row checked OK and is never written, so no lane reads what another
// writes.  16-byte accesses, plain vector stores; the candidate goes over the symbol when it differs, and the row's action byte gets
// the data bit (every lane that writes it writes the same value).
template <int FORM, class Q>
__global__ void __launch_bounds__(256)
k_rp_patch(const RpFile* __restrict__ files, const uint32_t* __restrict__ twp, const uint32_t* __restrict__ twq,
           const uint32_t* __restrict__ twqi, uint32_t n_total, uint32_t ncols) {
    constexpr uint32_t SYMB = FORM == PORLA_ICC_DECODE_EXACT ? 64u : 32u;
    constexpr uint32_t W = SYMB / 16u;
    const RpFile& F = files[blockIdx.y];
    const size_t per = (size_t)n_total * ncols;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2 * per) return;
    const uint32_t h = t >= per ? 1u : 0u;
    const size_t i = t - (h ? per : 0);
    const uint32_t j = (uint32_t)(i / ncols);
    if (F.status[h][j] != 0) return;
    if (F.status[h ^ 1u][j] != PORLA_RETRIEVE_ROW_OK) {
        if (i == (size_t)j * ncols) {
            F.action[h][j] = PORLA_REPAIR_LOST;
            if (h == 0u && F.counts) atomicAdd(F.counts + 6, 1u);
        }
        return;
    }
    const uint8_t* src = F.rows[h ^ 1u] + SYMB * i;
    uint4* dst = reinterpret_cast<uint4*>(F.rows[h] + SYMB * i);
    uint4 c[W];
    if (F.e == 0u) {
        const uint4* s = reinterpret_cast<const uint4*>(src);
#pragma unroll
        for (uint32_t w = 0; w < W; w++) c[w] = s[w];
    } else {
        const F30<IccFp> tp = h ? icc30_ld_pslot<IccFp>(twp + (size_t)F.e * ICC30_PSLOT_WORDS) : icd_tw<IccFp>(twp, n_total, F.e);
        F30<Q> tq{};
        if (FORM == PORLA_ICC_DECODE_EXACT) tq = h ? icc30_ld_pslot<Q>(twq + (size_t)F.e * ICC30_PSLOT_WORDS) : icd_tw<Q>(twqi, n_total, F.e);
        rp_scale_symbol<FORM, Q>(src, tp, tq, c);
    }
    uint32_t diff = 0;
#pragma unroll
    for (uint32_t w = 0; w < W; w++) {
        const uint4 m = dst[w];
        diff |= (c[w].x ^ m.x) | (c[w].y ^ m.y) | (c[w].z ^ m.z) | (c[w].w ^ m.w);
    }
    if (!diff) return;
#pragma unroll
    for (uint32_t w = 0; w < W; w++) dst[w] = c[w];
    F.action[h][j] = PORLA_REPAIR_DATA;
}

}  // namespace porla
