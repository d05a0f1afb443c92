// The ragged ICC decode: levels of UNEQUAL sizes in one call (include/porla_gpu.h: porla_icc_decode_ragged_batch_device).  The
// arithmetic, the tiles, the rounds and the bounds chain are icc_decode.hip.h's, unchanged: what differs is how a work-group learns
// which request and which tile it has.  The uniform kernels read the request from blockIdx.y and the shape of the pass (n, s0, ns,
// cc_log) from their arguments; here grid.x is the tile count of ALL requests of the launch and a block
//
//   * binary-searches the launch's tile starts (one entry per request plus one: request r owns the blocks [starts[r], starts[r + 1]))
//     for its request and its tile index inside it -- the row check's RtMapStarts at tile granularity;
//   * reads the request's shape from its descriptor (IcdRagDesc: log2 n_rows, the pass's s0 / ns / cc_log as the host planned them
//     with icc_pass_plan, the word offset of its residue planes) and its n_rows^-1 from a table indexed by log2 n_rows, both in the
//     uploaded list -- scalar loads, uniform over the block;
//   * builds its tile with icc30_block_tile's explicit map (IccTileAt) and goes on as the uniform kernels do.
//
// A launch holds the requests of one pass class only (FIRST && LAST: the one-pass requests; FIRST, then LAST: those of two passes),
// so FIRST and LAST stay template parameters and the launches of a call depend on the classes present, not on K or on the sizes.
// The kernel bodies repeat k_icd_exact / k_icd_residue instead of sharing a __forceinline__ body with them: that form cost the check
// kernels a wave per SIMD when it was tried there (DESIGN s4), and the uniform instances must keep their registers.
#pragma once
#include "icc_decode.hip.h"

namespace porla {

// a request of the ragged decode as the kernels see it: porla_icc_decode_req's four pointers, then the shape
struct IcdRagDesc {
    IcdDesc d;
    uint32_t logn;                 // log2 n_rows
    uint32_t shape[3];             // pass z of icc_pass_plan(logn, n_cols): s0 | ns << 8 | cc_log << 16
    unsigned long long work;       // the request's residue planes: a word offset into the workspace's planes (more than one pass)
    unsigned long long reserved;
};
static_assert(sizeof(IcdRagDesc) == 64, "IcdRagDesc: the request, its shape, its planes");
constexpr int ICD_RAG_MAX_PASSES = 3;
constexpr int ICD_RAG_MAX_LOG = 16;                     // n_total <= 2^16: the scale table has ICD_RAG_MAX_LOG + 1 entries

// the request and the tile of the calling block: starts[r] <= blockIdx.x < starts[r + 1], r < k (every request has a tile)
struct IcdRagAt { uint32_t req, tile, tiles; };
__device__ __forceinline__ IcdRagAt icd_rag_find(const uint32_t* __restrict__ starts, uint32_t k) {
    const uint32_t b = blockIdx.x;
    uint32_t lo = 0, hi = k;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (starts[mid] <= b) lo = mid;
        else hi = mid;
    }
    const uint32_t s = starts[lo];
    return IcdRagAt{lo, b - s, starts[lo + 1] - s};
}
__device__ __forceinline__ IccTile icd_rag_tile(const IcdRagDesc& R, const IcdRagAt& at, uint32_t ncols, int pz) {
    const uint32_t sh = R.shape[pz];
    return icc30_block_tile(1u << R.logn, ncols, (int)(sh & 0xffu), (int)((sh >> 8) & 0xffu), (int)(sh >> 16), false,
                            IccTileAt{at.tile, at.tiles});
}

// ---- PORLA_ICC_DECODE_EXACT: pass pz of the requests desc[0 .. k), both planes; k_icd_exact with the request and tile looked up
template <class Q, bool FIRST, bool LAST>
__global__ void __launch_bounds__(ICC30_SPLIT_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4)))
k_icd_exact_ragged(const IcdRagDesc* __restrict__ desc, const uint32_t* __restrict__ starts, uint32_t k, int pz,
                   const IcdScale* __restrict__ scales, uint32_t* __restrict__ work, const uint32_t* __restrict__ twp,
                   const uint32_t* __restrict__ twqi, uint32_t tw_n, uint32_t ncols) {
    __shared__ uint2 lds2[ICC_TILE_ELEMS * ICC30_PSLOT_WORDS / 2];
    uint32_t* lds = reinterpret_cast<uint32_t*>(lds2);
    constexpr int SRC = FIRST ? ICD_ROWS64 : ICD_WORK;
    const IcdRagAt at = icd_rag_find(starts, k);
    const IcdRagDesc& R = desc[at.req];
    const IcdDesc D = R.d;
    const IcdScale* const sc = scales + R.logn;
    uint32_t* work_p = work + R.work;
    uint32_t* work_q = work_p + ((size_t)ncols << R.logn) * ICC30_PLANE_WORDS;
    const IccTile T = icd_rag_tile(R, at, ncols, pz);
    uint32_t slot[4];
    {
        F30<IccFp> rp[4];
        icd_plane<IccFp, SRC>(lds, T, D.rows, work_p, twp, tw_n, rp, slot);
        const F30<IccFp> K = f30_unpack<IccFp>(sc->p);
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
        const F30<Q> K = f30_unpack<Q>(sc->q);
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
                    for (int j = 0; j < 8; j++) pq.v[j] = P.v[j];
                    fe_reduce_small<Q, Q::MAX_Q_P>(pq.v);                  // P < p_icc <= (MAX_Q_P + 1) q
                    const Fe<Q> df = fe_sub<Q>(aq, pq);
                    const Fe<Q> t = icc30_canonical<Q>(icc30_mul<Q>(f30_unpack<Q>(df.v), f30_const<Q>(Icc30Const<Q>::PINV270)));
                    uint32_t hi = 0;
#pragma unroll
                    for (int j = 1; j < 8; j++) hi |= t.v[j];
                    if (hi != 0 || t.v[0] > 1u) {
                        if (D.bad) atomicAdd(D.bad, 1u);
                    } else if (t.v[0] == 1u) {
                        Fe<IccFp> S;
                        uint32_t c = 0;
#pragma unroll
                        for (int j = 0; j < 8; j++) S.v[j] = adc32(P.v[j], IccFp::P[j], c);
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

// ---- PORLA_ICC_DECODE_RESIDUE64 / _RESIDUE32: pass pz of the requests desc[0 .. k), the p_icc plane alone; k_icd_residue with the
// request and tile looked up (steps: the request's own n_rows values)
template <int SRC, bool LAST>
__global__ void __launch_bounds__(ICC30_SPLIT_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4)))
k_icd_residue_ragged(const IcdRagDesc* __restrict__ desc, const uint32_t* __restrict__ starts, uint32_t k, int pz,
                     const IcdScale* __restrict__ scales, uint32_t* __restrict__ work, const uint32_t* __restrict__ twp, uint32_t tw_n,
                     int tw_log, uint32_t ncols) {
    __shared__ uint2 lds2[ICC_TILE_ELEMS * ICC30_PSLOT_WORDS / 2];
    uint32_t* lds = reinterpret_cast<uint32_t*>(lds2);
    const IcdRagAt at = icd_rag_find(starts, k);
    const IcdRagDesc& R = desc[at.req];
    const IcdDesc D = R.d;
    const IcdScale* const sc = scales + R.logn;
    uint32_t* work_p = work + R.work;
    const IccTile T = icd_rag_tile(R, at, ncols, pz);
    uint32_t slot[4];
    F30<IccFp> rp[4];
    icd_plane<IccFp, SRC>(lds, T, D.rows, work_p, twp, tw_n, rp, slot);
    const F30<IccFp> K = f30_unpack<IccFp>(sc->p);
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

// the counters of the requests that have one, zeroed in front of the passes
static __global__ void __launch_bounds__(256)
k_icd_clear_ragged(const IcdRagDesc* __restrict__ desc, uint32_t k) {
    const uint32_t a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a < k && desc[a].d.bad) *desc[a].d.bad = 0u;
}

}  // namespace porla
