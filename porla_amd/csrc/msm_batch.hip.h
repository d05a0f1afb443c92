// Batched MSM: K independent MSMs of 0 .. SMALL_MAX_N pairs each over one concatenated scalar / point array, in a fixed number
// of launches per launch round, with the fold and the affine conversion on the device (porla_*_msm_batch_device, include/porla_gpu.h).
//
// One call of porla_*_msm_device costs ~0.1 ms whatever its size below a few thousand pairs: one launch, a chain of ~15 dependent
// additions, a host fold.  K of them cost K times that while the chip idles.  Here the host turns the offsets into a work list and
// every entry takes the form that suits its size:
//
//   tiny entries (<= BATCH_TINY_MAX = 64 pairs, empty ones included): k_batch_tiny -- one QUAD per pair (64 per block) runs the MAC
//       encode's ladder, quad30.hip.h:macq_ladder (endomorphism split, 33 signed 4-bit windows over a table of the multiples 1 .. 8 of
//       the point, accumulator in the quad's registers); the entry's quads then add their products as a tree (log2 n levels) and its
//       first quad writes the entry's sum.  A 1-pair entry is ~130 doublings + ~70 additions on four lanes.
//   larger entries: k_batch_bucket -- k_small_msm's block body (msm_small.hip.h:small_block) with a work list instead of gridDim:
//       block (entry, window, slice) over the entry's own pairs and allotment; the last block of a window copies the window's folded
//       sums into the entry's window sums (HBM).
//       An entry gets fewer blocks than a lone k_small_msm (ceil(n / 64), at least the windows' count): a lone MSM buys latency with
//       idle lanes, a batch fills the chip with other entries instead.  When the round's entries would occupy no more than two
//       blocks per compute unit even with the lone MSM's allotment (192, 256 above 4 096 pairs), they get that.
//   k_batch_fold -- one quad per bucket entry: the Horner fold over the W x c single-bit window sums (the fold host_fold64.hpp:
//       h_fold_tree64 runs on the host for a lone MSM), accumulator in registers.  The GLV recombination needs no step of its own:
//       the second sub-scalar's points enter the buckets as phi(P) (msm_small.hip.h).
//   k_fb_finish (fixed_base.hip.h) -- XYZZ -> affine, one division-step inversion per four entries (Montgomery's trick), big-endian
//       X || Y straight into the caller's output (64 zero bytes = infinity).
//
// Same group law and the same input handling (scalars reduced mod the group order, coordinates reduced mod p as SetBytes does),
// so each output is the same group element as porla_*_msm_device's and its 64 bytes are identical.
#pragma once
#include "msm_small.hip.h"
#include "fixed_base.hip.h"
#include "quad30.hip.h"

namespace porla {

constexpr int BATCH_QUADS = 64;                     // quads per block of k_batch_tiny / k_batch_fold (256 lanes)
constexpr uint32_t BATCH_TINY_MAX = BATCH_QUADS;    // entries of up to this many pairs: k_batch_tiny (one block holds them; crossover: DESIGN.md §4)
constexpr size_t BATCH_ROUND_ENTRIES = 1u << 18;    // per launch round: entries (the round's sums: 32 MiB) ...
constexpr size_t BATCH_ROUND_PAIRS = 1u << 24;      // ... pairs (32-bit offsets inside a round) ...
constexpr uint32_t BATCH_ROUND_BLOCKS = 1u << 15;   // ... bucket blocks (their partial sums and window sums: 2 x 32 MiB) ...
constexpr uint32_t BATCH_ROUND_QUADS = 1u << 20;    // ... and quads of k_batch_tiny
constexpr uint32_t BATCH_IDLE = 0xffffffffu;        // a quad of k_batch_tiny without a pair (padding: an entry's quads share a block)

// one entry of a round's work list: its pairs [off, off + n) relative to the round's first pair; bucket entries own the bucket
// blocks [base, base + blocks) of the round (their slots of the partial sums, the window sums and the arrival counters)
struct BatchEntry {
    uint32_t off, n, base, blocks;
};

// the quad's register-form point (lane r: coordinate r) into memory form at dst; infinity = zero words.  final: the 2^256 form
template <class M>
__device__ __forceinline__ void batch_store_point(XYZZ<M>* dst, const F30<M>& c, bool inf, uint32_t r, bool final) {
    if (inf) {
        uint4* d = reinterpret_cast<uint4*>(reinterpret_cast<uint32_t*>(dst) + 8 * r);
        d[0] = make_uint4(0, 0, 0, 0); d[1] = d[0];
    } else {
        xyzz30_store_coord<M>(dst, (int)r, c, final);
    }
}
// quad30.hip.h:macq_add for an operand e that may be infinity (zero words: skipped).  All four lanes together.
template <class M>
__device__ __forceinline__ void batch_add_maybe_inf(F30<M>& c, bool& inf, const XYZZ<M>* e, XYZZ<M>* slot_a, XYZZ<M>* slot_b, uint32_t r,
                                                    uint32_t lane) {
    bool z;
    (void)xyzz30_load_coord<M>(e, 2, &z);
    if (macq_quad_any(z, lane)) return;
    macq_add<M>(c, inf, e, reinterpret_cast<const uint32_t*>(e), false, slot_a, slot_b, r, lane);
}

// ---------------------------------------------------------------- tiny entries: one quad per pair
template <class M>
struct BatchTinyLds {
    struct Quad {
        XYZZ<M> tbl[8];            // (i + 1) P
        uint32_t bx[8][8];         // beta X of tbl[i]: the endomorphism's half reads its X here
    };
    Quad qd[BATCH_QUADS];
    XYZZ<M> res[BATCH_QUADS], sa[BATCH_QUADS], sb[BATCH_QUADS];
};

// tq[quad] = entry | pair << 20 (BATCH_IDLE: padding); an entry's quads are consecutive and in one block, its first (pair 0) writes
// sums[entry] in the 2^256 form.  An empty entry has one quad, which writes infinity.
template <class C>
__global__ void __launch_bounds__(4 * BATCH_QUADS)
k_batch_tiny(const uint8_t* __restrict__ scalars, const uint8_t* __restrict__ points, const BatchEntry* __restrict__ ents,
             const uint32_t* __restrict__ tq, uint32_t nq, XYZZ<typename C::Fp>* __restrict__ sums) {
    using M = typename C::Fp;
    __shared__ BatchTinyLds<M> L;
    const uint32_t tid = threadIdx.x, q = tid >> 2, r = tid & 3u, lane = tid & 63u;
    const uint32_t gq = blockIdx.x * BATCH_QUADS + q;
    const uint32_t code = gq < nq ? tq[gq] : BATCH_IDLE;
    const bool idle = code == BATCH_IDLE;
    const uint32_t e = code & 0xfffffu, j = code >> 20;
    BatchEntry E = {0, 0, 0, 0};
    if (!idle) E = ents[e];
    F30<M> c;
    bool inf = true;
    if (!idle && j < E.n) {
        const size_t p = (size_t)E.off + j;
        Affine<M> a;
        load_be256(a.x.v, points + p * 64);
        load_be256(a.y.v, points + p * 64 + 32);
        fe_reduce_plain<M>(a.x.v, 6);                      // G1Affine.Unmarshal: SetBytes reduces
        fe_reduce_plain<M>(a.y.v, 6);
        uint32_t k[8];
        load_be256(k, scalars + p * 32);
        for (int t = 0; t < C::MAX_Q; t++) {               // fr.SetBytes: reduced mod the group order
            uint32_t d[8];
            uint32_t br = 0;
#pragma unroll
            for (int t2 = 0; t2 < 8; t2++) d[t2] = sbb32(k[t2], C::ORDER[t2], br);
            if (br) break;
#pragma unroll
            for (int t2 = 0; t2 < 8; t2++) k[t2] = d[t2];
        }
        if (!aff_is_inf<M>(a)) {
            // P in the register form with ZZ = ZZZ = 1 (the 2^270 form for the Montgomery field; plain residues otherwise)
            Fe<M> one = fe_zero<M>();
            one.v[0] = 1;
            F30<M> v = f30_from_fe<M>(r == 0u ? a.x : (r == 1u ? a.y : one));
            if constexpr (!M::PSEUDO_MERSENNE) v = f30_mul<M>(v, f30_const<M>(M::RR_30));
            batch_store_point<M>(&L.qd[q].tbl[0], v, false, r, false);
            macq_sync();                                   // the ladder reads tbl[0]'s other coordinates
            macq_ladder<C>(L.qd[q], &L.sa[q], &L.sb[q], r, lane, k, c, inf);
        }
    }
    // the entry's sum as a tree over its quads (pairs 0 .. n - 1 sit on consecutive quads of this block): at level h the quads of
    // pair j = 0 mod 2h add the partial sum h quads further on -- log2(n) dependent additions instead of n - 1
    batch_store_point<M>(&L.res[q], c, inf, r, false);
    const uint32_t cnt = idle ? 0u : E.n;
#pragma unroll 1
    for (uint32_t h = 1; h < (uint32_t)BATCH_QUADS; h <<= 1) {
        __syncthreads();                                   // (every lane of the block passes every level's barrier)
        if (!idle && (j & (2 * h - 1)) == 0 && j + h < cnt) {
            batch_add_maybe_inf<M>(c, inf, &L.res[q + h], &L.sa[q], &L.sb[q], r, lane);
            batch_store_point<M>(&L.res[q], c, inf, r, false);
        }
    }
    if (idle || j != 0) return;
    batch_store_point<M>(sums + e, c, inf, r, true);
}

// ---------------------------------------------------------------- larger entries: the blocks of k_small_msm from a work list
// blk[block] = entry.  Block b - base of entry e is block (w, s) of e's shape (small_cfg over e's own allotment of blocks); the last
// block of window w to arrive writes its c sums (S, M_0 .. M_(c-2), memory form) to fin[base * SMALL_MAX_C + w * c + k].  Block 0 of
// the entry writes the shape (W | c << 8) to shape[e].  counters[base .. base + W) start at zero (the host clears them per round).
template <class C>
__global__ void __launch_bounds__(SMALL_THREADS) __attribute__((amdgpu_waves_per_eu(1, 1)))
k_batch_bucket(const uint8_t* __restrict__ scalars_r, const uint8_t* __restrict__ points_r, const BatchEntry* __restrict__ ents,
               const uint32_t* __restrict__ blk, int c_flags, XYZZ<typename C::Fp>* __restrict__ part, uint32_t* __restrict__ counters,
               XYZZ<typename C::Fp>* __restrict__ fin, uint32_t* __restrict__ shape) {
    using M = typename C::Fp;
    const uint32_t eidx = blk[blockIdx.x];
    const BatchEntry E = ents[eidx];
    const uint32_t bx = blockIdx.x - E.base;
    const SmallWindow<M> win = small_block<C>(
        scalars_r + (size_t)E.off * 32, points_r + (size_t)E.off * 64, E.n, bx, (int)E.blocks, c_flags, 0, part + (size_t)E.base * SMALL_MAX_C,
        counters + E.base, [&](const SmallCfg& g) {
            // (the host sizes every allotment so that neither bound is ever met: W <= blocks, a slice fits the LDS)
            if (!small_fits(g, (int)E.blocks)) return false;
            if (bx == 0 && threadIdx.x == 0) shape[eidx] = (uint32_t)g.W | ((uint32_t)g.c << 8);
            return true;
        } SMALL_STAMP_PASS(nullptr));
    if (!win.sums) return;
    // the window's sums, as they are, into the entry's window sums (HBM)
    const uint32_t tid = threadIdx.x, c = (uint32_t)win.g.c;
    if (tid < c * 8) {
        const uint32_t kk = tid >> 3, q = tid & 7;
        reinterpret_cast<uint4*>(fin + (size_t)E.base * SMALL_MAX_C + win.w * c + kk)[q] = reinterpret_cast<const uint4*>(&win.sums[kk])[q];
    }
}

// ---------------------------------------------------------------- the window fold of the bucket entries: one quad per entry
// fold[i] = entry; its W x c window sums at fin[base * SMALL_MAX_C ..] (memory form), the sum goes to sums[entry] (2^256 form).
// The Horner fold of host_fold64.hpp:h_fold_tree64, in the same order.
template <class C>
__global__ void __launch_bounds__(4 * BATCH_QUADS)
k_batch_fold(const BatchEntry* __restrict__ ents, const uint32_t* __restrict__ fold, uint32_t nf, const XYZZ<typename C::Fp>* __restrict__ fin,
             const uint32_t* __restrict__ shape, XYZZ<typename C::Fp>* __restrict__ sums) {
    using M = typename C::Fp;
    __shared__ XYZZ<M> sa[BATCH_QUADS], sb[BATCH_QUADS];
    const uint32_t tid = threadIdx.x, q = tid >> 2, r = tid & 3u, lane = tid & 63u;
    const uint32_t i = blockIdx.x * BATCH_QUADS + q;
    if (i >= nf) return;                                     // whole quads leave together
    const uint32_t e = fold[i];
    const uint32_t sh = shape[e];
    int W = (int)(sh & 0xffu);
    const int c = (int)((sh >> 8) & 0xffu);
    const BatchEntry E = ents[e];
    if (c < 1 || c > SMALL_MAX_C || W > (int)E.blocks) W = 0;          // (never: the bucket kernel writes a shape inside its allotment)
    const XYZZ<M>* f0 = fin + (size_t)E.base * SMALL_MAX_C;
    F30<M> acc;
    bool inf = true;
#pragma unroll 1
    for (int w = W - 1; w >= 0; w--) {
        const XYZZ<M>* f = f0 + (size_t)w * c;
        if (!inf) xyzz30_dbl_quadreg<M>(acc, r);             // bit c-1 of the bucket index does not exist
#pragma unroll 1
        for (int k = c - 2; k >= 0; k--) {
            if (!inf) xyzz30_dbl_quadreg<M>(acc, r);
            batch_add_maybe_inf<M>(acc, inf, f + 1 + k, &sa[q], &sb[q], r, lane);
        }
        batch_add_maybe_inf<M>(acc, inf, f, &sa[q], &sb[q], r, lane);
    }
    batch_store_point<M>(sums + e, acc, inf, r, true);
}

}  // namespace porla
