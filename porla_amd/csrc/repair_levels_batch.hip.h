// Kernels of the lower-level repair (repair_levels_batch.hip: porla_{kzg,ipa}_repair_levels_batch_device): the damaged rows of a lower
// level's Y half are written back in place from the level's X half.  Row by row the two halves have nothing in common -- every block
// of the level was scaled by its own wt -- but the whole Y half is a function of the whole X half:
//
//     Y half = Encode(HAdd_y(DecodeExact(X half)))
//
// DecodeExact is the ragged decode (icc_decode.hip), HAdd_y the per-block arithmetic of k_update_hadd with the write steps of
// k_ex_ysteps (y_p = chunk_p wt_p mod p_icc, c_p = (y_p - chunk_p wt_p) mod q), Encode the one-shot data network of the server rebuild
// (icc30_split.hip.h's tile, planes and rounds) over the rows y_p, which agrees symbol for symbol, below LCM, with the chain of mixes
// Server::HRebuild ran.  Row j of the Y alignment store is the point network over Commit(c_p); a point butterfly multiplies by the
// integer v^i mod p_icc and so does the data network's q plane, so by linearity the row is Commit(N_j mod q), N the data network over
// the rows c_p: one more run of the network on the q plane and one commitment per row, no group-element network.
//
// Two layouts, per file, t = write_step % n_total, m = levels & t (the named resident levels):
//   the t layout   level i at row t & (2^i - 1): the statuses, the actions, the PRF values (the extraction's layout, extract_batch.hip.h)
//   the m layout   level i at row m & (2^i - 1): d_work's regions, the rows of alignment scalars, the candidate alignment rows
// d_work of a file, B = n_cols * 32: [0, m B) the decoded chunks, overwritten in place by the rows y_p; [m B, 2 m B) the rows c_p;
// [2 m B, 4 m B) the candidate data rows, 64 bytes a symbol; [4 m B, 4 m B + 72 m n_cols) the residue planes of the levels of more than
// one pass (9 words per symbol and plane).
//
// The state word of a level (RlFile::state[i]): bit 0 a Y row failed, bit 1 an X row failed (k_rl_plan), bit 2 a witness row differs
// (k_rl_compare); state[16 + i] is the X decode's bad-symbol count.  A level is UNDER REPAIR iff (state & 3) == 1; the stages between
// the plan and the write read that and leave at once otherwise (rl_under_repair).  It is written iff (state & 7) == 1 and no symbol
// was bad (rl_repaired).
#pragma once
#include "retrieve_batch.hip.h"
#include "icc30_split.hip.h"
#include "../../include/porla_gpu.h"

namespace porla {

constexpr int RL_MAX_LEVELS = 16;
constexpr int RL_STATE_WORDS = 2 * RL_MAX_LEVELS;
constexpr uint32_t RL_ROW_DIFFERS = 0x100u;            // a row's word of RlFile::rowbits: the PORLA_REPAIR_* bits, and this one

// one file as the kernels see it
struct RlFile {
    uint8_t* data_y[RL_MAX_LEVELS];     // the named levels' Y data stores (nullptr: not named)
    uint8_t* align_y[RL_MAX_LEVELS];    // ... and Y alignment stores
    const uint8_t* level0_x;            // level 0's X row when the level is named
    uint8_t* status_x;                  // d_status_x, d_status_y, d_action_y: t bytes each
    uint8_t* status_y;
    uint8_t* action_y;
    uint8_t* verdict;                   // d_level: 16 bytes
    uint32_t* counts;                   // d_counts or nullptr
    uint8_t* work;                      // d_work
    uint32_t* state;                    // RL_STATE_WORDS words of the call's workspace
    uint32_t* rowbits;                  // t words of it: what the write kernel did to the row; RL_ROW_DIFFERS
    uint8_t* permit;                    // t bytes of it: PORLA_RETRIEVE_ROW_OK = the write pass may write the row's MAC
    unsigned long long epoch;           // write_step - t
    uint32_t t, m;
    uint32_t row0;                      // the file's first row among the call's rows of alignment scalars (m layout, files end to end)
    uint32_t pad;
};
static_assert(sizeof(RlFile) == 360, "RlFile: 42 pointers, the epoch, four words");

// one named level of 2 rows and more as the data passes see it
struct RlItem {
    const uint8_t* y;                   // the rows y_p (32-byte chunks)
    const uint8_t* c;                   // the rows c_p
    uint8_t* cand;                      // the candidate data rows
    uint8_t* scalars;                   // the level's rows of alignment scalars, 32 bytes big-endian
    uint32_t* planes;                   // two residue planes (more than one pass)
    const uint32_t* state;              // the level's state word
};
static_assert(sizeof(RlItem) == 48, "RlItem: six pointers");

// the level of entry r of a file's ascending layout over the level mask `mask` (t or m), and the entry's place in the level; the epoch
// write step of entry p of level i (extract_batch.hip.h: ex_level_of_entry, ex_step_of -- that header's kernels belong to its one file)
__device__ __forceinline__ uint32_t rl_level_of_entry(uint32_t mask, uint32_t r, uint32_t& p) {
    uint32_t rest = mask, off = 0;
    for (;;) {
        const uint32_t i = (uint32_t)__ffs((int)rest) - 1u;
        if (r < off + (1u << i) || (rest & (rest - 1u)) == 0u) { p = r - off; return i; }
        off += 1u << i;
        rest &= rest - 1u;
    }
}
__device__ __forceinline__ uint32_t rl_step_of(uint32_t t, uint32_t i, uint32_t p) { return (t & ~((2u << i) - 1u)) + 1u + p; }

__device__ __forceinline__ bool rl_under_repair(uint32_t state) { return (state & 3u) == 1u; }
__device__ __forceinline__ bool rl_repaired(const RlFile& F, uint32_t i) { return (F.state[i] & 7u) == 1u && F.state[RL_MAX_LEVELS + i] == 0u; }

// the actions, verdicts, counters, states, row words and permits: zero; the statuses of the rows of unnamed levels
__global__ void __launch_bounds__(256)
k_rl_clear(const RlFile* __restrict__ files) {
    const RlFile& F = files[blockIdx.y];
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < (uint32_t)RL_MAX_LEVELS) F.verdict[r] = 0;
    if (r < (uint32_t)RL_STATE_WORDS) F.state[r] = 0;
    if (r < 8u && F.counts) F.counts[r] = 0;
    if (r >= F.t) return;
    F.action_y[r] = 0;
    F.rowbits[r] = 0;
    F.permit[r] = 0;
    uint32_t p;
    if (!(F.m >> rl_level_of_entry(F.t, r, p) & 1u)) {
        F.status_x[r] = PORLA_EXTRACT_ROW_NOT_TRIED;
        F.status_y[r] = PORLA_EXTRACT_ROW_NOT_TRIED;
    }
}

// the plan: a lane per row of the t layout; a failed row marks its level's state word
__global__ void __launch_bounds__(256)
k_rl_plan(const RlFile* __restrict__ files) {
    const RlFile& F = files[blockIdx.y];
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= F.t) return;
    uint32_t p;
    const uint32_t i = rl_level_of_entry(F.t, r, p);
    if (!(F.m >> i & 1u)) return;
    if (F.status_x[r] == 0) atomicOr(F.state + i, 2u);
    if (F.status_y[r] == 0) atomicOr(F.state + i, 1u);
}

// ---- HAdd over the decoded levels: a lane per (block, column) of the m layout of file blockIdx.y.  The chunk (level 0: the low half
// of the X row's symbol as it lies, a nonzero upper half counted as a bad symbol) times the block's own wt = w^e, e = reverse_bits(step
// % n_total), on both planes -- entry e of the encode's plane tables, as the top-level repair scales a row -- gives y_p, canonical,
// over the chunk, and c_p = (y_p - chunk wt) mod q, little-endian, as the 32-byte chunk the q plane's network reads.  scale (the IPA
// build): c_p is multiplied by alpha^-1 mod q first, because the rows are committed against the ALPHA generators; the network is linear,
// so the commitment is the one against the generators.  Level 0 is its own network: its candidate row is y_p zero-extended and its row
// of scalars c_p big-endian.
struct RlScale { uint32_t inv[8]; uint32_t on; };       // alpha^-1 mod q in the Montgomery form
template <class Q>
__global__ void __launch_bounds__(256)
k_rl_hadd(const RlFile* __restrict__ files, const uint32_t* __restrict__ twp, const uint32_t* __restrict__ twq, uint32_t n_total, int logn,
          uint32_t ncols, uint8_t* __restrict__ scalars, RlScale scale) {
    const RlFile& F = files[blockIdx.y];
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= (size_t)F.m * ncols) return;
    const uint32_t r = (uint32_t)(tid / ncols), c = (uint32_t)(tid - (size_t)r * ncols);
    uint32_t p;
    const uint32_t i = rl_level_of_entry(F.m, r, p);
    if (!rl_under_repair(F.state[i])) return;
    const size_t B = (size_t)ncols * 32;
    uint8_t* const y_at = F.work + 32 * tid;
    uint8_t* const c_rows = F.work + (size_t)F.m * B;
    Fe<IccFp> x;
    if (i == 0u) {
        const uint4* s = reinterpret_cast<const uint4*>(F.level0_x + 64 * (size_t)c);
        const uint4 a = s[0], b = s[1], u = s[2], v = s[3];
        x.v[0] = a.x; x.v[1] = a.y; x.v[2] = a.z; x.v[3] = a.w; x.v[4] = b.x; x.v[5] = b.y; x.v[6] = b.z; x.v[7] = b.w;
        if ((u.x | u.y | u.z | u.w | v.x | v.y | v.z | v.w) != 0u) atomicAdd(F.state + RL_MAX_LEVELS, 1u);
    } else {
        x = ld_fe<IccFp>(reinterpret_cast<const uint32_t*>(y_at));
    }
    const uint32_t step = (uint32_t)((F.epoch + rl_step_of(F.t, i, p)) & (n_total - 1u));
    const uint32_t e = __brev(step) >> (32 - logn);
    const Fe<IccFp> Y = icc30_finish_p(icc30_mul<IccFp>(icc30_ld_pslot<IccFp>(twp + (size_t)e * ICC30_PSLOT_WORDS), f30_unpack<IccFp>(x.v)));
    const F30<Q> xq = icc30_mul<Q>(icc30_ld_pslot<Q>(twq + (size_t)e * ICC30_PSLOT_WORDS), f30_unpack<Q>(x.v));
    st_fe<IccFp>(reinterpret_cast<uint32_t*>(y_at), Y);
    IccOut o;
    o.x = nullptr; o.al = nullptr; o.sc = c_rows; o.qres = nullptr; o.scalar_le = 1;
    icc30_finish_q<Q>(Y, xq, tid, o);
    if (scale.on) {
        const F30<Q> K = icc30_mul<Q>(f30_unpack<Q>(scale.inv), f30_const<Q>(Icc30Const<Q>::C284));
        const Fe<Q> cp = ld_fe<Q>(reinterpret_cast<const uint32_t*>(c_rows + 32 * tid));
        st_fe<Q>(reinterpret_cast<uint32_t*>(c_rows + 32 * tid), icc30_canonical<Q>(icc30_reduce_top<Q>(icc30_mul<Q>(K, f30_unpack<Q>(cp.v)))));
    }
    if (i != 0u) return;
    uint4* cand = reinterpret_cast<uint4*>(F.work + 2 * (size_t)F.m * B + 64 * tid);
    const uint4 zero = make_uint4(0, 0, 0, 0);
    cand[0] = make_uint4(Y.v[0], Y.v[1], Y.v[2], Y.v[3]);
    cand[1] = make_uint4(Y.v[4], Y.v[5], Y.v[6], Y.v[7]);
    cand[2] = zero;
    cand[3] = zero;
    const Fe<Q> cp = ld_fe<Q>(reinterpret_cast<const uint32_t*>(c_rows + 32 * tid));
    uint4* sc = reinterpret_cast<uint4*>(scalars + 32 * (((size_t)F.row0 + r) * ncols + c));
    sc[0] = make_uint4(__builtin_bswap32(cp.v[7]), __builtin_bswap32(cp.v[6]), __builtin_bswap32(cp.v[5]), __builtin_bswap32(cp.v[4]));
    sc[1] = make_uint4(__builtin_bswap32(cp.v[3]), __builtin_bswap32(cp.v[2]), __builtin_bswap32(cp.v[1]), __builtin_bswap32(cp.v[0]));
}

// ---- one pass of the forward data network over the named level blockIdx.y of a launch (all of one size): k_sr_data's tiles, planes
// and rounds on 32-byte chunk rows, with two finishes.  DATA: both planes over the rows y_p; the last pass joins them below LCM into
// the candidate data rows as k_sr_data's cached finish joins the X part (the p_icc plane parks its canonical residue in the symbol's own
// slot, the q plane -- the same lane -- reads it back).  !DATA: the q plane alone over the rows c_p; the last pass writes the canonical
// residue mod q, 32 bytes big-endian, into the level's rows of alignment scalars.  The twiddle tables are those of n_total and the tile
// is told so (icc30_block_tile's n only strides the tables): a level of 2^i rows runs the stages 1 .. i of that network, as the mixes
// that built it did.  A level that is not under repair leaves at once: the whole block, before any barrier.
template <class Q, bool FIRST, bool LAST, bool DATA>
__global__ void __launch_bounds__(ICC30_SPLIT_THREADS) __attribute__((amdgpu_waves_per_eu(LAST && DATA ? 3 : 4, 4)))
k_rl_data(const RlItem* __restrict__ items, size_t plane_words, const uint32_t* __restrict__ twp, const uint32_t* __restrict__ twq,
          uint32_t tw_n, uint32_t ncols, int s0, int ns, int cc_log) {
    __shared__ uint2 lds2[ICC_TILE_ELEMS * ICC30_PSLOT_WORDS / 2];
    uint32_t* lds = reinterpret_cast<uint32_t*>(lds2);
    const RlItem& I = items[blockIdx.y];
    if (!rl_under_repair(*I.state)) return;
    const uint8_t* raw = DATA ? I.y : I.c;
    uint32_t* work_p = I.planes;
    uint32_t* work_q = work_p + plane_words;
    const IccTile T = icc30_block_tile(tw_n, ncols, s0, ns, cc_log, FIRST);
    uint32_t slot[4];
    if (DATA) {
        F30<IccFp> rp[4];
        icc30_plane<IccFp, FIRST>(lds, T, raw, F30<IccFp>{}, work_p, twp, rp, slot);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (slot[i] != 0xffffffffu) {
                const size_t gi = icc30_symbol_index(T, slot[i]);
                if (LAST) st_fe<IccFp>(reinterpret_cast<uint32_t*>(I.cand + 64 * gi), icc30_finish_p(rp[i]));
                else icc30_st_work<IccFp>(work_p + gi * ICC30_PLANE_WORDS, rp[i]);
            }
        }
        __syncthreads();                                 // every lane has read its last round's symbols: the region is free
    }
    {
        F30<Q> rq[4];
        icc30_plane<Q, FIRST>(lds, T, raw, F30<Q>{}, work_q, twq, rq, slot);
        const IccOut o{DATA ? I.cand : nullptr, nullptr, nullptr, DATA ? nullptr : I.scalars, 0};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (slot[i] != 0xffffffffu) {
                const size_t gi = icc30_symbol_index(T, slot[i]);
                if (LAST) {
                    Fe<IccFp> P = fe_zero<IccFp>();
                    if (DATA) P = ld_fe<IccFp>(reinterpret_cast<const uint32_t*>(I.cand + 64 * gi));      // what this lane stored above
                    icc30_finish_q<Q>(P, rq[i], gi, o);
                } else {
                    icc30_st_work<Q>(work_q + gi * ICC30_PLANE_WORDS, rq[i]);
                }
            }
        }
    }
}

// ---- the candidate alignment rows: a lane per row of the commitment pass (sums, projective, row g at sums[g S]) to canonical affine
// bytes; an infinite sum -- a row of zero scalars -- gives 64 zero bytes
template <class C>
__global__ void __launch_bounds__(256)
k_rl_align(const XYZZ<typename C::Fp>* __restrict__ sums, uint32_t S, uint32_t rows, uint8_t* __restrict__ out) {
    using M = typename C::Fp;
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= rows) return;
    store_affine_be<M>(out + 64 * (size_t)g, load_xyzz<M>(sums + (size_t)g * S));
}

// the 64 bytes at a against those at b
__device__ __forceinline__ bool rl_differ64(const uint8_t* a, const uint8_t* b, uint4 (&av)[4]) {
    const uint4* a4 = reinterpret_cast<const uint4*>(a);
    const uint4* b4 = reinterpret_cast<const uint4*>(b);
    uint32_t diff = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        av[w] = a4[w];
        const uint4 y = b4[w];
        diff |= (av[w].x ^ y.x) | (av[w].y ^ y.y) | (av[w].z ^ y.z) | (av[w].w ^ y.w);
    }
    return diff != 0u;
}

// a lane per symbol of the m layout of file blockIdx.y: its level, its row there and in the t layout, the stored symbol and the
// candidate; false: nothing to do for this lane.  The lane of a row's column 0 also owns the row's alignment bytes.
struct RlLane {
    uint32_t i, rt, c;
    uint8_t* stored;
    const uint8_t* cand;
    uint8_t* align;
    const uint8_t* cand_align;
};
__device__ __forceinline__ bool rl_lane(const RlFile& F, uint32_t ncols, const uint8_t* __restrict__ cand_align, RlLane& L) {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= (size_t)F.m * ncols) return false;
    const uint32_t r = (uint32_t)(tid / ncols);
    L.c = (uint32_t)(tid - (size_t)r * ncols);
    uint32_t p;
    L.i = rl_level_of_entry(F.m, r, p);
    L.rt = (F.t & ((1u << L.i) - 1u)) + p;
    L.stored = F.data_y[L.i] + 64 * ((size_t)p * ncols + L.c);
    L.cand = F.work + 2 * (size_t)F.m * ncols * 32 + 64 * tid;
    L.align = F.align_y[L.i] + 64 * (size_t)p;
    L.cand_align = cand_align + 64 * ((size_t)F.row0 + r);
    return true;
}

// ---- the witnesses: a Y row that checked OK in a level under repair must hold its candidate, data and alignment, byte for byte.  A
// row that does not marks its level and is counted once.
__global__ void __launch_bounds__(256)
k_rl_compare(const RlFile* __restrict__ files, uint32_t ncols, const uint8_t* __restrict__ cand_align) {
    const RlFile& F = files[blockIdx.y];
    RlLane L;
    if (!rl_lane(F, ncols, cand_align, L)) return;
    if (!rl_under_repair(F.state[L.i]) || F.status_y[L.rt] != PORLA_RETRIEVE_ROW_OK) return;
    uint4 v[4];
    bool differs = rl_differ64(L.cand, L.stored, v);
    if (L.c == 0u) differs = rl_differ64(L.cand_align, L.align, v) || differs;
    if (!differs) return;
    atomicOr(F.state + L.i, 4u);
    if (!(atomicOr(F.rowbits + L.rt, RL_ROW_DIFFERS) & RL_ROW_DIFFERS) && F.counts) atomicAdd(F.counts + 7, 1u);
}

// ---- the write: the failed Y rows of a repaired level.  The candidate goes over the stored symbol where it differs, the candidate
// alignment over the stored alignment row likewise; 16-byte accesses, plain vector stores.  The row's word collects the bits (the lanes
// of a row write different ones) and its permit lets the write pass rewrite the MAC.
__global__ void __launch_bounds__(256)
k_rl_write(const RlFile* __restrict__ files, uint32_t ncols, const uint8_t* __restrict__ cand_align) {
    const RlFile& F = files[blockIdx.y];
    RlLane L;
    if (!rl_lane(F, ncols, cand_align, L)) return;
    if (!rl_repaired(F, L.i) || F.status_y[L.rt] != 0) return;
    uint4 v[4];
    if (rl_differ64(L.cand, L.stored, v)) {
        uint4* d = reinterpret_cast<uint4*>(L.stored);
#pragma unroll
        for (int w = 0; w < 4; w++) d[w] = v[w];
        atomicOr(F.rowbits + L.rt, (uint32_t)PORLA_REPAIR_DATA);
    }
    if (L.c != 0u) return;
    F.permit[L.rt] = PORLA_RETRIEVE_ROW_OK;
    if (rl_differ64(L.cand_align, L.align, v)) {
        uint4* d = reinterpret_cast<uint4*>(L.align);
#pragma unroll
        for (int w = 0; w < 4; w++) d[w] = v[w];
        atomicOr(F.rowbits + L.rt, (uint32_t)PORLA_REPAIR_ALIGN);
    }
}

// ---- the tally, behind the write pass (which put the MAC bit into the action bytes): a lane per row of the t layout joins the row's
// bits into its action byte and counts them; the lane of a named level's first row writes the verdict
__global__ void __launch_bounds__(256)
k_rl_tally(const RlFile* __restrict__ files) {
    const RlFile& F = files[blockIdx.y];
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= F.t) return;
    uint32_t p;
    const uint32_t i = rl_level_of_entry(F.t, r, p);
    if (!(F.m >> i & 1u)) return;
    const uint32_t a = F.action_y[r] | (F.rowbits[r] & 0xffu);
    F.action_y[r] = (uint8_t)a;
    if (F.counts) {
        if (a & PORLA_REPAIR_DATA) atomicAdd(F.counts + 2, 1u);
        if (a & PORLA_REPAIR_ALIGN) atomicAdd(F.counts + 3, 1u);
        if (a & PORLA_REPAIR_MAC) atomicAdd(F.counts + 4, 1u);
    }
    if (p != 0u) return;
    const uint32_t st = F.state[i];
    uint8_t v;
    if ((st & 3u) == 0u) v = PORLA_REPAIR_LEVEL_CLEAN;
    else if (st & 2u) v = PORLA_REPAIR_LEVEL_X_DAMAGED;
    else if (!rl_repaired(F, i)) v = PORLA_REPAIR_LEVEL_INCONSISTENT;
    else v = PORLA_REPAIR_LEVEL_REPAIRED;
    F.verdict[i] = v;
    if (F.counts && v == PORLA_REPAIR_LEVEL_REPAIRED) atomicAdd(F.counts + 5, 1u);
    if (F.counts && (v == PORLA_REPAIR_LEVEL_X_DAMAGED || v == PORLA_REPAIR_LEVEL_INCONSISTENT)) atomicAdd(F.counts + 6, 1u);
}

}  // namespace porla
