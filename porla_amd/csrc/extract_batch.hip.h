// Kernels of the verified file extraction (extract_batch.hip: porla_{kzg,ipa}_extract_batch_device): every resident level of K files
// is checked row by row, its X half decoded, and the decoded blocks merged per slot by "newest authentic copy wins".
//
// The row check is the aligned retrieval's (retrieve_batch.hip.h) with another row -> request map: a request is ONE HALF (one level of
// one file), the halves differ in size, and RtMapStarts finds a row's half by a binary search in the halves' start rows.  The check's
// kernels are k_rt_eval_lazy, k_rt_eval_horner, k_rt_pack, k_rt_compare and k_rt_compare_aligned instantiated with that map
// (retrieve_batch.hip launches them), so a status byte is what the retrieval calls write for the same row.
//
// The layout the merge works in, per file, t = write_step % n_total: the resident lower levels are the set bits of t, in ascending
// order, level i at offset o_i = t & (2^i - 1) with 2^i entries -- the row statuses (then the top level's n_total rows at offset t), the
// PRF values, and the decoded blocks in d_work all lie that way.  Entry o_i + p of level i is the block of epoch write step
// (t with bits 0 .. i cleared) + 1 + p, and the level's highest step is hi_i = t with the bits below i cleared.  The other way round
// step s, 1 .. t, lies in level i = the highest bit in which s - 1 and t differ, at p = (s - 1) & (2^i - 1).
// Ranks travel as rank + 1 in d_steps (0 = no candidate; a clean top level's blocks are candidates of rank 0), so that one atomicMax per
// decoded block picks the winner; k_ex_gather writes the documented values at the end.
//
// The second source (porla_*_extract_xy_batch_device): the tried Y halves lie in d_row_status_y, d_prf_y and d_work_y at the same
// offsets o_i, decoded mod p_icc.  A level whose X half failed and whose tried Y half is clean is Y-sourced: its blocks bid with the
// same ranks when chunk 0 mod p_icc names ONE index, and are set aside with a doubt (step + 1, a per-slot maximum) on the slots they
// may name when it names two -- r0 < D = 2^256 - p_icc: the chunk may be r0 + p_icc, whose low 64 bits are one more.
//
// The top level's second source (porla_*_extract_xyt_batch_device) works ROW BY ROW, not level by level: the rebuild that wrote the top
// level scaled every chunk by ONE wt = w^e, e = reverse_bits(top_step % n_total), and the network is linear, so Y_j = wt X_j mod LCM
// (mod p_icc in the RESIDUE32 form).  k_ex_top_patch writes the half the top level's one decode reads: row j as its X row lies when
// that row checked OK, else wt^-1 Y_j when its Y row checked OK -- the p_icc plane by entry (N - e) mod N of the decode's tw30p, the q
// plane by entry e of its table of inverses -- else the X row again (the level is failed then: k_ex_verdict).
#pragma once
#include "retrieve_batch.hip.h"
#include "icc_decode.hip.h"
#include "../../include/porla_gpu.h"

namespace porla {

// ---- the merge.  One file as its kernels see it.  The Y members are those of porla_*_extract_xy_batch_device: y_tried == 0 (the call
// without Y halves, or none tried) leaves every kernel below on the X path alone.
struct ExFile {
    const uint8_t* level0;     // level 0's one row of 64-byte symbols, or nullptr: not resident
    const uint8_t* status;     // d_row_status
    uint8_t* work;             // d_work
    uint8_t* blocks;           // d_blocks: a clean top level has been decoded into it
    uint32_t* steps;           // d_steps
    uint8_t* flags;            // d_flags
    uint32_t* counts;          // d_counts or nullptr
    uint32_t* scratch;         // EX_SCRATCH_WORDS words of the call's workspace: [0] the failed-level mask of the X halves (bit i = level
                               // i, bit log2 n_total = the top level), [1 + s] the bad-symbol count of the decode of 2^s rows,
                               // [EX_SCRATCH_FAILED_Y] the failed-level mask of the tried Y halves
    uint8_t* status_y;         // d_row_status_y or nullptr
    const uint8_t* work_y;     // d_work_y: the decoded Y halves, chunks mod p_icc
    uint32_t* doubt;           // n_total words of the call's workspace, or nullptr (no Y half tried): per slot the highest step + 1 of
                               // a Y block set aside as ambiguous that may belong there
    unsigned long long* ysteps;// t words of the call's workspace: the write steps of the file's lower-level entries (the Y unscale)
    unsigned long long epoch;  // write_step - t
    uint32_t t;                // write_step % n_total
    uint32_t has_top;
    uint32_t y_tried;          // y_levels & t
    uint32_t n_counts;         // 4, 6 in the call with Y halves, or 8 in the call with the top level's Y half
    // the top level's Y half (porla_*_extract_xyt_batch_device); top_y == 0 leaves every kernel on the paths above
    uint8_t* status_top_y;     // d_row_status_top_y or nullptr
    const uint8_t* top_x;      // d_top_rows
    const uint8_t* top_rows_y; // d_top_rows_y
    uint8_t* top_patch;        // d_top_patch: the half the top level's decode reads
    uint32_t top_y;            // 1: the top level's Y half is tried (top_y == 1 and a top level present)
    uint32_t top_e;            // reverse_bits(top_step % n_total, log2 n_total): wt = w^top_e
};
constexpr int EX_SCRATCH_WORDS = 20;
constexpr int EX_SCRATCH_FAILED_Y = 18;
constexpr int EX_SCRATCH_TOP_FROM_Y = 19;                                 // the top-level rows taken from the Y half
static_assert(sizeof(ExFile) == 160, "ExFile: sixteen pointers, the epoch and six words");

// the level of entry r < t of a file's ascending layout, and the entry's place in the level
__device__ __forceinline__ uint32_t ex_level_of_entry(uint32_t t, uint32_t r, uint32_t& p) {
    uint32_t rest = t, off = 0;
    for (;;) {
        const uint32_t i = (uint32_t)__ffs((int)rest) - 1u;
        if (r < off + (1u << i) || (rest & (rest - 1u)) == 0u) { p = r - off; return i; }
        off += 1u << i;
        rest &= rest - 1u;
    }
}
// the epoch write step of entry p of level i
__device__ __forceinline__ uint32_t ex_step_of(uint32_t t, uint32_t i, uint32_t p) { return (t & ~((2u << i) - 1u)) + 1u + p; }
// the source of top-level row j: 0 the X row, 1 the Y row, 2 none
__device__ __forceinline__ uint32_t ex_top_source(const ExFile& F, uint32_t j) {
    if (F.status[F.t + j] != 0) return 0u;
    return F.top_y && F.status_top_y[j] == PORLA_RETRIEVE_ROW_OK ? 1u : 2u;
}
// the levels whose source is the Y half: X failed, Y tried and clean
__device__ __forceinline__ uint32_t ex_y_sourced(const ExFile& F) { return F.scratch[0] & F.y_tried & ~F.scratch[EX_SCRATCH_FAILED_Y]; }

// counters, failed-level masks, decode counters, the ranks and doubts of every slot: zero; the Y statuses of untried levels and of
// an untried top level
__global__ void __launch_bounds__(256)
k_ex_clear(const ExFile* __restrict__ files, uint32_t n_total) {
    const ExFile& F = files[blockIdx.y];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_total) F.steps[i] = 0;
    if (i < n_total && F.doubt) F.doubt[i] = 0;
    if (i < (uint32_t)EX_SCRATCH_WORDS) F.scratch[i] = 0;
    if (i < F.n_counts && F.counts) F.counts[i] = 0;
    if (i < F.t && F.status_y) {
        uint32_t p;
        if (!(F.y_tried >> ex_level_of_entry(F.t, i, p) & 1u)) F.status_y[i] = PORLA_EXTRACT_ROW_NOT_TRIED;
    }
    if (i < n_total && F.status_top_y && !F.top_y) F.status_top_y[i] = PORLA_EXTRACT_ROW_NOT_TRIED;
}

// ---- the patched top half: a lane per symbol of file blockIdx.y.  FORM: PORLA_ICC_DECODE_EXACT (64-byte symbols, both planes, joined
// below LCM as the encode's finish joins them) or PORLA_ICC_DECODE_RESIDUE32 (32-byte symbols, the p_icc plane alone; Q is unused).
// A row from the X half, a row without a source and -- with wt = 1 -- a row from the Y half are copied as they lie.  Any 64 (32) input
// bytes are defined: the symbol enters below 2 p by the decode's load step (icd_load64; a 256-bit value is below 2 p_icc as it is), the
// product with the table entry is below p + 2^250, the finish makes it canonical.  16-byte accesses, plain vector stores.
template <int FORM, class Q>
__global__ void __launch_bounds__(256)
k_ex_top_patch(const ExFile* __restrict__ files, const uint32_t* __restrict__ twp, const uint32_t* __restrict__ twqi, uint32_t n_total,
               uint32_t ncols) {
    constexpr uint32_t SYMB = FORM == PORLA_ICC_DECODE_EXACT ? 64u : 32u;
    const ExFile& F = files[blockIdx.y];
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (!F.top_y || i >= (size_t)n_total * ncols) return;
    const uint32_t j = (uint32_t)(i / ncols);
    const bool from_y = ex_top_source(F, j) == 1u;
    const uint8_t* src = (from_y ? F.top_rows_y : F.top_x) + SYMB * i;
    uint8_t* dst = F.top_patch + SYMB * i;
    if (!from_y || F.top_e == 0u) {
        const uint4* s = reinterpret_cast<const uint4*>(src);
        uint4* d = reinterpret_cast<uint4*>(dst);
#pragma unroll
        for (uint32_t w = 0; w < SYMB / 16u; w++) d[w] = s[w];
        return;
    }
    if (FORM == PORLA_ICC_DECODE_EXACT) {
        const F30<IccFp> rp = icc30_mul<IccFp>(icd_tw<IccFp>(twp, n_total, F.top_e), icd_load64<IccFp>(src));
        const F30<Q> rq = icc30_mul<Q>(icd_tw<Q>(twqi, n_total, F.top_e), icd_load64<Q>(src));
        IccOut o;
        o.x = F.top_patch; o.al = nullptr; o.sc = nullptr; o.qres = nullptr; o.scalar_le = 0;
        icc30_finish_q<Q>(icc30_finish_p(rp), rq, i, o);
    } else {
        const F30<IccFp> y = f30_unpack<IccFp>(ld_fe<IccFp>(reinterpret_cast<const uint32_t*>(src)).v);
        st_fe<IccFp>(reinterpret_cast<uint32_t*>(dst), icc30_finish_p(icc30_mul<IccFp>(icd_tw<IccFp>(twp, n_total, F.top_e), y)));
    }
}

// the write steps of a file's lower-level entries, for the unscale of the Y decodes: a lane per entry
__global__ void __launch_bounds__(256)
k_ex_ysteps(const ExFile* __restrict__ files) {
    const ExFile& F = files[blockIdx.y];
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= F.t || !F.y_tried) return;
    uint32_t p;
    const uint32_t i = ex_level_of_entry(F.t, r, p);
    F.ysteps[r] = F.epoch + ex_step_of(F.t, i, p);
}

// level 0: one row, the decode is the identity on the low 32 bytes of each symbol; a nonzero upper half is a bad symbol
__global__ void __launch_bounds__(256)
k_ex_level0(const ExFile* __restrict__ files, uint32_t ncols) {
    const ExFile& F = files[blockIdx.y];
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (!F.level0 || c >= ncols) return;
    const uint4* s = reinterpret_cast<const uint4*>(F.level0 + 64 * (size_t)c);
    uint4* d = reinterpret_cast<uint4*>(F.work + 32 * (size_t)c);
    const uint4 a = s[0], b = s[1], x = s[2], y = s[3];
    d[0] = a;
    d[1] = b;
    if ((x.x | x.y | x.z | x.w | y.x | y.y | y.z | y.w) != 0u) atomicAdd(F.scratch + 1, 1u);
}

// the verdict: a lane per resident row; a row with status 0 fails its level -- an X row in word 0, a tried Y row in the Y word -- and a
// top-level row fails the top level when it has no source; the top-level rows taken from the Y half are counted
__global__ void __launch_bounds__(256)
k_ex_verdict(const ExFile* __restrict__ files, uint32_t n_total, uint32_t top_bit) {
    const ExFile& F = files[blockIdx.y];
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t rows = F.t + (F.has_top ? n_total : 0u);
    if (r == 0u && F.counts) {                                            // the decodes' bad symbols, summed
        uint32_t bad = 0;
        for (int s = 1; s < EX_SCRATCH_FAILED_Y; s++) bad += F.scratch[s];
        F.counts[1] = bad;
    }
    if (r >= rows) return;
    uint32_t p;
    if (r >= F.t) {
        const uint32_t source = ex_top_source(F, r - F.t);
        if (source == 2u) atomicOr(F.scratch, 1u << top_bit);
        if (source == 1u) {
            atomicAdd(F.scratch + EX_SCRATCH_TOP_FROM_Y, 1u);
            if (F.counts) atomicAdd(F.counts + 7, 1u);
        }
        return;
    }
    if (F.status[r] == 0) atomicOr(F.scratch, 1u << ex_level_of_entry(F.t, r, p));
    if (F.y_tried && F.status_y[r] == 0) atomicOr(F.scratch + EX_SCRATCH_FAILED_Y, 1u << ex_level_of_entry(F.t, r, p));
}

// r0 < D = 2^256 - p_icc = 49 * 2^248 - 1, r0 as eight little-endian words: then r0 + p_icc is a 256-bit chunk too
__device__ __forceinline__ bool ex_below_d(const uint4& lo, const uint4& hi) {
    if (hi.w != 0x30ffffffu) return hi.w < 0x30ffffffu;
    return (lo.x & lo.y & lo.z & lo.w & hi.x & hi.y & hi.z) != 0xffffffffu;                   // (all ones: r0 = D)
}

// rank: a lane per decoded block of a lower level; a clean level's block bids for the slot its first eight bytes name.  A block of a
// Y-sourced level is known mod p_icc: it bids when its index is certain, and is set aside with a doubt on the slots it may name when not
__global__ void __launch_bounds__(256)
k_ex_rank(const ExFile* __restrict__ files, uint32_t n_total, uint32_t ncols) {
    const ExFile& F = files[blockIdx.y];
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= F.t) return;
    uint32_t p;
    const uint32_t i = ex_level_of_entry(F.t, r, p);
    const uint32_t step = ex_step_of(F.t, i, p);
    if (!(F.scratch[0] >> i & 1u)) {
        const uint2 id = *reinterpret_cast<const uint2*>(F.work + (size_t)r * ncols * 32);
        if (id.y != 0u || id.x == 0u || id.x > n_total) {
            if (F.counts) atomicAdd(F.counts + 2, 1u);
            return;
        }
        atomicMax(F.steps + (id.x - 1u), step + 1u);
        return;
    }
    if (!(ex_y_sourced(F) >> i & 1u)) return;
    const uint4* c0 = reinterpret_cast<const uint4*>(F.work_y + (size_t)r * ncols * 32);
    const uint4 lo = c0[0], hi = c0[1];
    const uint64_t a = (uint64_t)lo.y << 32 | lo.x, b = a + 1u;           // (b wraps to 0: out of range)
    const bool in_a = a >= 1u && a <= n_total, in_b = b >= 1u && b <= n_total;
    if (!ex_below_d(lo, hi)) {
        if (in_a) atomicMax(F.steps + ((uint32_t)a - 1u), step + 1u);
        else if (F.counts) atomicAdd(F.counts + 2, 1u);
    } else if (!in_a && !in_b) {
        if (F.counts) atomicAdd(F.counts + 2, 1u);
    } else {
        if (F.counts) atomicAdd(F.counts + 5, 1u);
        if (in_a) atomicMax(F.doubt + ((uint32_t)a - 1u), step + 1u);
        if (in_b) atomicMax(F.doubt + ((uint32_t)b - 1u), step + 1u);
    }
}

// gather: a block per slot.  The winner's bytes (a top-level winner lies in d_blocks already), or zeros; step, flags, counts[3].  A
// top-level winner carries FROM_Y when any row of the patched half came from the Y half: every decoded block depends on every row
__global__ void __launch_bounds__(64)
k_ex_gather(const ExFile* __restrict__ files, uint32_t ncols, uint32_t top_bit, uint32_t residue) {
    const ExFile& F = files[blockIdx.y];
    const uint32_t slot = blockIdx.x, t = F.t;
    const uint32_t from_y = ex_y_sourced(F), failed = F.scratch[0] & ~from_y;
    uint32_t enc = F.steps[slot];
    __syncthreads();                                                      // (lane 0 rewrites the word below)
    if (enc == 0u && F.has_top && !(failed >> top_bit & 1u)) enc = 1u;
    bool unsure = enc == 0u && F.has_top && (failed >> top_bit & 1u);     // the top level's highest step is 0 > -1 only
    for (uint32_t rest = failed & t; rest; rest &= rest - 1u) {
        const uint32_t i = (uint32_t)__ffs((int)rest) - 1u;
        unsure = unsure || (uint64_t)(t & ~((1u << i) - 1u)) + 1u > enc;  // hi_i > rank
    }
    if (F.doubt) unsure = unsure || F.doubt[slot] > enc;                  // an ambiguous block's step > rank
    const size_t u4 = (size_t)ncols * 2;                                  // 16-byte words of a block
    uint4* dst = reinterpret_cast<uint4*>(F.blocks) + (size_t)slot * u4;
    bool y = false;
    if (enc > 1u) {
        const uint32_t s1 = enc - 2u;                                     // step - 1
        const uint32_t i = 31u - (uint32_t)__clz((int)(s1 ^ t));
        const size_t entry = (size_t)(t & ((1u << i) - 1u)) + (s1 & ((1u << i) - 1u));
        y = from_y >> i & 1u;
        const uint4* src = reinterpret_cast<const uint4*>(y ? F.work_y : F.work) + entry * u4;
        for (size_t w = threadIdx.x; w < u4; w += blockDim.x) dst[w] = src[w];
    } else if (enc == 0u) {
        for (size_t w = threadIdx.x; w < u4; w += blockDim.x) dst[w] = make_uint4(0, 0, 0, 0);
    }
    if (threadIdx.x == 0u) {
        F.steps[slot] = enc ? enc - 1u : 0xffffffffu;
        F.flags[slot] = (uint8_t)((enc ? PORLA_EXTRACT_FOUND : 0) | (unsure ? PORLA_EXTRACT_UNSURE : 0) |
                                  (enc == 1u && residue ? PORLA_EXTRACT_RESIDUE : 0) | (y ? PORLA_EXTRACT_RESIDUE | PORLA_EXTRACT_FROM_Y : 0) |
                                  (enc == 1u && F.scratch[EX_SCRATCH_TOP_FROM_Y] ? PORLA_EXTRACT_FROM_Y : 0));
        if ((enc == 0u || unsure) && F.counts) atomicAdd(F.counts + 3, 1u);
    }
}

}  // namespace porla
