// Kernels of the batched verified retrieval (retrieve_batch.hip: porla_{kzg,ipa}_retrieve_batch_device and
// porla_{kzg,ipa}_retrieve_aligned_batch_device): every coded row of a half is checked against its stored MAC row in the CODED domain.  The data network works mod LCM =
// p_icc q with integer multipliers vi < p_icc and the MAC network multiplies by the same vi reduced mod q, so coded row j reduced mod q
// is the Z_q network of the chunks and the half's MAC row j is
//
//     alpha * Commit(row_j mod q) + s_j * h,        s_j = the PRF value of the complement the client holds for that row
//
// -- no group-element network runs.  KZG: the client knows tau, so Commit is one polynomial evaluation per row (k_rt_eval_lazy, or
// k_rt_eval_horner for a long SRS) and the expected MAC a two-coefficient commitment against (G1[0], h_MAC).  IPA: the row's 128
// symbols reduced mod n are one commitment row against the alpha generators (k_rt_pack), the PRF value one row of the hiding base.
// k_rt_compare sets the status bytes from the expected MACs' canonical affine bytes.  The rows of all K requests are numbered through,
// g = request * n_rows + row, and a kernel finds its request by a shift (RtMapShift below; the file extraction's instances of the same
// kernels, whose requests differ in size, search for it: RtMapStarts).
//
// The aligned call: a half that holds residues mod p_icc only (the Y rows of HAdd / HRebuildY, the 32-byte aligned top level) keeps
// MAC[j] + alpha * align[j] == alpha * Commit(row_j mod q), with row_j the STORED symbol reduced mod q, so its MAC row j is
//
//     E_j - alpha * A_j,        E_j = the expected MAC above, A_j = row j of the half's alignment store
//
// and with every A_j at infinity this is the relation above.  k_rt_compare_aligned forms alpha * A_j with the four-lane uniform ladder
// of mac_fft.hip.h (alpha is one scalar for the whole launch) and skips it per block of rows that have no finite alignment.  SYMB: the
// symbol width of the rows the evaluation and pack kernels read, 64 bytes (below LCM) or 32 (below p_icc, the d_rows32 store).
#pragma once
#include "kzg_eval.hip.h"
#include "client_rebuild_batch.hip.h"

namespace porla {

// One request as the kernels see it: porla_retrieve_aligned_req field for field (a porla_retrieve_req is widened on the host: no
// alignment store, no write steps).
struct RtDesc {
    const uint8_t* rows;
    const uint8_t* macs;
    const uint8_t* prf;
    const uint8_t* align;
    const unsigned long long* steps;
    uint8_t* out;
    uint8_t* status;
    uint32_t* counts;
};
static_assert(sizeof(RtDesc) == 64, "RtDesc: eight pointers");

// the call zeroes both counters of every request that has them (static: the header is read by more than one file)
static __global__ void __launch_bounds__(256)
k_rt_clear(const RtDesc* __restrict__ desc, uint32_t k) {
    const uint32_t a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a < k && desc[a].counts) { desc[a].counts[0] = 0; desc[a].counts[1] = 0; }
}

// The row -> request map of a launch, a template parameter of the kernels below.  The rows of a call are numbered through; find(g, jr)
// gives the request of row g and sets jr to its row there.  RtMapShift (the default): every request has 2^n_rows_log rows -- the
// retrieval calls, whose kernels these instances are.  RtMapStarts: request a starts at row starts[a] (ascending from 0, n of them) and
// the requests may differ in size -- a binary search; the instances of the extraction (extract_batch.hip).
struct RtMapShift {
    uint32_t n_rows_log;
    __device__ __forceinline__ uint32_t find(uint32_t g, uint32_t& jr) const {
        jr = g & ((1u << n_rows_log) - 1u);
        return g >> n_rows_log;
    }
};
struct RtMapStarts {
    const uint32_t* starts;
    uint32_t n;
    __device__ __forceinline__ uint32_t find(uint32_t g, uint32_t& jr) const {
        uint32_t lo = 0, hi = n;
        while (hi - lo > 1u) {
            const uint32_t mid = (lo + hi) >> 1;
            if (starts[mid] <= g) lo = mid; else hi = mid;
        }
        jr = g - starts[lo];
        return lo;
    }
};

// 64-byte little-endian symbol -> its residue mod q in the plain stream, unreduced: hi * (2^256 in the 2^270 form) -- below q + 2^242
// -- plus the raw lower half, below 2^258 (icc30_load_symbol's q part)
// SYMB == 32: the symbol is below p_icc < 2^256 and is its own lower half -- no product
template <class Q, int SYMB = 64>
__device__ __forceinline__ F30<Q> rt_symbol_mod_q(const uint8_t* __restrict__ src) {
    const Fe<Q> lo = ld_fe<Q>(reinterpret_cast<const uint32_t*>(src));
    if constexpr (SYMB == 32) return f30_unpack<Q>(lo.v);
    const Fe<Q> hi = ld_fe<Q>(reinterpret_cast<const uint32_t*>(src + 32));
    return icc30_add<Q>(icc30_mul<Q>(f30_unpack<Q>(hi.v), f30_const<Q>(Icc30Const<Q>::C526)), f30_unpack<Q>(lo.v));
}

// ---- KZG: alpha * f_g(tau) of row g as the dot product of kzg_eval.hip.h on 64-byte symbols.  A 512-bit symbol needs no reduction
// of its own: it is lo + hi 2^256 against TWO tables, tau^i and 2^256 tau^i mod r, i.e. two coefficient-times-power products into the
// same 64-bit columns.  The column bound, redone for this form: limbs below 2^29 make every partial product < 2^58 and a column takes
// at most nine of them per coefficient-times-power, so one symbol adds less than 2 * 9 * 2^58 to a column and THREE symbols
// accumulate between two ripples (3 * 2 * 9 * 2^58 + 2^29 = 54 * 2^58 + 2^29 < 2^64: the same 54 products the six 256-bit
// coefficients of KZG_LAZY_GROUP make).  The lane's sum is below steps * 2 * 2^256 * r < 128 * 2^511 = 2^518 for 1024 coefficients,
// inside the 2^544 kzg_columns_join takes and the 2^551 of the 19 columns.
// The symbol is read little-endian as it lies, 4 x uint4, the 8 lanes of a row reading 8 consecutive symbols (512 contiguous bytes):
// no byte swap, no copy of the rows.  Out: 64 bytes per row, the evaluation and beside it the PRF value left-padded (lane 1) -- the
// two big-endian coefficients of the commitment against (G1[0], h_MAC).
// LDS: [8 * steps][2][KZG_LAZY_ENTRY_WORDS] words, zero beyond n_coeffs: 96 bytes per power, 12 KiB at 128 coefficients, 96 KiB at 1024.
// SYMB == 32 (symbols below p_icc < 2^256, 32 bytes each): the symbol is ONE 256-bit coefficient against ONE table, tau^i -- the half
// of every entry of the same resident table that is staged, 48 bytes per power in LDS.  The column bound again: nine limbs below 2^29
// (the ninth below 2^24), so one symbol adds less than 9 * 2^58 to a column and SIX symbols accumulate between two ripples
// (6 * 9 * 2^58 + 2^29 = 54 * 2^58 + 2^29 < 2^64, the same 54 products).  The lane's sum is below steps * 2^256 * r < 128 * 2^510 =
// 2^517 for 1024 coefficients, inside the same 2^544.
template <int SYMB> constexpr int rt_lazy_group() { return SYMB == 64 ? 3 : 6; }      // symbols accumulated between two ripples of the columns
constexpr int RT_LAZY_ENTRY_U4 = 2 * KZG_LAZY_ENTRY_WORDS / 4;                          // an entry of the resident table: both powers
template <int SYMB> constexpr int rt_lazy_lds_u4() { return SYMB / 32 * KZG_LAZY_ENTRY_WORDS / 4; }   // ... and what of it is staged

template <int SYMB, class Map = RtMapShift>
__global__ void __launch_bounds__(256)
k_rt_eval_lazy(const RtDesc* __restrict__ desc, const Map map, uint32_t total_rows, uint32_t n_coeffs,
               const uint32_t* __restrict__ tau29w, KzgAlpha270 A, uint8_t* __restrict__ out) {
    using Q = IccBn254Fr;
    extern __shared__ uint4 rt_lds_tau[];
    const uint32_t steps = (n_coeffs + 7) / 8;
    constexpr uint32_t EU4 = rt_lazy_lds_u4<SYMB>();
    for (uint32_t i = threadIdx.x; i < steps * 8u * EU4; i += blockDim.x)
        rt_lds_tau[i] = reinterpret_cast<const uint4*>(tau29w)[SYMB == 64 ? i : i / EU4 * RT_LAZY_ENTRY_U4 + i % EU4];
    __syncthreads();
    const uint32_t j = threadIdx.x & 7u;
    const uint4 zero = make_uint4(0, 0, 0, 0);
    // a block takes 32 rows at a time, grid-strided: the table above is staged once per block, not once per 32 rows
    // (counted in 64 bits: the call may hold up to 2^32 - 1 rows)
    for (size_t r0 = (size_t)blockIdx.x * (blockDim.x >> 3); r0 < total_rows; r0 += (size_t)gridDim.x * (blockDim.x >> 3)) {
        const size_t rr = r0 + (threadIdx.x >> 3);
        const bool live = rr < total_rows;
        const uint32_t g = live ? (uint32_t)rr : total_rows - 1;        // idle lanes redo the last row (the lane sum below is wave-wide)
        uint32_t jr;
        const RtDesc& D = desc[map.find(g, jr)];
        const uint8_t* row = D.rows + (size_t)jr * n_coeffs * SYMB;
        uint64_t col[19];
#pragma unroll
        for (int k = 0; k < 19; k++) col[k] = 0;
        uint32_t since = 0;
        uint4 n0 = zero, n1 = zero, n2 = zero, n3 = zero;     // the next step's symbol, read one step ahead of its products
        if (j < n_coeffs) {
            const uint4* q = reinterpret_cast<const uint4*>(row + (size_t)j * SYMB);
            n0 = q[0]; n1 = q[1];
            if constexpr (SYMB == 64) { n2 = q[2]; n3 = q[3]; }
        }
        for (uint32_t k = 0; k < steps; k++) {
            const uint32_t i = 8 * k + j;
            const uint4 s0 = n0, s1 = n1, s2 = n2, s3 = n3;
            n0 = zero; n1 = zero; n2 = zero; n3 = zero;
            if (i + 8 < n_coeffs) {
                const uint4* q = reinterpret_cast<const uint4*>(row + (size_t)(i + 8) * SYMB);
                n0 = q[0]; n1 = q[1];
                if constexpr (SYMB == 64) { n2 = q[2]; n3 = q[3]; }
            }
            const uint4* tp = rt_lds_tau + (size_t)i * EU4;
#pragma unroll
            for (int h = 0; h < SYMB / 32; h++) {             // the lower half against tau^i, the upper (SYMB == 64) against 2^256 tau^i
                const uint32_t c[8] = {h ? s2.x : s0.x, h ? s2.y : s0.y, h ? s2.z : s0.z, h ? s2.w : s0.w,
                                       h ? s3.x : s1.x, h ? s3.y : s1.y, h ? s3.z : s1.z, h ? s3.w : s1.w};
                uint32_t x[9];
                kzg_unpack29(c, x);
                const uint4 t0 = tp[3 * h], t1 = tp[3 * h + 1], t2 = tp[3 * h + 2];
                const uint32_t y[9] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w, t2.x};
#pragma unroll
                for (int a = 0; a < 9; a++)
#pragma unroll
                    for (int b = 0; b < 9; b++) col[a + b] += (uint64_t)x[a] * y[b];
            }
            if (++since == (uint32_t)rt_lazy_group<SYMB>()) { kzg_ripple29(col); since = 0; }
        }
        kzg_ripple29(col);
        const F30<Q> acc = kzg_columns_join<Q>(col);
        kzg_eval_finish<Q, true>(acc, live, j, (size_t)g, A.w, out, 64, D.prf + 16 * (size_t)jr);
    }
}

// The same for an SRS longer than KZG_LAZY_MAX_COEFFS: the Horner form of k_kzg_eval_rows30 with the symbol reduced to the plain stream
// on load (one product).  Bounds: the symbol is below 2^258, acc = acc tau^8 + symbol < r + 2^250 + 2^258 < 2^259 at every step, the
// lane sum of the eight products with tau^j below 2^258.  SYMB == 32: the symbol is loaded as it is, below 2^256: the same bounds.
template <int SYMB, class Map = RtMapShift>
__global__ void __launch_bounds__(256)
k_rt_eval_horner(const RtDesc* __restrict__ desc, const Map map, uint32_t total_rows, uint32_t n_coeffs, KzgEvalConsts K,
                 uint8_t* __restrict__ out) {
    using Q = IccBn254Fr;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;       // (eight lanes per row: 2^29 rows and more pass 32 bits)
    const uint32_t j = (uint32_t)t & 7u;
    const bool live = (t >> 3) < total_rows;
    const uint32_t g = live ? (uint32_t)(t >> 3) : total_rows - 1;      // idle lanes redo the last row (the lane sum is wave-wide)
    uint32_t jr;
    const RtDesc& D = desc[map.find(g, jr)];
    const uint8_t* row = D.rows + (size_t)jr * n_coeffs * SYMB;
    const F30<Q> T8 = f30_unpack<Q>(K.t8);
    F30<Q> acc;
#pragma unroll
    for (int l = 0; l < 9; l++) acc.v[l] = 0;
    for (uint32_t k = (n_coeffs + 7) / 8; k-- > 0;) {
        const uint32_t i = 8 * k + j;
        F30<Q> c;
#pragma unroll
        for (int l = 0; l < 9; l++) c.v[l] = 0;
        if (i < n_coeffs) c = rt_symbol_mod_q<Q, SYMB>(row + (size_t)i * SYMB);
        acc = icc30_add<Q>(icc30_mul<Q>(acc, T8), c);
    }
    uint32_t tj[8];
#pragma unroll
    for (int w = 0; w < 8; w++) {
        tj[w] = K.tj[0][w];
#pragma unroll
        for (int jj = 1; jj < 8; jj++) tj[w] = j == (uint32_t)jj ? K.tj[jj][w] : tj[w];
    }
    acc = icc30_mul<Q>(acc, f30_unpack<Q>(tj));
    kzg_eval_finish<Q, true>(acc, live, j, (size_t)g, K.alpha, out, 64, D.prf + 16 * (size_t)jr);
}

// ---- IPA: the rows g0 .. g0 + rows - 1 of the call as rows of the two passes.  A lane per symbol: sym mod n, canonical, as the 32-byte
// big-endian coefficient client_block_pass takes; then a lane per row: its PRF value as the scalar row of the h pass (cr_prf /
// cr_store_row: the client rebuild's reading of d_prf for the IPA build, r.d[0], r.d[1] as little-endian words).  SYMB == 32: a symbol
// below p_icc is still reduced mod n -- two different 256-bit moduli.
template <class Q, int SYMB, class Map = RtMapShift>
__global__ void __launch_bounds__(256)
k_rt_pack(const RtDesc* __restrict__ desc, const Map map, uint32_t g0, uint32_t rows, uint32_t ncols, uint8_t* __restrict__ coeffs,
          uint8_t* __restrict__ scalars) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t symbols = (size_t)rows * ncols;
    uint32_t jr;
    if (t < symbols) {
        const uint32_t gl = (uint32_t)(t / ncols), c = (uint32_t)(t - (size_t)gl * ncols), g = g0 + gl;
        const RtDesc& D = desc[map.find(g, jr)];
        const F30<Q> v = rt_symbol_mod_q<Q, SYMB>(D.rows + (size_t)SYMB * ((size_t)jr * ncols + c));
        cr_store_row<Q>(coeffs + 32 * t, icc30_canonical<Q>(icc30_reduce_top<Q>(v)));
    } else if (t - symbols < rows) {
        const uint32_t gl = (uint32_t)(t - symbols), g = g0 + gl;
        const RtDesc& D = desc[map.find(g, jr)];
        cr_store_row<Q>(scalars + 32 * (size_t)gl, cr_prf<Q, true>(D.prf, jr));
    }
}

// ---- compare: a lane per row g0 + gl.  ADD (IPA): the expected MAC is first formed in place, exp[gl] = exp[gl] + hpts[gl], with the
// client batches' addition (k_cr_place / k_cu_place: xyzz30_add_mem with its equal, opposite and infinity cases) and their conversion
// to canonical affine bytes.  Then the row's 64 expected bytes against its d_macs bytes as 16-byte loads: a stored coordinate >= p
// differs from the canonical form and is not OK, infinity is 64 zero bytes on both sides.  The failures are counted per request.
// the 64 expected bytes at `mine` against row jr of D's MAC store -> status, count
__device__ __forceinline__ void rt_compare_bytes(const RtDesc& D, uint32_t jr, const uint8_t* mine) {
    const uint4* e = reinterpret_cast<const uint4*>(mine);
    const uint4* m = reinterpret_cast<const uint4*>(D.macs + 64 * (size_t)jr);
    uint32_t diff = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint4 x = e[i], y = m[i];
        diff |= (x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w);
    }
    D.status[jr] = diff ? 0 : PORLA_RETRIEVE_ROW_OK;
    if (diff && D.counts) atomicAdd(D.counts, 1u);
}
// What the last kernel of the check does with a row's 64 expected bytes, a template parameter of the compare kernels.  RtActCompare (the
// default): judge -- rt_compare_bytes, the retrieval calls' and the extraction's instances.  RtActWrite: the top-level repair's second
// pass (repair_batch.hip), whose requests read the members the check does not use another way:
//   status   the half's row statuses as the check pass left them (read)
//   steps    the OTHER half's row statuses, n bytes (read)
//   out      the half's action bytes: the data bit is there already, this kernel adds the MAC bit
//   counts   two words or nullptr: [0] the half's data rows rewritten, [1] its MAC rows rewritten
// A row is written iff its own status is 0 and its sibling's is OK; the expected bytes go over the row's MAC bytes when they differ.
struct RtActCompare {
    static __device__ __forceinline__ void row(const RtDesc& D, uint32_t jr, const uint8_t* mine) { rt_compare_bytes(D, jr, mine); }
};
struct RtActWrite {
    static __device__ __forceinline__ void row(const RtDesc& D, uint32_t jr, const uint8_t* mine) {
        const uint8_t* other = reinterpret_cast<const uint8_t*>(D.steps);
        if (D.status[jr] != 0 || other[jr] != PORLA_RETRIEVE_ROW_OK) return;
        const uint4* e = reinterpret_cast<const uint4*>(mine);
        uint4* m = reinterpret_cast<uint4*>(const_cast<uint8_t*>(D.macs) + 64 * (size_t)jr);
        const uint4 e0 = e[0], e1 = e[1], e2 = e[2], e3 = e[3], m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3];
        const uint32_t diff = (e0.x ^ m0.x) | (e0.y ^ m0.y) | (e0.z ^ m0.z) | (e0.w ^ m0.w) | (e1.x ^ m1.x) | (e1.y ^ m1.y) | (e1.z ^ m1.z) |
                              (e1.w ^ m1.w) | (e2.x ^ m2.x) | (e2.y ^ m2.y) | (e2.z ^ m2.z) | (e2.w ^ m2.w) | (e3.x ^ m3.x) | (e3.y ^ m3.y) |
                              (e3.z ^ m3.z) | (e3.w ^ m3.w);
        const uint8_t data = D.out[jr];
        if (diff) {
            m[0] = e0; m[1] = e1; m[2] = e2; m[3] = e3;
            D.out[jr] = (uint8_t)(data | PORLA_REPAIR_MAC);
        }
        if (D.counts) {
            if (data & PORLA_REPAIR_DATA) atomicAdd(D.counts, 1u);
            if (diff) atomicAdd(D.counts + 1, 1u);
        }
    }
};
// row g0 + gl on the calling lane
template <class C, bool ADD, class Map, class Act = RtActCompare>
__device__ __forceinline__ void rt_compare_row(const RtDesc* __restrict__ desc, const Map map, uint32_t g0, uint32_t gl,
                                               uint8_t* __restrict__ exp, const uint8_t* __restrict__ hpts) {
    using M = typename C::Fp;
    uint32_t jr;
    const RtDesc& D = desc[map.find(g0 + gl, jr)];
    uint8_t* mine = exp + 64 * (size_t)gl;
    if constexpr (ADD) {
        XYZZ<M> a = load_affine_be_lazy<M>(mine);
        const XYZZ<M> b = load_affine_be_lazy<M>(hpts + 64 * (size_t)gl);
        xyzz30_add_mem<M>(&a, &b, 0, 0, nullptr);
        store_affine_be<M>(mine, xyzz30_to_xyzz<M>(xyzz30_load_lazy<M>(&a)));
    }
    Act::row(D, jr, mine);
}
template <class C, bool ADD, class Map = RtMapShift, class Act = RtActCompare>
__global__ void __launch_bounds__(64)
k_rt_compare(const RtDesc* __restrict__ desc, const Map map, uint32_t g0, uint32_t rows, uint8_t* __restrict__ exp,
             const uint8_t* __restrict__ hpts) {
    const size_t gl64 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gl64 >= rows) return;
    rt_compare_row<C, ADD, Map, Act>(desc, map, g0, (uint32_t)gl64, exp, hpts);
}

// ---- the aligned compare: a QUAD per row, RT_ALIGNED_ROWS = MACQ_BF rows per block of 256 lanes.  The stored MAC row must equal
// E_j - alpha A_j: E_j (ADD: exp + hpts first, as above) goes into the quad's `um`, A_j -- read as the MAC stores are read everywhere,
// load_affine_be_lazy: coordinates reduced, 64 zero bytes = infinity, not checked to be on the curve -- into its table slot, alpha A_j
// is the wave-uniform ladder (macq_ladder_uniform: alpha is the launch's one scalar), and um + (-(alpha A_j)) goes through the quad
// kernels' out path (macq_sum_out: tm at infinity, um at infinity, equal and opposite points through macq_add's general addition).
// Lane 0 of the quad converts to canonical affine bytes in place of the row's expected bytes and compares as k_rt_compare does (Act:
// or writes, RtActWrite above).
// The skip: a block none of whose rows has a nonzero byte in its alignment row (a request without d_align; an X half; a cached top
// level) pays for no ladder -- its first wave runs k_rt_compare's body, a lane per row, and the other three leave.  The decision is
// the block's (__syncthreads_or), so no wave with live quads diverges into the ladder; inside a block that runs it, a quad whose A_j
// is infinity leaves the ladder at once as in every quad kernel.  (An alignment row that is nonzero but reduces to infinity takes the
// ladder's path and gets the same answer there.)  Padding quads (rows beyond the last) hold infinity on both sides -- row 0's expected
// bytes may be in the middle of being rewritten by that row's own quad -- so they leave the ladder at once, and store nothing.
constexpr int RT_ALIGNED_ROWS = MACQ_BF;
template <class C, bool ADD, class Map = RtMapShift, class Act = RtActCompare>
__global__ void __launch_bounds__(4 * MACQ_BF) MACQ_GUEST_ATTR
k_rt_compare_aligned(const RtDesc* __restrict__ desc, const Map map, uint32_t g0, uint32_t rows, uint8_t* __restrict__ exp,
                     const uint8_t* __restrict__ hpts, MacScalar alpha) {
    using M = typename C::Fp;
    MACQ_LDS(L);
    const uint32_t q = threadIdx.x >> 2, r = threadIdx.x & 3u, lane = threadIdx.x & 63u;
    const size_t gl64 = (size_t)blockIdx.x * MACQ_BF + q;
    const bool valid = gl64 < rows;
    const uint32_t gl = valid ? (uint32_t)gl64 : 0u;
    uint32_t jr;
    const RtDesc& D = desc[map.find(g0 + gl, jr)];
    const uint8_t* ap = D.align ? D.align + 64 * (size_t)jr : nullptr;
    bool finite = false;
    if (valid && ap) {                                                     // lane r looks at its quarter of the row
        const uint4 v = reinterpret_cast<const uint4*>(ap)[r];
        finite = (v.x | v.y | v.z | v.w) != 0u;
    }
    if (!__syncthreads_or(finite)) {
        const size_t mine64 = (size_t)blockIdx.x * MACQ_BF + threadIdx.x;
        if (threadIdx.x < (uint32_t)MACQ_BF && mine64 < rows) rt_compare_row<C, ADD, Map, Act>(desc, map, g0, (uint32_t)mine64, exp, hpts);
        return;
    }
    uint8_t* mine = exp + 64 * (size_t)gl;
    if (r < 2u) {                                                          // lanes 0 and 1 side by side: E_j and A_j
        XYZZ<M> p = load_affine_be_lazy<M>(r && ap ? ap : mine);
        if (!valid || (r && !ap)) { p.x = fe_zero<M>(); p.y = p.x; p.zz = p.x; p.zzz = p.x; }
        if constexpr (ADD) {
            if (valid && r == 0u) {
                const XYZZ<M> b = load_affine_be_lazy<M>(hpts + 64 * (size_t)gl);
                xyzz30_add_mem<M>(&p, &b, 0, 0, nullptr);
            }
        }
        store_xyzz<M>(r ? &L.qd[q].tbl[0] : &L.um[q], p);
    }
    macq_sync();
    uint32_t sc[8];
#pragma unroll
    for (int j = 0; j < 8; j++) sc[j] = alpha.v[j];
    F30<M> c;
    bool inf;
    macq_ladder_uniform<C>(L, q, r, lane, threadIdx.x >> 6, sc, c, inf);
    const F30<M> cn = r == 1u ? f30_sub<M, 4>(F30<M>{}, c) : c;            // -(alpha A_j), as macq_butterfly_out negates
    macq_sum_out<M>(&L.um[q], &L.acc[q], &L.tmp[q], cn, inf, &L.qd[q].tbl[1], true, r, lane);      // (the table is done with)
    macq_sync();
    if (valid && r == 0u) {
        store_affine_be<M>(mine, xyzz30_to_xyzz<M>(xyzz30_load_lazy<M>(&L.qd[q].tbl[1])));
        Act::row(D, jr, mine);
    }
}

}  // namespace porla
