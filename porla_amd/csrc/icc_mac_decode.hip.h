// The ICC MAC decode: the MAC network of mac_fft.hip.h run BACKWARDS on group elements, for K independent levels in one call
// (include/porla_gpu.h: porla_icc_mac_decode_batch_device).  The MAC-side twin of icc_decode.hip.h: a level's coded MAC rows go back
// to the per-block MACs, so that a block recovered by the data decode can be checked against alpha * commit(block) + PRF * h.
//
// WHAT: stage s of the encode is (A, B) <- (A + vi B, A - vi B) on the rows k, k + 2^(s-1), vi the INTEGER (w^e mod p_icc) mod q
// handed to the group as a scalar.  Its inverse is (A, B) <- ((A + B) / 2, (A - B) / (2 vi)): the stages run from log2 n_rows down to
// 1 as (A, B) <- (A + B, vi^-1 (A - B)) and the 2^-1 of every stage is collected into ONE factor n_rows^-1 per row.  With write steps
// row i is also divided by wt_i = (w^reverse_bits(step_i % N, log2 N) mod p_icc) mod q: the close multiplies row i ONCE, by
// n_rows^-1 wt_i^-1 mod q.  All scalars are mod the group order q; vi^-1 and wt_i^-1 are true inversions mod q (division steps,
// inv30.hip.h).  It takes one complete half: with w of order N the 2 n rows of a level are no erasure code (most n-row subsets
// are rank-deficient).
//
// TABLES: the inverse twiddles as the ladders take a scalar (eight plain little-endian words per entry, mac_load_twiddle) are
// derived per (n_total, curve) from the data decode's table of inverses mod q (icc.hip: tw30qi, the 2^270 form; k_icd_twiddles_qinv)
// by one product with 1, and the wave-uniform stages' digit codes by k_mac_wnaf_codes on that plain table.  w^e mod p_icc for the write
// steps is entry e of the encode's p_icc plane table.  Both are read under the ICC workspace's lock and fence
// (icc_decode_tables_acquire); the derived tables live in this call family's own workspace behind its own lock and fence.
//
// KERNELS (launch sequence: upload, scalars, load, log2 n_rows stages, close -- it depends on n_rows, never on K):
//   k_imd_row_scalars   one lane per row: n_rows^-1 wt_i^-1 mod q, plain
//   k_imd_load          one lane per row: 64-byte big-endian affine (reduced as SetBytes does) minus the optional d_sub row -> the
//                       work array's lazy memory form; the K tables of n_rows rows lie end to end
//   k_imd_stage_quad    stages log2 n_rows .. 2, FOUR lanes per butterfly (the shape of k_mac_stage30_quad with the order turned
//                       round): A + B to work[k]; A - B into the quad's table slot; the ladder by the inverse twiddle; the product to
//                       work[k + m2].  Per-butterfly form (macq_ladder) and wave-uniform form (macq_ladder_uniform, n_rows / 2^s >=
//                       16).  BOTH take the total butterfly count K n_rows / 2 as their last argument and BOTH run on the K tables
//                       of one work array: n_rows / 2^s is a multiple of 16 in the uniform form, so the 16 butterflies of a wave lie in
//                       one table's stage and share j (mac_stage_index<16>), and every request reads the one table of (n_total,
//                       curve).  No eight-lane form is built.
//   k_imd_stage1_quad   stage 1 (twiddle 1: A + B, A - B, no ladder; cf. k_mac_stage1_quad), on imd_sum_dif
//   k_imd_close_quad    four lanes per row: the ladder by the row's scalar, then one lane converts to affine big-endian (64 zero bytes
//                       for infinity) with the division-step inversion, as k_mac_finish does
//
// COMPLETE ADDITIONS: in the decode equal operands, opposite operands and infinity are the ordinary case (the encode of a unit vector
// is a constant column: the first stage meets A == B in every butterfly -- a doubling in A + B, infinity in A - B -- and every later
// stage meets infinity).  imd_sum_dif is macq_butterfly_out with a live flag per output: infinity on either side is decided before any
// arithmetic, and macq_add falls back to the complete one-lane addition (xyzz30_add: doubling, opposite) when the quad meets equal x.
// macq_ladder / macq_ladder_uniform return infinity for an operand at infinity before they read anything else.
//
// BOUNDS: the ladders negate their operand's Y as 4p - Y, which takes Y <= 3p + 2^246 (f30_sub: limb 8 of the table is that of 4p minus
// 1).  Sums and ladder results are within that (xyzz30_add: Y3 <= 3p); a value that PASSES THROUGH a butterfly negated (A = infinity:
// A - B = -B) would be 4p - Y, above 3p whenever Y < p -- and a canonical Y from the load step below 2^240 would put it past the
// table's limb 8.  With infinities the ordinary case here, both places that negate a value they then store reduce it: k_imd_load
// negates d_sub's canonical Y as p - Y, imd_sum_dif multiplies 4p - Y by the Montgomery unit (one product on the rare path: < p + 2^246).
//
// Checked per form by tools/ladder_check.hip (istage_quad, istage_quad_uniform) on scalars and operands of the test's
// (tests/mac_decode_vectors.py), end to end against tests/mac_decode_model.py and the device encode (tests/test_icc_mac_decode_gpu.py).
#pragma once
#include "mac_fft.hip.h"
#include "icc_decode.hip.h"

namespace porla {

// a request as the kernels see it: the layout of porla_icc_mac_decode_req, uploaded as it is
struct ImdDesc {
    const uint8_t* macs;
    uint8_t* out;
    const unsigned long long* steps;
    const uint8_t* sub;
};
static_assert(sizeof(ImdDesc) == 32, "ImdDesc is porla_icc_mac_decode_req");

// n_rows^-1 mod q in the 2^270 form: the plain integer 2^(270 - log2 n_rows) mod q (the host reduces it)
struct ImdScale { uint32_t q[8]; };

template <class M>
__device__ __forceinline__ F30<M> imd_one30() {
    F30<M> r{};
    r.v[0] = 1u;
    return r;
}
__device__ __forceinline__ void imd_store_scalar(uint32_t* dst, const uint32_t (&t)[8]) {
    uint4* d = reinterpret_cast<uint4*>(dst);
    d[0] = make_uint4(t[0], t[1], t[2], t[3]);
    d[1] = make_uint4(t[4], t[5], t[6], t[7]);
}

// entry e of the plain inverse table = ((w^e mod p_icc) mod q)^-1 mod q, canonical, from the 2^270-form entry of tw30qi
template <class Q>
__global__ void __launch_bounds__(256)
k_imd_twiddles_plain(const uint32_t* __restrict__ twqi, uint32_t n, uint32_t* __restrict__ itws) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const F30<Q> t = icc30_ld_pslot<Q>(twqi + (size_t)e * ICC30_PSLOT_WORDS);
    const Fe<Q> s = icc30_canonical<Q>(icc30_mul<Q>(t, imd_one30<Q>()));       // / 2^270: plain, below q + 2^250 < 2 q
    imd_store_scalar(itws + (size_t)e * 8, s.v);
}

// scal[row] = n_rows^-1 * wt^-1 mod q (wt = 1 for a request without write steps), row = request * n_rows + i.  twp: the p_icc plane
// table of tw_n = n_total entries (w^e in the 2^270 form).  The division steps vote across the wave, so no lane leaves early.
template <class Q>
__global__ void __launch_bounds__(64)
k_imd_row_scalars(const ImdDesc* __restrict__ desc, uint32_t total, uint32_t n_rows, const uint32_t* __restrict__ twp, uint32_t tw_n,
                  int tw_log, ImdScale ninv, uint32_t* __restrict__ scal) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = i < total;
    const uint32_t row = in ? i : 0u;
    const unsigned long long* steps = desc[row / n_rows].steps;
    Fe<Q> v = fe_zero<Q>();
    v.v[0] = 1u;
    if (in && steps) {
        const uint32_t e = __brev((uint32_t)steps[row % n_rows] & (tw_n - 1u)) >> (32 - tw_log);
        const F30<IccFp> w = icc30_ld_pslot<IccFp>(twp + (size_t)e * ICC30_PSLOT_WORDS);
        const Fe<IccFp> P = icc30_finish_p(icc30_mul<IccFp>(w, imd_one30<IccFp>()));      // w^e mod p_icc, canonical
#pragma unroll
        for (int k = 0; k < 8; k++) v.v[k] = P.v[k];
        fe_reduce_small<Q, Q::MAX_Q_P>(v.v);                                               // ... mod q: not 0 (tests/test_icc_decode_cpu.py)
    }
    const F30<Q> r = f30_inv_safegcd_raw<Q>(v);                                            // v^-1 + k q, below 4 q
    const Fe<Q> s = icc30_canonical<Q>(icc30_mul<Q>(r, f30_unpack<Q>(ninv.q)));            // times n_rows^-1: plain, below 2 q
    if (in) imd_store_scalar(scal + (size_t)i * 8, s.v);
}

// work[row] = d_macs[i] - d_sub[i] of request row / n_rows, in the lazy memory form
template <class C>
__global__ void __launch_bounds__(64)
k_imd_load(const ImdDesc* __restrict__ desc, uint32_t total, uint32_t n_rows, XYZZ<typename C::Fp>* __restrict__ work) {
    using M = typename C::Fp;
    const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= total) return;
    const ImdDesc D = desc[row / n_rows];
    const size_t at = (size_t)(row % n_rows) * 64;
    const XYZZ<M> pm = load_affine_be_lazy<M>(D.macs + at);
    if (!D.sub) { store_xyzz<M>(work + row, pm); return; }
    const XYZZ<M> sm = load_affine_be_lazy<M>(D.sub + at);
    XYZZ<M> nm = sm;
    nm.y = fe_sub<M>(fe_zero<M>(), sm.y);                                  // -sub, Y canonical (infinity stays all zero)
    XYZZ30<M> a = xyzz30_load_lazy<M>(&pm), b = xyzz30_load_lazy<M>(&nm);
    xyzz30_add<M>(a, b);
    xyzz30_store_lazy<M>(work + row, a);
}

// sum = a + (c, inf), dif = a - (c, inf) in the memory form: a in LDS, (c, inf) in the quad's registers.  macq_butterfly_out with a
// live flag per output (the stages' dif is the quad's own LDS slot and always written) and a reduced Y where -B passes through
template <class M>
__device__ __forceinline__ void imd_sum_dif(const XYZZ<M>* a, XYZZ<M>* slot_a, XYZZ<M>* slot_b, const F30<M>& c, bool inf, XYZZ<M>* sum,
                                            bool sum_live, XYZZ<M>* dif, bool dif_live, uint32_t r, uint32_t lane) {
    bool z;
    const F30<M> u = macq_load_residue<M>(reinterpret_cast<const uint32_t*>(a) + 8 * r, &z);
    const bool a_inf = macq_quad_any(z && r == 2u, lane);
    if (inf) {                                                             // B = infinity: both outputs are A
        if (sum_live) macq_store_point<M>(sum, u, a_inf, r);
        if (dif_live) macq_store_point<M>(dif, u, a_inf, r);
        return;
    }
    const F30<M> cn = r == 1u ? f30_sub<M, 4>(F30<M>{}, c) : c;            // -B
    if (a_inf) {
        if (sum_live) macq_store_point<M>(sum, c, false, r);
        const F30<M> red = f30_mul<M>(cn, f30_const<M>(M::R1_30));         // (4p - Y) * 1: below p + 2^246 (see BOUNDS)
        if (dif_live) macq_store_point<M>(dif, r == 1u ? red : c, false, r);
        return;
    }
    F30<M> s = c;
    bool s_inf = false;
    macq_add<M>(s, s_inf, a, reinterpret_cast<const uint32_t*>(a), false, slot_a, slot_b, r, lane);
    if (sum_live) macq_store_point<M>(sum, s, s_inf, r);
    s = cn;
    s_inf = false;
    macq_add<M>(s, s_inf, a, reinterpret_cast<const uint32_t*>(a), false, slot_a, slot_b, r, lane);
    if (dif_live) macq_store_point<M>(dif, s, s_inf, r);
}

// Stage s (>= 2) of the network backwards over the tables of one work array: butterfly t < total on the rows (k, k + m2) found by
// mac_stage_index; itws: the plain inverse table of n_tab entries (n_tab = n_total: e = j * (n_tab >> (s-1)) is the exponent in THAT
// table, whatever the row count of the work array's tables).  UNIFORM (launched when n_rows >> s >= 16): the 16 quads of a wave share
// j; codes: k_mac_wnaf_codes of itws.  Padding quads compute butterfly 0 and store nothing (whole waves of them in the uniform form).
template <class C, bool UNIFORM>
__global__ void __launch_bounds__(4 * MACQ_BF) MACQ_GUEST_ATTR
k_imd_stage_quad(XYZZ<typename C::Fp>* __restrict__ work, const uint32_t* __restrict__ itws, uint32_t n_tab, int s,
                 const uint16_t* __restrict__ codes, uint32_t total) {
    using M = typename C::Fp;
    MACQ_LDS(L);
    __builtin_amdgcn_s_setprio(3);                                         // (as k_mac_stage30_quad: a latency-bound wave)
    const uint32_t q = threadIdx.x >> 2, r = threadIdx.x & 3u, lane = threadIdx.x & 63u;
    uint32_t t = blockIdx.x * MACQ_BF + q;
    const bool valid = t < total;
    if (!valid) t = 0;
    uint32_t k, m2, e, sc[8];
    mac_stage_index<UNIFORM ? 16u : 1u>(t, n_tab, s, k, m2, e);
    mac_load_twiddle(sc, itws, e);
    macq_copy_coord<M>(&L.um[q], work + k, r);
    bool z;
    F30<M> c = macq_load_residue<M>(reinterpret_cast<const uint32_t*>(work + k + m2) + 8 * r, &z);
    bool inf = macq_quad_any(z && r == 2u, lane);
    macq_sync();
    // work[k] = A + B; the quad's table slot = A - B
    imd_sum_dif<M>(&L.um[q], &L.acc[q], &L.tmp[q], c, inf, work + k, valid, &L.qd[q].tbl[0], true, r, lane);
    macq_sync();
    if constexpr (UNIFORM) macq_ladder_uniform<C>(L, q, r, lane, threadIdx.x >> 6, sc, c, inf,
                                                   codes + (size_t)(e >> MACQ_CODES_EXP_SHIFT) * MACQ_CODES_STRIDE);
    else macq_ladder<C>(L.qd[q], &L.acc[q], &L.tmp[q], r, lane, sc, c, inf);
    if (valid) macq_store_point<M>(work + k + m2, c, inf, r);              // work[k + m2] = vi^-1 (A - B)
}

// Stage 1 over all points / 2 butterflies (k, k + 1) of the work array: its twiddle is 1, so A + B and A - B and nothing else.
// 256 lanes = 64 butterflies per block.
template <class C>
__global__ void __launch_bounds__(256) MACQ_GUEST_ATTR
k_imd_stage1_quad(XYZZ<typename C::Fp>* __restrict__ work, uint32_t points) {
    using M = typename C::Fp;
    __shared__ XYZZ<M> um[64], slot_a[64], slot_b[64];                     // 24 KiB: several blocks per compute unit
    const uint32_t q = threadIdx.x >> 2, r = threadIdx.x & 3u, lane = threadIdx.x & 63u;
    uint32_t t = blockIdx.x * 64 + q;
    const bool valid = t < points / 2;
    if (!valid) t = 0;
    const uint32_t k = 2 * t;
    macq_copy_coord<M>(&um[q], work + k, r);
    bool z;
    const F30<M> c = macq_load_residue<M>(reinterpret_cast<const uint32_t*>(work + k + 1) + 8 * r, &z);
    const bool inf = macq_quad_any(z && r == 2u, lane);
    macq_sync();
    imd_sum_dif<M>(&um[q], &slot_a[q], &slot_b[q], c, inf, work + k, valid, work + k + 1, valid, r, lane);
}

// out row = scal[row] * work[row] as 64 bytes big-endian affine, row = request * n_rows + i: four lanes walk the ladder, lane 0 inverts
template <class C>
__global__ void __launch_bounds__(4 * MACQ_BF) MACQ_GUEST_ATTR
k_imd_close_quad(const XYZZ<typename C::Fp>* __restrict__ work, const uint32_t* __restrict__ scal, uint32_t total, uint32_t n_rows,
                 const ImdDesc* __restrict__ desc) {
    using M = typename C::Fp;
    MACQ_LDS(L);
    __builtin_amdgcn_s_setprio(3);
    const uint32_t q = threadIdx.x >> 2, r = threadIdx.x & 3u, lane = threadIdx.x & 63u;
    uint32_t row = blockIdx.x * MACQ_BF + q;
    const bool valid = row < total;
    if (!valid) row = 0;                                                   // padding quads compute row 0 and store nothing
    uint32_t sc[8];
    mac_load_twiddle(sc, scal, row);
    macq_copy_coord<M>(&L.qd[q].tbl[0], work + row, r);
    macq_sync();
    F30<M> c;
    bool inf;
    macq_ladder<C>(L.qd[q], &L.acc[q], &L.tmp[q], r, lane, sc, c, inf);
    macq_store_point<M>(&L.um[q], c, inf, r);
    macq_sync();
    if (valid && r == 0u)
        store_affine_be<M>(desc[row / n_rows].out + (size_t)(row % n_rows) * 64, xyzz30_to_xyzz<M>(xyzz30_load_lazy<M>(&L.um[q])));
}

// ---------------------------------------------------------------- host: what a launch of the four-lane kernels above needs
template <class C>
static void imd_lds_attributes() {
    static LdsOnce once;
    constexpr size_t quad = macq_lds_bytes<C>();
    once.set({lds_kernel(&k_imd_stage_quad<C, false>, quad), lds_kernel(&k_imd_stage_quad<C, true>, quad),
              lds_kernel(&k_imd_close_quad<C>, quad)});
}

// The launches of one stage / the close, shared by icc_mac_decode.hip and the per-form driver tools/ladder_check.hip
template <class C>
static void imd_launch_stage(bool uniform, XYZZ<typename C::Fp>* work, const uint32_t* itws, uint32_t n_tab, int s, const uint16_t* codes,
                             uint32_t total, hipStream_t stream) {
    const dim3 grid((total + MACQ_BF - 1) / MACQ_BF), block(4 * MACQ_BF);
    if (uniform) hipLaunchKernelGGL((k_imd_stage_quad<C, true>), grid, block, macq_lds_bytes<C>(), stream, work, itws, n_tab, s, codes, total);
    else hipLaunchKernelGGL((k_imd_stage_quad<C, false>), grid, block, macq_lds_bytes<C>(), stream, work, itws, n_tab, s, codes, total);
}
// is stage s of tables of n_rows rows launched in the wave-uniform form?
static inline bool imd_stage_uniform(size_t n_rows, int s) { return s >= 2 && (n_rows >> s) >= 16; }

}  // namespace porla
