// Kernels of the batched verified retrieval (retrieve_batch.hip: porla_kzg_retrieve_batch_device / porla_ipa_retrieve_batch_device):
// every coded row of an exact half is checked against its stored MAC row in the CODED domain.  The data network works mod LCM =
// p_icc q with integer multipliers vi < p_icc and the MAC network multiplies by the same vi reduced mod q, so coded row j reduced mod q
// is the Z_q network of the chunks and the half's MAC row j is
//
//     alpha * Commit(row_j mod q) + s_j * h,        s_j = the PRF value of the complement the client holds for that row
//
// -- no group-element network runs.  KZG: the client knows tau, so Commit is one polynomial evaluation per row (k_rt_eval_lazy, or
// k_rt_eval_horner for a long SRS) and the expected MAC a two-coefficient commitment against (G1[0], h_MAC).  IPA: the row's 128
// symbols reduced mod n are one commitment row against the alpha generators (k_rt_pack), the PRF value one row of the hiding base.
// k_rt_compare sets the status bytes from the expected MACs' canonical affine bytes.  The rows of all K requests are numbered through,
// g = request * n_rows + row, and a kernel finds its request by a shift.
#pragma once
#include "kzg_eval.hip.h"
#include "client_rebuild_batch.hip.h"

namespace porla {

// One request as the kernels see it: porla_retrieve_req field for field.
struct RtDesc {
    const uint8_t* rows;
    const uint8_t* macs;
    const uint8_t* prf;
    uint8_t* out;
    uint8_t* status;
    uint32_t* counts;
};
static_assert(sizeof(RtDesc) == 48, "RtDesc: six pointers");

// the call zeroes both counters of every request that has them
__global__ void __launch_bounds__(256)
k_rt_clear(const RtDesc* __restrict__ desc, uint32_t k) {
    const uint32_t a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a < k && desc[a].counts) { desc[a].counts[0] = 0; desc[a].counts[1] = 0; }
}

// 64-byte little-endian symbol -> its residue mod q in the plain stream, unreduced: hi * (2^256 in the 2^270 form) -- below q + 2^242
// -- plus the raw lower half, below 2^258 (icc30_load_symbol's q part)
template <class Q>
__device__ __forceinline__ F30<Q> rt_symbol_mod_q(const uint8_t* __restrict__ src) {
    const Fe<Q> lo = ld_fe<Q>(reinterpret_cast<const uint32_t*>(src));
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
constexpr int RT_LAZY_GROUP = 3;              // symbols accumulated between two ripples of the columns
constexpr int RT_LAZY_ENTRY_U4 = 2 * KZG_LAZY_ENTRY_WORDS / 4;

__global__ void __launch_bounds__(256)
k_rt_eval_lazy(const RtDesc* __restrict__ desc, uint32_t n_rows_log, uint32_t total_rows, uint32_t n_coeffs,
               const uint32_t* __restrict__ tau29w, KzgAlpha270 A, uint8_t* __restrict__ out) {
    using Q = IccBn254Fr;
    extern __shared__ uint4 rt_lds_tau[];
    const uint32_t steps = (n_coeffs + 7) / 8;
    for (uint32_t i = threadIdx.x; i < steps * 8u * RT_LAZY_ENTRY_U4; i += blockDim.x)
        rt_lds_tau[i] = reinterpret_cast<const uint4*>(tau29w)[i];
    __syncthreads();
    const uint32_t j = threadIdx.x & 7u;
    const uint4 zero = make_uint4(0, 0, 0, 0);
    // a block takes 32 rows at a time, grid-strided: the table above is staged once per block, not once per 32 rows
    // (counted in 64 bits: the call may hold up to 2^32 - 1 rows)
    for (size_t r0 = (size_t)blockIdx.x * (blockDim.x >> 3); r0 < total_rows; r0 += (size_t)gridDim.x * (blockDim.x >> 3)) {
        const size_t rr = r0 + (threadIdx.x >> 3);
        const bool live = rr < total_rows;
        const uint32_t g = live ? (uint32_t)rr : total_rows - 1;        // idle lanes redo the last row (the lane sum below is wave-wide)
        const RtDesc& D = desc[g >> n_rows_log];
        const uint32_t jr = g & ((1u << n_rows_log) - 1u);
        const uint8_t* row = D.rows + (size_t)jr * n_coeffs * 64;
        uint64_t col[19];
#pragma unroll
        for (int k = 0; k < 19; k++) col[k] = 0;
        uint32_t since = 0;
        uint4 n0 = zero, n1 = zero, n2 = zero, n3 = zero;     // the next step's symbol, read one step ahead of its products
        if (j < n_coeffs) {
            const uint4* q = reinterpret_cast<const uint4*>(row + (size_t)j * 64);
            n0 = q[0]; n1 = q[1]; n2 = q[2]; n3 = q[3];
        }
        for (uint32_t k = 0; k < steps; k++) {
            const uint32_t i = 8 * k + j;
            const uint4 s0 = n0, s1 = n1, s2 = n2, s3 = n3;
            n0 = zero; n1 = zero; n2 = zero; n3 = zero;
            if (i + 8 < n_coeffs) {
                const uint4* q = reinterpret_cast<const uint4*>(row + (size_t)(i + 8) * 64);
                n0 = q[0]; n1 = q[1]; n2 = q[2]; n3 = q[3];
            }
            const uint4* tp = rt_lds_tau + (size_t)i * RT_LAZY_ENTRY_U4;
#pragma unroll
            for (int h = 0; h < 2; h++) {                     // the lower half against tau^i, the upper against 2^256 tau^i
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
            if (++since == RT_LAZY_GROUP) { kzg_ripple29(col); since = 0; }
        }
        kzg_ripple29(col);
        const F30<Q> acc = kzg_columns_join<Q>(col);
        kzg_eval_finish<Q, true>(acc, live, j, (size_t)g, A.w, out, 64, D.prf + 16 * (size_t)jr);
    }
}

// The same for an SRS longer than KZG_LAZY_MAX_COEFFS: the Horner form of k_kzg_eval_rows30 with the symbol reduced to the plain stream
// on load (one product).  Bounds: the symbol is below 2^258, acc = acc tau^8 + symbol < r + 2^250 + 2^258 < 2^259 at every step, the
// lane sum of the eight products with tau^j below 2^258.
__global__ void __launch_bounds__(256)
k_rt_eval_horner(const RtDesc* __restrict__ desc, uint32_t n_rows_log, uint32_t total_rows, uint32_t n_coeffs, KzgEvalConsts K,
                 uint8_t* __restrict__ out) {
    using Q = IccBn254Fr;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;       // (eight lanes per row: 2^29 rows and more pass 32 bits)
    const uint32_t j = (uint32_t)t & 7u;
    const bool live = (t >> 3) < total_rows;
    const uint32_t g = live ? (uint32_t)(t >> 3) : total_rows - 1;      // idle lanes redo the last row (the lane sum is wave-wide)
    const RtDesc& D = desc[g >> n_rows_log];
    const uint32_t jr = g & ((1u << n_rows_log) - 1u);
    const uint8_t* row = D.rows + (size_t)jr * n_coeffs * 64;
    const F30<Q> T8 = f30_unpack<Q>(K.t8);
    F30<Q> acc;
#pragma unroll
    for (int l = 0; l < 9; l++) acc.v[l] = 0;
    for (uint32_t k = (n_coeffs + 7) / 8; k-- > 0;) {
        const uint32_t i = 8 * k + j;
        F30<Q> c;
#pragma unroll
        for (int l = 0; l < 9; l++) c.v[l] = 0;
        if (i < n_coeffs) c = rt_symbol_mod_q<Q>(row + (size_t)i * 64);
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
// cr_store_row: the client rebuild's reading of d_prf for the IPA build, r.d[0], r.d[1] as little-endian words).
template <class Q>
__global__ void __launch_bounds__(256)
k_rt_pack(const RtDesc* __restrict__ desc, uint32_t n_rows_log, uint32_t g0, uint32_t rows, uint32_t ncols, uint8_t* __restrict__ coeffs,
          uint8_t* __restrict__ scalars) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t symbols = (size_t)rows * ncols;
    const uint32_t mask = (1u << n_rows_log) - 1u;
    if (t < symbols) {
        const uint32_t gl = (uint32_t)(t / ncols), c = (uint32_t)(t - (size_t)gl * ncols), g = g0 + gl;
        const RtDesc& D = desc[g >> n_rows_log];
        const F30<Q> v = rt_symbol_mod_q<Q>(D.rows + 64 * ((size_t)(g & mask) * ncols + c));
        cr_store_row<Q>(coeffs + 32 * t, icc30_canonical<Q>(icc30_reduce_top<Q>(v)));
    } else if (t - symbols < rows) {
        const uint32_t gl = (uint32_t)(t - symbols), g = g0 + gl;
        const RtDesc& D = desc[g >> n_rows_log];
        cr_store_row<Q>(scalars + 32 * (size_t)gl, cr_prf<Q, true>(D.prf, g & mask));
    }
}

// ---- compare: a lane per row g0 + gl.  ADD (IPA): the expected MAC is first formed in place, exp[gl] = exp[gl] + hpts[gl], with the
// client batches' addition (k_cr_place / k_cu_place: xyzz30_add_mem with its equal, opposite and infinity cases) and their conversion
// to canonical affine bytes.  Then the row's 64 expected bytes against its d_macs bytes as 16-byte loads: a stored coordinate >= p
// differs from the canonical form and is not OK, infinity is 64 zero bytes on both sides.  The failures are counted per request.
template <class C, bool ADD>
__global__ void __launch_bounds__(64)
k_rt_compare(const RtDesc* __restrict__ desc, uint32_t n_rows_log, uint32_t g0, uint32_t rows, uint8_t* __restrict__ exp,
             const uint8_t* __restrict__ hpts) {
    using M = typename C::Fp;
    const size_t gl64 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gl64 >= rows) return;
    const uint32_t gl = (uint32_t)gl64, g = g0 + gl, jr = g & ((1u << n_rows_log) - 1u);
    const RtDesc& D = desc[g >> n_rows_log];
    uint8_t* mine = exp + 64 * (size_t)gl;
    if constexpr (ADD) {
        XYZZ<M> a = load_affine_be_lazy<M>(mine);
        const XYZZ<M> b = load_affine_be_lazy<M>(hpts + 64 * (size_t)gl);
        xyzz30_add_mem<M>(&a, &b, 0, 0, nullptr);
        store_affine_be<M>(mine, xyzz30_to_xyzz<M>(xyzz30_load_lazy<M>(&a)));
    }
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

}  // namespace porla
