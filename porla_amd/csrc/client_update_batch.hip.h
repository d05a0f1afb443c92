// Kernels of the batched client update (client_update_batch.hip: porla_kzg_client_update_batch_device /
// porla_ipa_client_update_batch_device): Client::update's preprocessing (porla/Client/Client.hpp:457-614) -- the block's MAC, the
// complements of every slot below the level the write lands on, Client::HAdd -> HRebuildX / HRebuildY on them (:978-1038, :921-976)
// and the differences "new complement - mixed complement" -- for K independent writes from one work list.  The butterflies are the
// server's (update_batch.hip.h: k_update_mix_points_*, here with two families per request: the complement parts X and Y); the
// complements live in a pyramid in the library's workspace, per request and part the levels 0 .. level laid out as the level stores of
// porla_icc_mac_hrebuild_host are (level i: 2^i resident points, then 2^i incoming ones), level i at byte 128 (2^i - 1).
#pragma once
#include "update_batch.hip.h"
#include "client_block_pass.hip.h"

namespace porla {

enum : uint32_t { CU_PART_X = 0, CU_PART_Y = 1, CU_PARTS = 2 };

// One request as the kernels see it.  prf0: the row of the request's first PRF value in the h pass (its 2^(level+2) - 1 rows follow
// each other in the order of porla_client_update_req.d_prf); wt_sc as UpdDesc's.
struct CuDesc {
    const uint8_t* block;
    const uint8_t* prf;
    uint8_t* mac_out;
    uint8_t* comp_out;
    uint32_t wt_sc[8];
    uint32_t level, prf0;
};
static_assert(sizeof(CuDesc) == 72, "CuDesc: 32 bytes of pointers, 32 of wt, level, prf0");

// pyramid level l of (request r, part) in the uploaded table: (Lmax + 1) slots per part
__device__ __forceinline__ uint8_t* cu_level(uint8_t* const* __restrict__ ptrs, uint32_t l1, uint32_t r, uint32_t part, uint32_t l) {
    return ptrs[((size_t)r * CU_PARTS + part) * l1 + l];
}
// the h-pass row of level i's resident complements (X part; the Y part 2^i rows further), and of the new ones, relative to prf0
__device__ __forceinline__ uint32_t cu_resident_row(uint32_t i) { return (2u << i) - 1u; }

// ---- expand: blockIdx.y = the request; a lane per chunk, then a lane per PRF value.  A chunk (32 bytes little-endian, any 256-bit
// value) becomes the big-endian coefficient of row r of the block pass; a PRF value (16 raw bytes) the big-endian scalar of its row of
// the h pass: LE_PRF false (KZG): a big-endian 128-bit integer, left-padded (compute_digest_complement); true (IPA): r.d[0], r.d[1] as
// little-endian 64-bit words (Client.hpp:435-436).  Both passes reduce mod the group order themselves.
template <bool LE_PRF>
__global__ void __launch_bounds__(256)
k_cu_expand(const CuDesc* __restrict__ desc, uint32_t ncols, uint8_t* __restrict__ rows, uint8_t* __restrict__ scalars) {
    const uint32_t q = blockIdx.y;
    const CuDesc& D = desc[q];
    const uint32_t nprf = (4u << D.level) - 1u;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < ncols) {
        cu_chunk_to_coeff(D.block, t, rows + 32 * ((size_t)q * ncols + t));
    } else if (t - ncols < nprf) {
        const uint32_t p = t - ncols;
        const uint4 v = reinterpret_cast<const uint4*>(D.prf)[p];
        uint4* d4 = reinterpret_cast<uint4*>(scalars + 32 * ((size_t)D.prf0 + p));
        d4[0] = make_uint4(0, 0, 0, 0);
        d4[1] = LE_PRF ? make_uint4(__builtin_bswap32(v.w), __builtin_bswap32(v.z), __builtin_bswap32(v.y), __builtin_bswap32(v.x)) : v;
    }
}

// ---- scatter: blockIdx.y = the request; the resident complements cH[i].X, cH[i].Y (i < level) from their rows of the h pass into the
// resident halves of the pyramid, 16 bytes per lane and turn
__global__ void __launch_bounds__(256)
k_cu_scatter(const CuDesc* __restrict__ desc, uint8_t* const* __restrict__ ptrs, uint32_t l1, const uint8_t* __restrict__ hpts) {
    const uint32_t q = blockIdx.y;
    const CuDesc& D = desc[q];
    const uint32_t units = ((2u << D.level) - 2u) * 4u;               // 2 (2^level - 1) points of four units
    const uint4* src = reinterpret_cast<const uint4*>(hpts + 64 * ((size_t)D.prf0 + 1));
    for (uint32_t u = blockIdx.x * blockDim.x + threadIdx.x; u < units; u += gridDim.x * blockDim.x) {
        const uint32_t pt = u >> 2;                                    // point pt of the request's resident complements
        const uint32_t i = 31u - (uint32_t)__clz(pt / 2u + 1u);      // level i holds points [2 (2^i - 1), 2 (2^(i+1) - 1))
        const uint32_t e = pt - ((2u << i) - 2u), part = e >> i, j = e & ((1u << i) - 1u);
        reinterpret_cast<uint4*>(cu_level(ptrs, l1, q, part, i) + 64 * (size_t)j)[u & 3u] = src[u];
    }
}

// ---- place: an octet per request, as k_update_place.  Y = wt * comp0 on the eight-lane ladder (maco_butterfly with um = infinity);
// beside it lane 4 adds comp0 to the block's commitment (row r of the block pass) for the MAC and lane 1 copies comp0 into the X part.
// The slot is row 0 of the pyramid's level 0 (level == 0) or row 1, the incoming half.
template <class C>
__global__ void __launch_bounds__(8 * MACO_BF) MACO_ATTR
k_cu_place(const CuDesc* __restrict__ desc, uint8_t* const* __restrict__ ptrs, uint32_t l1, uint32_t k, const uint8_t* __restrict__ blk,
           const uint8_t* __restrict__ hpts) {
    using M = typename C::Fp;
    MACO_LDS(L);
    const uint32_t o = threadIdx.x >> 3, half = (threadIdx.x >> 2) & 1u, r = threadIdx.x & 3u, lane = threadIdx.x & 63u;
    uint32_t q = blockIdx.x * MACO_BF + o;
    const bool valid = q < k;
    if (!valid) q = 0;                                                     // padding octets compute request 0 and store nothing
    const CuDesc& D = desc[q];
    const uint8_t* comp0 = hpts + 64 * (size_t)D.prf0;
    uint32_t sc[8];
#pragma unroll
    for (int j = 0; j < 8; j++) sc[j] = D.wt_sc[j];
    if (half) macq_store_point<M>(&L.um[o], F30<M>{}, true, r);
    else if (r == 0u) store_xyzz<M>(&L.qd[o].tbl[0], load_affine_be_lazy<M>(comp0));
    macq_sync();
    maco_butterfly<C>(L, o, half, r, lane, sc, &L.qd[o].tbl[1], &L.qd[o].tbl[2], true);
    macq_sync();
    if (!valid) return;
    const size_t slot = D.level ? 64 : 0;
    if (r == 0u) {
        if (half) {
            XYZZ<M> a = load_affine_be_lazy<M>(blk + 64 * (size_t)q);
            const XYZZ<M> b = load_affine_be_lazy<M>(comp0);
            xyzz30_add_mem<M>(&a, &b, 0, 0, nullptr);
            store_affine_be<M>(D.mac_out, xyzz30_to_xyzz<M>(xyzz30_load_lazy<M>(&a)));
        } else {
            store_affine_be<M>(cu_level(ptrs, l1, q, CU_PART_Y, 0) + slot, xyzz30_to_xyzz<M>(xyzz30_load_lazy<M>(&L.qd[o].tbl[1])));
        }
    } else if (r == 1u && !half) {
        uint4* d = reinterpret_cast<uint4*>(cu_level(ptrs, l1, q, CU_PART_X, 0) + slot);
        const uint4* s = reinterpret_cast<const uint4*>(comp0);
#pragma unroll
        for (int j = 0; j < 4; j++) d[j] = s[j];
    }
}

// ---- close: blockIdx.y = the request, a lane per output point: out[j] = new_X[j] - T_X[j], out[2^level + j] = new_Y[j] - T_Y[j], T
// the level-`level` result of the rebuild (its incoming half; at level 0 the row place wrote), as one general addition and one
// inversion per lane (infinity = 64 zero bytes).
template <class C>
__global__ void __launch_bounds__(64)
k_cu_close(const CuDesc* __restrict__ desc, uint8_t* const* __restrict__ ptrs, uint32_t l1, const uint8_t* __restrict__ hpts) {
    using M = typename C::Fp;
    const uint32_t q = blockIdx.y;
    const CuDesc& D = desc[q];
    const uint32_t lv = D.level, top = 1u << lv;
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= 2u * top) return;
    const uint32_t part = g < top ? CU_PART_X : CU_PART_Y, j = g & (top - 1u);
    const uint8_t* t = cu_level(ptrs, l1, q, part, lv) + 64 * (size_t)(lv ? top + j : j);
    XYZZ<M> a = load_affine_be_lazy<M>(hpts + 64 * ((size_t)D.prf0 + cu_resident_row(lv) + g));
    const XYZZ<M> b = load_affine_be_lazy<M>(t);
    xyzz30_add_mem<M>(&a, &b, 1, 0, nullptr);
    store_affine_be<M>(D.comp_out + 64 * (size_t)g, xyzz30_to_xyzz<M>(xyzz30_load_lazy<M>(&a)));
}

}  // namespace porla
