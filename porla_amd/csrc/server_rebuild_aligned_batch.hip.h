// Kernels of the server's rebuild write in the CRebuild_No_Cached form (server_rebuild_aligned_batch.hip:
// porla_kzg_server_rebuild_aligned_batch_device / porla_ipa_server_rebuild_aligned_batch_device; porla/Server/Server.hpp:1835-2255): the
// last stage of each part ends in align_MAC (:531-541, :1977-1980, :2061-2064), so a top-level data row is stored mod p_icc, 32 bytes a
// symbol, and its alignment is the commitment of the row of scalars c = (A mod p_icc - A) mod q.  Two kernels differ from the cached
// form's (server_rebuild_batch.hip.h, whose descriptors, store, MAC load, stages and scaling serve here unchanged): the last pass of the
// data network and the close.
#pragma once
#include "server_rebuild_batch.hip.h"

namespace porla {

// ---- the last pass of the data network of request blockIdx.y (of the group `desc` starts at): k_sr_data's tiles, planes and rounds,
// ending in the aligned finish.  Per symbol the p_icc plane's canonical residue goes straight into the symbol's 32-byte slot of the
// top-level row -- X from the registers of the last round, Y from one more product by wt -- and that slot is final: nothing is parked.
// The q plane reads it back (the same lane wrote it) and writes c into the request's rows of `scalars`, 32 bytes big-endian, the
// order k_update_hadd hands the commitment pass: request a of the group owns rows 2 a n .. 2 a n + n - 1 (X) and the n after (Y).
template <class Q, bool FIRST>
__global__ void __launch_bounds__(ICC30_SPLIT_THREADS) __attribute__((amdgpu_waves_per_eu(3, 4)))
k_sr_data_aligned(const SrDesc* __restrict__ desc, uint32_t* __restrict__ work, size_t plane_words, const uint32_t* __restrict__ twp,
                  const uint32_t* __restrict__ twq, uint32_t n, uint32_t ncols, int s0, int ns, int cc_log, uint8_t* __restrict__ scalars) {
    __shared__ uint2 lds2[ICC_TILE_ELEMS * ICC30_PSLOT_WORDS / 2];
    uint32_t* lds = reinterpret_cast<uint32_t*>(lds2);
    const SrDesc& D = desc[blockIdx.y];
    const uint8_t* raw = D.u_blocks;
    uint32_t* work_p = work + (size_t)blockIdx.y * 2 * plane_words;
    uint32_t* work_q = work_p + plane_words;
    IccTile T;
    T.n = n; T.ncols = ncols; T.s0 = s0; T.ns = ns; T.cc_log = (uint32_t)cc_log;
    T.elems = (1u << ns) << cc_log;
    T.raw = FIRST;
    T.lo_bits = (uint32_t)(s0 - 1);
    const uint32_t Cc = 1u << cc_log;
    const uint32_t col_tiles = (ncols + Cc - 1) >> cc_log;
    uint32_t tile = blockIdx.x;                                            // (an XCD owns a contiguous range of tiles, as k_icc_split30)
    if ((gridDim.x & 7u) == 0) tile = (blockIdx.x & 7u) * (gridDim.x >> 3) + (blockIdx.x >> 3);
    const uint32_t ct = tile % col_tiles;
    tile /= col_tiles;
    T.lo = tile & ((1u << T.lo_bits) - 1u);
    const uint32_t hi = tile >> T.lo_bits;
    T.row_base = (hi << (T.lo_bits + ns)) + T.lo;
    T.c0 = ct << cc_log;
    uint8_t* const ax = D.data_x;
    uint8_t* const ay = D.data_y;
    const size_t part = (size_t)n * ncols * 32;                            // bytes of one part's rows of scalars
    const IccOut ox{nullptr, nullptr, scalars + (size_t)blockIdx.y * 2 * part, nullptr, 0};
    const IccOut oy{nullptr, nullptr, ox.sc + part, nullptr, 0};
    uint32_t slot[4];
    {
        F30<IccFp> rp[4];
        icc30_plane<IccFp, FIRST>(lds, T, raw, F30<IccFp>{}, work_p, twp, rp, slot);
        Fe<IccFp> w;
#pragma unroll
        for (int j = 0; j < 8; j++) w.v[j] = D.wt_p[j];
        const F30<IccFp> Ky = icc30_mul<IccFp>(f30_unpack<IccFp>(w.v), f30_const<IccFp>(Icc30Const<IccFp>::C284));   // wt in the 2^270 form
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (slot[i] != 0xffffffffu) {
                const uint32_t mid = slot[i] >> cc_log, col = slot[i] & (Cc - 1);
                const size_t gi = (size_t)(T.row_base + (mid << T.lo_bits)) * ncols + T.c0 + col;
                st_fe<IccFp>(reinterpret_cast<uint32_t*>(ax + 32 * gi), icc30_finish_p(rp[i]));
                st_fe<IccFp>(reinterpret_cast<uint32_t*>(ay + 32 * gi), icc30_finish_p(icc30_mul<IccFp>(rp[i], Ky)));
            }
        }
        __syncthreads();                                 // every lane has read its last round's symbols: the region is free
    }
    {
        F30<Q> rq[4];
        icc30_plane<Q, FIRST>(lds, T, raw, F30<Q>{}, work_q, twq, rq, slot);
        Fe<Q> w;
#pragma unroll
        for (int j = 0; j < 8; j++) w.v[j] = D.wt_q[j];
        const F30<Q> Ky = icc30_mul<Q>(f30_unpack<Q>(w.v), f30_const<Q>(Icc30Const<Q>::C284));
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (slot[i] != 0xffffffffu) {
                const uint32_t mid = slot[i] >> cc_log, col = slot[i] & (Cc - 1);
                const size_t gi = (size_t)(T.row_base + (mid << T.lo_bits)) * ncols + T.c0 + col;
                icc30_finish_q<Q>(ld_fe<IccFp>(reinterpret_cast<const uint32_t*>(ax + 32 * gi)), rq[i], gi, ox);
                icc30_finish_q<Q>(ld_fe<IccFp>(reinterpret_cast<const uint32_t*>(ay + 32 * gi)), icc30_mul<Q>(rq[i], Ky), gi, oy);   // (wt X) mod q
            }
        }
    }
}

// ---- the close of request blockIdx.y (of the group): a lane per output point g < 2 n (X part, then Y).  k_sr_close's MAC part -- the
// network's result plus the complement, to affine -- and, where that kernel writes zeros, the alignment: row 2 n blockIdx.y + g of the
// group's commitment pass (sums, projective, row r at sums[r S]) to affine with one inversion, big-endian; an infinite sum (a row of
// zero scalars) gives 64 zero bytes.  B starts at infinity (Server.hpp:1882-1890), so the commitment is the whole alignment.
template <class C>
__global__ void __launch_bounds__(256)
k_sr_close_aligned(const SrDesc* __restrict__ desc, uint32_t n, const XYZZ<typename C::Fp>* __restrict__ work,
                   const XYZZ<typename C::Fp>* __restrict__ work_y, const XYZZ<typename C::Fp>* __restrict__ sums, uint32_t S) {
    using M = typename C::Fp;
    const SrDesc& D = desc[blockIdx.y];
    const size_t base = (size_t)blockIdx.y * n;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < 2 * (size_t)n; g += stride) {
        const bool y = g >= n;
        const size_t j = y ? g - n : g;
        XYZZ<M> a = load_xyzz<M>((y ? work_y : work) + base + j);
        if (D.comp) {
            const XYZZ<M> b = load_affine_be_lazy<M>(D.comp + 64 * g);
            xyzz30_add_mem<M>(&a, &b, 0, 0, nullptr);
        }
        store_affine_be<M>((y ? D.mac_y : D.mac_x) + 64 * j, xyzz30_to_xyzz<M>(xyzz30_load_lazy<M>(&a)));
        store_affine_be<M>((y ? D.align_y : D.align_x) + 64 * j, load_xyzz<M>(sums + (2 * base + g) * S));
    }
}

}  // namespace porla
