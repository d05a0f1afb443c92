// Kernels of the server's rebuild write for K independent files, in both forms: CRebuild_Cached (server_rebuild_batch.hip:
// porla_server_rebuild_batch_device; porla/Server/Server.hpp:413-469, :1487-1833) and CRebuild_No_Cached (server_rebuild_aligned_batch.hip:
// porla_kzg_ / porla_ipa_server_rebuild_aligned_batch_device; Server.hpp:1835-2255).  The arithmetic is that of the single-file encodes,
// and so is its code: the data passes are icc30_split.hip.h's tile, planes and rounds (icc30_block_tile, icc30_plane) with a finish of
// their own, the stages of the MAC network are mac_fft.hip's own stage loop and kernels (mac_stages_leased) on ONE work array of
// K * n_total points (request r at r * n_total), the Y scaling is mac_fft.hip.h's bodies (macq_scale_quad, mac_scale_lane).  What is
// here is the addressing: a kernel that needs a request's pointers is indexed blockIdx.y = request and reads them from the uploaded
// descriptors.  The two forms differ in the finish of the last data pass and in the alignment the close stores: in the aligned form
// the last stage of each part ends in align_MAC (Server.hpp:531-541, :1977-1980, :2061-2064), so a top-level data row is stored
// mod p_icc, 32 bytes a symbol, and its alignment is the commitment of the row of scalars c = (A mod p_icc - A) mod q.
#pragma once
#include "icc.hip.h"
#include "icc30.hip.h"
#include "icc30_split.hip.h"
#include "mac_fft.hip.h"

namespace porla {

// One request as the kernels see it.  wt = w^reverse_bits(write_step % N, height - 1): the Montgomery residue pair the data side
// multiplies by, and the plain integer reduced mod the group order (little-endian words) the MAC side multiplies by.
struct SrDesc {
    const uint8_t* block;
    const uint8_t* mac;
    const uint8_t* comp;          // 2 * n_total points (X, then Y), or nullptr
    uint8_t* u_blocks;
    uint8_t* u_macs;
    uint8_t* data_x; uint8_t* data_y;
    uint8_t* mac_x; uint8_t* mac_y;
    uint8_t* align_x; uint8_t* align_y;
    uint32_t wt_p[8], wt_q[8], wt_sc[8];
    uint32_t row, pad;            // row = index - 1: the row of U the block lands on
};
static_assert(sizeof(SrDesc) == 192, "SrDesc: 88 bytes of pointers, 96 of wt, the row");

// ---- the store: U[index - 1] = block, MAC_U[index - 1] = mac (Server.hpp:413-427), 16 bytes per lane and turn
// (static: no template, and two translation units include this file)
static __global__ void __launch_bounds__(256)
k_sr_store(const SrDesc* __restrict__ desc, uint32_t ncols) {
    const SrDesc& D = desc[blockIdx.y];
    const size_t bu = (size_t)ncols * 2;                                   // 16-byte units of a block; the MAC is four more
    const uint4* sb = reinterpret_cast<const uint4*>(D.block);
    const uint4* sm = reinterpret_cast<const uint4*>(D.mac);
    uint4* ub = reinterpret_cast<uint4*>(D.u_blocks + (size_t)D.row * ncols * 32);
    uint4* um = reinterpret_cast<uint4*>(D.u_macs + (size_t)D.row * 64);
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t u = (size_t)blockIdx.x * blockDim.x + threadIdx.x; u < bu + 4; u += stride) {
        if (u < bu) ub[u] = sb[u];
        else um[u - bu] = sm[u - bu];
    }
}

// ---- one pass of the data network of request blockIdx.y (of the group `desc` starts at): k_icc_split30's tiles, planes and rounds
// (icc30_split.hip.h) on the request's own store.  FIRST reads the raw chunks of U (the X part's network: no init scaling).  FIN is
// how the pass ends.  SR_PASS (not the last): the two residue planes stay in the request's slice of `work` (plane_words words per
// plane).  The last pass writes both parts, X from the registers of the last round, Y_k = wt X_k mod LCM from one more product per
// plane (the XY form); per symbol the p_icc plane stores its canonical residue and the q plane -- the same lane -- reads it back:
//   SR_CACHED   into the first 32 bytes of the symbol's own 64-byte slot of data X / data Y, which the q plane then overwrites with
//               the value mod LCM;
//   SR_ALIGNED  into the symbol's 32-byte slot of the top-level row, and that is final; the q plane writes c into the request's rows
//               of `scalars`, 32 bytes big-endian, the order k_update_hadd hands the commitment pass: request a of the group owns
//               rows 2 a n .. 2 a n + n - 1 (X) and the n after (Y).
enum SrFinish { SR_PASS = 0, SR_CACHED = 1, SR_ALIGNED = 2 };
template <class Q, bool FIRST, int FIN>
__global__ void __launch_bounds__(ICC30_SPLIT_THREADS) __attribute__((amdgpu_waves_per_eu(FIN != SR_PASS ? 3 : 4, 4)))
k_sr_data(const SrDesc* __restrict__ desc, uint32_t* __restrict__ work, size_t plane_words, const uint32_t* __restrict__ twp,
          const uint32_t* __restrict__ twq, uint32_t n, uint32_t ncols, int s0, int ns, int cc_log, uint8_t* __restrict__ scalars) {
    __shared__ uint2 lds2[ICC_TILE_ELEMS * ICC30_PSLOT_WORDS / 2];
    uint32_t* lds = reinterpret_cast<uint32_t*>(lds2);
    constexpr bool LAST = FIN != SR_PASS;
    constexpr size_t SLOT = FIN == SR_ALIGNED ? 32 : 64;                   // bytes of a symbol in data X / data Y
    const SrDesc& D = desc[blockIdx.y];
    const uint8_t* raw = D.u_blocks;
    uint32_t* work_p = work + (size_t)blockIdx.y * 2 * plane_words;
    uint32_t* work_q = work_p + plane_words;
    const IccTile T = icc30_block_tile(n, ncols, s0, ns, cc_log, FIRST);
    const size_t part = (size_t)n * ncols * 32;                            // bytes of one part's rows of scalars
    uint8_t* const sc_x = FIN == SR_ALIGNED ? scalars + (size_t)blockIdx.y * 2 * part : nullptr;
    const IccOut ox{FIN == SR_CACHED ? D.data_x : nullptr, nullptr, sc_x, nullptr, 0};
    const IccOut oy{FIN == SR_CACHED ? D.data_y : nullptr, nullptr, FIN == SR_ALIGNED ? sc_x + part : nullptr, nullptr, 0};
    uint32_t slot[4];
    {
        F30<IccFp> rp[4];
        icc30_plane<IccFp, FIRST>(lds, T, raw, F30<IccFp>{}, work_p, twp, rp, slot);
        F30<IccFp> Ky = F30<IccFp>{};
        if (LAST) Ky = icc30_mul<IccFp>(f30_unpack<IccFp>(D.wt_p), f30_const<IccFp>(Icc30Const<IccFp>::C284));   // wt in the 2^270 form
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (slot[i] != 0xffffffffu) {
                const size_t gi = icc30_symbol_index(T, slot[i]);
                if (LAST) {
                    st_fe<IccFp>(reinterpret_cast<uint32_t*>(D.data_x + SLOT * gi), icc30_finish_p(rp[i]));
                    st_fe<IccFp>(reinterpret_cast<uint32_t*>(D.data_y + SLOT * gi), icc30_finish_p(icc30_mul<IccFp>(rp[i], Ky)));
                } else {
                    icc30_st_work<IccFp>(work_p + gi * ICC30_PLANE_WORDS, rp[i]);
                }
            }
        }
        __syncthreads();                                 // every lane has read its last round's symbols: the region is free
    }
    {
        F30<Q> rq[4];
        icc30_plane<Q, FIRST>(lds, T, raw, F30<Q>{}, work_q, twq, rq, slot);
        F30<Q> Ky = F30<Q>{};
        if (LAST) Ky = icc30_mul<Q>(f30_unpack<Q>(D.wt_q), f30_const<Q>(Icc30Const<Q>::C284));
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (slot[i] != 0xffffffffu) {
                const size_t gi = icc30_symbol_index(T, slot[i]);
                if (LAST) {                                                // P: what this lane stored after the p_icc plane
                    icc30_finish_q<Q>(ld_fe<IccFp>(reinterpret_cast<const uint32_t*>(D.data_x + SLOT * gi)), rq[i], gi, ox);
                    icc30_finish_q<Q>(ld_fe<IccFp>(reinterpret_cast<const uint32_t*>(D.data_y + SLOT * gi)), icc30_mul<Q>(rq[i], Ky), gi,
                                      oy);                                 // (wt X) mod q
                } else {
                    icc30_st_work<Q>(work_q + gi * ICC30_PLANE_WORDS, rq[i]);
                }
            }
        }
    }
}

// ---- MAC_U of request blockIdx.y -> its n points of the work array (the lazy memory form): a lane per point
template <class C>
__global__ void __launch_bounds__(64)
k_sr_mac_load(const SrDesc* __restrict__ desc, uint32_t n, XYZZ<typename C::Fp>* __restrict__ work) {
    using M = typename C::Fp;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    store_xyzz<M>(work + (size_t)blockIdx.y * n + i, load_affine_be_lazy<M>(desc[blockIdx.y].u_macs + (size_t)i * 64));
}

// ---- the Y part: work_y[i] = wt * work[i] for the n points of request blockIdx.y (Y_k = wt X_k, mac_fft.hip:mac_encode_core).  A
// block belongs to one request, so every wave multiplies by one scalar: the bodies of k_mac_load30_quad / k_mac_scale30 with wt from
// the request's descriptor
template <class C>
__global__ void __launch_bounds__(4 * MACQ_BF) MACQ_GUEST_ATTR
k_sr_mac_scale_quad(const SrDesc* __restrict__ desc, uint32_t n, const XYZZ<typename C::Fp>* __restrict__ work,
                    XYZZ<typename C::Fp>* __restrict__ work_y) {
    const size_t base = (size_t)blockIdx.y * n;
    uint32_t sc[8];
#pragma unroll
    for (int j = 0; j < 8; j++) sc[j] = desc[blockIdx.y].wt_sc[j];
    macq_scale_quad<C, true>(reinterpret_cast<const uint8_t*>(work + base), n, work_y + base, sc);
}
template <class C>
__global__ void __launch_bounds__(64)
k_sr_mac_scale_lane(const SrDesc* __restrict__ desc, uint32_t n, const XYZZ<typename C::Fp>* __restrict__ work,
                    XYZZ<typename C::Fp>* __restrict__ work_y) {
    const size_t base = (size_t)blockIdx.y * n;
    uint32_t k[8];
#pragma unroll
    for (int j = 0; j < 8; j++) k[j] = desc[blockIdx.y].wt_sc[j];
    mac_scale_lane<C>(work + base, n, work_y + base, k);
}

// ---- the close of request blockIdx.y (of the group): a lane per output point g < 2 n (X part, then Y).  The MAC network's result
// (work / work_y, projective) plus the request's complement (Server.hpp:449-469 with updated_level = height - 1) as one general
// addition, to affine with one inversion per lane -- the network's finish folded in; without complements the result alone -- into the
// resident half of MAC X / MAC Y.  The same place of the resident half of align X / align Y gets the alignment.  Cached: 64 zero
// bytes (infinity, Server.hpp:1527-1535).  ALIGNED: row 2 n blockIdx.y + g of the group's commitment pass (sums, projective, row r
// at sums[r S]) to affine with one inversion, big-endian; an infinite sum (a row of zero scalars) gives 64 zero bytes.  B starts at
// infinity (Server.hpp:1882-1890), so the commitment is the whole alignment.
template <class C, bool ALIGNED>
__global__ void __launch_bounds__(256)
k_sr_close(const SrDesc* __restrict__ desc, uint32_t n, const XYZZ<typename C::Fp>* __restrict__ work,
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
        uint8_t* const al = (y ? D.align_y : D.align_x) + 64 * j;
        if (ALIGNED) {
            store_affine_be<M>(al, load_xyzz<M>(sums + (2 * base + g) * S));
        } else {
            const uint4 zero = make_uint4(0, 0, 0, 0);
            uint4* al4 = reinterpret_cast<uint4*>(al);
            al4[0] = zero; al4[1] = zero; al4[2] = zero; al4[3] = zero;
        }
    }
}

}  // namespace porla
