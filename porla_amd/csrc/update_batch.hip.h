// Kernels of the batched server update (update_batch.hip: porla_kzg_update_batch_device / porla_ipa_update_batch_device): Server::update's
// H path -- HAdd, HRebuildX / HRebuildY, the complement adds (porla/Server/Server.hpp:401-476, 1329-1477) -- for K independent files,
// every step of every file from one work list.  The arithmetic is that of the single-write kernels (icc.hip.h: k_icc_load / k_icc_finish,
// icc30.hip.h: k_icc_mix30, mac_fft.hip.h: k_mac_mix_oct / _quad / k_mac_mix), whose device functions these kernels call; what is new is
// the addressing: a lane, quad or octet finds its request, family and row from its global index, because every item of a step has the
// same size (2^i rows) and the requests are sorted by level, highest first, so that the requests a step still concerns are a prefix.
#pragma once
#include "icc.hip.h"
#include "icc30.hip.h"
#include "mac_fft.hip.h"

namespace porla {

// the six level families of a file, in the order of the request's pointer arrays
enum : uint32_t { UPD_DATA_X = 0, UPD_DATA_Y = 1, UPD_MAC_X = 2, UPD_MAC_Y = 3, UPD_ALIGN_X = 4, UPD_ALIGN_Y = 5, UPD_FAMILIES = 6 };

// One request as the kernels see it.  wt = w^reverse_bits(write_step % N, height - 1): the Montgomery residue pair the data side
// multiplies by, and the plain integer reduced mod the group order (little-endian words) the MAC side multiplies by.
struct UpdDesc {
    const uint8_t* block;
    const uint8_t* mac;
    const uint8_t* comp;      // 2 * 2^level points (X, then Y), or nullptr
    uint32_t wt_p[8], wt_q[8], wt_sc[8];
    uint32_t level, pad;
};
static_assert(sizeof(UpdDesc) == 128, "UpdDesc: 24 bytes of pointers, 96 of wt, level");

// level pointer of (request r, family f, level l) in the uploaded table: (Lmax + 1) slots per family
__device__ __forceinline__ uint8_t* upd_level(uint8_t* const* __restrict__ ptrs, uint32_t l1, uint32_t r, uint32_t f, uint32_t l) {
    return ptrs[((size_t)r * UPD_FAMILIES + f) * l1 + l];
}

// ---- HAdd, data side: a lane per (request, column).  X row = the raw chunk, Y row = (chunk * wt) mod p_icc, both zero-extended to 64
// bytes, at row 0 of level 0 (level == 0: the level was empty) or row 1 (the incoming half); c = (Y - chunk * wt) mod q, big-endian, to
// the request's scalar row.
template <class Q>
__global__ void __launch_bounds__(256)
k_update_hadd(const UpdDesc* __restrict__ desc, uint8_t* const* __restrict__ ptrs, uint32_t l1, uint32_t k, uint32_t ncols,
              uint8_t* __restrict__ scalars) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)k * ncols) return;
    const uint32_t r = (uint32_t)(t / ncols), c = (uint32_t)(t - (size_t)r * ncols);
    const UpdDesc& D = desc[r];
    IccElem<Q> wt;
#pragma unroll
    for (int j = 0; j < 8; j++) { wt.p.v[j] = D.wt_p[j]; wt.q.v[j] = D.wt_q[j]; }
    const size_t slot = ((size_t)(D.level ? 1u : 0u) * ncols + c) * 64;
    uint4* dx = reinterpret_cast<uint4*>(upd_level(ptrs, l1, r, UPD_DATA_X, 0) + slot);
    uint8_t* dy = upd_level(ptrs, l1, r, UPD_DATA_Y, 0) + slot;
    const uint8_t* src = D.block + 32 * (size_t)c;
    const uint4 zero = make_uint4(0, 0, 0, 0);
    const uint4* s4 = reinterpret_cast<const uint4*>(src);
    const uint4 lo = s4[0], hi = s4[1];
    dx[0] = lo; dx[1] = hi; dx[2] = zero; dx[3] = zero;
    IccOut o;
    o.x = nullptr; o.al = dy; o.sc = scalars + 32 * t; o.qres = nullptr; o.scalar_le = 0;
    icc_finish_elem<Q>(icc_load_elem<Q>(src, wt, 1), 0, o);
    reinterpret_cast<uint4*>(dy)[2] = zero;
    reinterpret_cast<uint4*>(dy)[3] = zero;
}

// ---- HAdd, the four point slots: an octet per request.  MAC Y = wt * MAC on the eight-lane ladder (maco_butterfly with um = infinity:
// its lower output is 0 + wt * MAC); beside it lane 4 takes the request's commitment sum (row r of the commitment pass, projective)
// to affine for align Y, lane 1 copies MAC into MAC X and lane 5 writes infinity into align X.
template <class C>
__global__ void __launch_bounds__(8 * MACO_BF) MACO_ATTR
k_update_place(const UpdDesc* __restrict__ desc, uint8_t* const* __restrict__ ptrs, uint32_t l1, uint32_t k,
               const XYZZ<typename C::Fp>* __restrict__ sums, uint32_t S) {
    using M = typename C::Fp;
    MACO_LDS(L);
    const uint32_t o = threadIdx.x >> 3, half = (threadIdx.x >> 2) & 1u, r = threadIdx.x & 3u, lane = threadIdx.x & 63u;
    uint32_t q = blockIdx.x * MACO_BF + o;
    const bool valid = q < k;
    if (!valid) q = 0;                                                     // padding octets compute request 0 and store nothing
    const UpdDesc& D = desc[q];
    uint32_t sc[8];
#pragma unroll
    for (int j = 0; j < 8; j++) sc[j] = D.wt_sc[j];
    if (half) macq_store_point<M>(&L.um[o], F30<M>{}, true, r);
    else if (r == 0u) store_xyzz<M>(&L.qd[o].tbl[0], load_affine_be_lazy<M>(D.mac));
    macq_sync();
    maco_butterfly<C>(L, o, half, r, lane, sc, &L.qd[o].tbl[1], &L.qd[o].tbl[2], true);
    macq_sync();
    if (!valid) return;
    const size_t slot = D.level ? 64 : 0;
    const uint4 zero = make_uint4(0, 0, 0, 0);
    if (r == 0u) {
        if (half) store_affine_be<M>(upd_level(ptrs, l1, q, UPD_ALIGN_Y, 0) + slot, load_xyzz<M>(sums + (size_t)q * S));
        else store_affine_be<M>(upd_level(ptrs, l1, q, UPD_MAC_Y, 0) + slot, xyzz30_to_xyzz<M>(xyzz30_load_lazy<M>(&L.qd[o].tbl[1])));
    } else if (r == 1u) {
        uint4* d = reinterpret_cast<uint4*>(upd_level(ptrs, l1, q, half ? UPD_ALIGN_X : UPD_MAC_X, 0) + slot);
        const uint4* s = reinterpret_cast<const uint4*>(D.mac);
#pragma unroll
        for (int j = 0; j < 4; j++) d[j] = half ? zero : s[j];
    }
}

// ---- step i of HRebuildX / HRebuildY, data rows: the halves of level i into the incoming half of level i + 1, for the parts X and Y of
// the first `active` requests (those with level > i).  A lane per (request, part, row, column): icc30_mix_elem, the body of k_icc_mix30.
template <class Q>
__global__ void __launch_bounds__(256)
k_update_mix_data(uint8_t* const* __restrict__ ptrs, uint32_t l1, uint32_t active, uint32_t i, uint32_t ncols, const uint32_t* __restrict__ tw30,
                  uint32_t tw_step) {
    const uint32_t len = 1u << i;
    const size_t per = (size_t)len * ncols;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= per * 2 * active) return;
    const uint32_t item = (uint32_t)(t / per);
    const size_t e = t - (size_t)item * per;
    const uint8_t* a0 = upd_level(ptrs, l1, item >> 1, item & 1u, i);
    uint8_t* out = upd_level(ptrs, l1, item >> 1, item & 1u, i + 1) + 2 * per * 64;
    icc30_mix_elem<Q>(a0, a0 + per * 64, e, len, ncols, tw30, tw_step, out);
}

// ---- step i, the point families of the first `active` requests: butterfly g of the step belongs to item g >> i = (request, family)
// and is row g & (2^i - 1) of it.  _oct / _quad / _lane: 8 / 4 / 1 lanes per butterfly, picked by update_mix_points_launch below.  A request's point families are
// 2^LOGF consecutive ones from FIRST on, of STRIDE families per request in the pointer table: the server's four (MAC X, MAC Y,
// align X, align Y) of its six by default; the client update batch (client_update_batch.hip.h) mixes its two complement parts.
template <class C, uint32_t LOGF, uint32_t FIRST, uint32_t STRIDE>
__device__ __forceinline__ void upd_point_item(uint8_t* const* __restrict__ ptrs, uint32_t l1, uint32_t i, uint32_t g, const uint8_t*& a0,
                                               uint8_t*& out, uint32_t& row) {
    const uint32_t item = g >> i;
    row = g & ((1u << i) - 1u);
    uint8_t* const* lv = ptrs + ((size_t)(item >> LOGF) * STRIDE + FIRST + (item & ((1u << LOGF) - 1u))) * l1 + i;
    a0 = lv[0];
    out = lv[1] + ((size_t)128 << i);
}
template <class C, uint32_t LOGF = 2, uint32_t FIRST = UPD_MAC_X, uint32_t STRIDE = UPD_FAMILIES>
__global__ void __launch_bounds__(8 * MACO_BF) MACO_ATTR
k_update_mix_points_oct(uint8_t* const* __restrict__ ptrs, uint32_t l1, uint32_t active, uint32_t i, const uint32_t* __restrict__ tws,
                        uint32_t tw_step) {
    using M = typename C::Fp;
    MACO_LDS(L);
    uint32_t g = blockIdx.x * MACO_BF + (threadIdx.x >> 3);
    const bool valid = g < ((active << LOGF) << i);
    if (!valid) g = 0;
    const uint8_t* a0; uint8_t* out; uint32_t row;
    upd_point_item<C, LOGF, FIRST, STRIDE>(ptrs, l1, i, g, a0, out, row);
    maco_mix_one<C>(L, a0, a0 + ((size_t)64 << i), row, 1u << i, valid, tws, tw_step, out);
}
template <class C, uint32_t LOGF = 2, uint32_t FIRST = UPD_MAC_X, uint32_t STRIDE = UPD_FAMILIES>
__global__ void __launch_bounds__(4 * MACQ_BF) MACQ_GUEST_ATTR
k_update_mix_points_quad(uint8_t* const* __restrict__ ptrs, uint32_t l1, uint32_t active, uint32_t i, const uint32_t* __restrict__ tws,
                         uint32_t tw_step) {
    using M = typename C::Fp;
    MACQ_LDS(L);
    uint32_t g = blockIdx.x * MACQ_BF + (threadIdx.x >> 2);
    const bool valid = g < ((active << LOGF) << i);
    if (!valid) g = 0;
    const uint8_t* a0; uint8_t* out; uint32_t row;
    upd_point_item<C, LOGF, FIRST, STRIDE>(ptrs, l1, i, g, a0, out, row);
    macq_mix_one<C>(L, a0, a0 + ((size_t)64 << i), row, 1u << i, valid, tws, tw_step, out);
}
template <class C, uint32_t LOGF = 2, uint32_t FIRST = UPD_MAC_X, uint32_t STRIDE = UPD_FAMILIES>
__global__ void __launch_bounds__(64)
k_update_mix_points_lane(uint8_t* const* __restrict__ ptrs, uint32_t l1, uint32_t active, uint32_t i, const uint32_t* __restrict__ tws,
                         uint32_t tw_step) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= ((active << LOGF) << i)) return;
    const uint8_t* a0; uint8_t* out; uint32_t row;
    upd_point_item<C, LOGF, FIRST, STRIDE>(ptrs, l1, i, g, a0, out, row);
    mac_mix_one<C>(a0, a0 + ((size_t)64 << i), row, 1u << i, tws, tw_step, out);
}
// host: step i's launch in the form mac_mix_form gives for its butterfly count (tws, quad_log: mac_mix_tables_acquire's, the lease
// held).  Dynamic LDS above 64 KiB is told here, once per device and instantiation (LdsOnce): what is told is what is launched.
template <class C, uint32_t LOGF = 2, uint32_t FIRST = UPD_MAC_X, uint32_t STRIDE = UPD_FAMILIES>
static void update_mix_points_launch(uint8_t* const* d_ptrs, uint32_t l1, uint32_t active, uint32_t i, const uint32_t* tws, uint32_t tw_step,
                                     int quad_log, hipStream_t stream) {
    using M = typename C::Fp;
    const size_t bf = ((size_t)active << LOGF) << i;
    const int form = mac_mix_form(bf, quad_log);       // (the step's butterflies: 2^LOGF families of 2^i rows per request)
    if (form == 8) {
        static LdsOnce once;
        once.set({lds_kernel(&k_update_mix_points_oct<C, LOGF, FIRST, STRIDE>, sizeof(MacOctLds<M>))});
        hipLaunchKernelGGL((k_update_mix_points_oct<C, LOGF, FIRST, STRIDE>), dim3((unsigned)((bf + MACO_BF - 1) / MACO_BF)), dim3(8 * MACO_BF),
                           sizeof(MacOctLds<M>), stream, d_ptrs, l1, active, i, tws, tw_step);
    } else if (form == 4) {
        static LdsOnce once;
        once.set({lds_kernel(&k_update_mix_points_quad<C, LOGF, FIRST, STRIDE>, sizeof(MacQuadLds<M>))});
        hipLaunchKernelGGL((k_update_mix_points_quad<C, LOGF, FIRST, STRIDE>), dim3((unsigned)((bf + MACQ_BF - 1) / MACQ_BF)), dim3(4 * MACQ_BF),
                           sizeof(MacQuadLds<M>), stream, d_ptrs, l1, active, i, tws, tw_step);
    } else
        hipLaunchKernelGGL((k_update_mix_points_lane<C, LOGF, FIRST, STRIDE>), dim3((unsigned)((bf + 63) / 64)), dim3(64), 0, stream, d_ptrs, l1,
                           active, i, tws, tw_step);
}

// ---- the close: blockIdx.y = the request.  The incoming half of level `level` over its resident half in all six families
// (HRebuildX / HRebuildY's last loops; nothing to copy at level 0, where HAdd wrote the resident row), and the complements onto the
// RESIDENT half of MAC X and MAC Y (Server.hpp:449-469): a lane per point, resident[j] = incoming[j] + comp[j] as one general addition
// and one inversion.  The incoming half keeps the value without complements.
template <class C>
__global__ void __launch_bounds__(256)
k_update_close(const UpdDesc* __restrict__ desc, uint8_t* const* __restrict__ ptrs, uint32_t l1, uint32_t ncols) {
    using M = typename C::Fp;
    const uint32_t q = blockIdx.y;
    const UpdDesc& D = desc[q];
    const uint32_t lv = D.level;
    const size_t top = (size_t)1 << lv;
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    if (D.comp) {
        for (size_t g = tid; g < 2 * top; g += stride) {
            const uint32_t f = g < top ? UPD_MAC_X : UPD_MAC_Y;
            const size_t j = g < top ? g : g - top;
            uint8_t* res = upd_level(ptrs, l1, q, f, lv) + 64 * j;
            XYZZ<M> a = load_affine_be_lazy<M>(lv ? res + 64 * top : res);
            const XYZZ<M> b = load_affine_be_lazy<M>(D.comp + 64 * g);
            xyzz30_add_mem<M>(&a, &b, 0, 0, nullptr);
            store_affine_be<M>(res, xyzz30_to_xyzz<M>(xyzz30_load_lazy<M>(&a)));
        }
    }
    if (lv == 0) return;
    // the copies, 16 bytes per lane and turn: data X, data Y (top * ncols * 4 units each), align X, align Y (top * 4 each) and,
    // without complements, MAC X and MAC Y
    const size_t du = top * ncols * 4, pu = top * 4;
    const uint32_t nfam = D.comp ? 4u : 6u;
#pragma unroll 1
    for (uint32_t n = 0; n < nfam; n++) {
        const size_t units = n < 2 ? du : pu;
        const uint32_t f = n < 2 ? n : (n < 4 ? n + 2 : n - 2);           // data X, data Y, align X, align Y, MAC X, MAC Y
        uint4* res = reinterpret_cast<uint4*>(upd_level(ptrs, l1, q, f, lv));
        const uint4* inc = res + units;
        for (size_t u = tid; u < units; u += stride) res[u] = inc[u];
    }
}

}  // namespace porla
