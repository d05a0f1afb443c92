// Client::update's preprocessing for K independent writes in ONE asynchronous call (include/porla_gpu.h:
// porla_kzg_client_update_batch_device / porla_ipa_client_update_batch_device): the block's MAC, the complements of every slot below
// the level the write lands on, Client::HAdd -> HRebuildX / HRebuildY on them and the differences that go on the wire
// (porla/Client/Client.hpp:457-614, 921-1038).  Its outputs are what porla_*_update_batch_device takes as d_mac and d_complements; the
// pyramid of intermediate complements stays in the workspace.  Every step is on the caller's stream, and the launch sequence depends
// on Lmax = the highest level of the call, never on K:
//
//   upload                   one copy of the host-built work list (descriptors with wt, the pyramid's level pointers) from pinned memory
//   k_cu_expand              chunks -> the K big-endian coefficient rows of the block pass, PRF bytes -> the scalar rows of the h pass
//   block pass               KZG: k_kzg_eval_rows_lazy and the one-point table of G1[0] (the digest row of
//                            porla_kzg_digest_batch_device); IPA: alpha_generators_fb over the 128 coefficients of a row -> K points
//   h pass                   every PRF scalar of the call against the one-point table of the hiding base (128-bit scalars: the upper
//                            windows are zero digits) -> sum over requests of 2^(level+2) - 1 points
//   k_cu_scatter             the resident complements into the pyramid
//   k_cu_place               comp0 and wt * comp0 into level 0, MAC = block commitment + comp0
//   for i < Lmax:            k_update_mix_points_* with two families (X, Y) of the requests with level > i
//   k_cu_close               new complement - mixed complement, to affine
//
// Both passes leave affine bytes (k_fb_finish: the table's own conversion), which is what the mix bodies read.  Shared: the passes and
// the KZG precheck (client_block_pass.hip.h), wt, level plan, IPA bases (write_batch_host.hpp), a step's form (update_batch.hip.h).
#include "client_update_batch.hip.h"
#include "write_batch_host.hpp"
#include "../../include/porla_gpu.h"

#include <algorithm>
#include <cstddef>
#include <mutex>
#include <string>
#include <unordered_set>
#include <vector>

namespace porla {

struct ClientUpdateWs {
    std::mutex mu;
    int device = -1;
    Buf list, rows, scalars, blk, hpts, pyramid;
    PinnedList h_list;
    UseFence fence;
};
static PerDevice<ClientUpdateWs> g_cu_ws;

struct CuPlan {
    const CuDesc* d_desc;
    uint8_t* const* d_ptrs;
    uint32_t l1, k;
    hipStream_t stream;
};

// the mixes of steps 0 .. lmax - 1 under the MAC side's table lease
template <class C>
static int cu_launch_steps(const CuPlan& P, const std::vector<uint32_t>& active, uint32_t lmax, size_t n_total) {
    const uint32_t* tws = nullptr;
    int quad_log = 0, rc;
    if ((rc = mac_mix_tables_acquire(IccCurve<C>::id, n_total, P.stream, &tws, &quad_log))) return rc;
    for (uint32_t i = 0; i < lmax && !rc; i++) {
        const uint32_t a = active[i], tw_step = (uint32_t)(n_total >> i);
        ProfScope ps("client_update_mix", P.stream);
        update_mix_points_launch<C, 1, 0, CU_PARTS>(P.d_ptrs, P.l1, a, i, tws, tw_step, quad_log, P.stream);   // the two parts: 2^1 families from 0
        if (hipGetLastError() != hipSuccess) { set_last_error("porla: client update batch: a mix launch failed"); rc = PORLA_ERR_HIP; }
    }
    const int r1 = mac_mix_tables_release(P.stream);
    return rc ? rc : r1;
}

// ws->mu held, ws->fence entered.  fb_alpha == nullptr: the KZG build (the resident key, SRS and hiding base).
template <class C>
static int cu_enqueue(ClientUpdateWs* ws, FixedBase<C>* fb_alpha, FixedBase<C>* fb_h, const porla_client_update_req* reqs, size_t k,
                      size_t ncols, size_t n_total, hipStream_t stream) {
    int rc;
    const LevelPlan plan(k, [&](size_t a) { return reqs[a].level; });
    const uint32_t lmax = plan.lmax, l1 = lmax + 1;
    // ---- sizes: the h pass' rows, and the pyramid at 4 * 2^level points per part and request
    size_t n_prf = 0, pyr_pts = 0;
    for (size_t a = 0; a < k; a++) {
        n_prf += ((size_t)4 << reqs[a].level) - 1;
        pyr_pts += (size_t)CU_PARTS * ((size_t)4 << reqs[a].level);
    }
    size_t rows_b, scal_b, hpts_b, pyr_b, ptr_b, desc_b;
    if (n_prf > 0xfffffff0u || !mul_ok(k * ncols, 32, &rows_b) || !mul_ok(n_prf, 32, &scal_b) || !mul_ok(n_prf, 64, &hpts_b) ||
        !mul_ok(pyr_pts, 64, &pyr_b) || !mul_ok(k * CU_PARTS * l1, sizeof(void*), &ptr_b) || !mul_ok(k, sizeof(CuDesc), &desc_b)) {
        set_last_error("porla: client update batch: the call's complements do not fit a workspace");
        return PORLA_ERR_ARG;
    }
    const size_t list_b = desc_b + ptr_b;
    if ((rc = ws->h_list.stage(list_b))) return rc;
    if ((rc = ws->list.ensure(list_b))) return rc;
    if ((rc = ws->rows.ensure(rows_b))) return rc;
    if ((rc = ws->scalars.ensure(scal_b))) return rc;
    if ((rc = ws->blk.ensure(k * 64))) return rc;
    if ((rc = ws->hpts.ensure(hpts_b))) return rc;
    if ((rc = ws->pyramid.ensure(pyr_b))) return rc;
    // ---- the work list: descriptors | pyramid level pointers, one pinned buffer, one copy
    {
        CuDesc* hd = (CuDesc*)ws->h_list.h;
        void** hp = (void**)((uint8_t*)ws->h_list.h + desc_b);
        size_t prf0 = 0;
        uint8_t* pyr = (uint8_t*)ws->pyramid.p;
        for (size_t a = 0; a < k; a++) {
            const porla_client_update_req& R = reqs[plan.order[a]];
            CuDesc& D = hd[a];
            D.block = (const uint8_t*)R.d_block; D.prf = (const uint8_t*)R.d_prf;
            D.mac_out = (uint8_t*)R.d_mac_out; D.comp_out = (uint8_t*)R.d_complements_out;
            write_wt<C>(n_total, R.write_step, D.wt_sc);
            D.level = (uint32_t)R.level; D.prf0 = (uint32_t)prf0;
            prf0 += ((size_t)4 << R.level) - 1;
            const size_t part_b = (size_t)256 << R.level;      // 4 * 2^level points
            for (uint32_t part = 0; part < CU_PARTS; part++, pyr += part_b)
                for (uint32_t l = 0; l < l1; l++)
                    hp[(a * CU_PARTS + part) * l1 + l] = l <= (uint32_t)R.level ? pyr + (size_t)128 * (((size_t)1 << l) - 1) : nullptr;
        }
    }
    if ((rc = ws->h_list.send(ws->list.p, list_b, stream))) return rc;
    CuPlan P;
    P.d_desc = (const CuDesc*)ws->list.p;
    P.d_ptrs = (uint8_t* const*)((const uint8_t*)ws->list.p + desc_b);
    P.l1 = l1; P.k = (uint32_t)k; P.stream = stream;
    uint8_t* d_rows = (uint8_t*)ws->rows.p;
    uint8_t* d_scal = (uint8_t*)ws->scalars.p;
    uint8_t* d_blk = (uint8_t*)ws->blk.p;
    uint8_t* d_hpts = (uint8_t*)ws->hpts.p;
    // ---- 1. the rows of the two passes
    {
        ProfScope ps("client_update_expand", stream);
        const size_t items = ncols + ((size_t)4 << lmax) - 1;
        hipLaunchKernelGGL((k_cu_expand<IccCurve<C>::id == 1>), dim3((unsigned)((items + 255) / 256), (unsigned)k), dim3(256), 0, stream, P.d_desc,
                           (uint32_t)ncols, d_rows, d_scal);
        PORLA_HIP(hipGetLastError());
    }
    // ---- 2. the block pass and the h pass
    if ((rc = client_block_pass<C>(fb_alpha, d_rows, k, ncols, d_blk, stream))) return rc;
    if ((rc = client_h_pass<C>(fb_h, d_scal, n_prf, d_hpts, stream))) return rc;
    // ---- 3. level 0 of the pyramid and the MAC
    if (lmax) {
        ProfScope ps("client_update_scatter", stream);
        const size_t units = (((size_t)2 << lmax) - 2) * 4;
        const unsigned gx = (unsigned)std::min<size_t>((units + 255) / 256, 256);
        hipLaunchKernelGGL(k_cu_scatter, dim3(gx, (unsigned)k), dim3(256), 0, stream, P.d_desc, P.d_ptrs, l1, d_hpts);
        PORLA_HIP(hipGetLastError());
    }
    {
        static LdsOnce once;                           // dynamic LDS above 64 KiB: told once per device
        once.set({lds_kernel(&k_cu_place<C>, sizeof(MacOctLds<typename C::Fp>))});
        ProfScope ps("client_update_place", stream);
        hipLaunchKernelGGL((k_cu_place<C>), dim3((unsigned)((k + MACO_BF - 1) / MACO_BF)), dim3(8 * MACO_BF), sizeof(MacOctLds<typename C::Fp>),
                           stream, P.d_desc, P.d_ptrs, l1, (uint32_t)k, d_blk, d_hpts);
        PORLA_HIP(hipGetLastError());
    }
    // ---- 4. the rebuild steps
    if (lmax && (rc = cu_launch_steps<C>(P, plan.active, lmax, n_total))) return rc;
    // ---- 5. the close
    {
        ProfScope ps("client_update_close", stream);
        hipLaunchKernelGGL((k_cu_close<C>), dim3((unsigned)((((size_t)2 << lmax) + 63) / 64), (unsigned)k), dim3(64), 0, stream, P.d_desc,
                           P.d_ptrs, l1, d_hpts);
        PORLA_HIP(hipGetLastError());
    }
    return PORLA_OK;
}

// the checks both entry points make before the device is touched
static int cu_check(const char* who, const porla_client_update_req* reqs, size_t k, size_t n_total) {
    auto bad = [&](const std::string& what) { return bad_arg(who, what); };
    if (k && !reqs) return bad("reqs is NULL");
    if (int rc = check_n_total(who, n_total, 30)) return rc;
    if (int rc = check_request_count(who, k)) return rc;
    std::unordered_set<const void*> seen;
    for (size_t a = 0; a < k; a++) {
        const porla_client_update_req& R = reqs[a];
        const std::string at = "request " + std::to_string(a) + ": ";
        if (!R.d_block || !R.d_prf || !R.d_mac_out || !R.d_complements_out) return bad(at + "a NULL block, prf or output pointer");
        if ((((uintptr_t)R.d_block | (uintptr_t)R.d_prf | (uintptr_t)R.d_mac_out | (uintptr_t)R.d_complements_out) & 15u) != 0)
            return bad(at + "a block, prf or output pointer that is not 16-byte aligned");
        if (R.pad != 0) return bad(at + "pad must be 0");
        if (R.level < 0 || R.level > 29 || ((size_t)1 << R.level) > n_total / 2) return bad(at + "level must be 0 .. log2(n_total) - 1");
        if (R.write_step % n_total == 0) return bad(at + "write_step % n_total == 0 is CRebuild's step, not an H update");
        if (!seen.insert(R.d_mac_out).second || !seen.insert(R.d_complements_out).second)
            return bad(at + "an output pointer another request (or output) of this call names too");
    }
    return PORLA_OK;
}

}  // namespace porla

using namespace porla;

static_assert(sizeof(porla_client_update_req) == PORLA_CLIENT_UPDATE_REQ_BYTES, "porla_client_update_req size");
static_assert(offsetof(porla_client_update_req, d_block) == 0 && offsetof(porla_client_update_req, d_prf) == 8 &&
              offsetof(porla_client_update_req, d_mac_out) == 16 && offsetof(porla_client_update_req, d_complements_out) == 24 &&
              offsetof(porla_client_update_req, write_step) == 32 && offsetof(porla_client_update_req, level) == 40 &&
              offsetof(porla_client_update_req, pad) == 44,
              "porla_client_update_req offsets (include/porla_gpu.h)");

extern "C" int porla_kzg_client_update_batch_device(const porla_client_update_req* reqs, size_t k, size_t n_total, void* hip_stream) {
    int rc = cu_check("porla_kzg_client_update_batch_device", reqs, k, n_total);
    if (rc) return rc;
    if (k == 0) return PORLA_OK;
    if ((rc = ensure_device())) return rc;
    size_t n;
    if ((rc = client_kzg_row_width(&n))) return rc;
    ClientUpdateWs* ws = nullptr;
    if ((rc = g_cu_ws.get(&ws))) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    return FencedCall(ws, stream).run([&] { return cu_enqueue<Bn254G1>(ws, nullptr, nullptr, reqs, k, n, n_total, stream); });
}

extern "C" int porla_ipa_client_update_batch_device(porla_fixed_base* alpha_generators_fb, porla_fixed_base* h_fb,
                                                    const porla_client_update_req* reqs, size_t k, size_t n_total, void* hip_stream) {
    static const char* who = "porla_ipa_client_update_batch_device";
    int rc = cu_check(who, reqs, k, n_total);
    if (rc) return rc;
    if (k == 0) return PORLA_OK;
    if (!alpha_generators_fb || !h_fb) return bad_arg(who, "a NULL base");
    if ((rc = ensure_device())) return rc;
    if ((rc = ipa_check_generators(who, "alpha_generators_fb", alpha_generators_fb))) return rc;
    if ((rc = ipa_check_hiding_base(who, "h_fb", h_fb))) return rc;
    ClientUpdateWs* ws = nullptr;
    if ((rc = g_cu_ws.get(&ws))) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    return FencedCall(ws, stream).run([&] {
        return cu_enqueue<Secp256k1G>(ws, &alpha_generators_fb->secp, &h_fb->secp, reqs, k, IPA_COLS, n_total, stream);
    });
}
