// The client's rebuild write for K independent files in ONE asynchronous call (include/porla_gpu.h:
// porla_kzg_client_rebuild_batch_device / porla_ipa_client_rebuild_batch_device): the write on which the reference calls
// Client::CRebuild (porla/Client/Client.hpp:483-502, :1040-1453, the wire loop :584-614) -- the block's MAC, all n_total complements
// through the whole MAC-side network, X part and Y part, and the 2 n_total differences that go on the wire.  It is the step the client
// update batch refuses (write_step % n_total == 0), computed in the scalar domain (client_rebuild_batch.hip.h).  Every step is on the
// caller's stream, and the launch sequence depends on n_total, never on K:
//
//   upload                   one copy of the host-built descriptors (pointers, wt mod q) from pinned memory
//   k_cr_expand              chunks -> the K coefficient rows of the block pass; complements_U's PRF values -> the work arrays
//   block pass               client_block_pass.hip.h, shared with the client update batch -> K points
//   k_cr_network             stages 1 .. log2 min(n_total, T) on LDS tiles, under the MAC side's table lease
//   k_cr_network_stage       one launch per later stage
//   k_cr_close               (new - T) mod q and (new - wt T) mod q as the big-endian rows of the h pass
//   h pass                   K (2 n_total + 1) one-coefficient rows against the one-point table of the hiding base -> affine bytes
//   k_cr_place               the 2 n_total points to d_complements_out, MAC = block commitment + comp0
// (the two passes and the KZG build's precheck: client_block_pass.hip.h; wt and the IPA bases: write_batch_host.hpp)
#include "client_rebuild_batch.hip.h"
#include "write_batch_host.hpp"

#include <cstddef>
#include <mutex>
#include <string>
#include <unordered_set>

namespace porla {

struct ClientRebuildWs {
    std::mutex mu;
    int device = -1;
    Buf list, rows, work, scalars, blk, hpts;
    PinnedList h_list;
    UseFence fence;
};
static PerDevice<ClientRebuildWs> g_cr_ws;

// the network on the K work arrays under the MAC side's table lease
template <class Q>
static int cr_launch_network(int curve, uint32_t* d_work, size_t k, size_t n_total, hipStream_t stream) {
    const uint32_t* tws = nullptr;
    int quad_log = 0, rc;
    if ((rc = mac_mix_tables_acquire(curve, n_total, stream, &tws, &quad_log))) return rc;
    const uint32_t logn = (uint32_t)ilog2u(n_total), tile_log = logn < CR_TILE_LOG ? logn : CR_TILE_LOG;
    {
        ProfScope ps("client_rebuild_network", stream);
        hipLaunchKernelGGL((k_cr_network<Q>), dim3((unsigned)(n_total >> tile_log), (unsigned)k), dim3(CR_THREADS), 0, stream, d_work,
                           (uint32_t)n_total, tile_log, tws);
    }
    for (uint32_t s = tile_log + 1; s <= logn; s++) {
        ProfScope ps("client_rebuild_stage", stream);
        hipLaunchKernelGGL((k_cr_network_stage<Q>), dim3((unsigned)((n_total / 2 + CR_THREADS - 1) / CR_THREADS), (unsigned)k), dim3(CR_THREADS),
                           0, stream, d_work, (uint32_t)n_total, s, tws);
    }
    if (hipGetLastError() != hipSuccess) { set_last_error("porla: client rebuild batch: a network launch failed"); rc = PORLA_ERR_HIP; }
    const int r1 = mac_mix_tables_release(stream);
    return rc ? rc : r1;
}

// ws->mu held, ws->fence entered.  fb_alpha == nullptr: the KZG build (the resident key, SRS and hiding base).
template <class C>
static int cr_enqueue(ClientRebuildWs* ws, FixedBase<C>* fb_alpha, FixedBase<C>* fb_h, const porla_client_rebuild_req* reqs, size_t k,
                      size_t ncols, size_t n_total, hipStream_t stream) {
    using Q = typename IccCurve<C>::Q;
    constexpr bool LE_PRF = IccCurve<C>::id == 1;
    int rc;
    const uint32_t n = (uint32_t)n_total;
    size_t n_rows, rows_b, work_b, scal_b, hpts_b, blk_b, desc_b;
    if (!mul_ok(k, cr_rows(n), &n_rows) || n_rows > 0xfffffff0u || !mul_ok(k * ncols, 32, &rows_b) || !mul_ok(k * n_total, 32, &work_b) ||
        !mul_ok(n_rows, 32, &scal_b) || !mul_ok(n_rows, 64, &hpts_b) || !mul_ok(k, 64, &blk_b) || !mul_ok(k, sizeof(CrDesc), &desc_b)) {
        set_last_error("porla: client rebuild batch: the call's complements do not fit a workspace");
        return PORLA_ERR_ARG;
    }
    if ((rc = ws->h_list.stage(desc_b))) return rc;
    if ((rc = ws->list.ensure(desc_b))) return rc;
    if ((rc = ws->rows.ensure(rows_b))) return rc;
    if ((rc = ws->work.ensure(work_b))) return rc;
    if ((rc = ws->scalars.ensure(scal_b))) return rc;
    if ((rc = ws->blk.ensure(blk_b))) return rc;
    if ((rc = ws->hpts.ensure(hpts_b))) return rc;
    // ---- the descriptors, one pinned buffer, one copy
    {
        CrDesc* hd = (CrDesc*)ws->h_list.h;
        for (size_t a = 0; a < k; a++) {
            const porla_client_rebuild_req& R = reqs[a];
            CrDesc& D = hd[a];
            D.block = (const uint8_t*)R.d_block; D.prf = (const uint8_t*)R.d_prf;
            D.mac_out = (uint8_t*)R.d_mac_out; D.comp_out = (uint8_t*)R.d_complements_out;
            write_wt<C>(n_total, R.write_step, D.wt_sc);
        }
    }
    if ((rc = ws->h_list.send(ws->list.p, desc_b, stream))) return rc;
    const CrDesc* d_desc = (const CrDesc*)ws->list.p;
    uint8_t* d_rows = (uint8_t*)ws->rows.p;
    uint32_t* d_work = (uint32_t*)ws->work.p;
    uint8_t* d_scal = (uint8_t*)ws->scalars.p;
    uint8_t* d_blk = (uint8_t*)ws->blk.p;
    uint8_t* d_hpts = (uint8_t*)ws->hpts.p;
    // ---- 1. the rows of the block pass, the network's inputs, comp0's row
    {
        ProfScope ps("client_rebuild_expand", stream);
        const size_t items = ncols + n_total + 1;
        hipLaunchKernelGGL((k_cr_expand<Q, LE_PRF>), dim3((unsigned)((items + 255) / 256), (unsigned)k), dim3(256), 0, stream, d_desc,
                           (uint32_t)ncols, n, d_rows, d_work, d_scal);
        PORLA_HIP(hipGetLastError());
    }
    // ---- 2. the block pass
    if ((rc = client_block_pass<C>(fb_alpha, d_rows, k, ncols, d_blk, stream))) return rc;
    // ---- 3. the network in Z_q and the rows of the h pass
    if ((rc = cr_launch_network<Q>(IccCurve<C>::id, d_work, k, n_total, stream))) return rc;
    {
        ProfScope ps("client_rebuild_close", stream);
        hipLaunchKernelGGL((k_cr_close<Q, LE_PRF>), dim3((unsigned)((2 * n_total + 255) / 256), (unsigned)k), dim3(256), 0, stream, d_desc, n,
                           d_work, d_scal);
        PORLA_HIP(hipGetLastError());
    }
    // ---- 4. the h pass
    if ((rc = client_h_pass<C>(fb_h, d_scal, n_rows, d_hpts, stream))) return rc;
    // ---- 5. the outputs
    {
        ProfScope ps("client_rebuild_place", stream);
        const size_t units = 8 * n_total;
        const unsigned gx = (unsigned)std::min<size_t>((units + 255) / 256, 1024);
        hipLaunchKernelGGL((k_cr_place<C>), dim3(gx, (unsigned)k), dim3(256), 0, stream, d_desc, n, d_blk, d_hpts);
        PORLA_HIP(hipGetLastError());
    }
    return PORLA_OK;
}

// the checks both entry points make before the device is touched
static int cr_check(const char* who, const porla_client_rebuild_req* reqs, size_t k, size_t n_total) {
    auto bad = [&](const std::string& what) { return bad_arg(who, what); };
    if (k && !reqs) return bad("reqs is NULL");
    if (int rc = check_n_total(who, n_total, 30)) return rc;
    if (int rc = check_request_count(who, k)) return rc;
    std::unordered_set<const void*> seen;
    for (size_t a = 0; a < k; a++) {
        const porla_client_rebuild_req& R = reqs[a];
        const std::string at = "request " + std::to_string(a) + ": ";
        if (!R.d_block || !R.d_prf || !R.d_mac_out || !R.d_complements_out) return bad(at + "a NULL block, prf or output pointer");
        if ((((uintptr_t)R.d_block | (uintptr_t)R.d_prf | (uintptr_t)R.d_mac_out | (uintptr_t)R.d_complements_out) & 15u) != 0)
            return bad(at + "a block, prf or output pointer that is not 16-byte aligned");
        if (!seen.insert(R.d_mac_out).second || !seen.insert(R.d_complements_out).second)
            return bad(at + "an output pointer another request (or output) of this call names too");
    }
    return PORLA_OK;
}

}  // namespace porla

using namespace porla;

static_assert(sizeof(porla_client_rebuild_req) == PORLA_CLIENT_REBUILD_REQ_BYTES, "porla_client_rebuild_req size");
static_assert(offsetof(porla_client_rebuild_req, d_block) == 0 && offsetof(porla_client_rebuild_req, d_prf) == 8 &&
              offsetof(porla_client_rebuild_req, d_mac_out) == 16 && offsetof(porla_client_rebuild_req, d_complements_out) == 24 &&
              offsetof(porla_client_rebuild_req, write_step) == 32,
              "porla_client_rebuild_req offsets (include/porla_gpu.h)");

extern "C" int porla_kzg_client_rebuild_batch_device(const porla_client_rebuild_req* reqs, size_t k, size_t n_total, void* hip_stream) {
    int rc = cr_check("porla_kzg_client_rebuild_batch_device", reqs, k, n_total);
    if (rc) return rc;
    if (k == 0) return PORLA_OK;
    if ((rc = ensure_device())) return rc;
    size_t ncols;
    if ((rc = client_kzg_row_width(&ncols))) return rc;
    ClientRebuildWs* ws = nullptr;
    if ((rc = g_cr_ws.get(&ws))) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    return FencedCall(ws, stream).run([&] { return cr_enqueue<Bn254G1>(ws, nullptr, nullptr, reqs, k, ncols, n_total, stream); });
}

extern "C" int porla_ipa_client_rebuild_batch_device(porla_fixed_base* alpha_generators_fb, porla_fixed_base* h_fb,
                                                     const porla_client_rebuild_req* reqs, size_t k, size_t n_total, void* hip_stream) {
    static const char* who = "porla_ipa_client_rebuild_batch_device";
    int rc = cr_check(who, reqs, k, n_total);
    if (rc) return rc;
    if (k == 0) return PORLA_OK;
    if (!alpha_generators_fb || !h_fb) return bad_arg(who, "a NULL base");
    if ((rc = ensure_device())) return rc;
    if ((rc = ipa_check_generators(who, "alpha_generators_fb", alpha_generators_fb))) return rc;
    if ((rc = ipa_check_hiding_base(who, "h_fb", h_fb))) return rc;
    ClientRebuildWs* ws = nullptr;
    if ((rc = g_cr_ws.get(&ws))) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    return FencedCall(ws, stream).run([&] {
        return cr_enqueue<Secp256k1G>(ws, &alpha_generators_fb->secp, &h_fb->secp, reqs, k, IPA_COLS, n_total, stream);
    });
}
