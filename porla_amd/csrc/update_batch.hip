// Server::update's H path for K independent files in ONE asynchronous call (include/porla_gpu.h: porla_kzg_update_batch_device /
// porla_ipa_update_batch_device): HAdd, HRebuildX / HRebuildY and the complement adds (porla/Server/Server.hpp:401-476, 1329-1477) on
// level stores that stay in HBM.  The host wrappers (porla_icc_hadd_host, porla_icc_hrebuild_host, porla_icc_mac_hrebuild_host) carry one
// block through host buffers and wait; here every step of every request is on the device and on the caller's stream, and the launch
// sequence depends on Lmax = the highest level of the call, never on K:
//
//   upload                   one copy of the host-built work list (descriptors with wt, the level pointers) from pinned memory
//   k_update_hadd            data X / data Y rows of level 0 in place, the K rows of alignment scalars to scratch
//   fb_commit / fb_fold      ONE commitment pass over the K scalar rows (the resident SRS table, or the generators' fixed base)
//   k_update_place           MAC X, MAC Y = wt * MAC, align X = infinity, align Y = Commit(c)
//   for i < Lmax:            k_update_mix_data (both parts) and k_update_mix_points (the four point families) of the requests with level > i
//   k_update_close           incoming half over resident half at the request's level, then the complements onto MAC X / MAC Y
// (what the write batches decide alike is written once: write_batch_host.hpp and the places it names; a mix's form: update_batch.hip.h)
#include "kzg_state.hpp"
#include "update_batch.hip.h"
#include "write_batch_host.hpp"
#include "../../include/porla_gpu.h"

#include <algorithm>
#include <cstddef>
#include <mutex>
#include <string>
#include <unordered_set>
#include <vector>

namespace porla {

struct UpdateBatchWs {
    std::mutex mu;
    int device = -1;
    Buf list, scalars;
    PinnedList h_list;
    UseFence fence;
};
static PerDevice<UpdateBatchWs> g_upd_ws;

struct UpdPlan {
    const UpdDesc* d_desc;
    uint8_t* const* d_ptrs;
    uint32_t l1, k, ncols;
    hipStream_t stream;
};

template <class C>
static int launch_place(const UpdPlan& P, const XYZZ<typename C::Fp>* sums, uint32_t S) {
    static LdsOnce once;                               // dynamic LDS above 64 KiB: told once per device
    once.set({lds_kernel(&k_update_place<C>, sizeof(MacOctLds<typename C::Fp>))});
    ProfScope ps("update_place", P.stream);
    hipLaunchKernelGGL((k_update_place<C>), dim3((P.k + MACO_BF - 1) / MACO_BF), dim3(8 * MACO_BF), sizeof(MacOctLds<typename C::Fp>), P.stream,
                       P.d_desc, P.d_ptrs, P.l1, P.k, sums, S);
    PORLA_HIP(hipGetLastError());
    return PORLA_OK;
}

// the mixes of steps 0 .. lmax - 1 under the table leases (the MAC side's lock first, as mac_fft.hip's matrix form takes them)
template <class C>
static int launch_steps(const UpdPlan& P, const std::vector<uint32_t>& active, uint32_t lmax, size_t n_total) {
    using Q = typename IccCurve<C>::Q;
    const uint32_t* tws = nullptr;
    const uint32_t* tw30 = nullptr;
    int quad_log = 0, rc;
    if ((rc = mac_mix_tables_acquire(IccCurve<C>::id, n_total, P.stream, &tws, &quad_log))) return rc;
    if ((rc = icc_mix_tables_acquire(IccCurve<C>::id, n_total, P.stream, &tw30))) { (void)mac_mix_tables_release(P.stream); return rc; }
    for (uint32_t i = 0; i < lmax && !rc; i++) {
        const uint32_t a = active[i], tw_step = (uint32_t)(n_total >> i);
        {
            ProfScope ps("update_mix_data", P.stream);
            const size_t total = ((size_t)2 * a * P.ncols) << i;
            hipLaunchKernelGGL((k_update_mix_data<Q>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, P.stream, P.d_ptrs, P.l1, a, i, P.ncols,
                               tw30, tw_step);
        }
        ProfScope ps("update_mix_points", P.stream);
        update_mix_points_launch<C>(P.d_ptrs, P.l1, a, i, tws, tw_step, quad_log, P.stream);
        if (hipGetLastError() != hipSuccess) { set_last_error("porla: update batch: a mix launch failed"); rc = PORLA_ERR_HIP; }
    }
    const int r1 = icc_mix_tables_release(P.stream), r2 = mac_mix_tables_release(P.stream);
    return rc ? rc : (r1 ? r1 : r2);
}

// ws->mu held, ws->fence entered.  fb == nullptr: the resident SRS (KZG).
template <class C>
static int update_enqueue(UpdateBatchWs* ws, FixedBase<C>* fb, const porla_update_req* reqs, size_t k, size_t ncols, size_t n_total,
                          hipStream_t stream) {
    using Q = typename IccCurve<C>::Q;
    int rc;
    const LevelPlan plan(k, [&](size_t a) { return reqs[a].level; });
    const uint32_t lmax = plan.lmax, l1 = lmax + 1;
    // ---- the work list: descriptors | level pointers, one pinned buffer, one copy
    const size_t desc_b = k * sizeof(UpdDesc), ptr_b = k * UPD_FAMILIES * l1 * sizeof(void*), list_b = desc_b + ptr_b;
    if ((rc = ws->h_list.stage(list_b))) return rc;
    {
        UpdDesc* hd = (UpdDesc*)ws->h_list.h;
        void** hp = (void**)((uint8_t*)ws->h_list.h + desc_b);
        for (size_t a = 0; a < k; a++) {
            const porla_update_req& R = reqs[plan.order[a]];
            UpdDesc& D = hd[a];
            D.block = (const uint8_t*)R.d_block; D.mac = (const uint8_t*)R.d_mac; D.comp = (const uint8_t*)R.d_complements;
            write_wt<C>(n_total, R.write_step, D.wt_sc, D.wt_p, D.wt_q);
            D.level = (uint32_t)R.level; D.pad = 0;
            void* const* fam[UPD_FAMILIES] = {R.data_x, R.data_y, R.mac_x, R.mac_y, R.align_x, R.align_y};
            for (uint32_t f = 0; f < UPD_FAMILIES; f++)
                for (uint32_t l = 0; l < l1; l++) hp[(a * UPD_FAMILIES + f) * l1 + l] = l <= (uint32_t)R.level ? fam[f][l] : nullptr;
        }
    }
    if ((rc = ws->list.ensure(list_b))) return rc;
    if ((rc = ws->scalars.ensure(k * ncols * 32))) return rc;
    if ((rc = ws->h_list.send(ws->list.p, list_b, stream))) return rc;
    UpdPlan P;
    P.d_desc = (const UpdDesc*)ws->list.p;
    P.d_ptrs = (uint8_t* const*)((const uint8_t*)ws->list.p + desc_b);
    P.l1 = l1; P.k = (uint32_t)k; P.ncols = (uint32_t)ncols; P.stream = stream;
    // ---- 1. HAdd, data side
    {
        ProfScope ps("update_hadd", stream);
        hipLaunchKernelGGL((k_update_hadd<Q>), dim3((unsigned)((k * ncols + 255) / 256)), dim3(256), 0, stream, P.d_desc, P.d_ptrs, l1, (uint32_t)k,
                           (uint32_t)ncols, (uint8_t*)ws->scalars.p);
        PORLA_HIP(hipGetLastError());
    }
    // ---- 2. the K commitments, then the four point slots
    auto place = [&](const XYZZ<typename C::Fp>* sums, uint32_t S) { return launch_place<C>(P, sums, S); };
    if ((rc = commit_rows_then(fb, (const uint8_t*)ws->scalars.p, k, ncols, stream, place))) return rc;
    // ---- 3. the rebuild steps
    if (lmax && (rc = launch_steps<C>(P, plan.active, lmax, n_total))) return rc;
    // ---- 4. the close
    {
        ProfScope ps("update_close", stream);
        const size_t units = ((size_t)ncols * 4) << lmax;          // 16-byte units of the largest data copy
        const unsigned gx = (unsigned)std::min<size_t>((units + 255) / 256, 512);
        hipLaunchKernelGGL((k_update_close<C>), dim3(gx, (unsigned)k), dim3(256), 0, stream, P.d_desc, P.d_ptrs, l1, (uint32_t)ncols);
        PORLA_HIP(hipGetLastError());
    }
    return PORLA_OK;
}

// the checks both entry points make before the device is touched
static int update_check(const char* who, const porla_update_req* reqs, size_t k, size_t n_total) {
    auto bad = [&](const std::string& what) { return bad_arg(who, what); };
    if (k && !reqs) return bad("reqs is NULL");
    if (int rc = check_n_total(who, n_total, 30)) return rc;
    if (int rc = check_request_count(who, k)) return rc;
    std::unordered_set<const void*> seen;
    for (size_t a = 0; a < k; a++) {
        const porla_update_req& R = reqs[a];
        const std::string at = "request " + std::to_string(a) + ": ";
        if (!R.d_block || !R.d_mac) return bad(at + "a NULL block or MAC");
        if (R.pad != 0) return bad(at + "pad must be 0");
        if (R.level < 0 || R.level > 30 || ((size_t)1 << R.level) > n_total) return bad(at + "level must be 0 .. log2(n_total)");
        if (R.write_step % n_total == 0) return bad(at + "write_step % n_total == 0 is CRebuild's step, not an H update");
        void* const* fam[UPD_FAMILIES] = {R.data_x, R.data_y, R.mac_x, R.mac_y, R.align_x, R.align_y};
        for (uint32_t f = 0; f < UPD_FAMILIES; f++) {
            if (!fam[f]) return bad(at + "a NULL family array");
            for (int l = 0; l <= R.level; l++) if (!fam[f][l]) return bad(at + "a NULL level pointer");
            if (!seen.insert(fam[f][0]).second) return bad(at + "a level-0 pointer another request (or family) of this call names too: requests must be disjoint");
        }
    }
    return PORLA_OK;
}

}  // namespace porla

using namespace porla;

static_assert(sizeof(porla_update_req) == PORLA_UPDATE_REQ_BYTES, "porla_update_req size");
static_assert(offsetof(porla_update_req, d_block) == 0 && offsetof(porla_update_req, d_mac) == 8 &&
              offsetof(porla_update_req, d_complements) == 16 && offsetof(porla_update_req, write_step) == 24 &&
              offsetof(porla_update_req, level) == 32 && offsetof(porla_update_req, pad) == 36 &&
              offsetof(porla_update_req, data_x) == 40 && offsetof(porla_update_req, data_y) == 48 &&
              offsetof(porla_update_req, mac_x) == 56 && offsetof(porla_update_req, mac_y) == 64 &&
              offsetof(porla_update_req, align_x) == 72 && offsetof(porla_update_req, align_y) == 80,
              "porla_update_req offsets (include/porla_gpu.h)");

extern "C" int porla_kzg_update_batch_device(const porla_update_req* reqs, size_t k, size_t n_total, void* hip_stream) {
    int rc = update_check("porla_kzg_update_batch_device", reqs, k, n_total);
    if (rc) return rc;
    if (k == 0) return PORLA_OK;
    if ((rc = ensure_device())) return rc;
    size_t n;
    if ((rc = kzg_row_width(&n))) return rc;
    UpdateBatchWs* ws = nullptr;
    if ((rc = g_upd_ws.get(&ws))) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    return FencedCall(ws, stream).run([&] { return update_enqueue<Bn254G1>(ws, nullptr, reqs, k, n, n_total, stream); });
}

extern "C" int porla_ipa_update_batch_device(porla_fixed_base* generators_fb, const porla_update_req* reqs, size_t k, size_t n_total,
                                             void* hip_stream) {
    static const char* who = "porla_ipa_update_batch_device";
    int rc = update_check(who, reqs, k, n_total);
    if (rc) return rc;
    if (k == 0) return PORLA_OK;
    if (!generators_fb) return bad_arg(who, "generators_fb is NULL");
    if ((rc = ensure_device())) return rc;
    if ((rc = ipa_check_generators(who, "generators_fb", generators_fb))) return rc;
    UpdateBatchWs* ws = nullptr;
    if ((rc = g_upd_ws.get(&ws))) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    return FencedCall(ws, stream).run(
        [&] { return update_enqueue<Secp256k1G>(ws, &generators_fb->secp, reqs, k, IPA_COLS, n_total, stream); });
}
