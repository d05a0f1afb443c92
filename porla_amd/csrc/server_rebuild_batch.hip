// The server's rebuild write for K independent files in ONE asynchronous call (include/porla_gpu.h: porla_server_rebuild_batch_device):
// the write on which Server::update calls CRebuild instead of HAdd (porla/Server/Server.hpp:413-469 with CRebuild_Cached :1487-1833) --
// the block and its MAC into the raw stores, the whole data network over U, the whole MAC network over MAC_U, X part and Y part, into
// the resident halves of the top level, the alignments to infinity and the complement adds.  It is the step the update batch refuses
// (write_step % n_total == 0), the other side of porla_*_client_rebuild_batch_device.  It commits nothing, so it needs no SRS, key or
// fixed base and one symbol serves both curves.  Every step is on the caller's stream, and the launch sequence depends on n_total,
// never on K:
//
//   upload                   one copy of the host-built descriptors (pointers, wt as the data side and the MAC side see it)
//   k_sr_store               block -> U[index - 1], mac -> MAC_U[index - 1]
//   k_sr_data                ceil(log2 n_total / 9) passes over 1 024-symbol tiles, grid.y = request, under the data side's table lease;
//                            the last pass (its SR_CACHED form) writes data X and data Y = wt X
//   k_sr_mac_load            MAC_U -> the work array of K * n_total points
//   stage 1 .. log2 n_total  mac_fft.hip's stage loop (mac_stages_leased: k_mac_stage1_quad, k_mac_stage30_oct / _quad / k_mac_stage30
//                            with per-butterfly scalars), one launch each over the whole work array, under the MAC side's table lease
//   k_sr_mac_scale_*         work_y = wt * work, grid.y = request
//   k_sr_close               + complements, to affine, into MAC X / MAC Y; align X / align Y = infinity
#include "server_rebuild_host.hpp"
#include "server_rebuild_batch.hip.h"

#include <algorithm>
#include <cstddef>
#include <string>
#include <unordered_set>

namespace porla {

static PerDevice<ServerRebuildWs> g_sr_ws;
int sr_workspace(ServerRebuildWs** out) { return g_sr_ws.get(out); }

// dynamic LDS above 64 KiB: the four-lane scaling is the one such kernel launched from this file (the stages are mac_fft.hip's)
static void sr_lds_attributes() {
    static LdsOnce once;
    once.set({lds_kernel(&k_sr_mac_scale_quad<Bn254G1>, sizeof(MacQuadLds<Bn254Fp>)),
              lds_kernel(&k_sr_mac_scale_quad<Secp256k1G>, sizeof(MacQuadLds<Secp256k1Fp>))});
}

// the data network of the K stores: icc_encode_core's passes (icc.hip), every pass one launch with grid.y = request; with_last =
// false leaves the last pass to the caller (the aligned form's own kernel)
template <class Q>
static int sr_launch_data(int curve, const SrDesc* d_desc, uint32_t* d_planes, size_t plane_words, size_t k, size_t n, size_t ncols,
                          bool with_last, hipStream_t stream) {
    IccPass plan[ICC_MAX_PASSES];
    const int passes = icc_pass_plan(ilog2u(n), ncols, plan);
    if (!with_last && passes == 1) return PORLA_OK;
    const uint32_t *twp = nullptr, *twq = nullptr;
    int rc;
    if ((rc = icc_encode_tables_acquire(curve, n, stream, &twp, &twq))) return rc;
    for (int pz = 0; pz < passes - (with_last ? 0 : 1); pz++) {
        const int s = plan[pz].s, ns = plan[pz].ns, cc_log = plan[pz].cc_log;
        const dim3 grid((unsigned)(plan[pz].col_tiles * (n >> ns)), (unsigned)k);
        const bool first = pz == 0, last = pz == passes - 1;
        ProfScope ps("server_rebuild_data", stream);
#define PORLA_SR_LAUNCH(F, FIN)                                                                                                    \
    hipLaunchKernelGGL((k_sr_data<Q, F, FIN>), grid, dim3(ICC30_SPLIT_THREADS), 0, stream, d_desc, d_planes, plane_words, twp, twq, \
                       (uint32_t)n, (uint32_t)ncols, s, ns, cc_log, (uint8_t*)nullptr)
        if (first && last) PORLA_SR_LAUNCH(true, SR_CACHED);
        else if (first) PORLA_SR_LAUNCH(true, SR_PASS);
        else if (last) PORLA_SR_LAUNCH(false, SR_CACHED);
        else PORLA_SR_LAUNCH(false, SR_PASS);
#undef PORLA_SR_LAUNCH
    }
    if (hipGetLastError() != hipSuccess) { set_last_error("porla: server rebuild batch: a data launch failed"); rc = PORLA_ERR_HIP; }
    const int r1 = icc_mix_tables_release(stream);
    return rc ? rc : r1;
}

// the MAC network of the K stores on one work array, the Y part and the close.  The forms: every stage with per-butterfly scalars --
// eight lanes per butterfly while the whole call has at most MACO_MAX_BUTTERFLIES of them, four above that up to 4 * 2^quad_log points
// (2^16 by default: where mac_encode_core leaves its four-lane forms), one lane beyond or with PORLA_MAC_QUAD_MAX = 0 (mac_fft.hip:
// mac_stages).  close = false leaves the close to the caller (the aligned form's, behind its commitments).
template <class C>
static int sr_launch_mac(ServerRebuildWs* ws, const SrDesc* d_desc, size_t k, size_t n, bool close, hipStream_t stream) {
    using M = typename C::Fp;
    const uint32_t* tws = nullptr;
    int quad_log = 0, rc;
    if ((rc = mac_mix_tables_acquire(IccCurve<C>::id, n, stream, &tws, &quad_log))) return rc;
    XYZZ<M>* work = (XYZZ<M>*)ws->work.p;
    XYZZ<M>* work_y = (XYZZ<M>*)ws->work_y.p;
    const size_t points = k * n;
    const bool quad = quad_log > 0 && points <= ((size_t)4 << quad_log);
    {
        ProfScope ps("server_rebuild_mac_load", stream);
        hipLaunchKernelGGL((k_sr_mac_load<C>), dim3((unsigned)((n + 63) / 64), (unsigned)k), dim3(64), 0, stream, d_desc, (uint32_t)n, work);
    }
    mac_stages_leased(IccCurve<C>::id, work, points, n, quad, tws, "server_rebuild_mac_stage", stream);
    {
        ProfScope ps("server_rebuild_mac_scale", stream);
        if (quad)
            hipLaunchKernelGGL((k_sr_mac_scale_quad<C>), dim3((unsigned)((n + MACQ_BF - 1) / MACQ_BF), (unsigned)k), dim3(4 * MACQ_BF),
                               sizeof(MacQuadLds<M>), stream, d_desc, (uint32_t)n, work, work_y);
        else
            hipLaunchKernelGGL((k_sr_mac_scale_lane<C>), dim3((unsigned)((n + 63) / 64), (unsigned)k), dim3(64), 0, stream, d_desc, (uint32_t)n,
                               work, work_y);
    }
    if (close) {
        ProfScope ps("server_rebuild_close", stream);
        const unsigned gx = (unsigned)std::min<size_t>((2 * n + 255) / 256, 512);
        hipLaunchKernelGGL((k_sr_close<C, false>), dim3(gx, (unsigned)k), dim3(256), 0, stream, d_desc, (uint32_t)n, work, work_y,
                           (const XYZZ<M>*)nullptr, 0u);
    }
    if (hipGetLastError() != hipSuccess) { set_last_error("porla: server rebuild batch: a MAC launch failed"); rc = PORLA_ERR_HIP; }
    const int r1 = mac_mix_tables_release(stream);
    return rc ? rc : r1;
}

// ws->mu held, ws->fence entered.  cached: the whole sequence of this call; otherwise its front for the aligned form
// (server_rebuild_host.hpp: sr_enqueue_front) -- without the last data pass and the close -- and F says where that form goes on
template <class C>
static int sr_enqueue(ServerRebuildWs* ws, const porla_server_rebuild_req* reqs, size_t k, size_t n, size_t ncols, bool cached, hipStream_t stream,
                      SrFront* F) {
    using Q = typename IccCurve<C>::Q;
    using M = typename C::Fp;
    int rc;
    const int logn = ilog2u(n);
    const bool planes = logn > ICC_TILE_LOG - 1;                           // more than one pass: the residue planes travel between them
    const size_t plane_words = n * ncols * ICC30_PLANE_WORDS;              // (sr_check: the products below do not overflow)
    const size_t desc_b = k * sizeof(SrDesc);
    if ((rc = ws->h_list.stage(desc_b))) return rc;
    if ((rc = ws->list.ensure(desc_b))) return rc;
    if (planes && (rc = ws->planes.ensure(k * 2 * plane_words * 4))) return rc;
    if ((rc = ws->work.ensure(k * n * sizeof(XYZZ<M>)))) return rc;
    if ((rc = ws->work_y.ensure(k * n * sizeof(XYZZ<M>)))) return rc;
    sr_lds_attributes();
    {
        SrDesc* hd = (SrDesc*)ws->h_list.h;
        for (size_t a = 0; a < k; a++) {
            const porla_server_rebuild_req& R = reqs[a];
            SrDesc& D = hd[a];
            D.block = (const uint8_t*)R.d_block; D.mac = (const uint8_t*)R.d_mac; D.comp = (const uint8_t*)R.d_complements;
            D.u_blocks = (uint8_t*)R.d_u_blocks; D.u_macs = (uint8_t*)R.d_u_macs;
            D.data_x = (uint8_t*)R.d_data_x; D.data_y = (uint8_t*)R.d_data_y;
            D.mac_x = (uint8_t*)R.d_mac_x; D.mac_y = (uint8_t*)R.d_mac_y;
            D.align_x = (uint8_t*)R.d_align_x; D.align_y = (uint8_t*)R.d_align_y;
            write_wt<C>(n, R.write_step, D.wt_sc, D.wt_p, D.wt_q);
            D.row = (uint32_t)(R.index - 1); D.pad = 0;
        }
    }
    if ((rc = ws->h_list.send(ws->list.p, desc_b, stream))) return rc;
    const SrDesc* d_desc = (const SrDesc*)ws->list.p;
    {
        ProfScope ps("server_rebuild_store", stream);
        const unsigned gx = (unsigned)std::min<size_t>((2 * ncols + 4 + 255) / 256, 64);
        hipLaunchKernelGGL(k_sr_store, dim3(gx, (unsigned)k), dim3(256), 0, stream, d_desc, (uint32_t)ncols);
        PORLA_HIP(hipGetLastError());
    }
    if (F) *F = SrFront{d_desc, (uint32_t*)ws->planes.p, plane_words, ws->work.p, ws->work_y.p};
    if ((rc = sr_launch_data<Q>(IccCurve<C>::id, d_desc, (uint32_t*)ws->planes.p, plane_words, k, n, ncols, cached, stream))) return rc;
    return sr_launch_mac<C>(ws, d_desc, k, n, cached, stream);
}

int sr_enqueue_front(ServerRebuildWs* ws, int curve, const porla_server_rebuild_req* reqs, size_t k, size_t n, size_t ncols, hipStream_t stream,
                     SrFront* F) {
    return curve == 0 ? sr_enqueue<Bn254G1>(ws, reqs, k, n, ncols, false, stream, F) : sr_enqueue<Secp256k1G>(ws, reqs, k, n, ncols, false, stream, F);
}

// the checks made before the device is touched
int sr_check(const char* who, const porla_server_rebuild_req* reqs, size_t k, size_t n_total, size_t n_cols, int curve) {
    auto bad = [&](const std::string& what) { return bad_arg(who, what); };
    if (k && !reqs) return bad("reqs is NULL");
    if (n_total > ((size_t)1 << 16) && (n_total & (n_total - 1)) == 0)
        return bad("n_total above 2^16: the batch stops at 2^16 rows; larger files go through the single-file calls "
                   "porla_icc_encode_xy_device and porla_icc_mac_encode_xy_device");
    if (int rc = check_n_total(who, n_total, 16)) return rc;
    if (n_cols == 0) return bad("n_cols is 0");
    if (curve != 0 && curve != 1) return bad("curve must be 0 (BN254 / KZG) or 1 (secp256k1 / IPA)");
    if (int rc = check_request_count(who, k)) return rc;
    size_t rows, t;
    if (!mul_ok(n_total, n_cols, &rows) || !mul_ok(rows, 128, &t) || !mul_ok(rows, 8 * ICC30_PLANE_WORDS, &t) || (k && !mul_ok(t, k, &t)))
        return bad("a byte size overflows: n_total * n_cols symbols do not fit a buffer");
    if (n_cols > 0xffffu) return bad("n_cols above 65535");
    std::unordered_set<const void*> seen;
    for (size_t a = 0; a < k; a++) {
        const porla_server_rebuild_req& R = reqs[a];
        const std::string at = "request " + std::to_string(a) + ": ";
        const void* in[3] = {R.d_block, R.d_mac, R.d_complements};
        void* const out[8] = {R.d_u_blocks, R.d_u_macs, R.d_data_x, R.d_data_y, R.d_mac_x, R.d_mac_y, R.d_align_x, R.d_align_y};
        if (!in[0] || !in[1]) return bad(at + "a NULL block or MAC");
        for (const void* p : out) if (!p) return bad(at + "a NULL store or top-level pointer");
        uintptr_t bits = (uintptr_t)in[0] | (uintptr_t)in[1] | (uintptr_t)in[2];
        for (const void* p : out) bits |= (uintptr_t)p;
        if (bits & 15u) return bad(at + "a pointer that is not 16-byte aligned");
        if (R.index < 1 || R.index > n_total) return bad(at + "index must be 1 .. n_total");
        for (const void* p : out)
            if (!seen.insert(p).second) return bad(at + "a store or top-level pointer another request (or field) of this call names too: requests must be disjoint");
    }
    return PORLA_OK;
}

}  // namespace porla

using namespace porla;

static_assert(sizeof(porla_server_rebuild_req) == PORLA_SERVER_REBUILD_REQ_BYTES, "porla_server_rebuild_req size");
static_assert(offsetof(porla_server_rebuild_req, d_block) == 0 && offsetof(porla_server_rebuild_req, d_mac) == 8 &&
              offsetof(porla_server_rebuild_req, d_complements) == 16 && offsetof(porla_server_rebuild_req, d_u_blocks) == 24 &&
              offsetof(porla_server_rebuild_req, d_u_macs) == 32 && offsetof(porla_server_rebuild_req, d_data_x) == 40 &&
              offsetof(porla_server_rebuild_req, d_data_y) == 48 && offsetof(porla_server_rebuild_req, d_mac_x) == 56 &&
              offsetof(porla_server_rebuild_req, d_mac_y) == 64 && offsetof(porla_server_rebuild_req, d_align_x) == 72 &&
              offsetof(porla_server_rebuild_req, d_align_y) == 80 && offsetof(porla_server_rebuild_req, write_step) == 88 &&
              offsetof(porla_server_rebuild_req, index) == 96,
              "porla_server_rebuild_req offsets (include/porla_gpu.h)");

extern "C" int porla_server_rebuild_batch_device(const porla_server_rebuild_req* reqs, size_t k, size_t n_total, size_t n_cols, int curve,
                                                 void* hip_stream) {
    int rc = sr_check("porla_server_rebuild_batch_device", reqs, k, n_total, n_cols, curve);
    if (rc) return rc;
    if (k == 0) return PORLA_OK;
    if ((rc = ensure_device())) return rc;
    ServerRebuildWs* ws = nullptr;
    if ((rc = g_sr_ws.get(&ws))) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    return FencedCall(ws, stream).run([&] {
        return curve == 0 ? sr_enqueue<Bn254G1>(ws, reqs, k, n_total, n_cols, true, stream, nullptr)
                          : sr_enqueue<Secp256k1G>(ws, reqs, k, n_total, n_cols, true, stream, nullptr);
    });
}
