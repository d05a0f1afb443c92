// The server's rebuild write in the CRebuild_No_Cached form for K independent files in ONE asynchronous call (include/porla_gpu.h:
// porla_kzg_server_rebuild_aligned_batch_device / porla_ipa_server_rebuild_aligned_batch_device): Server::update's CRebuild step as the
// reference runs it for height - 1 > TOP_CACHING_LEVEL (porla/Server/Server.hpp:1479-1485, :1835-2255) -- the top-level data rows
// mod p_icc in the 256-bit row format, an alignment commitment per row.  It commits, so the curve comes with the entry point.
// Every step is on the caller's stream; there is no side stream.  The requests are taken in groups whose rows of alignment scalars
// (2 n_total per request) fit the scalar workspace of at most PORLA_REBUILD_ROWS_MAX rows (default and ceiling 2^18; a group holds
// at least one request), so the launch sequence depends on n_total and on the number of groups, never on K within a group:
//
//   the front (server_rebuild_batch.hip: sr_enqueue_front), over all K requests
//     upload, k_sr_store, the passes of the data network but the last (k_sr_data), k_sr_mac_load, stage 1 .. log2 n_total, k_sr_mac_scale_*
//   per group
//     k_sr_data, SR_ALIGNED  the last pass: rows mod p_icc into data X / data Y, the alignment scalars into the workspace
//     fb_commit / fb_fold    ONE commitment pass over the group's rows (the resident SRS table, or the generators' fixed base), sums projective
//     k_sr_close, ALIGNED    + complements, to affine, into MAC X / MAC Y; the sums to affine into align X / align Y
// (the commitment pass of either build: kzg_state.hpp's commit_rows_then; the IPA row width and base check: write_batch_host.hpp)
#include "kzg_state.hpp"
#include "server_rebuild_host.hpp"
#include "server_rebuild_batch.hip.h"

#include <algorithm>
#include <cstdlib>

namespace porla {

constexpr size_t SRA_ROWS_CEIL = (size_t)1 << 18;

// rows of alignment scalars the workspace holds at most (PORLA_REBUILD_ROWS_MAX lowers it; read once per process)
static size_t sra_rows_max() {
    static const size_t v = [] {
        const char* e = getenv("PORLA_REBUILD_ROWS_MAX");
        const long long x = e ? atoll(e) : 0;
        return x > 0 && (size_t)x < SRA_ROWS_CEIL ? (size_t)x : SRA_ROWS_CEIL;
    }();
    return v;
}

// the last pass of the data network for requests g0 .. g0 + kg - 1, under the data side's table lease
template <class Q>
static int sra_launch_data(int curve, const SrFront& F, size_t g0, size_t kg, size_t n, size_t ncols, uint8_t* d_scalars, hipStream_t stream) {
    IccPass plan[ICC_MAX_PASSES];
    const int passes = icc_pass_plan(ilog2u(n), ncols, plan);
    const IccPass& P = plan[passes - 1];
    const uint32_t *twp = nullptr, *twq = nullptr;
    int rc;
    if ((rc = icc_encode_tables_acquire(curve, n, stream, &twp, &twq))) return rc;
    {
        ProfScope ps("server_rebuild_data_aligned", stream);
        const dim3 grid((unsigned)(P.col_tiles * (n >> P.ns)), (unsigned)kg);
        uint32_t* planes = F.planes ? F.planes + g0 * 2 * F.plane_words : nullptr;
#define PORLA_SRA_LAUNCH(FIRST)                                                                                                       \
    hipLaunchKernelGGL((k_sr_data<Q, FIRST, SR_ALIGNED>), grid, dim3(ICC30_SPLIT_THREADS), 0, stream, F.d_desc + g0, planes, F.plane_words, twp, \
                       twq, (uint32_t)n, (uint32_t)ncols, P.s, P.ns, P.cc_log, d_scalars)
        if (passes == 1) PORLA_SRA_LAUNCH(true);
        else PORLA_SRA_LAUNCH(false);
#undef PORLA_SRA_LAUNCH
    }
    if (hipGetLastError() != hipSuccess) { set_last_error("porla: server rebuild aligned batch: the data launch failed"); rc = PORLA_ERR_HIP; }
    const int r1 = icc_mix_tables_release(stream);
    return rc ? rc : r1;
}

// ws->mu held, ws->fence entered.  fb == nullptr: the resident SRS (KZG).
template <class C>
static int sra_enqueue(ServerRebuildWs* ws, FixedBase<C>* fb, const porla_server_rebuild_req* reqs, size_t k, size_t n, size_t ncols,
                       hipStream_t stream) {
    using Q = typename IccCurve<C>::Q;
    using M = typename C::Fp;
    int rc;
    const size_t per_group = std::max<size_t>(1, sra_rows_max() / (2 * n));
    const size_t kg_max = std::min(k, per_group);
    if ((rc = ws->scalars.ensure(kg_max * 2 * n * ncols * 32))) return rc;          // (sr_check: the product does not overflow)
    SrFront F;
    if ((rc = sr_enqueue_front(ws, IccCurve<C>::id, reqs, k, n, ncols, stream, &F))) return rc;
    uint8_t* d_scalars = (uint8_t*)ws->scalars.p;
    for (size_t g0 = 0; g0 < k; g0 += per_group) {
        const size_t kg = std::min(per_group, k - g0);
        if ((rc = sra_launch_data<Q>(IccCurve<C>::id, F, g0, kg, n, ncols, d_scalars, stream))) return rc;
        auto close = [&](const XYZZ<M>* sums, uint32_t S) {
            ProfScope ps("server_rebuild_close_aligned", stream);
            const unsigned gx = (unsigned)std::min<size_t>((2 * n + 255) / 256, 512);
            hipLaunchKernelGGL((k_sr_close<C, true>), dim3(gx, (unsigned)kg), dim3(256), 0, stream, F.d_desc + g0, (uint32_t)n,
                               (const XYZZ<M>*)F.work + g0 * n, (const XYZZ<M>*)F.work_y + g0 * n, sums, S);
            PORLA_HIP(hipGetLastError());
            return (int)PORLA_OK;
        };
        if ((rc = commit_rows_then(fb, d_scalars, kg * 2 * n, ncols, stream, close))) return rc;
    }
    return PORLA_OK;
}

}  // namespace porla

using namespace porla;

extern "C" int porla_kzg_server_rebuild_aligned_batch_device(const porla_server_rebuild_req* reqs, size_t k, size_t n_total, void* hip_stream) {
    static const char* who = "porla_kzg_server_rebuild_aligned_batch_device";
    const size_t n = kzg_n_samples();
    // (the row width is the SRS size; before there is one the requests are still checked, against a row of one symbol)
    int rc = sr_check(who, reqs, k, n_total, n ? n : 1, 0);
    if (rc) return rc;
    if (k == 0) return PORLA_OK;
    if ((rc = ensure_device())) return rc;
    if (n == 0) return kzg_no_srs();
    ServerRebuildWs* ws = nullptr;
    if ((rc = sr_workspace(&ws))) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    return FencedCall(ws, stream).run([&] { return sra_enqueue<Bn254G1>(ws, nullptr, reqs, k, n_total, n, stream); });
}

extern "C" int porla_ipa_server_rebuild_aligned_batch_device(porla_fixed_base* generators_fb, const porla_server_rebuild_req* reqs, size_t k,
                                                             size_t n_total, void* hip_stream) {
    static const char* who = "porla_ipa_server_rebuild_aligned_batch_device";
    int rc = sr_check(who, reqs, k, n_total, IPA_COLS, 1);
    if (rc) return rc;
    if (k == 0) return PORLA_OK;
    if (!generators_fb) return bad_arg(who, "generators_fb is NULL");
    if ((rc = ensure_device())) return rc;
    if ((rc = ipa_check_generators(who, "generators_fb", generators_fb))) return rc;
    ServerRebuildWs* ws = nullptr;
    if ((rc = sr_workspace(&ws))) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    return FencedCall(ws, stream).run(
        [&] { return sra_enqueue<Secp256k1G>(ws, &generators_fb->secp, reqs, k, n_total, IPA_COLS, stream); });
}
