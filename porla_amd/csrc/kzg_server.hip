// The server side of the KZG build over the resident SRS table (include/porla_gpu.h): the state's one instance and the guard of its
// table, the commit batches (device, host, device-to-host, multi-device), the CRebuild stage, the single-call audit, HAdd, and the
// calls that manage the table (window, shape, release, row length).
#include "kzg_state.hpp"
#include "host_fold64.hpp"

#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

using namespace porla;
using Fp = Bn254Fp;
using Fr = Bn254Fr;

KzgState porla::g_kzg;

int porla::current_dev(KzgDev** out) {
    int rc = ensure_device();
    if (rc) return rc;
    return g_kzg.devs.get(out);
}

int porla::refresh_srs_locked(KzgDev** out) {
    KzgDev* kd;
    int rc = current_dev(&kd);
    if (rc) return rc;
    *out = kd;
    if (kd->srs_version == g_kzg.version) return PORLA_OK;
    if (g_kzg.srs.empty()) return PORLA_ERR_STATE;
    const size_t bytes = g_kzg.srs.size() * sizeof(Affine<Fp>);
    if ((rc = kd->d_srs.ensure(bytes))) return rc;
    PORLA_HIP(hipMemcpy(kd->d_srs.p, g_kzg.srs.data(), bytes, hipMemcpyHostToDevice));
    {
        std::lock_guard<std::mutex> lk(kd->fb.mu);
        rc = kd->fb.build((const Affine<Fp>*)kd->d_srs.p, g_kzg.srs.size(), g_kzg.commit_window, engine_stream());
    }
    if (rc) return rc;
    kd->srs_version = g_kzg.version;
    return PORLA_OK;
}

int SrsTable::acquire(size_t want) {
    std::unique_lock<std::mutex> ls(g_kzg.mu);
    KzgDev* kd = nullptr;
    int rc = refresh_srs_locked(&kd);
    if (rc) {
        return rc == PORLA_ERR_STATE ? kzg_no_srs() : rc;
    }
    len = want == N_SAMPLES ? (size_t)g_kzg.n_samples : want;
    if (len > g_kzg.srs.size()) { set_last_error("porla: more coefficients than SRS points"); return PORLA_ERR_STATE; }
    fb = &kd->fb;
    lk = std::unique_lock<std::mutex>(fb->mu);
    return PORLA_OK;
}

int porla::kzg_commit_rows(const uint8_t* rows, bool device_ptrs, size_t n_rows, size_t len, uint8_t* out, hipStream_t stream, bool guest_room) {
    SrsTable t;
    int rc = t.acquire(len);
    if (rc) return rc;
    if (device_ptrs) return t.fb->commit_device(rows, n_rows, len, len * 32, out, stream, guest_room);
    return t.fb->commit_host(rows, n_rows, len, len * 32, out, engine_stream());
}

namespace {
// CRebuild's side stream and its two events, one set per device; `mu` is held across fork -> launches -> join
struct StageSide { std::mutex mu; int device = -1; hipStream_t s = nullptr; hipEvent_t fork = nullptr, join = nullptr; };
PerDevice<StageSide> g_stage_side;
// the single audit's staging: mapped, coherent pinned memory the combine writes B and the alignment scalars into
struct AuditPinned { int device = -1; uint8_t* h = nullptr; size_t cap = 0; };
std::mutex g_audit_call_mu;           // one audit at a time per process (the pinned staging and the audit slot are its own)
PerDevice<AuditPinned> g_audit_pinned;
}  // namespace

extern "C" {

// coefficients per commitment row = SRS size (0 before init_SRS*): callers that slice a row-major batch derive the row stride
// (32 bytes per coefficient) from it instead of assuming the reference's 128 (config.hpp NUM_CHUNKS)
int porla_kzg_row_coefficients(size_t* n_out) {
    if (!n_out) { set_last_error("porla: null argument"); return PORLA_ERR_ARG; }
    *n_out = kzg_n_samples();
    return PORLA_OK;
}
// ---- batched form of compute_digest_from_srs (include/porla_gpu.h) ----
int porla_kzg_commit_batch_device(const void* d_rows, size_t n_rows, void* d_out, void* hip_stream) {
    if (n_rows && (!d_rows || !d_out)) { set_last_error("porla: null argument"); return PORLA_ERR_ARG; }
    int rc = ensure_device();
    if (rc) return rc;
    return kzg_commit_rows((const uint8_t*)d_rows, true, n_rows, kzg_n_samples(), (uint8_t*)d_out, (hipStream_t)hip_stream);
}
// The last encode stage of a large CRebuild for the KZG build in ONE call (porla/Server/Server.hpp:1487-1833 cached, :1899-2254
// on disk): per part (X, Y): the data butterflies, align_MAC's row mod p_icc and alignment scalars (:531-541), one
// compute_digest_from_srs per row on those scalars (:550-560, :2059-2065) -- and, beside them, the MAC butterflies (:1590-1609,
// :1658-1676).  Two streams inside: the MAC network (15 dependent stages, one latency-bound wave per SIMD) starts FIRST on a side
// stream and keeps its slot on every SIMD for the length of the call, because the commitments of the 2 n rows run in the
// two-waves-per-SIMD form of their kernel (k_fb_commit<C, true>).  Asynchronous: hip_stream continues when both sides are done.
int porla_kzg_crebuild_stage_device(const void* d_rows_in, size_t n_rows, unsigned long long write_step, void* d_aligned_x,
                                    void* d_aligned_y, void* d_scalars_xy, void* d_commits_xy, const void* d_macs_in, void* d_macs_x,
                                    void* d_macs_y, void* hip_stream) {
    if (!d_rows_in || !d_scalars_xy || !d_commits_xy || !d_macs_in || !d_macs_x || !d_macs_y) {
        set_last_error("porla: null argument");
        return PORLA_ERR_ARG;
    }
    int rc = ensure_device();
    if (rc) return rc;
    const size_t n_cols = kzg_n_samples();
    if (n_cols == 0) return kzg_no_srs();
    StageSide* side = nullptr;
    if ((rc = g_stage_side.get(&side))) return rc;
    std::lock_guard<std::mutex> lk(side->mu);          // everything below only enqueues
    if (!side->s) {
        // built completely before it is entered; a failure half way destroys what exists (no stream or event is leaked) and
        // leaves the entry empty, so that the next call tries again
        hipStream_t s = nullptr;
        hipEvent_t fork = nullptr, join = nullptr;
        hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&fork, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&join, hipEventDisableTiming);
        if (e != hipSuccess) {
            if (join) (void)hipEventDestroy(join);
            if (fork) (void)hipEventDestroy(fork);
            if (s) (void)hipStreamDestroy(s);
            return ::porla::hip_fail(e, "crebuild stage: side stream / events", __FILE__, __LINE__);
        }
        side->s = s; side->fork = fork; side->join = join;
    }
    hipStream_t stream = (hipStream_t)hip_stream;
    PORLA_HIP(hipEventRecord(side->fork, stream));
    PORLA_HIP(hipStreamWaitEvent(side->s, side->fork, 0));
    // From here on the side stream may hold work that writes d_macs_x / d_macs_y: EVERY exit joins it back into hip_stream, also the
    // failing ones -- a caller that gets an error may free its buffers as soon as hip_stream has drained, and the next call's
    // fork / join records must not interleave with a stage still running
    rc = porla_icc_mac_encode_xy_device(d_macs_in, n_rows, 0, write_step, d_macs_x, d_macs_y, side->s);
    hipError_t je = hipEventRecord(side->join, side->s);
    uint8_t* sc = (uint8_t*)d_scalars_xy;
    if (!rc)
        rc = porla_icc_encode_xy_device(d_rows_in, n_rows, n_cols, 0, write_step, nullptr, d_aligned_x, sc, nullptr, d_aligned_y,
                                        sc + 32 * n_rows * n_cols, 0, stream);
    // both parts' alignment scalars lie back to back: ONE batch of 2 n rows
    if (!rc) rc = kzg_commit_rows(sc, true, 2 * n_rows, n_cols, (uint8_t*)d_commits_xy, stream, /*guest_room=*/true);
    if (je == hipSuccess) je = hipStreamWaitEvent(stream, side->join, 0);
    if (je != hipSuccess) {
        // the join itself failed: fall back to a host wait so that no side work outlives the call
        (void)hipStreamSynchronize(side->s);
        if (!rc) rc = ::porla::hip_fail(je, "crebuild stage: join of the side stream", __FILE__, __LINE__);
    }
    return rc;
}

// rows resident on the device, results wanted on the host NOW (the audit's align_MAC commitment, Server.hpp:903 -> :550-560, on the
// scalars porla_audit_combine_device left in HBM): up to 64 rows go through the single-launch kernel on `hip_stream` -- behind
// whatever produced the rows there -- and the host polls the pinned result; more rows: the batch kernels and one copy back
int porla_kzg_commit_batch_device_to_host(const void* d_rows, size_t n_rows, uint8_t* out, void* hip_stream) {
    if (n_rows && (!d_rows || !out)) { set_last_error("porla: null argument"); return PORLA_ERR_ARG; }
    int rc = ensure_device();
    if (rc) return rc;
    if (n_rows == 0) return PORLA_OK;
    const size_t len = kzg_n_samples();
    hipStream_t stream = (hipStream_t)hip_stream;
    if (FixedBase<Bn254G1>::small_ok(n_rows, len)) {
        SrsTable t;
        if ((rc = t.acquire(len))) return rc;
        uint8_t* op[FB_SMALL_MAX_ROWS];
        for (size_t r = 0; r < n_rows; r++) op[r] = out + 64 * r;
        return t.fb->commit_small(nullptr, n_rows, len, op, stream, (const uint8_t*)d_rows);
    }
    void* d_out = nullptr;
    PORLA_HIP(hipMalloc(&d_out, n_rows * 64));
    rc = kzg_commit_rows((const uint8_t*)d_rows, true, n_rows, len, (uint8_t*)d_out, stream);
    hipError_t e = rc ? hipSuccess : hipMemcpyAsync(out, d_out, n_rows * 64, hipMemcpyDeviceToHost, stream);
    hipError_t e2 = hipStreamSynchronize(stream);
    (void)hipFree(d_out);
    if (rc) return rc;
    if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync", __FILE__, __LINE__);
    if (e2 != hipSuccess) return hip_fail(e2, "hipStreamSynchronize", __FILE__, __LINE__);
    return PORLA_OK;
}
// Server::audit for the KZG build in ONE call (Server.hpp:564-931 after the challenge has been drawn), everything resident in HBM:
//   the two MSMs over the challenged MACs start first, on the audit slot's own stream (msm_pair_gather_begin);
//   meanwhile: row combine + alignment scalars (audit.hip) -> B and c land in pinned host memory; y = B(z) and the quotient h on
//   the host; ONE three-row launch commits c (align_MAC, :903 -> :550-560), B and h (create_proof, :907 -> main.go:153-175);
//   then the MSM pair is collected.
int porla_kzg_audit_device(const void* d_rows64, const uint64_t* d_idx64, const uint32_t* d_coef64, size_t n64, const void* d_rows32,
                           const uint64_t* d_idx32, const uint32_t* d_coef32, size_t n32, const void* d_mac_store,
                           const void* d_align_store, const uint64_t* d_mac_idx, const uint32_t* d_mac_coef, size_t n_macs,
                           unsigned long long random_point, uint8_t combined_mac[64], uint8_t combined_align[64],
                           uint8_t align_value[64], uint8_t commitment[64], uint8_t proof_h[64], uint8_t proof_point[32],
                           uint8_t proof_claim[32], uint8_t* b_out, void* hip_stream) {
    if (!combined_mac || !combined_align || !align_value || !commitment || !proof_h || !proof_point || !proof_claim ||
        (n_macs && (!d_mac_store || !d_align_store || !d_mac_idx || !d_mac_coef))) {
        set_last_error("porla: null argument");
        return PORLA_ERR_ARG;
    }
    int rc = ensure_device();
    if (rc) return rc;
    const size_t n = kzg_n_samples();
    if (n == 0) return kzg_no_srs();
    std::lock_guard<std::mutex> lk(g_audit_call_mu);
    AuditPinned* pin = nullptr;
    if ((rc = g_audit_pinned.get(&pin))) return rc;
    if (pin->cap < 64 * n) {
        if (pin->h) PORLA_HIP(hipHostFree(pin->h));
        pin->h = nullptr; pin->cap = 0;
        PORLA_HIP(hipHostMalloc((void**)&pin->h, 64 * n, hipHostMallocMapped | hipHostMallocCoherent));
        pin->cap = 64 * n;
    }
    void* pin_dev = nullptr;
    PORLA_HIP(hipHostGetDevicePointer(&pin_dev, pin->h, 0));
    uint8_t* h_b = pin->h;                  // B mod p_icc, n 32-byte big-endian values
    uint8_t* h_c = pin->h + 32 * n;         // the alignment scalars
    // hip_stream orders the INPUTS: the combine runs on it as given (NULL = the null stream), the pair on the audit slot's own
    // stream behind an event recorded on hip_stream now -- index / coefficient arrays the caller has just uploaded asynchronously
    // on it are complete before any kernel of the audit reads them (one record + one wait: ~4 us of a 150 us call)
    hipStream_t stream = (hipStream_t)hip_stream;
    Workspace* aw = nullptr;
    if ((rc = get_workspace_slot(MSM_AUDIT_SLOT, &aw))) return rc;
    if ((rc = order_after_caller(aw, (hipStream_t)hip_stream, stream, aw->own_stream))) return rc;
    const bool pair = n_macs >= 1 && n_macs <= 32768;
    bool pair_begun = false;
    auto collect_pair = [&]() -> int {
        if (!pair_begun) return PORLA_OK;
        XYZZ<Fp> ta, tb;
        int r2 = msm_pair_end<Bn254G1>(MSM_AUDIT_SLOT, &ta, &tb);
        if (r2) return r2;
        const XYZZ<Fp> both[2] = {ta, tb};
        Affine<Fp> aff[2];
        h_batch_xyzz_to_affine64<Fp>(both, 2, aff);          // one inversion for the two sums
        h_affine_to_bytes<Fp>(combined_mac, aff[0]);
        h_affine_to_bytes<Fp>(combined_align, aff[1]);
        return PORLA_OK;
    };
    // the combine is enqueued FIRST: its two short kernels take their compute units before the pair's 256 long-lived blocks do (begun
    // the other way round the combine was seen to wait ~85 us behind them), then the pair starts on the audit slot's own stream
    rc = porla_audit_combine_device(d_rows64, d_idx64, d_coef64, n64, d_rows32, d_idx32, d_coef32, n32, n, 0, nullptr, nullptr,
                                    pin_dev, (uint8_t*)pin_dev + 32 * n, stream);
    if (rc == PORLA_OK && pair) {
        rc = msm_pair_gather_begin<Bn254G1>(MSM_AUDIT_SLOT, (const uint8_t*)d_mac_store, (const uint8_t*)d_align_store, d_mac_idx,
                                                d_mac_coef, n_macs, aw->own_stream);
        pair_begun = rc == PORLA_OK;
    }
    if (rc == PORLA_OK && hipStreamSynchronize(stream) != hipSuccess) {
        set_last_error("porla: hipStreamSynchronize failed in the audit");
        rc = PORLA_ERR_HIP;
    }
    if (rc) { (void)collect_pair(); return rc; }
    std::vector<uint8_t> three(3 * 32 * n);
    memcpy(three.data(), h_c, 32 * n);
    memcpy(three.data() + 32 * n, h_b, 32 * n);
    kzg_open_rows(h_b, n, random_point, three.data() + 64 * n, proof_point, proof_claim);
    if (b_out) memcpy(b_out, h_b, 32 * n);
    uint8_t outs[192];
    // the three row sums stay projective until the pair's two sums are in: ONE inversion normalises all five points
    XYZZ<Fp> five[5];
    bool raw3 = false;
    if (pair_begun && FixedBase<Bn254G1>::small_ok(3, n)) {
        SrsTable t;
        if ((rc = t.acquire(n)) == PORLA_OK) {
            const uint8_t* rp[3] = {three.data(), three.data() + 32 * n, three.data() + 64 * n};
            rc = t.fb->commit_small(rp, 3, n, nullptr, engine_stream(), nullptr, five);
            raw3 = rc == PORLA_OK;
        }
    } else {
        rc = kzg_commit_rows(three.data(), false, 3, n, outs, nullptr);
    }
    int rc2;
    if (raw3) {
        rc2 = msm_pair_end<Bn254G1>(MSM_AUDIT_SLOT, &five[3], &five[4]);
        pair_begun = false;
        if (rc2 == PORLA_OK) {
            Affine<Fp> aff[5];
            h_batch_xyzz_to_affine64<Fp>(five, 5, aff);
            for (int i = 0; i < 3; i++) h_affine_to_bytes<Fp>(outs + 64 * i, aff[i]);
            h_affine_to_bytes<Fp>(combined_mac, aff[3]);
            h_affine_to_bytes<Fp>(combined_align, aff[4]);
        }
    } else {
        rc2 = collect_pair();
    }
    if (rc) return rc;
    if (rc2) return rc2;
    if (!pair) {
        // more challenged rows than the single-launch pair takes (or none): the blocking pair form
        if ((rc = porla_bn254_audit_msm_pair_device(d_mac_store, d_align_store, d_mac_idx, d_mac_coef, n_macs, combined_mac, combined_align, stream)))
            return rc;
    }
    memcpy(align_value, outs, 64);
    memcpy(commitment, outs + 64, 64);
    memcpy(proof_h, outs + 128, 64);
    return PORLA_OK;
}
int porla_kzg_commit_batch_host(const uint8_t* rows, size_t n_rows, uint8_t* out) {
    if (n_rows && (!rows || !out)) { set_last_error("porla: null argument"); return PORLA_ERR_ARG; }
    int rc = ensure_device();
    if (rc) return rc;
    return kzg_commit_rows(rows, false, n_rows, kzg_n_samples(), out, nullptr);
}
// Server::HAdd for the KZG build, everything it computes before the level bookkeeping (Server.hpp:1388-1428): data_B2 = data * wt
// aligned mod p_icc, MAC_B2 = wt * MAC, MAC_align_B2 = Commit(alignment scalars of data_B2) -- align_MAC's compute_digest_from_srs
// (Server.hpp:531-560) on the scalars the device derived.  n_cols = NUM_CHUNKS = the SRS size.
int porla_kzg_hadd_host(const uint8_t* data_in, const uint8_t mac_in[64], size_t n_total, unsigned long long write_step,
                        uint8_t* data_b2_out, uint8_t mac_b2_out[64], uint8_t mac_align_b2_out[64]) {
    if (!data_in || !mac_in || !data_b2_out || !mac_b2_out || !mac_align_b2_out) { set_last_error("porla: null argument"); return PORLA_ERR_ARG; }
    const size_t n_cols = kzg_n_samples();
    if (n_cols == 0) { set_last_error("porla: SRS not initialised"); return PORLA_ERR_STATE; }
    std::vector<uint8_t> scalars(32 * n_cols);
    uint8_t wt[32];
    int rc = porla_icc_hadd_host(data_in, n_cols, n_total, write_step, 0, data_b2_out, scalars.data(), 0, wt);
    if (rc) return rc;
    if ((rc = porla_icc_mac_scale_host(mac_in, n_total, write_step, 0, mac_b2_out))) return rc;
    return kzg_commit_coalesced(scalars.data(), mac_align_b2_out);      // infinity + Commit(c) (bn254_add(B, align_value), B = infinity)
}

// rows are independent: device g of `devices` commits the row range [g R / G, (g+1) R / G) from its own host thread against its
// own resident copy of the SRS table; the results land in the caller's `out`, nothing is exchanged
int porla_kzg_commit_batch_host_multi(const uint8_t* rows, size_t n_rows, uint8_t* out, int devices) {
    if (n_rows && (!rows || !out)) { set_last_error("porla: null argument"); return PORLA_ERR_ARG; }
    int rc = ensure_device();
    if (rc) return rc;
    int visible = 0, first = 0;
    PORLA_HIP(hipGetDeviceCount(&visible));
    PORLA_HIP(hipGetDevice(&first));
    int G = devices <= 0 ? visible : (devices < visible ? devices : visible);
    if ((size_t)G > n_rows) G = (int)n_rows;
    if (G < 1) G = 1;
    const size_t len = kzg_n_samples();
    std::vector<int> rcs((size_t)G, PORLA_OK);
    std::vector<std::string> errs((size_t)G);
    auto worker = [&](int d) {
        if (hipSetDevice((first + d) % visible) != hipSuccess) { rcs[d] = PORLA_ERR_HIP; errs[d] = "porla: hipSetDevice failed"; return; }
        size_t lo, hi;
        porla_shard_range(n_rows, d, G, &lo, &hi);
        rcs[d] = kzg_commit_rows(rows + lo * len * 32, false, hi - lo, len, out + 64 * lo, nullptr);
        if (rcs[d]) errs[d] = porla_gpu_last_error();
    };
    std::vector<std::thread> th;
    for (int d = 1; d < G; d++) th.emplace_back(worker, d);
    worker(0);
    for (auto& t : th) t.join();
    if (G > 1) (void)hipSetDevice(first);
    for (int d = 0; d < G; d++) if (rcs[d]) { set_last_error(errs[d]); return rcs[d]; }
    return PORLA_OK;
}
int porla_kzg_set_commit_window(int window_bits) {
    std::lock_guard<std::mutex> lk(g_kzg.mu);
    if (window_bits != g_kzg.commit_window) { g_kzg.commit_window = window_bits; g_kzg.version++; }
    return PORLA_OK;
}
// frees the HBM copies that belong to the KZG state (SRS, its window-multiples table -- 56 GB by default --, the one-point
// tables of the client-side batches and scratch); they are rebuilt by the next call that needs them
int porla_kzg_release_device_memory(void) {
    // the host batches' staging buffers first, outside g_kzg.mu: a host batch holds its staging mutex while the device entry it
    // calls takes g_kzg.mu
    kzg_client_staging_release();
    std::lock_guard<std::mutex> lk(g_kzg.mu);
    int cur = 0;
    (void)hipGetDevice(&cur);
    for (KzgDev* kd : g_kzg.devs.snapshot()) {
        // a commit that has let the state go still holds its table's mutex
        std::lock_guard<std::mutex> l1(kd->fb.mu), l2(kd->fb_g.mu), l3(kd->fb_h.mu), l4(kd->fb_gh.mu);
        (void)hipSetDevice(kd->device);
        kd->fb.release();
        kd->fb_g.release();
        kd->fb_h.release();
        kd->fb_gh.release();
        kd->d_srs.release();
        kd->d_eval.release();
        kd->d_tau29.release();
        kd->tau29_n = 0;
        kd->d_tau29w.release();
        kd->tau29w_n = 0;
        kd->srs_version = kd->g_version = kd->h_version = kd->gh_version = 0;
    }
    (void)hipSetDevice(cur);
    return PORLA_OK;
}

int porla_kzg_commit_shape(int* window_bits, int* windows) {
    std::lock_guard<std::mutex> lk(g_kzg.mu);
    int dev = 0;
    (void)hipGetDevice(&dev);
    const KzgDev* kd = nullptr;
    for (const KzgDev* d : g_kzg.devs.snapshot()) if (d->device == dev) kd = d;
    if (window_bits) *window_bits = kd ? kd->fb.c : 0;
    if (windows) *windows = kd ? kd->fb.W : 0;
    return PORLA_OK;
}

}  // extern "C"
