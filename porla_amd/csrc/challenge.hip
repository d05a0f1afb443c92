// AES on the device (include/porla_gpu.h: porla_mac_prf_*, porla_client_prf_runs, porla_audit_challenge_*,
// porla_audit_complement_scalar_*, porla_diag_audit_walk).  The definitions are challenge_host.hpp's, compiled here for both sides;
// this unit adds the three kernels and the entry points around them.  Every device call is one upload of a host-built list and one
// launch on the caller's stream:
//
//   k_mac_prf          one lane per AES block, 256 per work-group; the run a work-group starts in is searched once per work-group
//   k_audit_challenge  one lane per point, grid.y = request; a lane recomputes the one or two stream blocks its point reads
//   k_audit_scalar     one work-group per request; lanes stride over the points, exact 192-bit sums joined through LDS
//
// All three fill the one 1 KiB table (te0) in LDS from constant memory and take no other table.
#include "batch_host.hpp"
#include "challenge_host.hpp"

#include <cstddef>
#include <cstring>
#include <string>

namespace porla {

using namespace chal;

static const AesTe0 h_te0 = aes_make_te0();
__constant__ AesTe0 c_te0 = aes_make_te0();

constexpr unsigned CHAL_THREADS = 256;

// ---------------------------------------------------------------- kernels
// runs[r] covers slots [off[r], off[r + 1]); off[n_runs] = total
__global__ __launch_bounds__(256) void k_mac_prf(AesRk rk, const PrfRun* __restrict__ runs, const uint64_t* __restrict__ off,
                                                 uint32_t n_runs, uint64_t total, uint4* __restrict__ out) {
    __shared__ uint32_t te0[256];
    __shared__ uint32_t s_r0;
    te0[threadIdx.x] = c_te0.v[threadIdx.x];
    const uint64_t base = (uint64_t)blockIdx.x * CHAL_THREADS;
    if (threadIdx.x == 0) {
        uint32_t lo = 0, hi = n_runs - 1;                  // the last run that begins at or before the work-group's first slot
        while (lo < hi) {
            const uint32_t mid = (lo + hi + 1) >> 1;
            if (off[mid] <= base) lo = mid; else hi = mid - 1;
        }
        s_r0 = lo;
    }
    __syncthreads();
    const uint64_t slot = base + threadIdx.x;
    if (slot >= total) return;
    uint32_t r = s_r0;
    while (slot >= off[r + 1]) r++;                        // slot < total = off[n_runs]: stops inside the list
    uint32_t o[4];
    prf_run_slot(te0, rk, runs[r], slot - off[r], o);
    out[slot] = make_uint4(o[0], o[1], o[2], o[3]);
}

// one request of the challenge and scalar kernels
struct ChalLevel {
    uint64_t data_x, data_y, mac_x, mac_y;
    uint32_t form, list_base, pad0, pad1;                  // list_base: the level's first entry in the list its form names
};
struct ChalDesc {
    AesRk rk;                                              // the seed's round keys
    WalkPlan plan;
    const int32_t* stream;                                 // porla_diag_audit_walk: the caller's ints instead of the PRG's
    uint64_t* idx64; uint32_t* coef64;
    uint64_t* idx32; uint32_t* coef32;
    uint64_t* mac_idx; uint32_t* mac_coef;
    uint64_t write_step;
    ChalLevel lv[AUDIT_MAX_LEVELS];                        // by plan entry, not by level
};

template <class S>
__device__ static inline void chal_emit(const ChalDesc& D, uint32_t p, const S& s) {
    const uint32_t a = walk_level_of(D.plan, p);
    const WalkLevel& L = D.plan.lv[a];
    const ChalLevel& C = D.lv[a];
    const uint32_t j = p - L.first_point, l = 1u << L.level;
    uint32_t index, coef;
    walk_point(L, j, s, &index, &coef);
    const bool y = index >= l;
    const uint32_t row = y ? index - l : index;
    if (D.mac_idx) D.mac_idx[p] = (y ? C.mac_y : C.mac_x) + row;
    if (D.mac_coef) D.mac_coef[p] = coef;
    uint64_t* idx = C.form ? D.idx32 : D.idx64;
    uint32_t* cf = C.form ? D.coef32 : D.coef64;
    if (idx) idx[C.list_base + j] = (y ? C.data_y : C.data_x) + row;
    if (cf) cf[C.list_base + j] = coef;
}

__global__ __launch_bounds__(256) void k_audit_challenge(const ChalDesc* __restrict__ descs) {
    __shared__ uint32_t te0[256];
    te0[threadIdx.x] = c_te0.v[threadIdx.x];
    __syncthreads();
    const ChalDesc& D = descs[blockIdx.y];
    const uint32_t p = blockIdx.x * CHAL_THREADS + threadIdx.x;
    if (p >= D.plan.n_points) return;
    if (D.stream) chal_emit(D, p, IntStream{D.stream});
    else chal_emit(D, p, PrgStream{te0, &D.rk});
}

struct ScalarDesc {
    AesRk rk;
    WalkPlan plan;
    uint64_t write_step;
};

__global__ __launch_bounds__(256) void k_audit_scalar(AesRk prf_rk, const ScalarDesc* __restrict__ descs, int curve, uint8_t* __restrict__ out) {
    __shared__ uint32_t te0[256];
    __shared__ unsigned long long cols[6];                 // column sums of the lanes' limbs: 256 lanes * 2^32 < 2^40 each
    te0[threadIdx.x] = c_te0.v[threadIdx.x];
    if (threadIdx.x < 6) cols[threadIdx.x] = 0;
    __syncthreads();
    const ScalarDesc& D = descs[blockIdx.x];
    const PrgStream s{te0, &D.rk};
    Acc192 A = {{0, 0, 0, 0, 0, 0}};
    for (uint32_t p = threadIdx.x; p < D.plan.n_points; p += CHAL_THREADS) {
        const WalkLevel& L = D.plan.lv[walk_level_of(D.plan, p)];
        complement_term(te0, prf_rk, L, p - L.first_point, s, D.write_step, curve, &A);
    }
    for (int k = 0; k < 6; k++) atomicAdd(&cols[k], (unsigned long long)A.v[k]);
    __syncthreads();
    if (threadIdx.x == 0) {
        Acc192 T;
        unsigned long long carry = 0;
        for (int k = 0; k < 6; k++) {
            const unsigned long long t = cols[k] + carry;  // < 2^40 + 2^32
            T.v[k] = (uint32_t)t;
            carry = t >> 32;
        }
        uint8_t be[32];
        acc_store_be(T, be);
        uint4* dst = (uint4*)(out + (size_t)blockIdx.x * 32);
        uint32_t w[8];
        for (int k = 0; k < 8; k++) w[k] = load_le32(be + 4 * k);
        dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
        dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
    }
}

// ---------------------------------------------------------------- host side
struct ChalWs {
    std::mutex mu;
    int device = -1;
    Buf list, io;                                          // io: the diagnostic's device images
    PinnedList h_list;
    UseFence fence;
};
static PerDevice<ChalWs> g_chal_ws;

static int chal_check_blocks(const char* who, const std::string& at, unsigned long long num_blocks) {
    if (num_blocks >= 2 && (num_blocks & (num_blocks - 1)) == 0 && num_blocks <= (1ull << 24)) return PORLA_OK;
    return bad_arg(who, at + "num_blocks must be a power of two, 2 .. 2^24");
}

// ---- the MAC PRF
static int prf_check(const char* who, const uint8_t* key16, const porla_prf_run* runs, size_t n_runs, const void* out, bool device,
                     uint64_t* total) {
    *total = 0;
    if (n_runs && !runs) return bad_arg(who, "runs is NULL");
    for (size_t r = 0; r < n_runs; r++) {
        if (runs[r].count > (1ull << 38) || (*total += runs[r].count) > (1ull << 38)) return bad_arg(who, "more than 2^38 values in one call");
    }
    if (n_runs > 0xffffffffull) return bad_arg(who, "more than 2^32 - 1 runs");
    if (*total == 0) return PORLA_OK;
    if (!key16) return bad_arg(who, "key16 is NULL");
    if (!out) return bad_arg(who, device ? "d_out is NULL" : "out is NULL");
    if (device && ((uintptr_t)out & 15u)) return bad_arg(who, "d_out is not 16-byte aligned");
    return PORLA_OK;
}

static int prf_enqueue(ChalWs* ws, const AesRk& rk, const porla_prf_run* runs, size_t n_runs, uint64_t total, void* d_out, hipStream_t stream) {
    int rc;
    const size_t runs_b = n_runs * sizeof(PrfRun), bytes = runs_b + (n_runs + 1) * 8;
    if ((rc = ws->h_list.stage(bytes)) || (rc = ws->list.ensure(bytes))) return rc;
    memcpy(ws->h_list.h, runs, runs_b);
    uint64_t* off = (uint64_t*)((uint8_t*)ws->h_list.h + runs_b);
    off[0] = 0;
    for (size_t r = 0; r < n_runs; r++) off[r + 1] = off[r] + runs[r].count;
    if ((rc = ws->h_list.send(ws->list.p, bytes, stream))) return rc;
    const uint64_t blocks = (total + CHAL_THREADS - 1) / CHAL_THREADS;      // <= 2^31
    ProfScope ps("mac_prf", stream);
    hipLaunchKernelGGL(k_mac_prf, dim3((unsigned)blocks), dim3(CHAL_THREADS), 0, stream, rk, (const PrfRun*)ws->list.p,
                       (const uint64_t*)((uint8_t*)ws->list.p + runs_b), (uint32_t)n_runs, total, (uint4*)d_out);
    PORLA_HIP(hipGetLastError());
    return PORLA_OK;
}

// ---- the challenge
struct ChalPlanned {
    WalkPlan plan;
    ChalLevel lv[AUDIT_MAX_LEVELS];
    uint64_t n64, n32;
};
static void chal_plan_lists(unsigned long long write_step, unsigned long long num_blocks, const porla_audit_level* levels, ChalPlanned* P) {
    walk_plan(write_step, num_blocks, &P->plan);
    P->n64 = P->n32 = 0;
    for (uint32_t a = 0; a < P->plan.n_levels; a++) {
        const WalkLevel& L = P->plan.lv[a];
        const porla_audit_level& U = levels[L.level];
        uint64_t& n = U.form ? P->n32 : P->n64;
        P->lv[a] = ChalLevel{U.data_x, U.data_y, U.mac_x, U.mac_y, (uint32_t)U.form, (uint32_t)n, 0, 0};
        n += L.n;
    }
}
template <class S>
static void chal_info(const ChalPlanned& P, const S& s, porla_audit_challenge_info* I) {
    memset(I, 0, sizeof *I);
    I->n64 = P.n64; I->n32 = P.n32; I->n_macs = P.plan.n_points;
    uint64_t z; int32_t a;
    walk_tail(P.plan, s, &z, &a, I->a_value);
    I->random_point = z; I->a_raw = a;
}
template <class S>
static void chal_walk_host(const ChalPlanned& P, const S& s, uint64_t* idx64, uint32_t* coef64, uint64_t* idx32, uint32_t* coef32,
                           uint64_t* mac_idx, uint32_t* mac_coef) {
    for (uint32_t a = 0; a < P.plan.n_levels; a++) {
        const WalkLevel& L = P.plan.lv[a];
        const ChalLevel& C = P.lv[a];
        const uint32_t l = 1u << L.level;
        for (uint32_t j = 0; j < L.n; j++) {
            uint32_t index, coef;
            walk_point(L, j, s, &index, &coef);
            const bool y = index >= l;
            const uint32_t row = y ? index - l : index;
            if (mac_idx) mac_idx[L.first_point + j] = (y ? C.mac_y : C.mac_x) + row;
            if (mac_coef) mac_coef[L.first_point + j] = coef;
            uint64_t* idx = C.form ? idx32 : idx64;
            uint32_t* cf = C.form ? coef32 : coef64;
            if (idx) idx[C.list_base + j] = (y ? C.data_y : C.data_x) + row;
            if (cf) cf[C.list_base + j] = coef;
        }
    }
}

static bool chal_plan_only(const porla_audit_challenge_req& R) {
    return !R.d_idx64 && !R.d_coef64 && !R.d_idx32 && !R.d_coef32 && !R.d_mac_idx && !R.d_mac_coef;
}

static int chal_check_levels(const char* who, const std::string& at, unsigned long long num_blocks, const porla_audit_level* levels) {
    if (int rc = chal_check_blocks(who, at, num_blocks)) return rc;
    if (!levels) return bad_arg(who, at + "levels is NULL");
    int height = 1;
    while ((1ull << (height - 1)) < num_blocks) height++;
    for (int i = 0; i < height; i++) {
        if (levels[i].form != 0 && levels[i].form != 1) return bad_arg(who, at + "level " + std::to_string(i) + ": form must be 0 (64-byte rows) or 1 (32-byte rows)");
        if (levels[i].pad != 0) return bad_arg(who, at + "level " + std::to_string(i) + ": pad must be 0");
    }
    return PORLA_OK;
}

// the checks, the plans and the infos of k requests; work = the requests that have lists to write
static int chal_prepare(const char* who, const porla_audit_challenge_req* reqs, size_t k, porla_audit_challenge_info* infos, bool device,
                        std::vector<ChalPlanned>* plans, std::vector<AesRk>* rks, size_t* work) {
    *work = 0;
    if (k && !reqs) return bad_arg(who, "reqs is NULL");
    if (k && !infos) return bad_arg(who, "infos_out is NULL");
    if (int rc = check_request_count(who, k)) return rc;
    plans->resize(k);
    rks->resize(k);
    for (size_t a = 0; a < k; a++) {
        const porla_audit_challenge_req& R = reqs[a];
        const std::string at = "request " + std::to_string(a) + ": ";
        if (int rc = chal_check_levels(who, at, R.num_blocks, R.levels)) return rc;
        ChalPlanned& P = (*plans)[a];
        chal_plan_lists(R.write_step, R.num_blocks, R.levels, &P);
        if (chal_plan_only(R)) continue;
        ++*work;
        if ((P.n64 && (!R.d_idx64 || !R.d_coef64)) || (P.n32 && (!R.d_idx32 || !R.d_coef32)) || !R.d_mac_idx || !R.d_mac_coef)
            return bad_arg(who, at + "a NULL list whose count is > 0");
        if (device && ((((uintptr_t)R.d_idx64 | (uintptr_t)R.d_idx32 | (uintptr_t)R.d_mac_idx) & 7u) ||
                       (((uintptr_t)R.d_coef64 | (uintptr_t)R.d_coef32 | (uintptr_t)R.d_mac_coef) & 3u)))
            return bad_arg(who, at + "an index list that is not 8-byte or a coefficient list that is not 4-byte aligned");
    }
    for (size_t a = 0; a < k; a++) {
        aes128_expand(h_te0.v, reqs[a].seed, &(*rks)[a]);
        chal_info((*plans)[a], PrgStream{h_te0.v, &(*rks)[a]}, &infos[a]);
    }
    return PORLA_OK;
}

static void chal_fill_desc(ChalDesc* D, const ChalPlanned& P, const AesRk* rk, const int32_t* stream, uint64_t* idx64, uint32_t* coef64,
                           uint64_t* idx32, uint32_t* coef32, uint64_t* mac_idx, uint32_t* mac_coef) {
    memset(D, 0, sizeof *D);
    if (rk) D->rk = *rk;
    D->plan = P.plan;
    D->stream = stream;
    D->idx64 = idx64; D->coef64 = coef64; D->idx32 = idx32; D->coef32 = coef32; D->mac_idx = mac_idx; D->mac_coef = mac_coef;
    memcpy(D->lv, P.lv, sizeof D->lv);
}

// descs: n of them staged in ws->h_list.h
static int chal_launch(ChalWs* ws, size_t n, uint32_t max_points, hipStream_t stream) {
    int rc;
    if ((rc = ws->list.ensure(n * sizeof(ChalDesc)))) return rc;
    if ((rc = ws->h_list.send(ws->list.p, n * sizeof(ChalDesc), stream))) return rc;
    ProfScope ps("audit_challenge", stream);
    hipLaunchKernelGGL(k_audit_challenge, dim3((max_points + CHAL_THREADS - 1) / CHAL_THREADS, (unsigned)n), dim3(CHAL_THREADS), 0, stream,
                       (const ChalDesc*)ws->list.p);
    PORLA_HIP(hipGetLastError());
    return PORLA_OK;
}

static int scalar_check(const char* who, const uint8_t* key16, const porla_audit_scalar_req* reqs, size_t k, int curve, const void* out,
                        bool device) {
    if (k && !key16) return bad_arg(who, "key16 is NULL");
    if (k && !reqs) return bad_arg(who, "reqs is NULL");
    if (k && !out) return bad_arg(who, device ? "d_scalars is NULL" : "scalars is NULL");
    if (device && ((uintptr_t)out & 15u)) return bad_arg(who, "d_scalars is not 16-byte aligned");
    if (curve != 0 && curve != 1) return bad_arg(who, "curve must be 0 (BN254 / KZG) or 1 (secp256k1 / IPA)");
    if (int rc = check_request_count(who, k)) return rc;
    for (size_t a = 0; a < k; a++)
        if (int rc = chal_check_blocks(who, "request " + std::to_string(a) + ": ", reqs[a].num_blocks)) return rc;
    return PORLA_OK;
}

}  // namespace porla

using namespace porla;

static_assert(sizeof(porla_prf_run) == PORLA_PRF_RUN_BYTES && sizeof(PrfRun) == sizeof(porla_prf_run), "porla_prf_run size");
static_assert(offsetof(porla_prf_run, level) == 0 && offsetof(porla_prf_run, index0) == 4 && offsetof(porla_prf_run, count) == 8 &&
              offsetof(porla_prf_run, time0) == 16 && offsetof(porla_prf_run, time_stride) == 24, "porla_prf_run offsets (include/porla_gpu.h)");
static_assert(offsetof(PrfRun, level) == 0 && offsetof(PrfRun, index0) == 4 && offsetof(PrfRun, count) == 8 && offsetof(PrfRun, time0) == 16 &&
              offsetof(PrfRun, time_stride) == 24, "PrfRun is porla_prf_run field for field");
static_assert(sizeof(porla_audit_level) == PORLA_AUDIT_LEVEL_BYTES, "porla_audit_level size");
static_assert(offsetof(porla_audit_level, data_x) == 0 && offsetof(porla_audit_level, data_y) == 8 && offsetof(porla_audit_level, mac_x) == 16 &&
              offsetof(porla_audit_level, mac_y) == 24 && offsetof(porla_audit_level, form) == 32 && offsetof(porla_audit_level, pad) == 36,
              "porla_audit_level offsets (include/porla_gpu.h)");
static_assert(sizeof(porla_audit_challenge_req) == PORLA_AUDIT_CHALLENGE_REQ_BYTES, "porla_audit_challenge_req size");
static_assert(offsetof(porla_audit_challenge_req, seed) == 0 && offsetof(porla_audit_challenge_req, write_step) == 16 &&
              offsetof(porla_audit_challenge_req, num_blocks) == 24 && offsetof(porla_audit_challenge_req, levels) == 32 &&
              offsetof(porla_audit_challenge_req, d_idx64) == 40 && offsetof(porla_audit_challenge_req, d_coef64) == 48 &&
              offsetof(porla_audit_challenge_req, d_idx32) == 56 && offsetof(porla_audit_challenge_req, d_coef32) == 64 &&
              offsetof(porla_audit_challenge_req, d_mac_idx) == 72 && offsetof(porla_audit_challenge_req, d_mac_coef) == 80,
              "porla_audit_challenge_req offsets (include/porla_gpu.h)");
static_assert(sizeof(porla_audit_challenge_info) == PORLA_AUDIT_CHALLENGE_INFO_BYTES, "porla_audit_challenge_info size");
static_assert(offsetof(porla_audit_challenge_info, n64) == 0 && offsetof(porla_audit_challenge_info, n32) == 8 &&
              offsetof(porla_audit_challenge_info, n_macs) == 16 && offsetof(porla_audit_challenge_info, random_point) == 24 &&
              offsetof(porla_audit_challenge_info, a_raw) == 32 && offsetof(porla_audit_challenge_info, pad) == 36 &&
              offsetof(porla_audit_challenge_info, a_value) == 40, "porla_audit_challenge_info offsets (include/porla_gpu.h)");
static_assert(sizeof(porla_audit_scalar_req) == PORLA_AUDIT_SCALAR_REQ_BYTES, "porla_audit_scalar_req size");
static_assert(offsetof(porla_audit_scalar_req, seed) == 0 && offsetof(porla_audit_scalar_req, write_step) == 16 &&
              offsetof(porla_audit_scalar_req, num_blocks) == 24, "porla_audit_scalar_req offsets (include/porla_gpu.h)");

extern "C" int porla_mac_prf_batch_device(const uint8_t key16[16], const porla_prf_run* runs, size_t n_runs, void* d_out, void* hip_stream) {
    static const char* const who = "porla_mac_prf_batch_device";
    uint64_t total;
    int rc = prf_check(who, key16, runs, n_runs, d_out, true, &total);
    if (rc) return rc;
    if (total == 0) return PORLA_OK;
    if ((rc = ensure_device())) return rc;
    ChalWs* ws = nullptr;
    if ((rc = g_chal_ws.get(&ws))) return rc;
    AesRk rk;
    aes128_expand(h_te0.v, key16, &rk);
    hipStream_t stream = (hipStream_t)hip_stream;
    return FencedCall(ws, stream).run([&] { return prf_enqueue(ws, rk, runs, n_runs, total, d_out, stream); });
}

extern "C" int porla_mac_prf_host(const uint8_t key16[16], const porla_prf_run* runs, size_t n_runs, uint8_t* out) {
    uint64_t total;
    int rc = prf_check("porla_mac_prf_host", key16, runs, n_runs, out, false, &total);
    if (rc || total == 0) return rc;
    AesRk rk;
    aes128_expand(h_te0.v, key16, &rk);
    for (size_t r = 0; r < n_runs; r++) {
        PrfRun R;
        memcpy(&R, &runs[r], sizeof R);
        for (uint64_t t = 0; t < R.count; t++, out += 16) {
            uint32_t o[4];
            prf_run_slot(h_te0.v, rk, R, t, o);
            for (int c = 0; c < 4; c++) store_le32(out + 4 * c, o[c]);
        }
    }
    return PORLA_OK;
}

extern "C" int porla_client_prf_runs(int kind, int block_id, unsigned long long write_step, int level, size_t n_total, porla_prf_run* runs_out,
                                     size_t max_runs, size_t* n_runs, size_t* n_values) {
    static const char* const who = "porla_client_prf_runs";
    if (kind != PORLA_PRF_UPDATE && kind != PORLA_PRF_REBUILD) return bad_arg(who, "kind must be PORLA_PRF_UPDATE or PORLA_PRF_REBUILD");
    if (!runs_out || !n_runs || !n_values) return bad_arg(who, "runs_out, n_runs or n_values is NULL");
    if (int rc = check_n_total(who, n_total, 30)) return rc;
    PrfRun tmp[32];
    size_t n;
    if (kind == PORLA_PRF_UPDATE) {
        if (level < 0 || level > 29 || ((size_t)1 << level) > n_total / 2) return bad_arg(who, "level must be 0 .. log2(n_total) - 1");
        if (write_step % n_total == 0) return bad_arg(who, "write_step % n_total == 0 is CRebuild's step, not an H update");
        if (max_runs < (size_t)level + 2) return bad_arg(who, "max_runs is too small: an update write has level + 2 runs");
        n = prf_runs_update(block_id, write_step, level, tmp);
    } else {
        if (max_runs < 3) return bad_arg(who, "max_runs is too small: a rebuild write has 3 runs");
        n = prf_runs_rebuild(block_id, write_step, n_total, tmp);
    }
    size_t values = 0;
    for (size_t r = 0; r < n; r++) values += tmp[r].count;
    memcpy(runs_out, tmp, n * sizeof(PrfRun));
    *n_runs = n;
    *n_values = values;
    return PORLA_OK;
}

extern "C" int porla_audit_challenge_host(const porla_audit_challenge_req* reqs, size_t k, porla_audit_challenge_info* infos_out) {
    std::vector<ChalPlanned> plans;
    std::vector<AesRk> rks;
    size_t work;
    int rc = chal_prepare("porla_audit_challenge_host", reqs, k, infos_out, false, &plans, &rks, &work);
    if (rc) return rc;
    for (size_t a = 0; a < k; a++) {
        const porla_audit_challenge_req& R = reqs[a];
        if (chal_plan_only(R)) continue;
        chal_walk_host(plans[a], PrgStream{h_te0.v, &rks[a]}, R.d_idx64, R.d_coef64, R.d_idx32, R.d_coef32, R.d_mac_idx, R.d_mac_coef);
    }
    return PORLA_OK;
}

extern "C" int porla_audit_challenge_batch_device(const porla_audit_challenge_req* reqs, size_t k, porla_audit_challenge_info* infos_out,
                                                  void* hip_stream) {
    std::vector<ChalPlanned> plans;
    std::vector<AesRk> rks;
    size_t work;
    int rc = chal_prepare("porla_audit_challenge_batch_device", reqs, k, infos_out, true, &plans, &rks, &work);
    if (rc) return rc;
    if (work == 0) return PORLA_OK;
    if ((rc = ensure_device())) return rc;
    ChalWs* ws = nullptr;
    if ((rc = g_chal_ws.get(&ws))) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    return FencedCall(ws, stream).run([&] {
        int r;
        if ((r = ws->h_list.stage(work * sizeof(ChalDesc)))) return r;
        ChalDesc* D = (ChalDesc*)ws->h_list.h;
        uint32_t max_points = 0;
        for (size_t a = 0; a < k; a++) {
            const porla_audit_challenge_req& R = reqs[a];
            if (chal_plan_only(R)) continue;
            chal_fill_desc(D++, plans[a], &rks[a], nullptr, R.d_idx64, R.d_coef64, R.d_idx32, R.d_coef32, R.d_mac_idx, R.d_mac_coef);
            if (plans[a].plan.n_points > max_points) max_points = plans[a].plan.n_points;
        }
        return chal_launch(ws, work, max_points, stream);
    });
}

static void scalar_descs(const porla_audit_scalar_req* reqs, size_t k, ScalarDesc* D) {
    for (size_t a = 0; a < k; a++) {
        aes128_expand(h_te0.v, reqs[a].seed, &D[a].rk);
        walk_plan(reqs[a].write_step, reqs[a].num_blocks, &D[a].plan);
        D[a].write_step = reqs[a].write_step;
    }
}

extern "C" int porla_audit_complement_scalar_host(const uint8_t key16[16], const porla_audit_scalar_req* reqs, size_t k, int curve,
                                                  uint8_t* scalars) {
    int rc = scalar_check("porla_audit_complement_scalar_host", key16, reqs, k, curve, scalars, false);
    if (rc || k == 0) return rc;
    AesRk prf_rk;
    aes128_expand(h_te0.v, key16, &prf_rk);
    std::vector<ScalarDesc> D(k);
    scalar_descs(reqs, k, D.data());
    for (size_t a = 0; a < k; a++) {
        const PrgStream s{h_te0.v, &D[a].rk};
        Acc192 A = {{0, 0, 0, 0, 0, 0}};
        for (uint32_t l = 0; l < D[a].plan.n_levels; l++)
            for (uint32_t j = 0; j < D[a].plan.lv[l].n; j++)
                complement_term(h_te0.v, prf_rk, D[a].plan.lv[l], j, s, D[a].write_step, curve, &A);
        acc_store_be(A, scalars + 32 * a);
    }
    return PORLA_OK;
}

extern "C" int porla_audit_complement_scalar_batch_device(const uint8_t key16[16], const porla_audit_scalar_req* reqs, size_t k, int curve,
                                                          void* d_scalars, void* hip_stream) {
    int rc = scalar_check("porla_audit_complement_scalar_batch_device", key16, reqs, k, curve, d_scalars, true);
    if (rc || k == 0) return rc;
    if ((rc = ensure_device())) return rc;
    ChalWs* ws = nullptr;
    if ((rc = g_chal_ws.get(&ws))) return rc;
    AesRk prf_rk;
    aes128_expand(h_te0.v, key16, &prf_rk);
    hipStream_t stream = (hipStream_t)hip_stream;
    return FencedCall(ws, stream).run([&] {
        int r;
        const size_t bytes = k * sizeof(ScalarDesc);
        if ((r = ws->h_list.stage(bytes)) || (r = ws->list.ensure(bytes))) return r;
        scalar_descs(reqs, k, (ScalarDesc*)ws->h_list.h);
        if ((r = ws->h_list.send(ws->list.p, bytes, stream))) return r;
        ProfScope ps("audit_scalar", stream);
        hipLaunchKernelGGL(k_audit_scalar, dim3((unsigned)k), dim3(CHAL_THREADS), 0, stream, prf_rk, (const ScalarDesc*)ws->list.p, curve,
                           (uint8_t*)d_scalars);
        PORLA_HIP(hipGetLastError());
        return (int)PORLA_OK;
    });
}

extern "C" int porla_diag_audit_walk(const int32_t* stream_ints, size_t n_ints, unsigned long long write_step, unsigned long long num_blocks,
                                     const porla_audit_level* levels, int on_device, uint64_t* idx64, uint32_t* coef64, uint64_t* idx32,
                                     uint32_t* coef32, uint64_t* mac_idx, uint32_t* mac_coef, porla_audit_challenge_info* info) {
    static const char* const who = "porla_diag_audit_walk";
    if (!stream_ints || !idx64 || !coef64 || !idx32 || !coef32 || !mac_idx || !mac_coef || !info) return bad_arg(who, "a NULL argument");
    if (int rc = chal_check_levels(who, "", num_blocks, levels)) return rc;
    ChalPlanned P;
    chal_plan_lists(write_step, num_blocks, levels, &P);
    if (n_ints <= P.plan.pos_end || n_ints <= P.plan.n_points) return bad_arg(who, "n_ints does not cover the ints the walk and its tail read");
    const IntStream s{stream_ints};
    chal_info(P, s, info);
    if (!on_device) {
        chal_walk_host(P, s, idx64, coef64, idx32, coef32, mac_idx, mac_coef);
        return PORLA_OK;
    }
    int rc;
    if ((rc = ensure_device())) return rc;
    ChalWs* ws = nullptr;
    if ((rc = g_chal_ws.get(&ws))) return rc;
    hipStream_t st = engine_stream();
    // the device images: the ints, then three index lists and three coefficient lists of n_points entries each
    const size_t np = P.plan.n_points, ints_b = (n_ints * 4 + 7) & ~(size_t)7;
    FencedCall call(ws, st);
    rc = call.run([&] {
        int r;
        if ((r = ws->io.ensure(ints_b + np * 36)) || (r = ws->h_list.stage(sizeof(ChalDesc)))) return r;
        uint8_t* base = (uint8_t*)ws->io.p;
        uint64_t* d_idx = (uint64_t*)(base + ints_b);
        uint32_t* d_cf = (uint32_t*)(base + ints_b + np * 24);
        PORLA_HIP(hipMemcpyAsync(base, stream_ints, n_ints * 4, hipMemcpyHostToDevice, st));
        chal_fill_desc((ChalDesc*)ws->h_list.h, P, nullptr, (const int32_t*)base, d_idx, d_cf, d_idx + np, d_cf + np, d_idx + 2 * np, d_cf + 2 * np);
        if ((r = chal_launch(ws, 1, (uint32_t)np, st))) return r;
        if (P.n64) {
            PORLA_HIP(hipMemcpyAsync(idx64, d_idx, P.n64 * 8, hipMemcpyDeviceToHost, st));
            PORLA_HIP(hipMemcpyAsync(coef64, d_cf, P.n64 * 4, hipMemcpyDeviceToHost, st));
        }
        if (P.n32) {
            PORLA_HIP(hipMemcpyAsync(idx32, d_idx + np, P.n32 * 8, hipMemcpyDeviceToHost, st));
            PORLA_HIP(hipMemcpyAsync(coef32, d_cf + np, P.n32 * 4, hipMemcpyDeviceToHost, st));
        }
        PORLA_HIP(hipMemcpyAsync(mac_idx, d_idx + 2 * np, np * 8, hipMemcpyDeviceToHost, st));
        PORLA_HIP(hipMemcpyAsync(mac_coef, d_cf + 2 * np, np * 4, hipMemcpyDeviceToHost, st));
        return (int)PORLA_OK;
    });
    if (rc) return rc;
    PORLA_HIP(hipStreamSynchronize(st));       // (the lock is held to here: the images are this call's until the copies are done)
    return PORLA_OK;
}
