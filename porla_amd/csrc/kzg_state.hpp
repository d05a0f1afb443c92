// The KZG plug-in's state (key, SRS, the per-device HBM copies and tables) and the one way to its resident SRS table, shared by
// kzg_abi.hip (the Go boundary), kzg_client_batch.hip, kzg_server.hip and the batched entry points that commit against the SRS.
#pragma once
#include "batch_host.hpp"
#include "pairing_host.hpp"

#include <type_traits>

namespace porla {

// HBM copies, one set per device that has been used (the row-range splitter of porla_kzg_commit_batch_host_multi runs one host thread
// per device; a process pinned to one GPU only ever creates its own)
struct KzgDev {
    int device = -1;
    Buf d_srs;                    // resident Montgomery copy of the SRS
    unsigned long long srs_version = 0, g_version = 0, h_version = 0, gh_version = 0;   // what the tables below were built from
    FixedBase<Bn254G1> fb;        // window-multiples table of the SRS (fixed_base.hip.h)
    FixedBase<Bn254G1> fb_g, fb_h;   // one-point tables of G1[0] and of the MAC hiding base (client-side batches)
    FixedBase<Bn254G1> fb_gh;        // the two of them as one 2-point table (porla_kzg_mac_batch_device)
    Buf d_eval;                   // scratch: evaluated scalars of a digest batch
    Buf d_tau29;                  // powers of tau in 29-bit limbs (k_kzg_eval_rows_lazy), for the key and row length below
    Fe<Bn254Fr> tau29_tau;
    uint32_t tau29_n = 0;
    Buf d_tau29w;                 // per power two entries, tau^i and 2^256 tau^i (retrieve_batch.hip: k_rt_eval_lazy), kept as d_tau29 is
    Fe<Bn254Fr> tau29w_tau;
    uint32_t tau29w_n = 0;
};

struct KzgState {
    std::mutex mu;
    bool have_key = false;
    Fe<Bn254Fr> tau, alpha;       // Montgomery form mod r
    uint8_t tau_raw[32] = {0};    // big.Int of the raw key bytes, reduced mod r, big-endian
    long long n_samples = 0;
    std::vector<Affine<Bn254Fp>> srs;   // SRS.G1, Montgomery form (host copy)
    unsigned long long version = 1;   // bumped whenever the SRS, the hiding base or the table window changes
    int commit_window = 0;        // 0 = automatic
    PerDevice<KzgDev> devs;
    bool have_g2 = false;
    G2Affine g2[2];               // SRS.G2[0], SRS.G2[1]
    Affine<Bn254Fp> h_mac;        // MAC hiding base (main.go:28,58-59)
};
extern KzgState g_kzg;            // kzg_server.hip

// the current device's copies (g_kzg.mu held)
int current_dev(KzgDev** out);
// make this device's HBM copies (Montgomery SRS + its window-multiples table) current; g_kzg.mu held by the caller
int refresh_srs_locked(KzgDev** out);

// the SRS size as the state holds it now (g_kzg.mu: init_SRS / init_SRS_from_data may run on another thread)
static inline size_t kzg_n_samples() {
    std::lock_guard<std::mutex> lk(g_kzg.mu);
    return (size_t)g_kzg.n_samples;
}

// the refusal of a call that needs the SRS before there is one
static inline int kzg_no_srs() {
    set_last_error("porla: SRS not initialised (call init_SRS / init_SRS_from_data first)");
    return PORLA_ERR_STATE;
}

// the SRS size as the width of a commitment row, refused before there is an SRS and above what a row takes
static inline int kzg_row_width(size_t* n) {
    *n = kzg_n_samples();
    if (*n == 0) return kzg_no_srs();
    if (*n > 0xffffu) { set_last_error("porla: SRS longer than a commitment row takes"); return PORLA_ERR_STATE; }
    return PORLA_OK;
}

// The one way to the resident SRS table.  Lock order: the state, then a table; a registry's mutex (PerDevice) is a leaf, held for
// lookup only.  acquire() makes the table current under the state's lock and takes the table's mutex BEFORE the state is let go, so
// that neither init_SRS_from_data / porla_kzg_set_commit_window nor porla_kzg_release_device_memory can rebuild or free the table
// between the checks and the commit (compute_digest_from_srs comes from 8 pool threads, Server.hpp:550-560).  The table's mutex is
// held until the guard dies.
struct SrsTable {
    static constexpr size_t N_SAMPLES = ~(size_t)0;    // acquire(): rows of n_samples coefficients, as the state holds it at the time
    FixedBase<Bn254G1>* fb = nullptr;
    size_t len = 0;               // coefficients per row, resolved and <= the SRS size
    std::unique_lock<std::mutex> lk;
    int acquire(size_t want = N_SAMPLES);
};

// kzg.Commit(f, srs) (main.go:114,164) for `n_rows` coefficient rows of host or device memory: fixed-base table path
int kzg_commit_rows(const uint8_t* rows, bool device_ptrs, size_t n_rows, size_t len, uint8_t* out, hipStream_t stream,
                    bool guest_room = false);
// kzg_abi.hip: one row per call, coalesced with the calls it meets (compute_digest_from_srs)
int kzg_commit_coalesced(const uint8_t* row, uint8_t out[64]);
// kzg_abi.hip: y = f(z) and the quotient h = (f - y)/(X - z) of create_proof (main.go:153-175), on the host
void kzg_open_rows(const uint8_t* d, size_t n, unsigned long long random_point, uint8_t* h_row, uint8_t point[32], uint8_t claim[32]);
// kzg_client_batch.hip: a table of one or two points, rebuilt from `points` if it was built from an older state (g_kzg.mu held); x *
// 2^270 mod r as canonical words, x in the Montgomery form
int kzg_small_table(FixedBase<Bn254G1>& fb, unsigned long long& built_version, std::initializer_list<Affine<Bn254Fp>> points);
void kzg_to270(const Fe<Bn254Fr>& xm, uint32_t dst[8]);
// kzg_client_batch.hip: the dot-product evaluations' table of powers of tau, one entry per power or (wide) two (g_kzg.mu held)
std::vector<uint32_t> kzg_tau29_table(uint32_t n_coeffs, bool wide);
// kzg_client_batch.hip: frees the host batches' staging buffers (takes their mutexes: call it outside g_kzg.mu)
void kzg_client_staging_release();

// commit n_rows contiguous rows of n_samples coefficients against the resident SRS table, leave the row sums in the table's partials,
// and run `then(sums, S)` (row r at sums[r * S]) under the table's lock before its fence is recorded again
template <class Then>
static int kzg_commit_rows_raw(const uint8_t* d_rows, size_t n_rows, hipStream_t stream, Then then) {
    SrsTable t;
    int rc = t.acquire();
    if (rc) return rc;
    if (t.len == 0) { set_last_error("porla: more coefficients than SRS points"); return PORLA_ERR_STATE; }
    return commit_then_locked(*t.fb, d_rows, n_rows, t.len, stream, then);
}
// the same for either build of a write batch: the caller's fixed base (IPA), or fb == nullptr: the resident SRS (KZG, its own width)
template <class C, class Then>
static int commit_rows_then(FixedBase<C>* fb, const uint8_t* d_rows, size_t n_rows, size_t n_coeffs, hipStream_t stream, Then then) {
    if constexpr (std::is_same<C, Bn254G1>::value)
        if (!fb) return kzg_commit_rows_raw(d_rows, n_rows, stream, then);
    return commit_then(*fb, d_rows, n_rows, n_coeffs, stream, then);
}

// for the batched verifier (kzg_verify_batch.hip): G1[0] as 64 bytes big-endian affine, PORLA_ERR_STATE without an SRS and its G2
// points; verify_proof's predicate on a record's commitment | proof_h | point | claim (192 bytes), without its message; and the
// folded check e(P, G2[0]) * e(-Q, G2[1]) == 1 over 64-byte big-endian affine P and Q (coordinates < p)
int kzg_verify_base(uint8_t g_be[64]);
bool kzg_opening_holds(const uint8_t rec[192]);
bool kzg_folded_opening_holds(const uint8_t p_be[64], const uint8_t q_be[64]);

}  // namespace porla
