// The 14 cgo symbols of the reference's libmultiexp.so (porla/Utils/libmultiexp.h:71-84, generated from
// porla/main.go:31-230), re-implemented over the MI355X engine.  Same names, same GoSlice ABI, same
// (absent) error behaviour: failures of the GPU path print one line and abort(), as there is no error
// channel at this boundary and silently wrong MACs would be worse.
//
//   MSMs (compute_multi_exp, compute_digest_from_srs, create_proof)  -> HIP kernels (engine.hip / msm.hip.h)
//   single-point ops, Horner evaluation, pairing check               -> host (latency-bound, 64-byte operands)
// Beside them only what stands at the same boundary: the coalescing front of compute_digest_from_srs, the pairing diagnostics and
// the batched verifier's accessors.  The state is kzg_state.hpp's; the batched entry points are in kzg_client_batch.hip and
// kzg_server.hip.
#include "kzg_state.hpp"
#include "host_fold64.hpp"
#include "../../include/libmultiexp.h"

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <random>
#include <string>
#include <vector>

using namespace porla;
using Fp = Bn254Fp;
using Fr = Bn254Fr;

namespace {

[[noreturn]] void die(const char* where, int rc) {
    fprintf(stderr, "libmultiexp (MI355X): %s failed (%d): %s\n", where, rc, porla_gpu_last_error());
    abort();
}

Affine<Fp> generator() {
    Affine<Fp> a;
    a.x = fe_zero<Fp>(); a.x.v[0] = 1; a.x = fe_to_mont<Fp>(a.x);
    a.y = fe_zero<Fp>(); a.y.v[0] = 2; a.y = fe_to_mont<Fp>(a.y);
    return a;
}

// G1Affine.Unmarshal on a 64-byte slice (main.go:130,144,198,...): flag bits 00 -> uncompressed.
// gnark would treat flag bits 10/11/01 as a compressed encoding; Porla never produces them in
// 64-byte buffers (coordinates are < p < 2^254), they are decoded the gnark way for completeness.
Affine<Fp> unmarshal64(const uint8_t* b) {
    uint8_t flags = b[0] & 0xC0;
    if (flags == 0x00) return h_affine_from_bytes<Fp>(b);
    Affine<Fp> a;
    if (flags == 0x40 || !g1_decompress(b, &a)) { a.x = fe_zero<Fp>(); a.y = fe_zero<Fp>(); }
    return a;
}

void fr_plain_be(uint8_t out[32], const Fe<Fr>& a) { h_fe_to_be<Fr>(out, a); }

// compute_digest_from_srs arrives ONE row per call from up to 8 pool threads at once (Server.hpp:550-560, 1054-1078, 1530-1535):
// calls that meet here are coalesced -- whoever finds no batch in progress becomes the leader, takes every row queued so far
// (its own included), commits them in ONE launch (FixedBase::commit_small) and hands the results back; rows that arrive while a
// batch is in flight form the next one.  A lone caller pays nothing for it (a batch of one).
struct CommitQueue {
    struct Item { const uint8_t* row; uint8_t* out; int rc; std::atomic<bool> done; std::string err; };
    std::mutex mu;
    std::condition_variable cv;
    std::vector<Item*> q;
    std::atomic<bool> leader{false};
    bool contended = false;      // a caller found a batch in flight since the last batch was formed
};
CommitQueue cq;
constexpr int COMMIT_LINGER_US = 12;
}  // namespace

int porla::kzg_commit_coalesced(const uint8_t* row, uint8_t out[64]) {
    CommitQueue::Item it;
    it.row = row; it.out = out; it.rc = PORLA_OK; it.done.store(false);
    std::unique_lock<std::mutex> lk(cq.mu);
    cq.q.push_back(&it);
    for (;;) {
        if (it.done.load()) { if (it.rc) set_last_error(it.err); return it.rc; }
        if (cq.leader.load()) { cq.contended = true; cq.cv.wait(lk); continue; }
        cq.leader = true;
        if (cq.contended) {
            // Several threads are calling (the reference's pool threads, Server.hpp:550-560): the callers of the batch that just
            // finished are on their way back.  Without a pause the first one back leads a batch of whoever happens to be queued
            // (sizes 1 .. 8 evenly); 12 us let them form ONE batch: 59 k -> 87 k
            // commits/s from 8 C threads, 33 k -> 46 k from 4 (profiles/r02_t_commit_queue_linger.txt).  A lone caller never waits.
            cq.contended = false;
            lk.unlock();
            const auto t0 = std::chrono::steady_clock::now();
            while (std::chrono::steady_clock::now() - t0 < std::chrono::microseconds(COMMIT_LINGER_US)) __builtin_ia32_pause();
            lk.lock();
        }
        std::vector<CommitQueue::Item*> batch;
        const size_t take = cq.q.size() < (size_t)FB_SMALL_MAX_ROWS ? cq.q.size() : (size_t)FB_SMALL_MAX_ROWS;
        batch.assign(cq.q.begin(), cq.q.begin() + (long)take);
        cq.q.erase(cq.q.begin(), cq.q.begin() + (long)take);
        lk.unlock();
        int rc;
        std::string err;
        {
            SrsTable t;
            rc = t.acquire();
            if (!rc) {
                const size_t len = t.len;
                const uint8_t* rp[FB_SMALL_MAX_ROWS];
                uint8_t* op[FB_SMALL_MAX_ROWS];
                for (size_t i = 0; i < batch.size(); i++) { rp[i] = batch[i]->row; op[i] = batch[i]->out; }
                if (FixedBase<Bn254G1>::small_ok(batch.size(), len)) {
                    rc = t.fb->commit_small(rp, batch.size(), len, op, engine_stream());
                } else {
                    for (size_t i = 0; i < batch.size() && !rc; i++) rc = t.fb->commit_host(rp[i], 1, len, len * 32, op[i], engine_stream());
                }
            }
            if (rc) err = porla_gpu_last_error();
        }
        lk.lock();
        for (auto* b : batch) { b->rc = rc; b->err = err; b->done.store(true, std::memory_order_release); }
        cq.leader.store(false, std::memory_order_release);
        cq.cv.notify_all();
    }
}

namespace {
void copy_out(GoSlice* dst, const uint8_t* src, size_t n) {  // Go copy(): min(len(dst), len(src))
    size_t m = (size_t)(dst->len < 0 ? 0 : dst->len);
    if (m > n) m = n;
    memcpy(dst->data, src, m);
}
}  // namespace

// main.go:153-175 without the commitments: y = f(z) and the quotient h = (f - y)/(X - z) of the polynomial whose n coefficients are
// given as 32-byte big-endian values (fr.SetBytes: reduced mod r); h_row receives n coefficients (the top one zero)
void porla::kzg_open_rows(const uint8_t* d, size_t n, unsigned long long random_point, uint8_t* h_row, uint8_t point[32], uint8_t claim[32]) {
    uint8_t zb[32] = {0};
    for (int i = 0; i < 8; i++) zb[31 - i] = (uint8_t)(random_point >> (8 * i));
    // Horner and the synthetic division in 4 x 64-bit limbs (host_fold64.hpp): the coefficients and the running values stay
    // PLAIN residues, only z is in the Montgomery form -- a Montgomery product of a plain value with z R is the plain product,
    // so the 2 n products need no conversion on either side (510 products in the 8 x 32-bit code before)
    static const Fp64<Fr> F;
    typedef Fp64<Fr>::E E64;
    auto from_be_plain = [&](const uint8_t* b) {          // fr.SetBytes: big-endian, reduced mod r
        uint64_t t[4];
        for (int i = 0; i < 4; i++) {
            uint64_t w = 0;
            for (int k = 0; k < 8; k++) w = (w << 8) | b[8 * (3 - i) + k];
            t[i] = w;
        }
        E64 v = F.cond_sub(t, 0);
        for (int q = 0; q < 5; q++) v = F.cond_sub(v.v, 0);      // 2^256 < 6 r
        return v;
    };
    auto to_be = [&](uint8_t* out, const E64& a) {
        for (int i = 0; i < 4; i++)
            for (int k = 0; k < 8; k++) out[8 * (3 - i) + k] = (uint8_t)(a.v[i] >> (8 * (7 - k)));
    };
    Fe<Fr> r2f;
    for (int i = 0; i < 8; i++) r2f.v[i] = Fr::R2[i];
    const E64 z = from_be_plain(zb);
    const E64 zM = F.mul(z, Fp64<Fr>::from(r2f));          // z R
    std::vector<E64> f(n);
    for (size_t i = 0; i < n; i++) f[i] = from_be_plain(d + 32 * i);
    E64 y;
    for (int i = 0; i < 4; i++) y.v[i] = 0;
    for (size_t i = n; i-- > 0;) y = F.add(F.mul(y, zM), f[i]);
    // synthetic division: h[n-2] = f[n-1]; h[i-1] = f[i] + z*h[i]
    memset(h_row, 0, 32 * n);
    E64 carry;
    for (int i = 0; i < 4; i++) carry.v[i] = 0;
    for (size_t i = n; i-- > 1;) {
        carry = F.add(F.mul(carry, zM), f[i]);
        to_be(&h_row[32 * (i - 1)], carry);
    }
    to_be(point, z);
    to_be(claim, y);
}

extern "C" {

// main.go:31-40
void init_key(GoSlice* tau_key_in, GoSlice* alpha_key_in) {
    std::lock_guard<std::mutex> lk(g_kzg.mu);
    g_kzg.tau = h_fe_from_be_var<Fr>((const uint8_t*)tau_key_in->data, (size_t)tau_key_in->len);
    g_kzg.alpha = h_fe_from_be_var<Fr>((const uint8_t*)alpha_key_in->data, (size_t)alpha_key_in->len);
    fr_plain_be(g_kzg.tau_raw, g_kzg.tau);
    g_kzg.have_key = true;
}

// main.go:42-60.  kzg.NewSRS: G1[i] = tau^i * G, G2 = {G2gen, tau * G2gen}; WriteTo: 4-byte BE count,
// n compressed G1 (32 B), 2 compressed G2 (64 B) = 32n + 132 bytes (Client.hpp:350-357).
void init_SRS(GoInt SRS_size, GoSlice* out, GoInt64* out_len) {
    std::lock_guard<std::mutex> lk(g_kzg.mu);
    if (!g_kzg.have_key || SRS_size <= 0) { fprintf(stderr, "libmultiexp (MI355X): init_SRS before init_key\n"); abort(); }
    g_kzg.n_samples = SRS_size;
    g_kzg.srs.assign((size_t)SRS_size, Affine<Fp>());
    Affine<Fp> G = generator();
    Fe<Fr> t = fe_one<Fr>();
    std::vector<XYZZ<Fp>> proj((size_t)SRS_size);
    for (long long i = 0; i < SRS_size; i++) {
        uint32_t k[8];
        h_fe_to_plain<Fr>(k, t);
        static HostFixedBase<Fp> fb_gen;              // every power of tau multiplies the same generator: table of its multiples
        proj[(size_t)i] = fb_gen.mul(G, k);
        t = fe_mul<Fr>(t, g_kzg.tau);
    }
    h_batch_xyzz_to_affine64<Fp>(proj.data(), (size_t)SRS_size, g_kzg.srs.data());       // one inversion per 64 points
    uint32_t tau_plain[8];
    h_fe_to_plain<Fr>(tau_plain, g_kzg.tau);
    g_kzg.g2[0] = g2_generator();
    g_kzg.g2[1] = g2_scalar_mul(g_kzg.g2[0], tau_plain);
    g_kzg.have_g2 = true;

    std::vector<uint8_t> blob(4 + 32 * (size_t)SRS_size + 128);
    blob[0] = (uint8_t)(SRS_size >> 24); blob[1] = (uint8_t)(SRS_size >> 16);
    blob[2] = (uint8_t)(SRS_size >> 8);  blob[3] = (uint8_t)SRS_size;
    for (long long i = 0; i < SRS_size; i++) g1_compress(&blob[4 + 32 * (size_t)i], g_kzg.srs[(size_t)i]);
    g2_compress(&blob[4 + 32 * (size_t)SRS_size], g_kzg.g2[0]);
    g2_compress(&blob[4 + 32 * (size_t)SRS_size + 64], g_kzg.g2[1]);
    if (out_len) *out_len = (GoInt64)blob.size();
    copy_out(out, blob.data(), blob.size());

    // MAC hiding h = random * G1[0] (main.go:52-59: fr.SetRandom -> crypto/rand; non-reproducible by design)
    std::random_device rd;
    uint8_t rb[32];
    for (int i = 0; i < 32; i += 4) { uint32_t v = rd(); memcpy(rb + i, &v, 4); }
    Fe<Fr> rnd = h_fe_from_be<Fr>(rb);
    uint32_t k[8];
    h_fe_to_plain<Fr>(k, rnd);
    g_kzg.h_mac = h_xyzz_to_affine64<Fp>(h_scalar_mul64<Fp>(g_kzg.srs[0], k));

    g_kzg.version++;  // the HBM copies are rebuilt on first use by a commit (the client side never needs the GPU)
}

// main.go:62-68: SRS.ReadFrom
void init_SRS_from_data(GoInt SRS_size, GoSlice* in) {
    std::lock_guard<std::mutex> lk(g_kzg.mu);
    const uint8_t* b = (const uint8_t*)in->data;
    size_t len = (size_t)in->len;
    g_kzg.n_samples = SRS_size;
    if (len < 4) { fprintf(stderr, "libmultiexp (MI355X): init_SRS_from_data: short buffer\n"); abort(); }
    size_t cnt = ((size_t)b[0] << 24) | ((size_t)b[1] << 16) | ((size_t)b[2] << 8) | b[3];
    if (len < 4 + 32 * cnt) { fprintf(stderr, "libmultiexp (MI355X): init_SRS_from_data: short buffer\n"); abort(); }
    g_kzg.srs.assign(cnt, Affine<Fp>());
    for (size_t i = 0; i < cnt; i++) {
        if (!g1_decompress(b + 4 + 32 * i, &g_kzg.srs[i])) {
            fprintf(stderr, "libmultiexp (MI355X): init_SRS_from_data: G1[%zu] is not on the curve\n", i);
            abort();
        }
    }
    g_kzg.have_g2 = false;
    if (len >= 4 + 32 * cnt + 128) {
        g_kzg.have_g2 = g2_decompress(b + 4 + 32 * cnt, &g_kzg.g2[0]) && g2_decompress(b + 4 + 32 * cnt + 64, &g_kzg.g2[1]);
    }
    g_kzg.version++;
}

// main.go:70-89: alpha * f(tau) * G1[0] -- Horner over Fr and ONE scalar multiplication (host)
void compute_digest(GoSlice* data_in, GoSlice* data_out) {
    const uint8_t* d = (const uint8_t*)data_in->data;
    Fe<Fr> acc = fe_zero<Fr>();
    for (long long i = g_kzg.n_samples - 1; i >= 0; i--)
        acc = fe_add<Fr>(fe_mul<Fr>(acc, g_kzg.tau), h_fe_from_be<Fr>(d + 32 * i));
    acc = fe_mul<Fr>(acc, g_kzg.alpha);
    uint32_t k[8];
    h_fe_to_plain<Fr>(k, acc);
    uint8_t out[64];
    static HostFixedBase<Fp> fbG;                 // table of multiples of SRS.G1[0] (rebuilt when the SRS changes)
    const XYZZ<Fp> prod = fbG.mul(g_kzg.srs[0], k);
    h_affine_to_bytes<Fp>(out, h_xyzz_to_affine64<Fp>(prod));
    copy_out(data_out, out, 64);
}

// main.go:91-101
void compute_digest_complement(GoSlice* data_in, GoSlice* data_out) {
    Fe<Fr> s = h_fe_from_be_var<Fr>((const uint8_t*)data_in->data, (size_t)data_in->len);
    uint32_t k[8];
    h_fe_to_plain<Fr>(k, s);
    uint8_t out[64];
    static HostFixedBase<Fp> fbH;                 // table of multiples of the MAC hiding base
    const XYZZ<Fp> prod = fbH.mul(g_kzg.h_mac, k);
    h_affine_to_bytes<Fp>(out, h_xyzz_to_affine64<Fp>(prod));
    copy_out(data_out, out, 64);
}

// main.go:103-116: kzg.Commit -- GPU MSM against the resident SRS
void compute_digest_from_srs(GoSlice* data_in, GoSlice* data_out) {
    uint8_t out[64];
    int rc = kzg_commit_coalesced((const uint8_t*)data_in->data, out);
    if (rc) die("compute_digest_from_srs", rc);
    copy_out(data_out, out, 64);
}

// main.go:118-138: the large MSM -- GPU
void compute_multi_exp(GoSlice* scalars, GoSlice* points, GoInt length, GoSlice* result_out) {
    uint8_t out[64];
    int rc = porla_bn254_msm_host((const uint8_t*)scalars->data, (const uint8_t*)points->data,
                                  (size_t)(length < 0 ? 0 : length), out);
    if (rc) die("compute_multi_exp", rc);
    copy_out(result_out, out, 64);
}

// main.go:140-151
GoUint8 compare_commitment(GoSlice* commitment_a, GoSlice* commitment_b) {
    Affine<Fp> a = unmarshal64((const uint8_t*)commitment_a->data);
    Affine<Fp> b = unmarshal64((const uint8_t*)commitment_b->data);
    if (!(fe_eq<Fp>(a.x, b.x) && fe_eq<Fp>(a.y, b.y))) {
        printf("error KZG commitment\n");
        return 0;
    }
    return 1;
}

// main.go:153-175: commitment = Commit(f); y = f(z); h = (f - y)/(X - z); H = Commit(h)
void create_proof(GoUint64 random_point, GoSlice* data_in, GoSlice* commitment_out, GoSlice* proof_H,
                  GoSlice* proof_point, GoSlice* proof_claim) {
    const uint8_t* d = (const uint8_t*)data_in->data;
    size_t n = (size_t)g_kzg.n_samples;
    // Both commitments go out as ONE batch of two rows of n coefficients (h padded with a zero top coefficient: the same
    // commitment), one launch instead of two.
    std::vector<uint8_t> two(2 * 32 * n, 0);
    memcpy(two.data(), d, 32 * n);
    uint8_t zt[32], yt[32];
    kzg_open_rows(d, n, random_point, two.data() + 32 * n, zt, yt);
    uint8_t both[128];
    int rc = n ? kzg_commit_rows(two.data(), false, 2, n, both, nullptr) : PORLA_OK;
    if (n == 0) memset(both, 0, sizeof both);
    if (rc) die("create_proof", rc);
    copy_out(commitment_out, both, 64);
    copy_out(proof_H, both + 64, 64);
    copy_out(proof_point, zt, 32);
    copy_out(proof_claim, yt, 32);
}

// main.go:177-193: kzg.Verify -- e(C - y*G1, G2) == e(H, tau*G2 - z*G2), as one product of two pairings (rearranged, below); needs g_kzg.have_g2
static bool opening_holds(const Affine<Fp>& C, const Affine<Fp>& H, const Fe<Fr>& z, const Fe<Fr>& y) {
    uint32_t yk[8], zk[8];
    h_fe_to_plain<Fr>(yk, y);
    h_fe_to_plain<Fr>(zk, z);
    // e(C - y G1, G2) == e(H, (tau - z) G2)  <=>  e(C - y G1 + z H, G2) * e(-H, tau G2) == 1: the factor z moves to the G1 side,
    // where a scalar multiplication costs ~45 us (endomorphism split) instead of ~300 us in G2, and both G2 operands are the
    // SRS's own points
    XYZZ<Fp> A = h_scalar_mul64_glv<Fp, GlvBn254>(g_kzg.srs.empty() ? generator() : g_kzg.srs[0], yk);
    A.y = fe_neg<Fp>(A.y);
    if (!aff_is_inf<Fp>(C)) xyzz_madd<Fp>(A, C);
    const Affine<Fp> zH = h_xyzz_to_affine64<Fp>(h_scalar_mul64_glv<Fp, GlvBn254>(H, zk));
    if (!aff_is_inf<Fp>(zH)) xyzz_madd<Fp>(A, zH);
    Affine<Fp> Aaff = h_xyzz_to_affine64<Fp>(A);
    Affine<Fp> negH = aff_neg_if<Fp>(H, true);
    if (aff_is_inf<Fp>(H)) negH = H;
    return pairing_product_is_one(Aaff, g_kzg.g2[0], negH, g_kzg.g2[1]);
}

GoUint8 verify_proof(GoSlice* commitment_in, GoSlice* proof_H, GoSlice* proof_point, GoSlice* proof_claim) {
    Affine<Fp> C = unmarshal64((const uint8_t*)commitment_in->data);
    Affine<Fp> H = unmarshal64((const uint8_t*)proof_H->data);
    Fe<Fr> z = h_fe_from_be_var<Fr>((const uint8_t*)proof_point->data, (size_t)proof_point->len);
    Fe<Fr> y = h_fe_from_be_var<Fr>((const uint8_t*)proof_claim->data, (size_t)proof_claim->len);
    if (!g_kzg.have_g2 || !opening_holds(C, H, z, y)) {
        printf("Verifying is wrong\n");
        return 0;
    }
    return 1;
}

// main.go:195-202
void add_point(GoSlice* point_a, GoSlice* point_b) {
    Affine<Fp> a = unmarshal64((const uint8_t*)point_a->data);
    Affine<Fp> b = unmarshal64((const uint8_t*)point_b->data);
    XYZZ<Fp> p = xyzz_from_affine<Fp>(a);
    xyzz_madd<Fp>(p, b);
    uint8_t out[64];
    h_affine_to_bytes<Fp>(out, h_xyzz_to_affine64<Fp>(p));
    copy_out(point_a, out, 64);
}

// main.go:204-214
void mult_point(GoSlice* point_a, GoSlice* scalar) {
    Affine<Fp> a = unmarshal64((const uint8_t*)point_a->data);
    Fe<Fr> s = h_fe_from_be_var<Fr>((const uint8_t*)scalar->data, (size_t)scalar->len);
    uint32_t k[8];
    h_fe_to_plain<Fr>(k, s);
    uint8_t out[64];
    h_affine_to_bytes<Fp>(out, h_xyzz_to_affine64<Fp>(h_scalar_mul64_glv<Fp, GlvBn254>(a, k)));     // k is reduced (h_fe_from_be_var)
    copy_out(point_a, out, 64);
}

// main.go:216-222
void neg_point(GoSlice* point) {
    Affine<Fp> a = unmarshal64((const uint8_t*)point->data);
    if (!aff_is_inf<Fp>(a)) a.y = fe_neg<Fp>(a.y);
    uint8_t out[64];
    h_affine_to_bytes<Fp>(out, a);
    copy_out(point, out, 64);
}

// main.go:224-230
void set_inf_point(GoSlice* point) {
    uint8_t out[64] = {0};
    copy_out(point, out, 64);
}

// ---- diagnostics of the host pairing (verify_proof's engine): lets the tests check bilinearity and compare the fast
// final exponentiation / projective Miller loop with the literal reference form
static void g2_to_bytes(uint8_t out[128], const G2Affine& q) {
    if (q.inf) { memset(out, 0, 128); return; }
    h_fe_to_be<Fp>(out, q.x.a1); h_fe_to_be<Fp>(out + 32, q.x.a0); h_fe_to_be<Fp>(out + 64, q.y.a1); h_fe_to_be<Fp>(out + 96, q.y.a0);
}
static G2Affine g2_from_bytes(const uint8_t in[128]) {
    G2Affine q;
    q.x.a1 = h_fe_from_be<Fp>(in); q.x.a0 = h_fe_from_be<Fp>(in + 32); q.y.a1 = h_fe_from_be<Fp>(in + 64); q.y.a0 = h_fe_from_be<Fp>(in + 96);
    q.inf = f2_is_zero(q.x) && f2_is_zero(q.y);
    return q;
}
int porla_bn254_g2_mul_generator(const uint8_t scalar_be[32], uint8_t out[128]) {
    if (!scalar_be || !out) return PORLA_ERR_ARG;
    Fe<Fr> s = h_fe_from_be<Fr>(scalar_be);
    uint32_t k[8];
    h_fe_to_plain<Fr>(k, s);
    g2_to_bytes(out, g2_scalar_mul(g2_generator(), k));
    return PORLA_OK;
}
int porla_bn254_pairing_product_is_one(const uint8_t p1[64], const uint8_t q1[128], const uint8_t p2[64], const uint8_t q2[128],
                                       int slow) {
    if (!p1 || !q1 || !p2 || !q2) return PORLA_ERR_ARG;
    return pairing_product_is_one(h_affine_from_bytes<Fp>(p1), g2_from_bytes(q1), h_affine_from_bytes<Fp>(p2), g2_from_bytes(q2),
                                  slow != 0) ? 1 : 0;
}

// the EIP-197 predicate on its own input layout: n pairs of 192 bytes (G1 X || Y, G2 x_im || x_re || y_im || y_re, all 32-byte
// big-endian; zeros = infinity).  PORLA_ERR_ARG for what the precompile rejects (a coordinate >= p, a point off its curve, a G2
// point outside the order-r subgroup); else 1 / 0.  Pairs go two at a time through the shared Miller loop of verify_proof.
int porla_bn254_pairing_check(const uint8_t* input, size_t n_pairs, int slow) {
    if (!input && n_pairs) return PORLA_ERR_ARG;
    static const uint8_t P_BE[32] = {0x30, 0x64, 0x4e, 0x72, 0xe1, 0x31, 0xa0, 0x29, 0xb8, 0x50, 0x45, 0xb6, 0x81, 0x81, 0x58, 0x5d,
                                     0x97, 0x81, 0x6a, 0x91, 0x68, 0x71, 0xca, 0x8d, 0x3c, 0x20, 0x8c, 0x16, 0xd8, 0x7c, 0xfd, 0x47};
    static const uint32_t R_LE[8] = {0xf0000001u, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};
    std::vector<Affine<Fp>> ps(n_pairs);
    std::vector<G2Affine> qs(n_pairs);
    for (size_t i = 0; i < n_pairs; i++) {
        const uint8_t* in = input + 192 * i;
        for (int w = 0; w < 6; w++)
            if (memcmp(in + 32 * w, P_BE, 32) >= 0) { set_last_error("porla: pairing input coordinate >= p"); return PORLA_ERR_ARG; }
        ps[i] = h_affine_from_bytes<Fp>(in);
        if (!aff_is_inf<Fp>(ps[i])) {
            const Fe<Fp> rhs = fe_add<Fp>(fe_mul<Fp>(fe_mul<Fp>(ps[i].x, ps[i].x), ps[i].x), fp_small(3));
            if (!fe_eq<Fp>(fe_mul<Fp>(ps[i].y, ps[i].y), rhs)) { set_last_error("porla: pairing input G1 point not on the curve"); return PORLA_ERR_ARG; }
        }
        qs[i] = g2_from_bytes(in + 64);
        if (!qs[i].inf) {
            const Fp2 rhs = f2_add(f2_mul(f2_sqr(qs[i].x), qs[i].x), g2_b());
            if (!f2_eq(f2_sqr(qs[i].y), rhs)) { set_last_error("porla: pairing input G2 point not on the twist"); return PORLA_ERR_ARG; }
            if (!g2_scalar_mul(qs[i], R_LE).inf) { set_last_error("porla: pairing input G2 point not in the order-r subgroup"); return PORLA_ERR_ARG; }
        }
    }
    const Affine<Fp> p_inf = h_affine_from_bytes<Fp>(std::vector<uint8_t>(64, 0).data());
    const G2Affine q_inf{f2_zero(), f2_zero(), true};
    Fp12 f = f12_one();
    if (slow) {
        for (size_t i = 0; i < n_pairs; i++) f = f12_mul(f, miller_ate_affine(ps[i], qs[i]));
        return f12_is_one(f12_pow_final(f)) ? 1 : 0;
    }
    for (size_t i = 0; i < n_pairs; i += 2)
        f = f12_mul(f, i + 1 < n_pairs ? miller_opt_ate2(ps[i], qs[i], ps[i + 1], qs[i + 1]) : miller_opt_ate2(ps[i], qs[i], p_inf, q_inf));
    return f12_is_one(f12_final_exp(f)) ? 1 : 0;
}

}  // extern "C"

// ---- the batched verifier's share of the KZG state (kzg_verify_batch.hip)
int porla::kzg_verify_base(uint8_t g_be[64]) {
    std::lock_guard<std::mutex> lk(g_kzg.mu);
    if (g_kzg.srs.empty() || !g_kzg.have_g2) {
        set_last_error("porla: SRS and its G2 points not initialised (call init_SRS / init_SRS_from_data first)");
        return PORLA_ERR_STATE;
    }
    h_affine_to_bytes<Fp>(g_be, g_kzg.srs[0]);
    return PORLA_OK;
}

bool porla::kzg_opening_holds(const uint8_t rec[192]) {
    return opening_holds(unmarshal64(rec), unmarshal64(rec + 64), h_fe_from_be_var<Fr>(rec + 128, 32), h_fe_from_be_var<Fr>(rec + 160, 32));
}

bool porla::kzg_folded_opening_holds(const uint8_t p_be[64], const uint8_t q_be[64]) {
    const Affine<Fp> P = h_affine_from_bytes<Fp>(p_be), Q = h_affine_from_bytes<Fp>(q_be);
    return pairing_product_is_one(P, g_kzg.g2[0], aff_neg_if<Fp>(Q, true), g_kzg.g2[1]);   // -infinity = infinity (fe_neg_if of 0)
}
