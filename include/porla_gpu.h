/* porla_gpu.h -- C ABI of the MI355X engine beyond the 14 cgo symbols of libmultiexp.h.
 *
 * Plain pointers and sizes only.  "d_" pointers are device (HBM) addresses on the current HIP
 * device; `hip_stream` is a hipStream_t passed as void* (NULL = default stream).  All functions
 * return 0 on success and a negative code on failure (porla_gpu_last_error() gives the text);
 * nothing here ever falls back to a CPU implementation of the hot path.
 *
 * What each entry point replaces in the reference:
 *   porla_bn254_msm_*        compute_multi_exp, porla/main.go:118-138 (libmultiexp.h:77), for callers that
 *                            keep the (scalar, point) arrays resident in HBM (bench, multi-GPU sharding)
 *   porla_bn254_jac_sum      the partial-sum fold of range-sharded MSMs; the reference does the same fold
 *                            across its 8 pool threads with gej_add_var, porla/Client/Client.hpp:761-787
 *   porla_kzg_commit_batch_* compute_digest_from_srs (main.go:103-116) hoisted over many rows
 *                            (callers Server.hpp:550-560, 1077-1078, 2061-2062); uses the SRS loaded by
 *                            init_SRS / init_SRS_from_data of libmultiexp.h
 *   porla_fixed_base_*       the same batched commitment against any fixed base: the IPA twin is the Pedersen
 *                            commitment over the fixed generators[] (compute_commitment, Client.hpp:374-406,
 *                            Server.hpp:329-361 -> secp256k1_ecmult_multi_var over 128 fixed points)
 *   porla_secp256k1_msm_*    secp256k1_ecmult_multi_var with g_sc = 0,
 *                            porla/Utils/secp256k1_lib/ecmult_impl.h:814-860 (call sites Server.hpp:842-848,
 *                            Client.hpp:395,778), reached through the include shim in INTEGRATION.md
 *   porla_icc_encode_*       the CRebuild_Cached butterfly network, porla/Server/Server.hpp:1548-1687, and the
 *                            align_MAC scalar derivation, Server.hpp:531-541 (no function boundary exists
 *                            in the reference: INTEGRATION.md documents the patch site)
 *   porla_icc_mac_encode_*   the MAC halves of the same network ("FFT in the exponent"), Server.hpp:1590-1609, 1658-1676
 *   porla_icc_mix_*, porla_icc_mac_mix_*, porla_server_mix_device
 *                            Server::mix, Server.hpp:1209-1328 (data rows, MAC commitments, MAC alignments; the last: all three)
 *   porla_audit_combine_device, porla_*_msm_pair_*, porla_*_audit_msm_pair_*, porla_kzg_audit_device, porla_ipa_audit_device
 *                            Server::audit after the challenge, Server.hpp:790-907: the row combine (:790-828), the two MSMs over
 *                            one scalar array (:842-848 / :900-901), and -- the last two -- the whole audit in one call
 *   porla_kzg_audit_batch_device
 *                            Server::audit (KZG) of many files or clients at once: K complete audits in one asynchronous
 *                            call, each record the reply Server.hpp:897-915 sends
 *   porla_ipa_audit_batch_device, porla_ipa_prove_batch_device
 *                            Server::audit (IPA) of many files or clients at once, the inner-product proof included
 *                            (Server.hpp:790-892, :2279-2452): K complete replies in one asynchronous call; the prover alone
 *   porla_kzg_verify_batch_device
 *                            Client::audit's check (KZG) of many replies at once, Client.hpp:685-778 and :849-869: K MAC
 *                            checks and ONE folded pairing check per call, a verdict per reply
 *   porla_kzg_{digest,complement,mac}_batch_{device,host}
 *                            compute_digest / compute_digest_complement hoisted over the blocks of Client::initialize,
 *                            Client.hpp:408-455; the last: both and the add_point that joins them (Client.hpp:229-236, 468-478)
 *
 * Byte formats (identical to the reference's wire formats):
 *   scalar   32 bytes big-endian (bn254_scalar, utils.h:64,307-318); reduced mod the group order
 *   point    64 bytes X||Y big-endian, regular (non-Montgomery) form; 64 zero bytes = infinity
 *            (KZG MAC_Block, utils.h:65; config.hpp:26)
 *   jacobian 96 bytes X||Y||Z big-endian regular form, x = X/Z^2, y = Y/Z^3, Z = 0 = infinity
 */
#ifndef PORLA_GPU_H
#define PORLA_GPU_H
#include <stddef.h>
#include <stdint.h>

#if defined(__GNUC__)
#pragma GCC visibility push(default)   /* the engine itself is built with -fvisibility=hidden: only this ABI is exported */
#endif
#ifdef __cplusplus
extern "C" {
#endif

#define PORLA_OK            0
#define PORLA_ERR_NO_DEVICE (-1)   /* no gfx950 device / HIP runtime failure */
#define PORLA_ERR_HIP       (-2)   /* a HIP call failed (see porla_gpu_last_error) */
#define PORLA_ERR_ARG       (-3)   /* bad argument */
#define PORLA_ERR_STATE     (-4)   /* e.g. SRS not initialised */

#define PORLA_JACOBIAN_BYTES 96    /* X||Y||Z big-endian, the partial sum of one pair range */
#define PORLA_DIST_ID_BYTES  128   /* an ncclUniqueId */

/* ---- runtime ---- */
int         porla_gpu_device_count(void);
int         porla_gpu_set_device(int device);
const char *porla_gpu_last_error(void);
/* the range rule of every split in the engine (MSM pair ranges, commitment rows, ICC columns): shard `rank` of `world` owns
 * units [rank n / world, (rank + 1) n / world).  One process per GPU: each rank calls the ordinary entry points on its own
 * range (rows, columns) -- those paths need no collective. */
int         porla_shard_range(size_t n, int rank, int world, size_t *begin, size_t *end);
/* Per-kernel timing with HIP events recorded on the launch stream.  enable=1 starts (and clears) the
 * accumulation for every kernel, enable=2 for each workload's dominant kernel only (two event packets per recorded
 * kernel leave the GPU idle for ~10 us around it -- bench.py times with 2 and takes the full breakdown separately); porla_gpu_profile_get(i, ...) returns kernel name, summed milliseconds and launch count
 * for slot i, or a negative value past the last slot. */
int         porla_gpu_profile_enable(int enable);
int         porla_gpu_profile_get(int slot, char *name, size_t name_cap, double *total_ms, long long *launches);
/* frees the MSM scratch of every workspace slot of every device (reallocated by the next MSM); PORLA_ERR_STATE while a
 * two-phase MSM is pending */
int         porla_gpu_release_msm_workspaces(void);
/* MSM tuning override (0 = automatic): window bits c */
int         porla_gpu_set_msm_window(int c);
/* inputs of up to 32768 pairs (every MSM the reference issues: n_points <= 3200, Server.hpp:585-587) take a single-launch path;
 * on = 0 sends them through the general path instead, window_bits in 2..8 fixes its window width (0 = automatic) */
int         porla_gpu_set_msm_small(int on, int window_bits);
/* 1: split every scalar with the curve endomorphism (half the windows); 0: plain windows over the full scalar;
 * -1 (default): per curve -- secp256k1 on (as the reference does, ecmult_impl.h:621-634), BN254 off (measured slower) */
int         porla_gpu_set_msm_glv(int on);
/* diagnostic: window bits, window count and GLV flag of the most recently launched MSM (what the automatic choice was) */
int         porla_gpu_last_msm_shape(int *c, int *windows, int *glv);
/* diagnostic: HOST execution of the single-launch MSM's shape function and launch decision (no device needed), for `count` elements:
 *   curve 0 = BN254, 1 = secp256k1;  n in 1 .. 32 768;  used_bits in 0 .. 256: bit length of the OR of the scalars;
 *   c_flags: forced window bits 0 .. 8 in the low byte (0 = automatic, porla_gpu_set_msm_small), 0x100 = never split (porla_gpu_set_msm_glv(0));
 *   form: PORLA_SMALL_FORM_LONE      one MSM on the lone call's blocks, the shape the kernel derives from used_bits;
 *         PORLA_SMALL_FORM_PAIR      one point set of a pair on the pair's blocks, the shape the kernel derives from used_bits;
 *         PORLA_SMALL_FORM_PAIR_HINT the same with used_bits (>= 1) passed as the caller's bound, as the audit's pairs pass 32;
 *         PORLA_SMALL_FORM_PAIR_ANY  the pair as the host decides it with no bound: single-launch only if EVERY bit length 0 .. 256 fits
 *                                    (used_bits is ignored; the shape reported is that of 256-bit scalars).
 * out[6 i ..]: 1 = the shape fits and is launched / 0 = it does not fit (more windows than blocks, or a slice of more than 8 192
 * sub-scalars) and is not launched, blocks, split flag, window bits c, windows W, slices per window S.  The kernels refuse exactly the shapes reported 0.
 * A pair reported 0 -- secp256k1 only: above 28 672 pairs with scalars over 128 bits, above 24 576 with the split off and scalars of
 * 250 bits and more -- runs as two MSMs, one after the other, each of them a lone single launch of its own on 256 blocks (lone shapes
 * always fit).  PORLA_ERR_ARG for an element out of range; nothing is written then. */
#define PORLA_SMALL_FORM_LONE      0
#define PORLA_SMALL_FORM_PAIR      1
#define PORLA_SMALL_FORM_PAIR_HINT 2
#define PORLA_SMALL_FORM_PAIR_ANY  3
int         porla_msm_small_shape(size_t count, const int32_t *curve, const uint32_t *n, const int32_t *used_bits,
                                  const int32_t *c_flags, const int32_t *form, int32_t *out);
/* diagnostic: HOST execution of the 8 x 32-bit field helpers the kernels are built from (borrow / carry chains, negation, the
 * bounded reduction of the ICC finish step), for the CPU test suite.  op 0: reduce a value below 5 x modulus (modulus 0 = BN254
 * group order) or below the modulus + 2^256 - n (modulus 1 = secp256k1 group order: one conditional subtraction) to its residue;
 * 1: negate; 2: conditional negate (taken); 3: a - b; 4: a + b (operands canonical).  32-byte little-endian values. */
int         porla_diag_fe_op(int op, int modulus, const uint8_t a_le[32], const uint8_t b_le[32], uint8_t out_le[32]);
/* diagnostic: the scalar split the digit kernel applies (host execution of the same code): scalar mod n = k1 + lambda*k2,
 * magnitudes as 16-byte big-endian, signs as 0/1.  curve: 0 = BN254, 1 = secp256k1. */
int         porla_glv_split(int curve, const uint8_t scalar_be[32], uint8_t k1_mag_be[16], int *k1_neg,
                            uint8_t k2_mag_be[16], int *k2_neg);

/* ---- BN254 G1 MSM ---- */
int porla_bn254_msm_device(const void *d_scalars, const void *d_points, size_t n, uint8_t out_affine[64],
                           void *hip_stream);
int porla_bn254_msm_device_partial(const void *d_scalars, const void *d_points, size_t n, uint8_t out_jacobian[96],
                                   void *hip_stream);
/* The audit's pair: ONE scalar array over TWO point arrays -- replaces the two back-to-back calls
 *   bn254_multi_exp(combined_MAC, ptc, sc, n); bn254_multi_exp(combined_align, pta, sc, n);    (porla/Server/Server.hpp:900-901,
 *   and the secp256k1 twins secp256k1_ecmult_multi_var x2 at :842-848)
 * For n <= 32 768 both run in ONE kernel launch (half the chip each) where the shape fits the launch (porla_msm_small_shape; every
 * BN254 size does, secp256k1 up to 28 672 pairs, 24 576 with the split off); otherwise they run one after the other, one lone single launch per point set.
 * out_a = sum scalars[i] * points_a[i], out_b = sum scalars[i] * points_b[i]; encodings as porla_bn254_msm_device. */
int porla_bn254_msm_pair_device(const void *d_scalars, const void *d_points_a, const void *d_points_b, size_t n,
                                uint8_t out_a[64], uint8_t out_b[64], void *hip_stream);
int porla_bn254_msm_pair_host(const uint8_t *scalars, const uint8_t *points_a, const uint8_t *points_b, size_t n,
                              uint8_t out_a[64], uint8_t out_b[64]);
/* ... and straight from the server's resident MAC arrays: per challenged row i the points store_a[idx[i]], store_b[idx[i]] (64-byte
 * affine each) and the scalar coef[i] (abs(int32), bn254_scalar_set_int, utils.h:271-275) -- the gather Server::audit does on the
 * host into ptc / pta / sc (Server.hpp:838-848, 893-899) runs on the device; idx / coef are the arrays porla_audit_combine_device
 * takes.  All pointers device pointers; outputs host. */
int porla_bn254_audit_msm_pair_device(const void *d_store_a, const void *d_store_b, const uint64_t *d_idx, const uint32_t *d_coef,
                                      size_t n, uint8_t out_a[64], uint8_t out_b[64], void *hip_stream);
/* two-phase form (slots 1..3 as porla_bn254_msm_device_begin): begin gathers and launches on hip_stream and returns, end waits and
 * folds -- the audit's other chain (row combine -> alignment commitment -> proof) runs in between; 1 .. 32 768 challenged rows */
int porla_bn254_audit_msm_pair_begin(int slot, const void *d_store_a, const void *d_store_b, const uint64_t *d_idx,
                                     const uint32_t *d_coef, size_t n, void *hip_stream);
int porla_bn254_audit_msm_pair_end(int slot, uint8_t out_a[64], uint8_t out_b[64]);
/* Two-phase form for independent MSMs in flight at once (e.g. the audit's two MSMs, Server.hpp:900-901): begin enqueues
 * every kernel of one MSM on hip_stream and returns; end waits for that slot, folds the reduction tree's sums on the host and writes
 * 64 bytes affine (jacobian = 0) or 96 bytes Jacobian (jacobian = 1).  slot in 1..3 (0 is used by the blocking calls);
 * one begin per slot until its end.  Overlap comes from using a different stream per slot.  A slot belongs to the device that
 * was current at begin: end must run with the same current device (PORLA_ERR_STATE otherwise, or without a begin). */
int porla_bn254_msm_device_begin(int slot, const void *d_scalars, const void *d_points, size_t n, void *hip_stream);
int porla_bn254_msm_device_end(int slot, uint8_t *out, int jacobian);
int porla_bn254_msm_host(const uint8_t *scalars, const uint8_t *points, size_t n, uint8_t out_affine[64]);
/* The same over several pair ranges and devices of this process -- the multi-GPU form that stays behind the C ABI (the
 * reference folds the partial sums of its 8 pool threads the same way, porla/Client/Client.hpp:761-787): the pairs are cut
 * into `shards` contiguous ranges, device g of `devices` (counted from the current device, modulo the visible ones) owns a
 * contiguous block of ranges and runs them from its own host thread, stream and workspace slots, uploading range k+1 under
 * the kernels of range k; the range totals are added on the host.  shards <= 0 / devices <= 0: automatic (devices: as many
 * visible ones as get >= 2^17 pairs each, or PORLA_MSM_DEVICES; shards: up to 4 ranges of >= 2^17 pairs per device).
 * porla_bn254_msm_host -- and therefore compute_multi_exp -- takes this path from 2^18 pairs on (PORLA_MSM_SPLIT_MIN).
 * Any (shards, devices) gives the same 64 bytes. */
int porla_bn254_msm_host_multi(const uint8_t *scalars, const uint8_t *points, size_t n, int shards, int devices,
                               uint8_t out_affine[64]);
/* diagnostic: ranges and devices the most recent *_msm_host_multi used */
int porla_gpu_last_msm_multi(int *shards, int *devices);
int porla_bn254_jac_sum(const uint8_t *jacobians, size_t count, uint8_t out_affine[64]);
/* the MSM's host tail on its own (no device needed): the bucket-reduction tree leaves, per window w < windows, S_w and
 * M_{w,k} (k < window_bits - 1) -- here as 64-byte affine points, sums[w * window_bits + 0] = S_w, [.. + 1 + k] = M_{w,k} --
 * and the result is sum_w 2^(window_bits * w) * (S_w + sum_k 2^k M_{w,k}).  Exists for the CPU test of that fold. */
int porla_bn254_tree_fold(const uint8_t *sums_affine, int windows, int window_bits, uint8_t out_affine[64]);

/* ---- secp256k1 MSM (canonical encodings: 32-byte BE scalar, 64-byte x||y BE affine, zeros = infinity) ---- */
int porla_secp256k1_msm_device(const void *d_scalars, const void *d_points, size_t n, uint8_t out_affine[64],
                               void *hip_stream);
int porla_secp256k1_msm_pair_device(const void *d_scalars, const void *d_points_a, const void *d_points_b, size_t n,
                                    uint8_t out_a[64], uint8_t out_b[64], void *hip_stream);
int porla_secp256k1_msm_pair_host(const uint8_t *scalars, const uint8_t *points_a, const uint8_t *points_b, size_t n,
                                  uint8_t out_a[64], uint8_t out_b[64]);
int porla_secp256k1_audit_msm_pair_device(const void *d_store_a, const void *d_store_b, const uint64_t *d_idx,
                                          const uint32_t *d_coef, size_t n, uint8_t out_a[64], uint8_t out_b[64], void *hip_stream);
int porla_secp256k1_audit_msm_pair_begin(int slot, const void *d_store_a, const void *d_store_b, const uint64_t *d_idx,
                                         const uint32_t *d_coef, size_t n, void *hip_stream);
int porla_secp256k1_audit_msm_pair_end(int slot, uint8_t out_a[64], uint8_t out_b[64]);
int porla_secp256k1_msm_device_partial(const void *d_scalars, const void *d_points, size_t n,
                                       uint8_t out_jacobian[96], void *hip_stream);
int porla_secp256k1_msm_device_begin(int slot, const void *d_scalars, const void *d_points, size_t n, void *hip_stream);
int porla_secp256k1_msm_device_end(int slot, uint8_t *out, int jacobian);   /* the two MSMs of the IPA audit, Server.hpp:842-848 */
int porla_secp256k1_msm_host(const uint8_t *scalars, const uint8_t *points, size_t n, uint8_t out_affine[64]);
int porla_secp256k1_msm_host_multi(const uint8_t *scalars, const uint8_t *points, size_t n, int shards, int devices,
                                   uint8_t out_affine[64]);
int porla_secp256k1_jac_sum(const uint8_t *jacobians, size_t count, uint8_t out_affine[64]);
int porla_secp256k1_tree_fold(const uint8_t *sums_affine, int windows, int window_bits, uint8_t out_affine[64]);

/* ---- batched MSM: many independent small MSMs in one call (both curves) ----
 * K independent MSMs.  Entry k covers pairs [offsets[k], offsets[k+1]) of the concatenated arrays:
 *   out[k] = sum scalars[i] * points[i] over that range.
 * Encodings as porla_bn254_msm_device / porla_secp256k1_msm_device: scalars 32-byte big-endian (values >= r allowed, reduced),
 * points 64-byte X||Y big-endian (64 zero bytes = infinity), each output 64 bytes affine (64 zero bytes = infinity; an empty entry
 * gives infinity) -- byte for byte what porla_*_msm_device returns for that entry.
 * offsets is a HOST array of k+1 non-decreasing values with offsets[0] = 0.  Each entry holds at most 32 768 pairs (SMALL_MAX_N);
 * larger MSMs go through porla_*_msm_device.  d_scalars, d_points and d_out are device pointers; only d_out[0 .. k*64) is written.
 * Asynchronous: the call enqueues on hip_stream and returns without waiting for this call's work.  The work waits for whatever the
 * caller had enqueued on hip_stream when it called; d_out is complete when hip_stream is.  The call
 * never waits on the host for earlier work.
 * PORLA_ERR_ARG (message in porla_gpu_last_error), checked before the device is touched: offsets not non-decreasing or
 * offsets[0] != 0, an entry of more than 32 768 pairs, offsets NULL or d_out NULL while k > 0, d_scalars or d_points NULL while
 * there is at least one pair, a total whose byte size overflows (unreachable within the entry limit, checked all the same).  k = 0 returns 0 and writes nothing.  Without a device, valid
 * arguments return PORLA_ERR_NO_DEVICE.
 * Any k and any total that fit in memory: the library cuts the batch into launch rounds of at most 2^18 entries, 2^24 pairs,
 * 32 768 bucket blocks and 2^20 quads of the tiny-entry kernel; a round is a fixed sequence of launches whatever its K (work-list
 * upload, counter clear, k_batch_tiny, k_batch_bucket, k_batch_fold, k_fb_finish).  Workspace slots and locking as
 * porla_*_msm_device; porla_gpu_release_msm_workspaces frees the batch scratch.  porla_gpu_set_msm_glv(0) and the window
 * override of porla_gpu_set_msm_small apply to the bucket-path entries (> 64 pairs) as to the single-launch MSM; entries of up
 * to 64 pairs always use the endomorphism-split ladder. */
int porla_bn254_msm_batch_device(const void *d_scalars, const void *d_points, const uint64_t *offsets, size_t k,
                                 void *d_out, void *hip_stream);
int porla_bn254_msm_batch_host(const uint8_t *scalars, const uint8_t *points, const uint64_t *offsets, size_t k,
                               uint8_t *out);   /* blocking; host buffers; out: k * 64 bytes */
int porla_secp256k1_msm_batch_device(const void *d_scalars, const void *d_points, const uint64_t *offsets, size_t k,
                                     void *d_out, void *hip_stream);
int porla_secp256k1_msm_batch_host(const uint8_t *scalars, const uint8_t *points, const uint64_t *offsets, size_t k,
                                   uint8_t *out);

/* ---- one process per GPU: the range-sharded MSM across processes (BASELINE config 3) ----
 * Every rank owns a pair range resident in its GPU's HBM, runs a full MSM over it and contributes ONE 96-byte partial
 * Jacobian sum; the only exchange step is one ncclAllGather of world x 96 bytes (RCCL over xGMI, issued from C++ on the
 * engine's own stream), followed by world - 1 group additions and one inversion on every rank's host.  RCCL is bound with
 * dlopen at the first porla_dist_* call (PORLA_RCCL_LIB overrides the library name).
 *   rank 0: porla_dist_unique_id(id), hand the 128 bytes to the other ranks by any means (the launcher's store, MPI, a file)
 *   all   : porla_gpu_set_device(local_rank); porla_dist_init(id, rank, world)      [collective]
 *   all   : porla_bn254_msm_device_dist(my range ...) -> the whole job's 64-byte result on every rank   [collective]
 *           or a partial from porla_*_msm_device_partial / _device_end(slot, out, 1) handed to porla_*_dist_fold
 *   all   : porla_dist_finalize()
 * porla_dist_init is bounded: a peer that never arrives makes it fail with PORLA_ERR_STATE after PORLA_DIST_INIT_TIMEOUT_S
 * (default 180 s) instead of waiting forever.  The pending RCCL call cannot be cancelled: its helper thread is marked abandoned
 * (a communicator it still obtains is aborted at once), every later porla_dist_* call of the process fails with
 * PORLA_ERR_STATE, and the caller must leave with a non-zero _exit() -- not exit(): static destructors would run under a
 * thread that is still inside RCCL -- and continue, if at all, in a fresh child process. */
int porla_dist_unique_id(uint8_t id_out[PORLA_DIST_ID_BYTES]);
int porla_dist_init(const uint8_t id[PORLA_DIST_ID_BYTES], int rank, int world);
int porla_dist_info(int *rank, int *world);     /* world = 0 before porla_dist_init */
int porla_dist_finalize(void);
int porla_dist_allgather_partials(const uint8_t partial[PORLA_JACOBIAN_BYTES], uint8_t *all_out /* world * 96 bytes */);
int porla_bn254_dist_fold(const uint8_t partial[PORLA_JACOBIAN_BYTES], uint8_t out_affine[64]);
int porla_secp256k1_dist_fold(const uint8_t partial[PORLA_JACOBIAN_BYTES], uint8_t out_affine[64]);
int porla_bn254_msm_device_dist(const void *d_scalars, const void *d_points, size_t n_local, uint8_t out_affine[64],
                                void *hip_stream);
int porla_secp256k1_msm_device_dist(const void *d_scalars, const void *d_points, size_t n_local, uint8_t out_affine[64],
                                    void *hip_stream);

/* ---- batched fixed-base commitments ----
 * out[r] = sum_{i < n_coeffs} (row_r[i] mod order) * base[i] for every row r, as 64-byte X||Y big-endian affine points.
 * rows: coefficient i of row r at rows + r*row_stride + 32*i, 32 bytes big-endian (bn254_scalar, utils.h:307-318).
 * The base is expanded once into a table of window multiples resident in HBM (window_bits c, 0 = automatic: the
 * widest c <= 20 whose table fits min(a quarter of the free HBM, PORLA_COMMIT_TABLE_GB = 64 GB): 20 bits = 56 GB for
 * 128 BN254 points on a 288 GB MI355X); a commitment is then n_coeffs * ceil((bits+1)/c) mixed additions.  curve: 0 = BN254 G1, 1 = secp256k1. */
typedef struct porla_fixed_base porla_fixed_base;
int  porla_fixed_base_create(int curve, const uint8_t *points, size_t n_points, int window_bits, porla_fixed_base **out);
int  porla_fixed_base_info(const porla_fixed_base *fb, int *window_bits, int *windows, unsigned long long *table_bytes);
int  porla_fixed_base_commit_device(porla_fixed_base *fb, const void *d_rows, size_t n_rows, size_t n_coeffs,
                                    size_t row_stride, void *d_out, void *hip_stream);
int  porla_fixed_base_commit_host(porla_fixed_base *fb, const uint8_t *rows, size_t n_rows, size_t n_coeffs,
                                  size_t row_stride, uint8_t *out);
/* Server::audit for the IPA build up to the inner-product proof, in ONE call (porla/Server/Server.hpp:790-857): row combine and
 * alignment scalars, the two secp256k1 MSMs over the challenged MACs (arguments as porla_secp256k1_audit_msm_pair_device), and the
 * two Pedersen commitments over the fixed generators -- compute_commitment(c) of align_MAC (:495-529) and compute_commitment(B)
 * (:856) -- as one two-row launch.  generators_fb = porla_fixed_base_create(1, generators, n_cols, ...).  b_out (may be NULL): B mod
 * p_icc as n_cols 32-byte big-endian values, the input of inner_product_prove.  Outputs on the host; blocking. */
int porla_ipa_audit_device(porla_fixed_base *generators_fb, const void *d_rows64, const uint64_t *d_idx64,
                           const uint32_t *d_coef64, size_t n64, const void *d_rows32, const uint64_t *d_idx32,
                           const uint32_t *d_coef32, size_t n32, size_t n_cols, const void *d_mac_store,
                           const void *d_align_store, const uint64_t *d_mac_idx, const uint32_t *d_mac_coef, size_t n_macs,
                           uint8_t combined_mac[64], uint8_t combined_align[64], uint8_t align_value[64],
                           uint8_t commitment[64], uint8_t *b_out, void *hip_stream);
void porla_fixed_base_destroy(porla_fixed_base *fb);
/* KZG: rows of n_samples coefficients (4096 bytes per row for NUM_CHUNKS = 128) against the resident SRS */
int  porla_kzg_commit_batch_device(const void *d_rows, size_t n_rows, void *d_out, void *hip_stream);
int  porla_kzg_commit_batch_host(const uint8_t *rows, size_t n_rows, uint8_t *out);
/* Server::audit (KZG build) after the challenge has been drawn, in ONE call (porla/Server/Server.hpp:564-931): the row combine and
 * alignment scalars (arguments as porla_audit_combine_device, n_cols = the SRS size), the two MSMs over the challenged MACs
 * (arguments as porla_bn254_audit_msm_pair_device; they run on a stream of their own beside the rest), align_MAC's commitment and
 * create_proof(random_point, B) -- the three commitments as one launch.  Outputs on the host: combined_MAC, combined_align,
 * align_value = Commit(c), and the proof (commitment = Commit(B), H, point, claim; main.go:153-175); b_out (may be NULL): B mod
 * p_icc as n_cols 32-byte big-endian values.  Everything else device pointers; blocking; one audit at a time per process.
 * Stream contract (also porla_ipa_audit_device): hip_stream orders the INPUTS -- every kernel of the audit, on whichever
 * internal stream it runs, waits for what the caller had enqueued on hip_stream (NULL: the null stream) when the call was made,
 * so index / coefficient arrays uploaded asynchronously on that stream just before the call are safe. */
int  porla_kzg_audit_device(const void *d_rows64, const uint64_t *d_idx64, const uint32_t *d_coef64, size_t n64,
                            const void *d_rows32, const uint64_t *d_idx32, const uint32_t *d_coef32, size_t n32,
                            const void *d_mac_store, const void *d_align_store, const uint64_t *d_mac_idx,
                            const uint32_t *d_mac_coef, size_t n_macs, unsigned long long random_point,
                            uint8_t combined_mac[64], uint8_t combined_align[64], uint8_t align_value[64],
                            uint8_t commitment[64], uint8_t proof_h[64], uint8_t proof_point[32], uint8_t proof_claim[32],
                            uint8_t *b_out, void *hip_stream);
/* Server::audit (KZG build) for K independent audits in ONE call (one per file or client, Server.hpp:564-931 each): everything on
 * the device and on hip_stream.  reqs is a HOST array of K audits; each field means what the same argument of
 * porla_kzg_audit_device means, and every audit has its own stores (different files' levels may live in different allocations).
 * d_out receives K records of PORLA_KZG_AUDIT_RECORD_BYTES, the reply of Server::audit (Server.hpp:897-915):
 *   commitment(64) | proof_h(64) | point(32) | claim(32) | combined_mac(64) | combined_align(64)
 * where combined_align is the value AFTER align_MAC (Server.hpp:903, :531-561): MSM(align store) + Commit(c).  Points 64-byte
 * big-endian affine, infinity = 64 zero bytes.  Record k is byte-identical to porla_kzg_audit_device's outputs for audit k, with
 * bn254_add(combined_align, align_value) as its last field.  d_b_out (may be NULL): K x n x 32 bytes, B mod p_icc big-endian per
 * audit, the single call's b_out (n = the SRS size).
 * Asynchronous: enqueued on hip_stream, returns without waiting on the host; the work waits for whatever the caller had enqueued on
 * hip_stream before the call; d_out is complete when hip_stream is.  No internal side stream.
 * PORLA_ERR_ARG (message in porla_gpu_last_error), checked before the device is touched: reqs or d_out NULL while k > 0; a NULL
 * array whose count is > 0; n_macs > 32 768 (the batched MSM's entry limit: larger audits keep using porla_kzg_audit_device);
 * n64 + n32 >= 2^32; a byte size that overflows.  k = 0 returns 0 and writes nothing.  No SRS loaded: PORLA_ERR_STATE.  Valid
 * arguments without a device: PORLA_ERR_NO_DEVICE.
 * One fixed sequence of launches per call: the row combine of all K audits (two launches), the KZG opening (a wave per audit), the
 * MSM gather, the batched MSM over the 2K entries, ONE commitment pass over the 3K rows [c_k, B_k, h_k], and the join that adds
 * align_value, normalises each audit's four points with one inversion and writes the records.  Calls from several threads on
 * several streams, and beside porla_kzg_audit_device, are safe. */
#define PORLA_KZG_AUDIT_RECORD_BYTES 320
#define PORLA_KZG_AUDIT_REQ_BYTES    112   /* sizeof(porla_kzg_audit_req) on LP64; the library static_asserts it and each offset */
typedef struct {
    const void *d_rows64; const uint64_t *d_idx64; const uint32_t *d_coef64; size_t n64;   /* offsets 0, 8, 16, 24 */
    const void *d_rows32; const uint64_t *d_idx32; const uint32_t *d_coef32; size_t n32;   /* 32, 40, 48, 56 */
    const void *d_mac_store; const void *d_align_store;                                     /* 64, 72 */
    const uint64_t *d_mac_idx; const uint32_t *d_mac_coef; size_t n_macs;                   /* 80, 88, 96 */
    unsigned long long random_point;                                                        /* 104 */
} porla_kzg_audit_req;
int  porla_kzg_audit_batch_device(const porla_kzg_audit_req *reqs, size_t k, void *d_out, void *d_b_out, void *hip_stream);
/* Server::audit (IPA build) for K independent audits in ONE call, inner-product proofs included (Server.hpp:790-892 and
 * Server::inner_product_prove, :2279-2452, each): everything on the device and on hip_stream.  porla_ipa_audit_device stops before
 * the proof; this call goes through it.  gens_u_fb: a secp256k1 fixed base over the 129 points generators[0..127] || u
 * (porla_fixed_base_create(1, ...)): the audit's two Pedersen commitments use its first 128 points, the prover's rows all 129.  Fewer
 * than 129 points, or a BN254 base: PORLA_ERR_ARG.  n_cols is fixed at 128: the prover's index pattern is written for NUM_CHUNKS = 128.
 * reqs is a HOST array of K audits; the first 13 fields are porla_kzg_audit_req's, with secp256k1 stores; a_value is
 * audit_values[n_points] (Server.hpp:861) as 32 bytes big-endian, taken mod the group order n.
 * d_out receives K records of PORLA_IPA_AUDIT_RECORD_BYTES, packed back to back, the reply of Server::audit (Server.hpp:880-892):
 *   commitment(33) | combined_MAC(33) | combined_align(33) | proof(556)
 * commitment = Commit(B) over the 128 generators; combined_align is the value AFTER align_MAC (Server.hpp:850, :495-529): MSM(align
 * store) + Commit(c).  Points in libsecp256k1's compressed form: 0x02 | (y & 1), then X big-endian.  The reference cannot serialise
 * infinity (secp256k1_eckey_pubkey_serialize returns 0 and writes nothing); this library writes 33 ZERO bytes there, in the record
 * and in the proof, and hashes those 33 bytes into the transcript.
 *   proof = c(32) | 6 x (L(33) | R(33)) | a0(32) b0(32) a1(32) b1(32)
 * scalars as eight little-endian 32-bit words from the low word up (convert_ZZ_to_arr, utils.h:353-364), i.e. 32 bytes little-endian;
 * the proof of a = B, b = (v, v^2, v^4, ..., v^(2^127)), v = a_value -- repeated squaring, Server.hpp:863-867.  The transcript is the
 * reference's: one SHA-256 object that keeps being written to after each finalize, which zeroes its state while its byte counter runs
 * on (secp256k1_lib/hash_impl.h:151-165).
 * d_b_out (may be NULL): K x 128 x 32 bytes, B mod p_icc big-endian per audit, as porla_ipa_audit_device's b_out.
 * commitment, combined_MAC and B equal porla_ipa_audit_device's outputs for the same audit, and combined_align equals the secp256k1
 * sum of its combined_align and align_value.
 * Asynchronous: enqueued on hip_stream, returns without waiting on the host; the work waits for whatever the caller had enqueued on
 * hip_stream before the call; d_out is complete when hip_stream is.  No internal side stream.
 * PORLA_ERR_ARG (message in porla_gpu_last_error), checked before the device is touched: reqs, d_out or gens_u_fb NULL while k > 0; a
 * NULL array whose count is > 0; n_macs > 32 768 (the batched MSM's entry limit: larger audits keep using porla_ipa_audit_device);
 * n64 + n32 >= 2^32; a byte size that overflows.  k = 0 returns 0 and writes nothing.  Valid arguments without a device:
 * PORLA_ERR_NO_DEVICE (a fixed base exists only where a device does, so its curve and point count are read after that check).
 * One fixed sequence of launches per call, whatever K: the row combine of all K audits (two launches), the MSM gather, the batched MSM
 * over the 2K entries, ONE commitment pass over the 2K rows [c_k, B_k] and the join that writes the three points; then the prover:
 * its opening (c, the first hash), and six times the round's rows [L_k, R_k] (129 coefficients), ONE commitment pass over these 2K
 * rows, and the round's close (L, R into the proof, the next challenge, the fold of a and b).  The host round trips of the
 * single-call path are what the batch saves: measured on an MI355X it draws level with K single-call audits at K = 8 and is 6x
 * their rate at K = 64 (profiles/r09_a_ipa_audit_batch.jsonl); below 8 audits the fixed sequence (about 4.3 ms, mostly the six
 * rounds' inversion chains) is not amortised and porla_ipa_audit_device with the rounds on the host is the faster path.
 * Calls from several threads on several streams, and beside porla_ipa_audit_device and the fixed base's other users, are safe. */
#define PORLA_IPA_AUDIT_RECORD_BYTES 655   /* 33 * 3 + PORLA_IPA_PROOF_BYTES */
#define PORLA_IPA_PROOF_BYTES        556   /* 32 + 6 * 66 + 128 */
#define PORLA_IPA_AUDIT_REQ_BYTES    136   /* sizeof(porla_ipa_audit_req) on LP64; the library static_asserts it and each offset */
typedef struct {
    const void *d_rows64; const uint64_t *d_idx64; const uint32_t *d_coef64; size_t n64;   /* offsets 0, 8, 16, 24 */
    const void *d_rows32; const uint64_t *d_idx32; const uint32_t *d_coef32; size_t n32;   /* 32, 40, 48, 56 */
    const void *d_mac_store; const void *d_align_store;                                     /* 64, 72 */
    const uint64_t *d_mac_idx; const uint32_t *d_mac_coef; size_t n_macs;                   /* 80, 88, 96 */
    uint8_t a_value[32];                                                                    /* 104 */
} porla_ipa_audit_req;
int  porla_ipa_audit_batch_device(porla_fixed_base *gens_u_fb, const porla_ipa_audit_req *reqs, size_t k, void *d_out,
                                  void *d_b_out, void *hip_stream);
/* The prover alone: K proofs of Server::inner_product_prove(a, b, proof).  d_a, d_b: K x 128 x 32 bytes big-endian on the device
 * (16-byte aligned), taken mod n; d_proofs: K x PORLA_IPA_PROOF_BYTES, packed.  gens_u_fb, the proof's bytes and the contract
 * (asynchronous on hip_stream, argument checks, k = 0, no device) as porla_ipa_audit_batch_device, which runs the same code on
 * (B_k, powers of a_value). */
int  porla_ipa_prove_batch_device(porla_fixed_base *gens_u_fb, const void *d_a, const void *d_b, size_t k, void *d_proofs,
                                  void *hip_stream);
/* Client::audit's check (IPA build, Client.hpp:633-880) of K replies in ONE asynchronous call: reply k is record k of d_records
 * (PORLA_IPA_AUDIT_RECORD_BYTES each, the layout porla_ipa_audit_batch_device writes: commitment C (33) | combined_MAC M (33) |
 * combined_align A (33) | proof (556)), reqs[k] the client's side of that audit: the level's MAC complements d_comp_store (64-byte
 * big-endian affine secp256k1 points, zeros = infinity, indexed like the server's MAC store), the challenge (d_idx, d_coef, n: the
 * arrays the server's MAC MSM used), the client's alpha (32 bytes big-endian, taken mod n; the reference's is 128 bits) and a_value
 * as in porla_ipa_audit_req.  gens_u_fb: the fixed base porla_ipa_audit_batch_device takes.  d_status[k], ON THE DEVICE, receives
 *   PORLA_IPA_VERIFY_FULL       alpha C + sum_j coef_j comp[idx_j] == M + alpha A                     (Client.hpp:801-829)
 *   PORLA_IPA_VERIFY_PROOF      Client::inner_product_verify's final ge_equals_ge holds              (Client.hpp:1465-1628)
 *   PORLA_IPA_VERIFY_BVEC       b_i == sum_(j = i mod 2) a_value^(2^j) x_values[j] (mod n) for i = 0, 1, x_values the verifier's own
 *                               array after the six rounds: the proof's b0, b1 are the fold of the audit's b = (v, v^2, v^4, ...)
 *   PORLA_IPA_VERIFY_MALFORMED  one of the record's 3 + 12 compressed points breaks secp256k1_eckey_pubkey_parse's rules (first byte
 *                               2 or 3, X < p, X^3 + 7 a square) and is not the 33 zero bytes this library writes for infinity; the
 *                               other bits are then clear, and nothing is computed on the record
 * The reference's verdict is FULL | PROOF.  BVEC is an extension: inner_product_verify takes b0, b1 on trust, so a proof made for ANY
 * vector b passes it (porla_ipa_prove_batch_device with an arbitrary d_b makes such proofs); a client that wants the proof bound to
 * its challenge asks for FULL | PROOF | BVEC.  BVEC changes neither of the other two bits.  The proof's scalars (c, a0, b0, a1, b1)
 * are any 32 little-endian bytes, reduced mod n.  A challenge that is 0 mod n (probability 2^-256; NTL raises an error there) has no
 * inverse: the six inverses come from one inversion of the challenges' product, so all six are then taken as 0, and the equation
 * decides.
 * Exact per reply: no random folding, no fallback, no pairing.  Each MAC check is a pair of batched-MSM entries that sum to infinity
 * iff it holds (the complements, then (alpha, C), (n - alpha, A), (n - 1, M)); each proof check is the 13-pair entry (1, C),
 * (x_r^2, L_r), (x_r^-2, R_r) minus one row of 129 coefficients (a_(j & 1) x_values[j]; a0 b0 + a1 b1 - c for u) on gens_u_fb.
 * Asynchronous: enqueued on hip_stream, returns without waiting on the host; the work waits for whatever the caller had enqueued on
 * hip_stream before the call (d_records can come straight from porla_ipa_audit_batch_device on the same stream); d_status is
 * complete when hip_stream is.  No internal side stream.
 * PORLA_ERR_ARG (message in porla_gpu_last_error), checked before the device is touched: reqs, d_records, d_status or gens_u_fb NULL
 * while k > 0; a NULL array whose count n is > 0; n > 32 768 (the batched MSM's entry limit); a byte size that overflows.  k = 0
 * returns 0 and writes nothing.  There is no cap on k.  Valid arguments without a device: PORLA_ERR_NO_DEVICE; then a base with fewer
 * than 129 points or on BN254: PORLA_ERR_ARG.
 * One fixed sequence of launches per call, whatever K: the work-list upload, k_ipa_verify_prep (a block per reply: the transcript's
 * six challenges, ONE inversion mod n, x_values, the row, the 3-pair and 13-pair entries, the fifteen decompressions, BVEC),
 * k_ipa_verify_gather (the complement entries), the batched MSM over the 3K entries, ONE commitment pass over the K rows and
 * k_ipa_verify_join (a lane per reply: both sums against infinity, the status byte).  Not yet measured on an MI355X
 * (tools/bench_ipa_verify_batch.py; DESIGN.md section 4 has what is expected).  Calls from several threads on several
 * streams, and beside porla_ipa_audit_batch_device and the fixed base's other users, are safe. */
#define PORLA_IPA_VERIFY_REQ_BYTES 96      /* sizeof(porla_ipa_verify_req) on LP64; the library static_asserts it and each offset */
#define PORLA_IPA_VERIFY_FULL      1
#define PORLA_IPA_VERIFY_PROOF     2
#define PORLA_IPA_VERIFY_MALFORMED 4
#define PORLA_IPA_VERIFY_BVEC      8
typedef struct {
    const void *d_comp_store;                                  /* 0 */
    const uint64_t *d_idx; const uint32_t *d_coef; size_t n;   /* 8, 16, 24 */
    uint8_t alpha[32];                                         /* 32 */
    uint8_t a_value[32];                                       /* 64 */
} porla_ipa_verify_req;
int  porla_ipa_verify_batch_device(porla_fixed_base *gens_u_fb, const porla_ipa_verify_req *reqs, size_t k, const void *d_records,
                                   uint8_t *d_status, void *hip_stream);
/* Client::audit's check (KZG build, Client.hpp:633-880) of K replies in ONE call: reply k is the 320-byte record k of d_records
 * (the layout porla_kzg_audit_batch_device writes: commitment C | proof_h H | point z | claim y | combined_mac M | combined_align A),
 * reqs[k] the client's side of that audit: the level's MAC complements d_comp_store (64-byte big-endian affine points, as
 * compute_digest_complement / porla_kzg_complement_batch_device give them, indexed like the server's MAC store), the challenge
 * (d_idx, d_coef, n: the arrays the server's MAC MSM used) and the client's alpha (32 bytes big-endian, taken mod r as mult_point
 * takes its scalar; the reference's is SECRET_KEY in bytes 16..31).  status[k] receives
 *   PORLA_KZG_VERIFY_FULL       alpha C + sum_j coef_j comp[idx_j] == M + alpha A      (the MAC check, Client.hpp:849-869)
 *   PORLA_KZG_VERIFY_PROOF      the opening verifies: verify_proof(C, H, z, y)           (Client.hpp:868, main.go:177-193)
 *   PORLA_KZG_VERIFY_MALFORMED  a point of the record has a coordinate >= p or is off y^2 = x^3 + 3 (64 zero bytes = infinity is
 *                               well-formed); the other two bits are then clear
 * and the audit passes iff status == FULL | PROOF.  For a well-formed record both bits are exactly the reference's verdicts
 * (compute_multi_exp, mult_point, add_point and compare_commitment for FULL; verify_proof for PROOF).
 * How: each MAC check is one MSM entry that sums to infinity iff it holds (the complements, then (alpha, C), (r - alpha, A),
 * (r - 1, M)); the K openings are weighted with secret random 128-bit scalars w_k and folded into ONE two-pairing check
 *   e(P, G2) * e(-Q, tau G2) == 1,   P = sum w_k (C_k - y_k G + z_k H_k),   Q = sum w_k H_k   (G = G1[0] of the SRS)
 * -- verify_proof's form summed over k.  The MSMs run on the device (the batched MSM: K complement entries, K 3-pair entries, P
 * with 3K pairs and Q), the pairing on the host.  When the folded check holds, every well-formed reply gets PROOF; when it fails,
 * verify_proof's predicate runs for every well-formed reply on up to 16 host threads (about 0.9 ms of CPU per reply), so a batch
 * with a bad opening costs K single checks on top of the batch, and its verdicts stay exact.
 * Soundness: with weights uniformly random, nonzero, 128-bit and unknown to the prover, a batch that contains an invalid opening
 * passes the folded check with probability <= 2^-128.  weights = NULL (the normal use): drawn per call from the operating system's
 * random source (getrandom).  Caller-supplied weights (k x 16 bytes big-endian, nonzero) must be just as secret and random;
 * equal weights, for instance, let two openings whose claims are off by +d and -d cancel.
 * Blocking: the call returns when status is written (the pairing runs on the host).  Its device work runs on hip_stream and waits
 * for whatever the caller had enqueued there before the call, so d_records can come straight from porla_kzg_audit_batch_device on
 * the same stream with no host wait in between.  d_comp_store, d_idx, d_coef and d_records are device pointers; reqs, weights and
 * status are host memory.
 * PORLA_ERR_ARG (message in porla_gpu_last_error), checked before the device is touched: reqs, d_records or status NULL while
 * k > 0; a NULL array whose count n is > 0; n > 32 768 (the batched MSM's entry limit, as for the server batch); an all-zero
 * weight; k > PORLA_KZG_VERIFY_MAX_K (the folded entry P holds 3 pairs per reply, at most 32 768: larger batches go in several
 * calls); a byte size that overflows.  k = 0 returns 0 and writes nothing.  No SRS or no G2 points loaded: PORLA_ERR_STATE.  Valid
 * arguments without a device: PORLA_ERR_NO_DEVICE.
 * One fixed sequence of launches per call: the work-list upload, k_kzg_verify_prep (a lane per reply: validation, the 3-pair and
 * folded entries), k_kzg_verify_gather (the complement entries), the batched MSM over the 2K + 2 entries with projective sums,
 * k_kzg_verify_join (the MAC verdicts, P and Q to affine with one inversion), one copy back of 128 + K bytes.  Calls from several
 * threads on several streams, and beside verify_proof and porla_kzg_audit_batch_device, are safe. */
#define PORLA_KZG_VERIFY_REQ_BYTES 64      /* sizeof(porla_kzg_verify_req) on LP64; the library static_asserts it and each offset */
#define PORLA_KZG_VERIFY_MAX_K     10922   /* floor(32768 / 3) replies per call */
#define PORLA_KZG_VERIFY_FULL      1
#define PORLA_KZG_VERIFY_PROOF     2
#define PORLA_KZG_VERIFY_MALFORMED 4
typedef struct {
    const void *d_comp_store;                                  /* 0 */
    const uint64_t *d_idx; const uint32_t *d_coef; size_t n;   /* 8, 16, 24 */
    uint8_t alpha[32];                                         /* 32 */
} porla_kzg_verify_req;
int  porla_kzg_verify_batch_device(const porla_kzg_verify_req *reqs, size_t k, const void *d_records, const uint8_t *weights,
                                   uint8_t *status, void *hip_stream);
/* The last encode stage of a large CRebuild (KZG build) in ONE call, everything resident in HBM (porla/Server/Server.hpp:1487-1833,
 * :2059-2065): rows_in = n_rows x n_samples raw 32-byte chunks; outputs per part (X, Y): the rows mod p_icc (aligned_x / aligned_y:
 * n_rows * n_samples * 32 bytes each, may be NULL), the alignment scalars of BOTH parts back to back (scalars_xy: 2 * n_rows *
 * n_samples * 32 bytes, X first), their commitments (commits_xy: 2 * n_rows * 64 bytes: compute_digest_from_srs per row), and the
 * two MAC encodes (macs_in / macs_x / macs_y: n_rows points of 64 bytes).  = porla_icc_encode_xy_device + ONE
 * porla_kzg_commit_batch_device over the 2 n rows + porla_icc_mac_encode_xy_device, the MAC network on a second stream inside,
 * started first and with register room kept for it on every SIMD (the two sides overlap instead of queueing).  Asynchronous on
 * hip_stream; same bytes as the separate calls. */
int  porla_kzg_crebuild_stage_device(const void *d_rows_in, size_t n_rows, unsigned long long write_step, void *d_aligned_x,
                                     void *d_aligned_y, void *d_scalars_xy, void *d_commits_xy, const void *d_macs_in,
                                     void *d_macs_x, void *d_macs_y, void *hip_stream);
/* rows resident on the device, results wanted on the host at once (the audit's align_MAC commitment on the scalars
 * porla_audit_combine_device left in HBM, Server.hpp:903 -> :550-560): up to 64 rows run as ONE launch on hip_stream, behind whatever
 * produced the rows there, and the call returns when the pinned result has arrived; blocking */
int  porla_kzg_commit_batch_device_to_host(const void *d_rows, size_t n_rows, uint8_t *out /* n_rows * 64 */, void *hip_stream);
/* the same with the row range split over `devices` GPUs of this process (0 = every visible one), one host thread and one
 * resident copy of the SRS table per device; rows are independent, nothing is exchanged (Server.hpp:1077-1078, 2061-2062) */
int  porla_kzg_commit_batch_host_multi(const uint8_t *rows, size_t n_rows, uint8_t *out, int devices);
/* frees the HBM copies of the KZG state (SRS + window table, one-point tables, scratch); rebuilt on the next use */
int  porla_kzg_release_device_memory(void);
/* Client side, batched (Client::initialize computes both per block, porla/Client/Client.hpp:408-455):
 *   digest     = compute_digest (main.go:70-89) per row: alpha * f(tau) * G1[0]; rows as for commit_batch
 *   complement = compute_digest_complement (main.go:91-101) per scalar: s * h_MAC; scalars 32 bytes big-endian each
 *                (the reference passes its 16-byte AES output: left-pad it with 16 zero bytes)
 * Needs init_key + init_SRS in this process (tau, alpha and the hiding base are the client's secrets). */
int  porla_kzg_digest_batch_device(const void *d_rows, size_t n_rows, void *d_out, void *hip_stream);
int  porla_kzg_complement_batch_device(const void *d_scalars, size_t n, void *d_out, void *hip_stream);
/* the block's MAC as the client sends it -- digest(row r) + complement(scalar r), the add_point of Client.hpp:229-236 / 468-478
 * included -- as one two-coefficient commitment per row against the table of (G1[0], h_MAC): d_out[r] = 64 bytes */
int  porla_kzg_mac_batch_device(const void *d_rows, const void *d_scalars, size_t n_rows, void *d_out, void *hip_stream);
/* the three batches on caller-owned host buffers (pageable is fine): staged, computed on the engine's stream, copied back; blocking.
 * The copies dominate -- 4 KiB per block over PCIe */
int  porla_kzg_digest_batch_host(const uint8_t *rows, size_t n_rows, uint8_t *out);
int  porla_kzg_complement_batch_host(const uint8_t *scalars, size_t n, uint8_t *out);
int  porla_kzg_mac_batch_host(const uint8_t *rows, const uint8_t *scalars, size_t n_rows, uint8_t *out);
/* diagnostics of the host pairing behind verify_proof (main.go:177-193): scalar * G2 generator as 128 bytes
 * X.A1 || X.A0 || Y.A1 || Y.A0 big-endian; e(p1, q1) * e(p2, q2) == 1 ? (returns 1 / 0; slow = 1: the literal form with
 * affine Miller steps and the exponent (p^12 - 1)/r, kept as the reference for the fast form) */
int  porla_bn254_g2_mul_generator(const uint8_t scalar_be[32], uint8_t out[128]);
int  porla_bn254_pairing_product_is_one(const uint8_t p1[64], const uint8_t q1[128], const uint8_t p2[64], const uint8_t q2[128],
                                        int slow);
/* the same predicate on EIP-197's own input layout, any number of pairs: n_pairs x 192 bytes (G1 X || Y, then G2
 * x_im || x_re || y_im || y_re, 32-byte big-endian each; zeros = infinity).  1 / 0; PORLA_ERR_ARG for inputs the precompile
 * rejects (coordinate >= p, point off its curve, G2 point outside the order-r subgroup).  Host code, no device needed. */
int  porla_bn254_pairing_check(const uint8_t *input, size_t n_pairs, int slow);
/* window bits used when the SRS table is (re)built; 0 = automatic */
int  porla_kzg_set_commit_window(int window_bits);
/* diagnostic: window bits / windows per coefficient of the SRS table currently resident (0, 0 before the first batch) */
int  porla_kzg_commit_shape(int *window_bits, int *windows);
/* coefficients per commitment row = the SRS size given to init_SRS / init_SRS_from_data (main.go:45-68; the reference's
 * NUM_CHUNKS = 128, config.hpp), 0 before either ran: the row stride of every *_batch_* entry point is 32 bytes times this */
int  porla_kzg_row_coefficients(size_t *n_out);

/* ---- ICC encode (CRebuild_Cached data part + align_MAC scalar part) ----
 * rows_in : n_rows * n_cols elements, 32 bytes little-endian each (8 x uint32 LE words, utils.h:353-364; the layout
 *           of the U/<i> block files, utils.h:592-608), row-major; n_rows a power of two >= 2; n_cols = NUM_CHUNKS = 128
 * curve   : 0 = BN254 order (ENABLE_KZG), 1 = secp256k1 order (IPA)  -- selects q in LCM = p_icc * q (utils.h:33-34,42-43)
 * part    : 0 = X part; 1 = Y part (elements pre-scaled by wt = w^reverse_bits(write_step % n_rows, height-1),
 *           Server.hpp:1494,1522)
 * x_out   : n_rows * n_cols * 64 bytes, values in [0, LCM) little-endian (512-bit row format, utils.h:473-517)  (or NULL)
 * aligned : n_rows * n_cols * 32 bytes, values mod p_icc little-endian (256-bit row format)                     (or NULL)
 * scalars : n_rows * n_cols * 32 bytes, alignment scalars c = (A mod p_icc - A) mod q (Server.hpp:535-538),
 *           big-endian (bn254_scalar, utils.h:307-318) or, with scalar_le = 1, little-endian limbs
 *           (secp256k1_scalar d[4], scalar_4x64.h:13-15)                                                        (or NULL) */
int porla_icc_encode_device(const void *d_rows_in, size_t n_rows, size_t n_cols, int curve, unsigned long long write_step,
                            int part, void *d_x_out, void *d_aligned_out, void *d_scalars_out, int scalar_le,
                            void *hip_stream);
int porla_icc_encode_host(const uint8_t *rows_in, size_t n_rows, size_t n_cols, int curve, unsigned long long write_step,
                          int part, uint8_t *x_out, uint8_t *aligned_out, uint8_t *scalars_out, int scalar_le);
/* Column sharding (the reference splits the columns of every stage over its 8 pool threads, Server.hpp:1564-1686; the 128
 * per-column transforms are independent): only columns [col_begin, col_end) of the row-major input are uploaded (strided),
 * encoded and written back into the same columns of the full-width outputs.  One process per GPU: rank g passes
 * porla_shard_range(n_cols, g, G) -- 16 columns each on 8 GPUs; or let _host_multi run `devices` GPUs of this process
 * (0 = every visible one) from one host thread each.  No collective. */
/* BOTH parts from one run of the network (device pointers; any output may be NULL): the network is linear over Z/LCM and the Y
 * part's chunks are the X part's times wt (Server.hpp:1494, :1512-1522), so Y_k = wt X_k mod LCM -- one product per residue and
 * symbol in the last pass instead of a second encode; the bytes are those of the part = 0 and part = 1 calls */
int porla_icc_encode_xy_device(const void *d_rows_in, size_t n_rows, size_t n_cols, int curve, unsigned long long write_step,
                               void *d_x_out, void *d_aligned_out, void *d_scalars_out, void *d_y_x_out, void *d_y_aligned_out,
                               void *d_y_scalars_out, int scalar_le, void *hip_stream);
int porla_icc_encode_cols_host(const uint8_t *rows_in, size_t n_rows, size_t n_cols, size_t col_begin, size_t col_end, int curve,
                               unsigned long long write_step, int part, uint8_t *x_out, uint8_t *aligned_out,
                               uint8_t *scalars_out, int scalar_le);
int porla_icc_encode_host_multi(const uint8_t *rows_in, size_t n_rows, size_t n_cols, int curve, unsigned long long write_step,
                                int part, uint8_t *x_out, uint8_t *aligned_out, uint8_t *scalars_out, int scalar_le, int devices);

/* ---- MAC-side ICC encode ("FFT in the exponent": the MAC halves of CRebuild_Cached, Server.hpp:1523-1536 init
 * scaling, :1590-1609 / :1658-1676 butterflies tm = v^j * MAC[k+m2]; MAC[k] = um + tm; MAC[k+m2] = um - tm; client twin
 * Client.hpp:1040-1453) ----
 * macs_in / macs_out : n_rows points, 64 bytes X||Y big-endian affine each (KZG MAC_Block, utils.h:65; for IPA the
 *           include shim converts secp256k1_gej <-> this canonical form), n_rows a power of two >= 2
 * curve, write_step, part : as for porla_icc_encode_* (part 1 = Y: inputs pre-multiplied by wt) */
int porla_icc_mac_encode_device(const void *d_macs_in, size_t n_rows, int curve, unsigned long long write_step, int part,
                                void *d_macs_out, void *hip_stream);
/* BOTH parts from one butterfly network (what CRebuild_Cached needs: Server.hpp:1548-1687 X part, :1691-1830 Y part): the network
 * is linear over Z_q and the Y part's inputs are wt * MAC_U (:1528-1536), so Y_k = wt * X_k -- one scalar multiplication per
 * row instead of a second run of log2(n_rows) dependent stages; the 64 output bytes per point are those of the two single-part
 * calls */
int porla_icc_mac_encode_xy_device(const void *d_macs_in, size_t n_rows, int curve, unsigned long long write_step,
                                   void *d_macs_x_out, void *d_macs_y_out, void *hip_stream);
int porla_icc_mac_encode_xy_host(const uint8_t *macs_in, size_t n_rows, int curve, unsigned long long write_step,
                                 uint8_t *macs_x_out, uint8_t *macs_y_out);
int porla_icc_mac_encode_host(const uint8_t *macs_in, size_t n_rows, int curve, unsigned long long write_step, int part,
                              uint8_t *macs_out);
/* row counts <= n_rows use the matrix form (N commitments against the per-call base), larger ones the stage-by-stage ladder
 * form.  Default 0 = always the ladder, which since round 5 is the faster one at every size; the matrix form stays as an
 * independent formulation of the same map (the tests run both).  Both are bit-exact. */
int porla_icc_mac_set_matrix_max(size_t n_rows);

/* ---- Server::mix, the incremental form of one butterfly stage between two sub-levels (Server.hpp:1209-1328) ----
 * data part (Server.hpp:1269-1278): out[i] = (A0[i] + v^i A1[i]) % LCM, out[i+len] = (A0[i] - v^i A1[i]) % LCM, v = w^(n_total/len)
 *   a0, a1 : len x n_cols symbols, 64 bytes little-endian each, values < LCM (512-bit rows, utils.h:473-517); out : 2*len rows
 * MAC part (Server.hpp:1281-1318, used for the MACs and for the alignments): the same on 64-byte big-endian affine points.
 * len and n_total (= num_blocks, which fixes w) are powers of two, len <= n_total. */
int porla_icc_mix_device(const void *d_a0, const void *d_a1, size_t len, size_t n_cols, size_t n_total, int curve, void *d_out,
                         void *hip_stream);
int porla_icc_mix_host(const uint8_t *a0, const uint8_t *a1, size_t len, size_t n_cols, size_t n_total, int curve, uint8_t *out);
int porla_icc_mac_mix_device(const void *d_a0, const void *d_a1, size_t len, size_t n_total, int curve, void *d_out, void *hip_stream);
/* both point butterflies of a mix -- the MAC commitments (a) and the MAC alignments (b), same v^i -- in one launch */
int porla_icc_mac_mix_pair_device(const void *d_a0, const void *d_a1, const void *d_b0, const void *d_b1, size_t len, size_t n_total,
                                  int curve, void *d_out_a, void *d_out_b, void *hip_stream);
int porla_icc_mac_mix_host(const uint8_t *a0, const uint8_t *a1, size_t len, size_t n_total, int curve, uint8_t *out);
/* Server::mix(is_x, level) in one call: the data rows on hip_stream, both point arrays on a second stream beside them; asynchronous
 * (hip_stream continues when all three outputs are written) */
int porla_server_mix_device(const void *d_data_a0, const void *d_data_a1, const void *d_mac_a0, const void *d_mac_a1,
                            const void *d_align_a0, const void *d_align_a1, size_t len, size_t n_cols, size_t n_total, int curve,
                            void *d_data_out, void *d_mac_out, void *d_align_out, void *hip_stream);

/* ---- Server::HAdd / Client::HAdd and the HRebuild chains (Server.hpp:1388-1477, 1329-1386; Client.hpp:978-1038) ----
 * HAdd's arithmetic on ONE incoming block (the level bookkeeping around it stays the caller's):
 *   porla_icc_hadd_host      data_b2[i] = (data[i] * wt) mod p_icc and the alignment scalars c_i = (data_b2[i] - data[i] * wt) mod q
 *                            (align_MAC, Server.hpp:531-541 / 495-504), wt = w^reverse_bits(write_step % n_total, height-1);
 *                            wt_scalar_out: wt as the 32-byte big-endian scalar of the MAC side (convert_ZZ_to_scalar)
 *   porla_icc_mac_scale_host MAC_B2 = wt * MAC (host: one 64-byte operand; also Client::HAdd, Client.hpp:996-1014)
 *   porla_kzg_hadd_host      all three outputs of Server::HAdd for the KZG build: data_B2, MAC_B2 and MAC_align_B2 = Commit(c)
 *                            (IPA: take the scalars of porla_icc_hadd_host with scalar_le = 1 to the generators' fixed base,
 *                            porla_fixed_base_commit_host, or to secp256k1_ecmult_multi_var through the shim)
 * HRebuildX / HRebuildY: the chain of mixes that carries the block up to `level`, on the device in one call.  levels[i] points at
 * level i's rows (i <= level): 2 * 2^i rows, the first 2^i resident, the second 2^i incoming (levels[0] + one row = the new block);
 * step i mixes the halves of level i (Server::mix / Client::mix) into the incoming half of level i + 1; at the end level
 * `level`'s incoming half is copied over its resident half, as the reference does.  A row is n_cols 64-byte symbols
 * (porla_icc_hrebuild_host: the data levels) or one 64-byte affine point (porla_icc_mac_hrebuild_host: MAC commitments,
 * MAC alignments, the client's complements). */
int porla_icc_hadd_host(const uint8_t *data_in, size_t n_cols, size_t n_total, unsigned long long write_step, int curve,
                        uint8_t *data_b2_out, uint8_t *scalars_out, int scalar_le, uint8_t wt_scalar_out[32]);
int porla_icc_mac_scale_host(const uint8_t mac_in[64], size_t n_total, unsigned long long write_step, int curve, uint8_t mac_out[64]);
int porla_kzg_hadd_host(const uint8_t *data_in, const uint8_t mac_in[64], size_t n_total, unsigned long long write_step,
                        uint8_t *data_b2_out, uint8_t mac_b2_out[64], uint8_t mac_align_b2_out[64]);
int porla_icc_hrebuild_host(uint8_t *const *levels, int level, size_t n_cols, size_t n_total, int curve);
int porla_icc_mac_hrebuild_host(uint8_t *const *levels, int level, size_t n_total, int curve);

/* ---- Server::update's H path for K independent files in ONE asynchronous call (Server.hpp:401-476: HAdd :1388-1477, HRebuildX /
 * HRebuildY :1329-1386, mix :1209-1328, the complement adds :449-469) ----
 * The level stores -- data rows, MAC commitments, MAC alignments, X and Y parts -- stay in HBM, where the batched audits read them;
 * the host wrappers above carry one block through host buffers and wait.  Request a is one write to one file:
 *   d_block        n_cols x 32 bytes little-endian raw chunks (any 256-bit values)
 *   d_mac          the block's MAC, 64 bytes big-endian affine (zeros = infinity)
 *   d_complements  2 * 2^level points of 64 bytes (2^level for the X part, then 2^level for Y), or NULL = none
 *   write_step     the value HAdd sees (after the ++ of Server.hpp:431); write_step % n_total == 0 is CRebuild's step and refused
 *                  (that step: porla_server_rebuild_batch_device; the client's side of it: porla_*_client_rebuild_batch_device)
 *   level          the level HAdd lands on (0 = level 0 was empty); pad must be 0
 *   data_x .. align_y  HOST arrays of level + 1 DEVICE pointers: family[i] = level i's 2 * 2^i rows as porla_icc_hrebuild_host lays them
 *                  out (the first 2^i resident, the second 2^i incoming; a data row = n_cols 64-byte little-endian symbols < LCM, a
 *                  point row = one 64-byte affine point)
 * n_cols = the SRS size (KZG) or 128 (IPA); n_total = num_blocks, a power of two >= 2; the curve is the entry point's.
 * Per request, byte for byte the reference's sequence:
 *   HAdd      wt = w^reverse_bits(write_step % n_total, height-1); data X row = the chunks, data Y row = (chunk * wt) mod p_icc (both
 *             zero-extended to 64 bytes); MAC X = MAC, MAC Y = wt * MAC; align X = infinity, align Y = Commit(c), c = (Y - chunk * wt)
 *             mod q, against the resident SRS (KZG) or generators_fb's first 128 points (IPA).  level == 0: row 0 of level 0, and the
 *             request is done apart from its complements; otherwise row 1, the incoming half.
 *   HRebuild  for i < level: the halves of family[i] mixed into the incoming half of family[i+1] (the arithmetic of
 *             porla_icc_mix_device / porla_icc_mac_mix_pair_device, v = w^(n_total / 2^i)), all six families; then the incoming half
 *             of family[level] copied over its resident half.
 *   complements  mac_x[level][j] += comp[j], mac_y[level][j] += comp[2^level + j], j < 2^level: the RESIDENT half only.
 * Rows the reference does not write stay untouched.
 * Contract: asynchronous on hip_stream -- no host wait, no internal side stream; the work waits for whatever was enqueued on
 * hip_stream before the call and the levels are complete when the stream is.  Two writes to the same file go in two calls on one
 * stream, with no host synchronisation between them.  The launch sequence depends on the highest level of the call, not on k.
 * PORLA_ERR_ARG (with a message, before the device is touched): NULL reqs with k > 0; a NULL block, MAC, family array or level
 * pointer; n_total not a power of two or < 2; level < 0 or 2^level > n_total; write_step % n_total == 0; pad != 0; two requests of
 * one call naming the same level-0 pointer in any family (requests must be disjoint); IPA: a NULL base, a BN254 base, a base with
 * fewer than 128 points.  k = 0 returns 0 and does nothing; no SRS (KZG): PORLA_ERR_STATE; valid arguments without a device:
 * PORLA_ERR_NO_DEVICE.  Thread-safe beside the audits and the mixes (the twiddle tables are used under the workspace locks and fences
 * of porla_icc_mix_device / porla_icc_mac_mix_device).
 * Not yet measured on an MI355X: tools/bench_update_batch.py times it against the composition of the single-step entry points. */
#define PORLA_UPDATE_REQ_BYTES 88   /* sizeof(porla_update_req) on LP64; the library static_asserts it and each offset */
typedef struct {
    const void *d_block;
    const void *d_mac;
    const void *d_complements;
    unsigned long long write_step;
    int level; int pad;
    void *const *data_x, *const *data_y;
    void *const *mac_x,  *const *mac_y;
    void *const *align_x, *const *align_y;
} porla_update_req;
int porla_kzg_update_batch_device(const porla_update_req *reqs, size_t k, size_t n_total, void *hip_stream);
int porla_ipa_update_batch_device(porla_fixed_base *generators_fb, const porla_update_req *reqs, size_t k, size_t n_total,
                                  void *hip_stream);

/* ---- Client::update's preprocessing for K independent writes in ONE asynchronous call (Client.hpp:457-614: the block's MAC,
 * compute_MAC_complement for every slot below the level the write lands on, Client::HAdd -> HRebuildX / HRebuildY :978-1038 on them,
 * mix :921-976, and the differences "new complement - mixed complement" that go on the wire) ----
 * The other side of porla_*_update_batch_device: d_mac_out and d_complements_out are what porla_update_req takes as d_mac and
 * d_complements, and d_block is the SAME buffer.  AES may stay on the host -- the caller passes the 16-byte AES_encrypt outputs of
 * compute_MAC_complement raw -- or d_prf is made on the device by porla_mac_prf_batch_device from porla_client_prf_runs' list.
 * Request a is one write:
 *   d_block            n_cols x 32 bytes little-endian raw chunks (any 256-bit values; reduced mod the group order)
 *   d_prf              2^(level+2) - 1 PRF outputs of 16 raw bytes: [0] the block's own complement (compute_MAC_complement(0, block_id),
 *                      :467); then for i = 0 .. level-1 level i's resident complements, X part j = 0 .. 2^i-1, then Y part (the values
 *                      of :525-534); then the 2 * 2^level new ones of :586-588 in loop order.  A value is read as the reference reads
 *                      it: KZG a big-endian 128-bit integer (compute_digest_complement), IPA r.d[0], r.d[1] as little-endian 64-bit
 *                      words (:435-436)
 *   d_mac_out          64 bytes big-endian affine (zeros = infinity)
 *   d_complements_out  2 * 2^level points of 64 bytes, X part then Y part
 *   write_step         the value Client::HAdd sees (after the ++ of :480); level: the level the write lands on; pad must be 0
 * All four pointers are device memory, 16-byte aligned.  n_cols = the SRS size (KZG) or 128 (IPA); n_total = num_blocks.
 * Per request, byte for byte the reference's sequence:
 *   1. comp0 = prf[0] * h; MAC = Commit_alpha(block) + comp0.  KZG: compute_digest of the chunks (alpha f(tau) G1[0]) and h = h_MAC:
 *      the bytes of porla_kzg_mac_batch_device on the big-endian form of the same chunks.  IPA: sum (chunk_i mod n) *
 *      alpha_generators[i] over the first 128 points of alpha_generators_fb, h = the one point of h_fb.
 *   2. cH[i].X[j], cH[i].Y[j] = prf * h for i < level.
 *   3. Client::HAdd(comp0, level), wt = w^reverse_bits(write_step % n_total, height-1) as the MAC side's scalar: level 0: X[0] = comp0,
 *      Y[0] = wt * comp0; otherwise X[1] = comp0, Y[1] = wt * comp0 and for i < level the halves of level i mixed into the incoming
 *      half of level i + 1 (the arithmetic of porla_icc_mac_mix_device, v = w^(n_total / 2^i)), X and Y.  T = the level-`level` result.
 *   4. out[j] = new_X[j] - T_X[j], out[2^level + j] = new_Y[j] - T_Y[j], j < 2^level.
 * The pyramid of intermediate complements (4 * 2^level points per part and request) lives in the library's workspace.
 * Contract: that of porla_*_update_batch_device -- asynchronous on hip_stream, no host wait, no internal side stream; the work waits
 * for whatever was enqueued on hip_stream before the call and the outputs are complete when the stream is, so the server update batch
 * can be enqueued right behind it on the same stream and buffers with no synchronisation.  The launch sequence depends on the
 * highest level of the call, not on k: two fixed-base passes per call (the k block rows; every PRF scalar of the call).
 * PORLA_ERR_ARG (with a message, before the device is touched): NULL reqs with k > 0; a NULL or misaligned block, prf or output
 * pointer; n_total not a power of two or < 2; level < 0 or 2^level > n_total / 2; write_step % n_total == 0 (CRebuild's step:
 * porla_*_client_rebuild_batch_device); pad
 * != 0; two requests naming the same output pointer; IPA: a NULL base, a BN254 base, alpha_generators_fb with fewer than 128 points,
 * h_fb without exactly one point.  k = 0 returns 0; KZG without init_key + init_SRS: PORLA_ERR_STATE; no device: PORLA_ERR_NO_DEVICE.
 * tools/bench_client_update_batch.py times it against the composition of the entry points a caller had before
 * (profiles/r13_a_client_update_batch.jsonl, DESIGN s4). */
#define PORLA_CLIENT_UPDATE_REQ_BYTES 48   /* sizeof(porla_client_update_req) on LP64; the library static_asserts it and each offset */
typedef struct {
    const void *d_block;
    const void *d_prf;
    void       *d_mac_out;
    void       *d_complements_out;
    unsigned long long write_step;
    int level; int pad;
} porla_client_update_req;
int porla_kzg_client_update_batch_device(const porla_client_update_req *reqs, size_t k, size_t n_total, void *hip_stream);
int porla_ipa_client_update_batch_device(porla_fixed_base *alpha_generators_fb, porla_fixed_base *h_fb,
                                         const porla_client_update_req *reqs, size_t k, size_t n_total, void *hip_stream);

/* ---- the client's rebuild write, Client::CRebuild's step, for K independent writes in ONE asynchronous call (Client.hpp:483-502: all
 * n_total complements recomputed, the whole MAC-side network over them :1040-1453, X part and Y part, and the 2 * n_total differences
 * of the wire loop :584-614) ----
 * The write porla_*_client_update_batch_device refuses (write_step % n_total == 0), behind the same contract.  On the client every
 * point of this step is a known scalar times the ONE hiding point h, and the network is linear over Z_q (its multipliers are the
 * integers v^j mod p_icc, which the group reduces mod its order), so the library runs the butterflies on scalars mod q and spends one
 * fixed-base pass on the results: out = (new - T) * h.  Request a is one write:
 *   d_block            n_cols x 32 bytes little-endian raw chunks, as porla_client_update_req
 *   d_prf              3 * n_total + 1 PRF outputs of 16 raw bytes in the order the reference draws them: [0] the block's own complement
 *                      (:467); [1 .. n_total] complements_U[0 .. n_total-1] (:494-497); then the 2 * n_total new ones of :586-588 in
 *                      loop order, X then Y.  A value is read as porla_client_update_req.d_prf documents (KZG big-endian, IPA r.d[0],
 *                      r.d[1] little-endian words)
 *   d_mac_out          64 bytes big-endian affine (zeros = infinity)
 *   d_complements_out  2 * n_total points of 64 bytes, X part then Y part
 *   write_step         the value Client::CRebuild sees.  The protocol passes a multiple of n_total (wt = 1); any value is accepted
 * All four pointers are device memory, 16-byte aligned.  n_cols = the SRS size (KZG) or 128 (IPA); n_total = num_blocks.
 * Per request, byte for byte the reference's sequence:
 *   1. comp0 = prf[0] * h; MAC = Commit_alpha(block) + comp0: step 1 of the client update batch, the same block pass.
 *   2. X_i = complements_U[i] = prf[1 + i] * h, Y_i = wt * X_i, wt = w^reverse_bits(write_step % n_total, height-1) as the MAC side's
 *      scalar; then the stages s = 1 .. height-1 of :1083-1450: the result of porla_icc_mac_encode_xy_device on the complements.
 *   3. out[j] = new_X[j] - X_j, out[n_total + j] = new_Y[j] - Y_j, j < n_total.
 * The server's side of this write: porla_server_rebuild_batch_device takes d_mac_out and d_complements_out as its d_mac and
 * d_complements, on the same stream with no synchronisation in between.
 * Contract: that of porla_*_client_update_batch_device -- asynchronous on hip_stream, no host wait, no internal side stream; the
 * outputs are complete when the stream is.  The launch sequence depends on n_total, not on k: the block pass over the k rows, the
 * network (the stages up to T = 1024 symbols in one launch on LDS tiles, one launch per later stage), ONE fixed-base pass over the
 * k * (2 * n_total + 1) scalars.  The twiddles are the MAC side's table, used under its lock and fence.
 * PORLA_ERR_ARG (with a message, before the device is touched): NULL reqs with k > 0; a NULL or misaligned block, prf or output
 * pointer; n_total not a power of two or < 2; two requests naming the same output pointer; IPA: a NULL base, a BN254 base,
 * alpha_generators_fb with fewer than 128 points, h_fb without exactly one point.  k = 0 returns 0; KZG without init_key + init_SRS:
 * PORLA_ERR_STATE; no device: PORLA_ERR_NO_DEVICE.
 * NOT MEASURED on an MI355X yet: tools/bench_client_rebuild.py times it against the composition of the entry points a caller had
 * before (two complement passes, porla_icc_mac_encode_xy_device, host subtractions; profiles/r14_a_client_rebuild.jsonl, DESIGN s4). */
#define PORLA_CLIENT_REBUILD_REQ_BYTES 40   /* sizeof(porla_client_rebuild_req) on LP64; the library static_asserts it and each offset */
typedef struct {
    const void *d_block;
    const void *d_prf;
    void       *d_mac_out;
    void       *d_complements_out;
    unsigned long long write_step;
} porla_client_rebuild_req;
int porla_kzg_client_rebuild_batch_device(const porla_client_rebuild_req *reqs, size_t k, size_t n_total, void *hip_stream);
int porla_ipa_client_rebuild_batch_device(porla_fixed_base *alpha_generators_fb, porla_fixed_base *h_fb,
                                          const porla_client_rebuild_req *reqs, size_t k, size_t n_total, void *hip_stream);

/* ---- the server's rebuild write, the step of Server::update that calls CRebuild instead of HAdd, for K independent files in ONE
 * asynchronous call (Server.hpp:413-469 with CRebuild_Cached :1487-1833) ----
 * The write porla_*_update_batch_device refuses (write_step % n_total == 0) and the other side of
 * porla_*_client_rebuild_batch_device: d_mac and d_complements are that call's d_mac_out and d_complements_out, d_block the SAME
 * buffer.  This form of the rebuild commits nothing, so it needs no SRS, key or fixed base: the curve is an argument (0 = BN254 / KZG,
 * 1 = secp256k1 / IPA) and one symbol serves both builds.  Request a is one write to one file:
 *   d_block        n_cols x 32 bytes little-endian raw chunks: the incoming block
 *   d_mac          its MAC, 64 bytes big-endian affine (zeros = infinity)
 *   d_complements  2 * n_total points of 64 bytes, X part then Y part, or NULL = none
 *   d_u_blocks     the file's raw store U: n_total x n_cols x 32 bytes;  d_u_macs: MAC_commitments_U, n_total x 64 bytes
 *   d_data_x .. d_align_y  the TOP level (log2 n_total) of the six families in the layout porla_update_req's families have there:
 *                  2 * n_total rows, the resident half first, then the incoming half (a data row = n_cols 64-byte little-endian symbols
 *                  < LCM, a point row = one 64-byte affine point).  A pointer the update batch was given as family[log2 n_total] is
 *                  passed here unchanged
 *   write_step     the value CRebuild sees (after the ++ of Server.hpp:431).  The protocol passes a multiple of n_total (wt = 1); any
 *                  value is accepted;  index: the block id of the message, 1 .. n_total (Server.hpp:407)
 * Per request, byte for byte the reference's sequence:
 *   1. U[index-1] = block, MAC_U[index-1] = mac (:413-427); the rebuild reads the stores with this write in them.
 *   2. the resident half of data X = the X part of the network over the n_total rows of U, of data Y = the Y part,
 *      wt = w^reverse_bits(write_step % n_total, height-1): the bytes porla_icc_encode_xy_device writes to d_x_out and d_y_x_out.
 *   3. the resident halves of MAC X / MAC Y = the bytes of porla_icc_mac_encode_xy_device on MAC_U.
 *   4. the resident halves of align X / align Y = infinity, 64 zero bytes per point (:1527-1535; the stage loops never touch them).
 *   5. mac_x[j] += comp[j], mac_y[j] += comp[n_total + j], j < n_total (:449-469 with updated_level = height-1): general additions that
 *      leave affine bytes, infinity on either side and equal or opposite points included.
 * The incoming halves and every lower level stay untouched; clear_H_data, clear_H_MAC and the `empty` flags are the caller's
 * bookkeeping, as with the update batch.  The CRebuild_No_Cached form (:1835-2255: rows mod p_icc, an alignment commitment per row)
 * is porla_kzg_server_rebuild_aligned_batch_device / porla_ipa_server_rebuild_aligned_batch_device below.
 * Contract: that of porla_*_update_batch_device -- asynchronous on hip_stream, no host wait, no internal side stream; the work waits
 * for whatever was enqueued on hip_stream before the call and the outputs are complete when the stream is, so the call can sit right
 * behind porla_*_client_rebuild_batch_device on the same stream and buffers and right in front of a batched audit.  The launch sequence
 * depends on n_total, not on k: the store, ceil(log2 n_total / 9) passes of the data network, the MAC load, log2 n_total MAC stages, the
 * Y scaling and the close.  The twiddle tables are the single-file encodes', used under their workspace locks and fences;
 * PORLA_MAC_QUAD_MAX moves the MAC stages between their eight- / four-lane and one-lane forms as it does there (the bytes are the same).
 * PORLA_ERR_ARG (with a message, before the device is touched): NULL reqs with k > 0; any NULL pointer other than d_complements; any
 * pointer not 16-byte aligned; n_total not a power of two, < 2 or > 2^16 (larger files: the single-file calls
 * porla_icc_encode_xy_device and porla_icc_mac_encode_xy_device); n_cols == 0 or > 65535; curve not 0 or 1; index outside 1 .. n_total;
 * two requests (or two fields of one) sharing a store or top-level pointer; more than 65535 requests; a byte size that overflows.
 * k = 0 returns 0; valid arguments without a device: PORLA_ERR_NO_DEVICE.
 * tools/bench_server_rebuild.py times it against the composition of the entry points a caller had before, every output byte compared
 * (profiles/r15_a_server_rebuild.jsonl, DESIGN s4: 64 files of 2^10 blocks in 11 ms, 19x the single-file encodes in sequence; 8 files of
 * 2^15 in 43 ms, 1.4x; the host point additions a caller needed for the complements not counted). */
#define PORLA_SERVER_REBUILD_REQ_BYTES 104   /* sizeof(porla_server_rebuild_req) on LP64; the library static_asserts it and each offset */
typedef struct {
    const void *d_block;
    const void *d_mac;
    const void *d_complements;
    void *d_u_blocks;
    void *d_u_macs;
    void *d_data_x, *d_data_y;
    void *d_mac_x, *d_mac_y;
    void *d_align_x, *d_align_y;
    unsigned long long write_step;
    unsigned long long index;
} porla_server_rebuild_req;
int porla_server_rebuild_batch_device(const porla_server_rebuild_req *reqs, size_t k, size_t n_total, size_t n_cols, int curve,
                                      void *hip_stream);

/* ---- the same write in the CRebuild_No_Cached form (Server.hpp:1835-2255), the form the reference runs while height - 1 >
 * TOP_CACHING_LEVEL, that is for every file above 2^10 blocks (:1479-1485), the protocol's 2^15 among them ----
 * The last stage of each part ends in align_MAC (:531-541, :1977-1980, :2061-2064 and the Y twins): the top-level row is stored mod
 * p_icc and its alignment is Commit(c), c = (A mod p_icc - A) mod q.  These calls commit, so the curve comes with the entry point, as
 * with the update batch: the KZG call commits against the resident SRS (n_cols = porla_kzg_row_coefficients), the IPA call against the
 * first 128 points of generators_fb (n_cols = 128).  The request is porla_server_rebuild_req and every field means what it means
 * above, except the layout of d_data_x / d_data_y: the top level in the 256-BIT ROW FORMAT -- 2 * n_total rows of n_cols 32-byte
 * little-endian symbols below p_icc, the resident half first: the store the audits take as d_rows32, half the bytes per row of the
 * cached form for the audit's row combine to read.  Whether a file uses this form or the cached one is the caller's decision (the
 * reference: height - 1 > 10); both accept any power of two from 2 to 2^16.
 * Per request, byte for byte what Server::update with CRebuild_No_Cached leaves:
 *   1. U[index-1] = block, MAC_U[index-1] = mac (:413-427).
 *   2. the resident half of data X = A mod p_icc of the X part's network over U, of data Y = the same of the Y part,
 *      wt = w^reverse_bits(write_step % n_total, height-1): the bytes porla_icc_encode_xy_device writes to d_aligned_out / d_y_aligned_out.
 *   3. the resident halves of MAC X / MAC Y = the bytes of porla_icc_mac_encode_xy_device on MAC_U.
 *   4. the resident halves of align X / align Y, row by row: row j = the commitment of that part's row j of alignment scalars (the
 *      `scalars` outputs of the same encode), 64 bytes big-endian affine; B starts at infinity (:1882-1890), so the commitment is the
 *      whole value; a row of zero scalars gives 64 zero bytes.
 *   5. mac_x[j] += comp[j], mac_y[j] += comp[n_total + j] (:449-469).
 * The incoming halves and every lower level stay untouched.
 * Contract: that of porla_server_rebuild_batch_device -- asynchronous on hip_stream, no host wait, no internal side stream (the
 * single-file porla_kzg_crebuild_stage_device overlaps the MAC network and the commitments on a second stream; here they run one
 * behind the other), so the client's rebuild call -> this call -> a batched audit -> a batched verify runs in HBM on one stream.  The
 * rows of alignment scalars (2 * n_total per request) go through a workspace of at most 2^18 rows: the requests are taken in groups that
 * fit (a group holds at least one request), and per group the last pass of the data network, ONE commitment pass over the group's rows
 * and the close run one after the other.  So the launch sequence depends on n_total and on the number of groups, not on k within a
 * group: the store, the passes of the data network but the last, the MAC load, log2 n_total MAC stages and the Y scaling over all k
 * requests; then per group the last data pass, the commitment pass and the close.  PORLA_REBUILD_ROWS_MAX (rows, read once per process)
 * lowers the workspace's bound.
 * PORLA_ERR_ARG (with a message, before the device is touched): every refusal of porla_server_rebuild_batch_device that concerns reqs,
 * k and n_total; generators_fb NULL, a BN254 base or one with fewer than 128 points.  No SRS loaded (KZG): PORLA_ERR_STATE.  k = 0
 * returns 0; valid arguments without a device: PORLA_ERR_NO_DEVICE.
 * tools/bench_server_rebuild_aligned.py times the calls against what a caller had, every output byte compared
 * (profiles/r16_a_server_rebuild_aligned.jsonl, DESIGN s4: 64 files of 2^10 blocks in 27 ms, 8.0x porla_kzg_crebuild_stage_device run per
 * file; 8 files of 2^15 in 103 ms, 1.18x; one file 0.91x / 0.96x -- slower: the stage call's side stream hides the MAC network beside
 * the commitments; the host point additions a caller needed for the complements not counted). */
int porla_kzg_server_rebuild_aligned_batch_device(const porla_server_rebuild_req *reqs, size_t k, size_t n_total, void *hip_stream);
int porla_ipa_server_rebuild_aligned_batch_device(porla_fixed_base *generators_fb, const porla_server_rebuild_req *reqs, size_t k,
                                                  size_t n_total, void *hip_stream);

/* ---- the ICC decode: the coded rows of a level back to its blocks, for K independent levels in ONE asynchronous call ----
 * The retrieval step of the protocol, which the reference never wrote in C++ (its icc/ toy demonstrates it): the inverse of the data
 * network.  Output row i is input i of the network whose output is d_rows -- the inverse of porla_icc_encode_device with part = 0 and
 * equally of the chain of porla_icc_mix_device calls that built a level: the X half of level l decodes to its 2^l blocks in write
 * order, oldest first.  Request a is one level:
 *   d_rows         n_rows x n_cols symbols of the form's width, row-major
 *   d_out          n_rows x n_cols x 32 bytes little-endian
 *   d_write_steps  n_rows values, or NULL (residue forms only): output position i is multiplied by wt_i^-1 =
 *                  w^(N - reverse_bits(step_i % N, log2 N)), N = n_total -- a Y half, whose rows are (chunk * wt_i) mod p_icc, gives
 *                  chunk mod p_icc
 *   d_bad          one counter, or NULL (EXACT only; the call zeroes it)
 * form:
 *   PORLA_ICC_DECODE_EXACT      64-byte rows < LCM -> the 256-bit chunks, both residues joined.  A symbol whose joined value is >= 2^256
 *                               cannot be a chunk (an altered row decodes to such values in its whole column): it is written as its
 *                               residue mod p_icc and counted in *d_bad.
 *   PORLA_ICC_DECODE_RESIDUE64  64-byte rows < LCM -> chunk mod p_icc, canonical; only the p_icc plane runs
 *   PORLA_ICC_DECODE_RESIDUE32  32-byte rows < p_icc (the aligned store, d_rows32) -> chunk mod p_icc
 * n_rows: a power of two, 2 .. 2^16, <= n_total.  n_total: a power of two <= 2^16 that fixes w for the unscale (and which resident
 * twiddle table is used: the twiddles of the network itself do not depend on it).
 * Contract: that of the other batches -- asynchronous on hip_stream, no host wait, no side stream; the launch sequence depends on
 * n_rows, not on k (the upload, the counters' reset, ceil(log2 n_rows / 9) passes with the request in blockIdx.y); the twiddle tables
 * are the encode's, plus one table of inverses mod q per (n_total, curve), used under the ICC workspace's lock and fence.
 * PORLA_ERR_ARG (with a message, before the device is touched): NULL reqs with k > 0; NULL d_rows or d_out; d_rows or d_out not
 * 16-byte aligned, d_write_steps not 8-byte aligned, d_bad not 4-byte aligned; a bad n_rows, n_total, n_cols (0 or > 65535), curve or
 * form; d_write_steps or d_bad given with a form that does not take it; an output overlapping any request's input or output; more than
 * 65535 requests; a byte size that overflows.  k = 0 returns 0; valid arguments without a device: PORLA_ERR_NO_DEVICE.
 * porla_icc_decode_host is one level from host memory (upload, the same kernels, download; it waits).
 * tools/bench_icc_decode.py times the EXACT form beside porla_icc_encode_device on the same rows in the same run, every output byte
 * compared with the encode's input (profiles/r17_a_icc_decode.jsonl, DESIGN s4: one level of 2^15 x 128 in 0.95 ms, 1.41x the encode;
 * 8 levels in 6.4 ms, 1.32x; 64 levels of 2^10 in 1.29 ms, 0.40x the 64 encode calls). */
#define PORLA_ICC_DECODE_EXACT      0
#define PORLA_ICC_DECODE_RESIDUE64  1
#define PORLA_ICC_DECODE_RESIDUE32  2
#define PORLA_ICC_DECODE_REQ_BYTES 32   /* sizeof(porla_icc_decode_req) on LP64; the library static_asserts it and each offset */
typedef struct {
    const void *d_rows;
    void *d_out;
    const unsigned long long *d_write_steps;
    unsigned int *d_bad;
} porla_icc_decode_req;
int porla_icc_decode_batch_device(const porla_icc_decode_req *reqs, size_t k, size_t n_rows, size_t n_cols, size_t n_total, int curve,
                                  int form, void *hip_stream);
int porla_icc_decode_host(const uint8_t *rows, size_t n_rows, size_t n_cols, size_t n_total, int curve, int form,
                          const unsigned long long *write_steps, uint8_t *out, unsigned int *bad);

/* ---- the ragged ICC decode: K levels of UNEQUAL sizes in ONE asynchronous call ----
 * porla_icc_decode_batch_device with n_rows moved from the call into the request: a hierarchy's resident levels are never of one size,
 * and one call per size pays the upload, the counters' reset, the workspace's lock and fence and the table lease each time for a few
 * tiles of work.  Request a is one level: the four pointers of porla_icc_decode_req with the same meaning, alignment and form rules
 * (d_write_steps: that request's n_rows values), then
 *   n_rows         a power of two, 2 .. n_total (levels of one row stay with the callers that handle them today)
 * One form, one n_cols, one curve per call.  For every request d_out and *d_bad are byte for byte what
 * porla_icc_decode_batch_device writes for that request alone; they do not depend on the order of the requests.
 * Contract: that of the uniform call -- asynchronous on hip_stream, no host wait, no side stream -- and the launch sequence depends on
 * the PASS CLASSES present (n_rows <= 2^9: one pass; above: two), never on k and never on which sizes are present: one upload (the
 * requests with their shapes, largest first, the n_rows^-1 table, the tile starts), the counters' reset (EXACT), one launch over all
 * one-pass requests, two over all two-pass requests; a work-group finds its request and tile by binary search in the launch's tile
 * starts.  The workspace's lock and fence and the table lease are taken once.
 * PORLA_ERR_ARG (with a message, before the device is touched): every refusal of porla_icc_decode_batch_device, n_rows judged per
 * request and the overlap rule applied with each request's own byte sizes; more tiles in one launch than a grid holds (2^24 - 1:
 * beyond 16 Gi symbols).  k = 0 returns 0; valid arguments without a device: PORLA_ERR_NO_DEVICE.
 * tools/bench_icc_decode_ragged.py times it beside one uniform call per size on the same stores, every output byte compared
 * (DESIGN s4, profiles/r25_a_decode_ragged.jsonl). */
#define PORLA_ICC_DECODE_RAGGED_REQ_BYTES 40   /* sizeof(porla_icc_decode_ragged_req) on LP64; static_asserted with each offset */
typedef struct {
    const void *d_rows;                       /*  0  as porla_icc_decode_req */
    void *d_out;                              /*  8 */
    const unsigned long long *d_write_steps;  /* 16 */
    unsigned int *d_bad;                      /* 24 */
    unsigned long long n_rows;                /* 32: this level's rows */
} porla_icc_decode_ragged_req;
int porla_icc_decode_ragged_batch_device(const porla_icc_decode_ragged_req *reqs, size_t k, size_t n_cols, size_t n_total, int curve,
                                         int form, void *hip_stream);

/* ---- the ICC MAC decode: the coded MAC rows of a level back to its per-block MACs, for K independent levels in ONE asynchronous call ----
 * The MAC-side twin of the ICC decode: a block recovered by porla_icc_decode_batch_device counts only once it has been checked against
 * its MAC, alpha * commit(block) + PRF * h, and the per-block MACs of a level exist only in coded form (mac_x / mac_y: the MAC network
 * over MAC_U plus the complements).  Output row i is input i of the network whose output is d_macs - d_sub -- the inverse of
 * porla_icc_mac_encode_device with part = 0 and equally of the chain of porla_icc_mac_mix_device calls that builds a level.  The stages
 * run from log2 n_rows down to 1 as (A, B) <- (A + B, vi^-1 (A - B)), vi the integer (w^e mod p_icc) mod q the encode multiplies by and
 * vi^-1 its inverse mod the group order q; one factor n_rows^-1 mod q per row is applied at the end.  Request a is one level:
 *   d_macs         n_rows points, 64 bytes X||Y big-endian affine each (reduced as SetBytes does), 64 zero bytes = infinity
 *   d_out          n_rows points in the same form
 *   d_write_steps  n_rows values, or NULL: output position i is additionally multiplied by wt_i^-1 mod q, wt_i =
 *                  (w^reverse_bits(step_i % N, log2 N) mod p_icc) mod q, N = n_total -- the inverse of porla_icc_mac_scale_host and of
 *                  the Y half's init scaling.  n_rows^-1 wt_i^-1 mod q is computed on the device (one division-step inversion per
 *                  row) and applied as ONE scalar multiplication per row
 *   d_sub          n_rows points, or NULL: subtracted from d_macs row by row before the network.  The server rebuild batches leave
 *                  mac_x[j] = network(MAC_U)[j] + comp[j]: with d_sub = comp the output is MAC_U, byte for byte
 * It takes one complete half and is no erasure decoder: w has order N and Y = X at every CRebuild, so most n-row subsets of the 2 n
 * rows of a level are rank-deficient.
 * n_rows: a power of two, 2 .. 2^16, <= n_total.  n_total: a power of two <= 2^16 that fixes w for the write steps (and which resident
 * table is used: the twiddles of the network itself do not depend on it).  curve: 0 (BN254) or 1 (secp256k1).
 * Contract: that of the other batches -- asynchronous on hip_stream, no host wait, no side stream; the launch sequence depends on
 * n_rows, not on k (the upload, the rows' scalars, the load, log2 n_rows stage launches over the K tables of one work array, the
 * close); the inverse twiddles as plain scalars and their digit codes are derived per (n_total, curve) from the data decode's table of
 * inverses mod q, read under the ICC workspace's lock and fence.
 * PORLA_ERR_ARG (with a message, before the device is touched): NULL reqs with k > 0; NULL d_macs or d_out; d_macs, d_out or d_sub not
 * 16-byte aligned, d_write_steps not 8-byte aligned; a bad n_rows, n_total or curve; an output overlapping any request's input, sub or
 * output; more than 65535 requests; a byte size that overflows.  k = 0 returns 0; valid arguments without a device:
 * PORLA_ERR_NO_DEVICE.  porla_icc_mac_decode_host is one level from host memory (upload, the same kernels, download; it waits).
 * tools/bench_icc_mac_decode.py times the decode beside porla_icc_mac_encode_device on the same rows in the same run, every output
 * byte compared with the encode's input (profiles/r20_a_mac_decode.jsonl, DESIGN s4: one level of 2^15 in 6.3 ms, 1.15x the encode;
 * 8 levels in 50 ms, 1.16x; 64 levels of 2^10 in 9.6 ms, 0.055x the 64 encode calls). */
#define PORLA_ICC_MAC_DECODE_REQ_BYTES 32   /* sizeof(porla_icc_mac_decode_req) on LP64; the library static_asserts it and each offset */
typedef struct {
    const void *d_macs;
    void *d_out;
    const unsigned long long *d_write_steps;
    const void *d_sub;
} porla_icc_mac_decode_req;
int porla_icc_mac_decode_batch_device(const porla_icc_mac_decode_req *reqs, size_t k, size_t n_rows, size_t n_total, int curve,
                                      void *hip_stream);
int porla_icc_mac_decode_host(const uint8_t *macs, size_t n_rows, size_t n_total, int curve, const unsigned long long *write_steps,
                              const uint8_t *sub, uint8_t *out);

/* ---- verified retrieval: the coded rows of a level checked against its stored MAC rows, then decoded, for K levels in ONE call ----
 * "Give me this level back and tell me it is authentic" without the MAC decode.  The data network works mod LCM = p_icc q with integer
 * multipliers vi < p_icc and the MAC network multiplies by the same vi reduced mod q, so coded row j of an exact half, reduced mod q,
 * is the Z_q network of the chunks, and the half's MAC row j is alpha * Commit(row_j mod q) + s_j * h with s_j the PRF value of the
 * complement the client currently holds for that row.  Every coded row is therefore checked against its stored MAC row directly -- KZG:
 * one polynomial evaluation per row (the client knows tau) and a two-coefficient fixed-base commitment; IPA: one 128-coefficient
 * commitment plus one multiple of the hiding base -- and no group-element network runs.  One altered symbol fails exactly its row, one
 * altered MAC row exactly that row: the caller learns which stored row is damaged.  Request a is one half:
 *   d_rows    n_rows x n_cols symbols of 64 bytes, little-endian, < LCM, row-major: ONE EXACT half (below)
 *   d_macs    n_rows points, 64 bytes X||Y big-endian affine, 64 zero bytes = infinity: that half's MAC rows as stored, complements included
 *   d_prf     n_rows PRF outputs of 16 raw bytes: row j's current complement, read as porla_client_update_req.d_prf is read (KZG: a
 *             big-endian 128-bit integer; IPA: r.d[0], r.d[1] as little-endian words)
 *   d_out     n_rows x n_cols x 32 bytes: the blocks, byte for byte what porla_icc_decode_batch_device writes for d_rows in the form
 *             PORLA_ICC_DECODE_EXACT; NULL = check only.  The decode runs whatever the statuses are: the caller decides what to do with
 *             a level that has failed rows
 *   d_status  n_rows bytes: PORLA_RETRIEVE_ROW_OK iff the 64 bytes of d_macs row j EQUAL the bytes of the expected MAC in its canonical
 *             affine form, otherwise 0.  A stored coordinate >= p is not OK; infinity is 64 zero bytes on both sides.  The expected MAC,
 *             KZG: the bytes porla_kzg_mac_batch_device gives for the row's coefficients sym mod r and the PRF value left-padded to 32
 *             bytes, i.e. alpha f(tau) G1[0] + prf h_MAC.  IPA: step 1 of porla_ipa_client_update_batch_device, sum_c (sym_c mod n)
 *             alpha_generators[c] over the first 128 points of alpha_generators_fb plus prf h (h the one point of h_fb), formed by that
 *             call's own addition
 *   d_counts  two counters, or NULL; the call zeroes both: [0] the rows with status 0, [1] the data decode's *d_bad (0 when d_out is NULL)
 * n_cols is the SRS size (KZG) or 128 (IPA), the rule of the client update batch.
 * Which halves are valid input: an EXACT half, one where every symbol carries both residues -- the X half of every level, and both halves
 * of the top level porla_server_rebuild_batch_device (CRebuild_Cached) leaves.  A half that holds residues mod p_icc only (the Y rows
 * HAdd writes, the 32-byte aligned top level) needs its alignment store in the relation (M + alpha A, as in the batched verifier):
 * that is porla_*_retrieve_aligned_batch_device below, which covers every half of every level.  THIS call has no alignment store to
 * look at, so on such a half its statuses are 0 on every row whose alignment is finite.
 * n_rows: a power of two, 2 .. 2^16, <= n_total.  n_total: a power of two <= 2^16 (it selects the decode's resident table; no result
 * depends on it).
 * Contract: that of the other batches -- asynchronous on hip_stream, no host wait, no side stream; the launch sequence depends on
 * n_rows, not on k (IPA: while k n_rows 128 x 32 bytes of coefficient rows fit 256 MiB; beyond that the rows go through in groups of
 * 2^16); the ICC workspace's tables are used under its lock and fence, the KZG state's two-point table and evaluation scratch under
 * their mutexes and fences, as porla_kzg_mac_batch_device uses them.  One host wait there is, as in that call: the KZG build's table
 * of powers of tau is uploaded with a blocking copy on the first call and after a change of the key or the SRS size.
 * PORLA_ERR_ARG (with a message, before the device is touched): NULL reqs with k > 0; NULL d_rows, d_macs, d_prf or d_status; d_rows,
 * d_macs, d_prf or d_out not 16-byte aligned, d_counts not 4-byte aligned; n_rows not a power of two in 2 .. 2^16 or > n_total; n_total
 * not a power of two <= 2^16; any output (d_out, d_status, d_counts) overlapping any input or output of any request of the call; more than
 * 65535 requests; a byte size that overflows; IPA: a NULL base, and (where a base can exist: behind the device check) a BN254 base,
 * alpha_generators_fb with fewer than 128 points, h_fb without exactly one point.  k = 0 returns 0; KZG without init_key + init_SRS:
 * PORLA_ERR_STATE; valid arguments without a device: PORLA_ERR_NO_DEVICE.
 * porla_*_retrieve_host is one level from host memory (upload, the same kernels, download; it waits): out and counts may be NULL.
 * tools/bench_retrieve.py times the call with and without d_out beside the data decode, the MAC decode and the four-call sequence on
 * the same level in the same run (DESIGN s4). */
#define PORLA_RETRIEVE_REQ_BYTES 48    /* sizeof(porla_retrieve_req) on LP64; the library static_asserts it and each offset */
#define PORLA_RETRIEVE_ROW_OK 1
typedef struct {
    const void    *d_rows;    /* 0 */
    const void    *d_macs;    /* 8 */
    const void    *d_prf;     /* 16 */
    void          *d_out;     /* 24 */
    unsigned char *d_status;  /* 32 */
    unsigned int  *d_counts;  /* 40 */
} porla_retrieve_req;
int porla_kzg_retrieve_batch_device(const porla_retrieve_req *reqs, size_t k, size_t n_rows, size_t n_total, void *hip_stream);
int porla_ipa_retrieve_batch_device(porla_fixed_base *alpha_generators_fb, porla_fixed_base *h_fb, const porla_retrieve_req *reqs,
                                    size_t k, size_t n_rows, size_t n_total, void *hip_stream);
int porla_kzg_retrieve_host(const uint8_t *rows, const uint8_t *macs, const uint8_t *prf, size_t n_rows, size_t n_total, uint8_t *out,
                            uint8_t *status, unsigned int *counts);
int porla_ipa_retrieve_host(porla_fixed_base *alpha_generators_fb, porla_fixed_base *h_fb, const uint8_t *rows, const uint8_t *macs,
                            const uint8_t *prf, size_t n_rows, size_t n_total, uint8_t *out, uint8_t *status, unsigned int *counts);

/* ---- verified retrieval of ANY half: the alignment store joins the relation ----
 * Every row of every non-empty level, X and Y, keeps MAC[j] + alpha * align[j] == alpha * Commit(row[j] mod q) (+ s_j h with the
 * complements), row[j] being the STORED symbol reduced mod the group order q: the rows mix mod LCM and both point stores mix by the
 * same multipliers mod q (tests/test_update_batch_cpu.py), and the aligned top level has it by construction (c = (A mod p_icc - A) mod
 * q, alignment = Commit(c)).  So for every half
 *     status_j = (bytes of d_macs row j == canonical affine bytes of E_j - alpha * A_j)
 * with E_j the expected MAC of porla_*_retrieve_batch_device above and A_j row j of the half's alignment store; with every A_j at
 * infinity this IS that call.  Request a is one half; d_rows, d_macs, d_prf, d_status, d_counts as in porla_retrieve_req, and
 *   d_align        n_rows points, 64 bytes X||Y big-endian affine, 64 zero bytes = infinity: the half's alignment rows, read the way the
 *                  MAC stores are read everywhere (coordinates reduced mod p; NOT checked to be on the curve: a garbage A_j gives a
 *                  defined, fault-free result, which will be status 0).  NULL = every alignment at infinity
 *   d_write_steps  n_rows values or NULL; residue forms only: the data decode's unscale of a Y half (porla_icc_decode_req)
 *   d_out          n_rows x n_cols x 32 bytes, byte for byte what porla_icc_decode_batch_device writes for the same rows, form and write
 *                  steps; NULL = check only
 *   d_counts[1]    that call's *d_bad for PORLA_ICC_DECODE_EXACT, 0 for the residue forms
 * form, one of the decode's constants, fixes the row width the check reads AND the decode that runs when d_out is given:
 * PORLA_ICC_DECODE_EXACT and PORLA_ICC_DECODE_RESIDUE64 read 64-byte little-endian symbols below LCM, PORLA_ICC_DECODE_RESIDUE32 reads
 * 32-byte little-endian symbols below p_icc (the d_rows32 store of porla_*_server_rebuild_aligned_batch_device).
 * Which call on which store: a cached top level or an X half -- either call (form EXACT); a Y half of 64-byte rows -- this call with
 * RESIDUE64, the half's alignment store and the blocks' write steps; the aligned top level -- this call with RESIDUE32.
 * alpha.  KZG: the state's key, the value the expected MACs are made with.  IPA: alpha_be, 32 big-endian bytes, reduced mod n; it must be
 * the scalar with alpha_generators[c] = alpha * generators[c].  The call CANNOT check that: a wrong alpha fails every row whose
 * alignment is finite (and no other).
 * Infinity on both sides is 64 zero bytes; a stored coordinate >= p in d_macs is not OK.
 * Launches: those of porla_*_retrieve_batch_device; when a request of the call has a d_align, k_rt_compare_aligned (a quad of lanes per
 * row, alpha * A_j by the four-lane uniform ladder of the MAC network) stands in for k_rt_compare, and a block of 64 rows without a
 * nonzero alignment byte runs k_rt_compare's body instead of the ladder; then the data decode of `form`.  Contract, locks and fences:
 * as porla_*_retrieve_batch_device -- asynchronous on hip_stream, no side stream, no host wait beyond that call's, the launch sequence
 * depends on n_rows and not on k.
 * PORLA_ERR_ARG (with a message, before the device is touched): everything porla_*_retrieve_batch_device refuses, the byte sizes being
 * computed from the form's row width; a form that is none of the three; d_align not 16-byte aligned; d_write_steps not 8-byte aligned,
 * or given with PORLA_ICC_DECODE_EXACT; NULL alpha_be (IPA); an output overlapping any input (d_align and d_write_steps included) or any
 * output of any request.  k = 0 returns 0; KZG without init_key + init_SRS: PORLA_ERR_STATE; valid arguments without a device:
 * PORLA_ERR_NO_DEVICE.
 * porla_*_retrieve_aligned_host is one level from host memory (it waits): align, write_steps, out and counts may be NULL.
 * tools/bench_retrieve_aligned.py times the call beside porla_*_retrieve_batch_device on the same level (DESIGN s4). */
#define PORLA_RETRIEVE_ALIGNED_REQ_BYTES 64   /* sizeof(porla_retrieve_aligned_req) on LP64; the library static_asserts it and each offset */
typedef struct {
    const void               *d_rows;         /*  0 */
    const void               *d_macs;         /*  8 */
    const void               *d_prf;          /* 16 */
    const void               *d_align;        /* 24 */
    const unsigned long long *d_write_steps;  /* 32 */
    void                     *d_out;          /* 40 */
    unsigned char            *d_status;       /* 48 */
    unsigned int             *d_counts;       /* 56 */
} porla_retrieve_aligned_req;
int porla_kzg_retrieve_aligned_batch_device(const porla_retrieve_aligned_req *reqs, size_t k, size_t n_rows, size_t n_total, int form,
                                            void *hip_stream);
int porla_ipa_retrieve_aligned_batch_device(porla_fixed_base *alpha_generators_fb, porla_fixed_base *h_fb, const uint8_t alpha_be[32],
                                            const porla_retrieve_aligned_req *reqs, size_t k, size_t n_rows, size_t n_total, int form,
                                            void *hip_stream);
int porla_kzg_retrieve_aligned_host(const uint8_t *rows, const uint8_t *macs, const uint8_t *prf, const uint8_t *align,
                                    const unsigned long long *write_steps, size_t n_rows, size_t n_total, int form, uint8_t *out,
                                    uint8_t *status, unsigned int *counts);
int porla_ipa_retrieve_aligned_host(porla_fixed_base *alpha_generators_fb, porla_fixed_base *h_fb, const uint8_t alpha_be[32],
                                    const uint8_t *rows, const uint8_t *macs, const uint8_t *prf, const uint8_t *align,
                                    const unsigned long long *write_steps, size_t n_rows, size_t n_total, int form, uint8_t *out,
                                    uint8_t *status, unsigned int *counts);

/* ---- verified file extraction: every resident level of K files checked, decoded and merged, newest authentic copy wins ----
 * The retrieval calls above give ONE level back; a proof of retrievability promises the FILE.  This call takes K files with their
 * hierarchies as they lie in HBM, checks every resident row, decodes every resident X half and merges the decoded blocks into the
 * file's block store.  What the hierarchy gives (Server::HAdd / HRebuildX / HRebuildY, Server.hpp:1330-1477; tests/update_model.py):
 * with t = write_step % n_total, level i < log2 n_total is resident iff bit i of t is set and its X half holds the blocks of the epoch
 * write steps hi_i - 2^i + 1 .. hi_i, hi_i = t with the bits below i cleared, decoded in write order, oldest first; lower levels are
 * newer; the top level holds U as of the last rebuild, block b at position b, older than everything below it; with t == 0 only the top
 * level is resident.  The X half of a lower level is exact (64-byte symbols below LCM; level 0's one row is the chunks zero-extended);
 * the top level's X half is exact after porla_server_rebuild_batch_device, or 32-byte residues mod p_icc with an alignment store
 * after porla_*_server_rebuild_aligned_batch_device: top_form, PORLA_ICC_DECODE_EXACT or PORLA_ICC_DECODE_RESIDUE32, for the whole call.
 * A block names its slot: the low 8 bytes of chunk 0, a little-endian 64-bit integer, are the block index counted from 1 (the
 * reference's wire format, Client.hpp:367-372 / Server.hpp:404-414); chunk 0 is under the row check like the rest.
 * Request a is one file (the fields below).  n_cols is the SRS size (KZG) or 128 (IPA); n_total a power of two, 2 .. 2^16.
 *   1. Row check.  Every resident row gets the status of porla_*_retrieve_aligned_batch_device, byte for byte: PORLA_RETRIEVE_ROW_OK
 *      iff the stored MAC bytes equal the canonical bytes of E_j - alpha A_j, the lower levels without an alignment store, the top
 *      level with d_top_align.  Level 0's single row is checked by the same relation.
 *   2. Failed levels.  A level with a status-0 row is failed, the top level included; a decoded block depends on every row of its
 *      level, so no block of a failed level is ever taken.
 *   3. Merge.  A block of a clean lower level whose index id is in 1 .. n_total is a candidate for slot id - 1 with its epoch write
 *      step as rank; block b of a clean top level is a candidate for slot b with rank 0.  The highest rank wins; ranks are distinct.
 *   4. Per slot: d_blocks = the winner's n_cols x 32 bytes, or zeros; d_steps = the winner's rank, or 0xffffffff; d_flags = FOUND iff
 *      there is a winner, RESIDUE iff the winner is a top-level block and top_form is RESIDUE32, UNSURE iff some failed level's
 *      highest write step (hi_i; 0 for the top level) is greater than the winner's rank, a slot without a winner having rank -1.
 *   5. A block of a clean lower level whose index is 0 or above n_total is counted and dropped.
 *   6. d_counts: [0] the rows with status 0, [1] the sum of the exact decodes' bad-symbol counts (level 0: symbols with a nonzero
 *      upper half), [2] the blocks dropped under 5, [3] the slots that are not FOUND or are UNSURE.
 * Launches: one upload; one clear; the aligned retrieval's check launches ONCE over all 64-byte rows of all files and levels and once
 * more over the RESIDUE32 top levels (the rows find their half by a binary search in the halves' start rows; IPA in its coefficient
 * workspace groups) -- their number depends on the symbol widths present, not on K and not on which levels are resident; ONE ragged
 * data decode (porla_icc_decode_ragged_batch_device's body) over the lower levels of two rows and more and the exact top levels of
 * all files (top level straight into d_blocks, lower levels into d_work): at most three pass launches, by whether levels of up to
 * 2^9 rows and larger ones are present, not by which sizes; the uniform decode for RESIDUE32 top levels; level 0 by a copy kernel;
 * three merge kernels.  Contract: that of the other batches -- asynchronous on hip_stream, no side stream, no host wait beyond the retrieval
 * calls' first-use upload of the tau table; workspaces under their locks and fences.
 * PORLA_ERR_ARG (with a message, before the device is touched): NULL reqs with k > 0; NULL d_blocks, d_steps or d_flags; NULL d_prf or
 * d_row_status with a resident row; NULL d_top_macs beside d_top_rows; NULL data_x, mac_x or d_work with t > 0 (they may be NULL only when
 * t == 0); a resident level with a NULL pointer; a level pointer, d_top_rows, d_top_macs, d_top_align, d_prf, d_work or d_blocks not
 * 16-byte aligned, d_steps or d_counts not 4-byte aligned; n_total not a power of two in 2 .. 2^16; a top_form that is neither of the
 * two; NULL alpha_be or bases (IPA); more than 65535 requests; a byte size that overflows; any output (d_work counts as one)
 * overlapping any input or output of the call.  k = 0 returns 0; KZG without init_key + init_SRS: PORLA_ERR_STATE; valid arguments
 * without a device: PORLA_ERR_NO_DEVICE.
 * A level's Y half when its X half fails: porla_*_extract_xy_batch_device below.  Not in this call: a host-memory form; n_total >
 * 2^16.  tools/bench_extract.py times the call beside one aligned retrieval call per resident level size
 * on the same stores (profiles/r23_a_extract.jsonl, DESIGN s4: one file of 2^15 blocks x 128, every level resident, in 4.4 ms (KZG) /
 * 11.8 ms (IPA) against 8.1 / 19.6 ms for the fifteen calls, which merge nothing and skip level 0; one run, wide spread). */
#define PORLA_EXTRACT_REQ_BYTES 104   /* sizeof(porla_extract_req) on LP64; the library static_asserts it and each offset */
#define PORLA_EXTRACT_FOUND    1   /* the slot holds a copy taken from a level whose rows all checked OK */
#define PORLA_EXTRACT_UNSURE   2   /* a level with a failed row could hold a newer copy of this slot */
#define PORLA_EXTRACT_RESIDUE  4   /* the copy comes from a RESIDUE32 top level: chunks mod p_icc */
typedef struct {
    unsigned long long  write_step;   /*  0: the server's counter; t = write_step % n_total */
    void *const        *data_x;       /*  8: HOST array of log2(n_total) DEVICE pointers: level i's data store as porla_update_req lays it
                                             out; the first 2^i rows (the resident X half) are read.  Entries of non-resident levels are ignored */
    void *const        *mac_x;        /* 16: the same for the MAC stores */
    const void         *d_top_rows;   /* 24: the top level's X half, n_total rows in top_form; NULL = no top level */
    const void         *d_top_macs;   /* 32 */
    const void         *d_top_align;  /* 40: NULL = every alignment at infinity */
    const void         *d_prf;        /* 48: 16 raw bytes per resident row, read as porla_retrieve_req.d_prf is read: resident levels in
                                             ascending order, 2^i values each, then n_total values for the top level if there is one */
    void               *d_work;       /* 56: t x n_cols x 32 bytes of scratch for the decoded lower levels */
    void               *d_blocks;     /* 64: n_total x n_cols x 32 bytes: slot b = block index b + 1 */
    unsigned int       *d_steps;      /* 72: n_total words: the epoch write step of the copy taken, 0 = top level, 0xffffffff = none */
    unsigned char      *d_flags;      /* 80: n_total bytes of the PORLA_EXTRACT_* bits */
    unsigned char      *d_row_status; /* 88: one byte per resident row, laid out like d_prf: PORLA_RETRIEVE_ROW_OK or 0 */
    unsigned int       *d_counts;     /* 96: four words or NULL, zeroed by the call */
} porla_extract_req;
int porla_kzg_extract_batch_device(const porla_extract_req *reqs, size_t k, size_t n_total, int top_form, void *hip_stream);
int porla_ipa_extract_batch_device(porla_fixed_base *alpha_generators_fb, porla_fixed_base *h_fb, const uint8_t alpha_be[32],
                                   const porla_extract_req *reqs, size_t k, size_t n_total, int top_form, void *hip_stream);

/* ---- verified file extraction with the Y halves: a lower level whose X half fails is recovered from its second copy ----
 * The hierarchy stores every lower level twice: the X half holds the exact symbols, the Y half chunk * wt mod p_icc with an alignment
 * store (Server::HAdd).  The call above drops all 2^i blocks of a level with one damaged X row; this one takes the arguments of that
 * call over porla_extract_xy_req -- porla_extract_req field for field in its first 104 bytes, then the Y stores -- and falls back to
 * the Y half of the levels the caller names in y_levels.  The mask is the caller's because the launch shapes are fixed on the host:
 * pass the levels an earlier extraction reported as failed, or all ones for a full scrub of both halves (which also reports damaged Y
 * rows).  With y_levels & t == 0 every output of the call above comes back byte for byte and the Y pointers may be NULL.
 * Steps 1 and 2 of the call above hold for the X halves and the top level.  Beside them:
 *   1y. Y row check.  Every row of every tried Y half gets the status of porla_*_retrieve_aligned_batch_device on that half with form
 *       PORLA_ICC_DECODE_RESIDUE64, its align_y store and its slice of d_prf_y, in d_row_status_y; the rows of untried levels get
 *       PORLA_EXTRACT_ROW_NOT_TRIED.  Level 0's single Y row is checked by the same relation.  The tried Y halves are further halves of
 *       the ONE pass over the 64-byte rows: the check's launch count does not grow.
 *   2y. Source of a level: X if its X half is clean; else Y if the level was tried and its Y half is clean; else the level is failed.
 *       The top level has no Y fall-back here.
 *   3y. Y decode.  Every tried Y half goes through the RESIDUE64 decode into d_work_y with the write steps of its blocks (entry p of
 *       level i: write_step - t + (t with bits 0 .. i cleared) + 1 + p, written on the device); level 0's one row is unscaled by
 *       wt^-1 = w^(N - reverse_bits(step % N)) mod p_icc.  Outputs are canonical, below p_icc.
 *   4y. Merge.  A block of an X-sourced level bids as in the call above.  A block of a Y-sourced level is known mod p_icc only; its
 *       rank is its epoch write step; if it wins, the slot gets its n_cols x 32 bytes (chunks mod p_icc) and the flags FOUND | RESIDUE
 *       | FROM_Y.
 *   5y. Ambiguous index.  r0 = the decoded chunk 0 of a Y-sourced block, D = 2^256 - p_icc = 49 * 2^248 - 1.  The true chunk 0 is r0 or
 *       r0 + p_icc, the second iff r0 < D; p_icc = 1 mod 2^64, so the two name the indices a = low64(r0) and a + 1 mod 2^64.  r0 >= D:
 *       the index is a; in 1 .. n_total the block is a candidate, otherwise it is counted and dropped (rule 5).  r0 < D and neither
 *       index in 1 .. n_total: counted and dropped (rule 5).  r0 < D otherwise: the block is set aside -- NEVER taken, the wrong slot
 *       would be a silent error -- counted in d_counts[5], and each candidate slot in range records the block's step as a doubt.  With
 *       random 256-bit chunks about 38 % of the Y blocks are ambiguous (r0 < D for a chunk below D and for one at or above p_icc: 2 D / 2^256): a caller
 *       who wants the full fall-back keeps chunk 0 of every block in [D, p_icc).
 *   6y. UNSURE iff some failed level (2y; the top level as above) has hi_i greater than the winner's rank, or the slot's doubt is
 *       greater than the winner's rank; a slot without a winner has rank -1.
 *   7y. d_counts, SIX words: [0] the X and top rows with status 0, [1] as above, [2] the blocks dropped for their index, from either
 *       source, [3] the slots that are not FOUND or are UNSURE, [4] the tried Y rows with status 0, [5] the blocks set aside as ambiguous.
 * Launches: those of the call above, plus the step-array kernel, ONE ragged RESIDUE64 decode over the tried Y halves of two rows and
 * more, and the level-0 Y kernel.  The sequence depends on the symbol widths and on the pass classes present (levels of up to 2^9
 * rows, larger ones) among the X halves and among the tried Y halves, never on K and never on which sizes are present.  Contract: as the call above.
 * PORLA_ERR_ARG (with a message, before the device is touched): everything the call above refuses (d_counts is 24 bytes here); with
 * y_levels & t != 0 a NULL data_y, mac_y, align_y (the array itself), d_prf_y, d_work_y or d_row_status_y, and a tried level with a NULL
 * entry in data_y or mac_y; whenever the pointer is given, a tried level's pointer of the three Y families, d_prf_y or d_work_y not
 * 16-byte aligned, and a byte size that wraps; d_work_y and d_row_status_y are outputs in the overlap walk, the Y inputs may be shared
 * between requests.  k = 0, PORLA_ERR_STATE and PORLA_ERR_NO_DEVICE as in the call above.
 * Not in this call: the top level's Y half (a failed top level behaves as above; porla_*_extract_xyt_batch_device below takes it row
 * by row); a host-memory form; n_total > 2^16; a cross-check
 * of a Y decode against a clean X decode of the same level.  tools/bench_extract_xy.py times it (profiles/r24_a_extract_xy.jsonl). */
#define PORLA_EXTRACT_XY_REQ_BYTES 160   /* sizeof(porla_extract_xy_req) on LP64; the library static_asserts it and each offset */
#define PORLA_EXTRACT_FROM_Y        8    /* d_flags: the copy comes from a level's Y half.  A lower level's: chunks mod p_icc, RESIDUE is
                                            set too.  The top level's (porla_*_extract_xyt_batch_device): RESIDUE follows top_form alone */
#define PORLA_EXTRACT_ROW_NOT_TRIED 2    /* d_row_status_y: the row's level is not in y_levels */
typedef struct {
    unsigned long long  write_step;     /*   0: the fields of porla_extract_req, at its offsets */
    void *const        *data_x;         /*   8 */
    void *const        *mac_x;          /*  16 */
    const void         *d_top_rows;     /*  24 */
    const void         *d_top_macs;     /*  32 */
    const void         *d_top_align;    /*  40 */
    const void         *d_prf;          /*  48 */
    void               *d_work;         /*  56 */
    void               *d_blocks;       /*  64 */
    unsigned int       *d_steps;        /*  72 */
    unsigned char      *d_flags;        /*  80 */
    unsigned char      *d_row_status;   /*  88 */
    unsigned int       *d_counts;       /*  96: SIX words or NULL, zeroed by the call */
    void *const        *data_y;         /* 104: HOST array of log2(n_total) DEVICE pointers: level i's Y data store as porla_update_req
                                                lays it out; the first 2^i rows (the resident half) are read.  Entries of untried levels are ignored */
    void *const        *mac_y;          /* 112: the same for the Y MAC stores */
    void *const        *align_y;        /* 120: the same for the Y alignment stores; an entry may be 0: every alignment of that half at infinity */
    const void         *d_prf_y;        /* 128: 16 raw bytes per lower-level row, laid out like the lower-level part of d_prf (t entries);
                                                only the entries of tried levels are read */
    void               *d_work_y;       /* 136: t x n_cols x 32 bytes of scratch for the decoded Y halves, laid out like d_work */
    unsigned char      *d_row_status_y; /* 144: t bytes, laid out like the lower-level part of d_row_status */
    unsigned long long  y_levels;       /* 152: bit i = try level i's Y half; only the bits of y_levels & t count */
} porla_extract_xy_req;
int porla_kzg_extract_xy_batch_device(const porla_extract_xy_req *reqs, size_t k, size_t n_total, int top_form, void *hip_stream);
int porla_ipa_extract_xy_batch_device(porla_fixed_base *alpha_generators_fb, porla_fixed_base *h_fb, const uint8_t alpha_be[32],
                                      const porla_extract_xy_req *reqs, size_t k, size_t n_total, int top_form, void *hip_stream);

/* ---- verified file extraction with the top level's Y half: a damaged top level is rebuilt row by row from its second copy ----
 * The top level holds U, every block not rewritten since the last rebuild, and the calls above drop all of it for one damaged X row.
 * Its Y half is written by ONE rebuild with ONE wt = w^reverse_bits(top_step % n_total, log2 n_total) for all rows, and the network
 * is linear: row by row Y_j = wt X_j mod LCM (porla_icc_encode_xy_device above), and mod p_icc in the aligned form of
 * porla_*_server_rebuild_aligned_batch_device.  So no second decode is needed and no half has to be entirely clean: every damaged X
 * row is replaced by wt^-1 times its own Y row, and the top level's one decode runs on the patched half.  A top level damaged in BOTH
 * halves survives as long as no row index is damaged in both; in the exact form the recovered blocks are the exact 256-bit chunks.
 * This call takes the arguments of the call above over porla_extract_xyt_req -- porla_extract_xy_req field for field in its first
 * 160 bytes, then the top level's Y half.  With top_y == 1 and a top level present, everything else being the call above's:
 *   1t. Check.  Every top-level Y row gets the status of porla_*_retrieve_aligned_batch_device on that half in top_form's symbol
 *       width, with d_top_align_y and d_prf_top_y, in d_row_status_top_y.  The half is one more half of a pass that exists already
 *       (the 64-byte pass for PORLA_ICC_DECODE_EXACT, the RESIDUE32 pass otherwise): the check's launch count does not grow.
 *   2t. Source of a top-level row: X if its X status is OK; else Y if its Y status is OK; else none.  The top level is failed iff some
 *       row has no source; bit log2 n_total of the failed mask and UNSURE then are as in rules 4 / 6y.
 *   3t. Patch.  d_top_patch row j is X row j as it lies, or wt^-1 Y_j, canonical: below LCM as 64 little-endian bytes in the exact
 *       form, below p_icc in the RESIDUE32 form.  wt^-1 has two planes: mod p_icc the factor w^(N - e) the residue decode's unscale
 *       uses for that write step, mod q the inverse of (wt mod q).  Any 64 (32) bytes of a Y row are defined: they are reduced as
 *       the decode's load reduces them.  With top_step % n_total == 0 (wt = 1) the Y row is copied as it lies; a row without a source
 *       keeps its X row.
 *   4t. Decode.  The top level's ONE decode (the ragged exact decode, or the uniform RESIDUE32 decode) reads d_top_patch instead of
 *       d_top_rows and writes into d_blocks; its bad-symbol count goes into d_counts[1].
 *   5t. A slot the top level wins: FOUND; RESIDUE iff top_form is RESIDUE32; FROM_Y iff d_counts[7] > 0 -- every decoded block
 *       depends on every row.
 *   6t. d_counts, EIGHT words: [0 .. 5] as above ([0] the X and top X rows with status 0), [6] the tried top-level Y rows with status
 *       0, [7] the top-level rows taken from the Y half.  d_row_status is unchanged.
 * With top_y == 0, or without a top level, the six outputs and d_counts[0 .. 5] of the call above come back byte for byte, d_counts[6
 * .. 7] are 0, d_row_status_top_y -- if given -- is filled with PORLA_EXTRACT_ROW_NOT_TRIED and the six new pointers may be NULL.  With
 * top_y == 1 and a clean X half the patched half is the X half and those outputs are the call above's again.
 * Launches: when some file of the call has its top Y half tried, ONE patch kernel between the check and the decodes (a lane per symbol,
 * one read and one write of the half) and the larger clear; files with and without top_y mix in one call.  The sequence depends on
 * the symbol widths and pass classes present and on whether a top Y half is tried at all, never on K.  Contract: as the calls above.
 * PORLA_ERR_ARG (with a message, before the device is touched): everything the call above refuses (d_counts is 32 bytes here); with
 * top_y == 1 and a top level a NULL d_top_rows_y, d_top_macs_y, d_prf_top_y, d_top_patch or d_row_status_top_y; any of the six new
 * pointers not 16-byte aligned, wherever given; top_y above 1; a byte size that wraps; d_top_patch and d_row_status_top_y are outputs
 * in the overlap walk, the three Y inputs may be shared between requests.  k = 0, PORLA_ERR_STATE and PORLA_ERR_NO_DEVICE as above.
 * Not in this call: a host-memory form; n_total > 2^16; a row damaged in both halves.  Writing the repaired rows back into the
 * server's store is porla_*_repair_top_batch_device below.  tools/bench_extract_xyt.py times it (profiles/r26_a_extract_xyt.jsonl). */
#define PORLA_EXTRACT_XYT_REQ_BYTES 224   /* sizeof(porla_extract_xyt_req) on LP64; the library static_asserts it and each offset */
typedef struct {
    unsigned long long  write_step;         /*   0: the fields of porla_extract_xy_req, at its offsets */
    void *const        *data_x;             /*   8 */
    void *const        *mac_x;              /*  16 */
    const void         *d_top_rows;         /*  24 */
    const void         *d_top_macs;         /*  32 */
    const void         *d_top_align;        /*  40 */
    const void         *d_prf;              /*  48 */
    void               *d_work;             /*  56 */
    void               *d_blocks;           /*  64 */
    unsigned int       *d_steps;            /*  72 */
    unsigned char      *d_flags;            /*  80 */
    unsigned char      *d_row_status;       /*  88 */
    unsigned int       *d_counts;           /*  96: EIGHT words or NULL, zeroed by the call */
    void *const        *data_y;             /* 104 */
    void *const        *mac_y;              /* 112 */
    void *const        *align_y;            /* 120 */
    const void         *d_prf_y;            /* 128 */
    void               *d_work_y;           /* 136 */
    unsigned char      *d_row_status_y;     /* 144 */
    unsigned long long  y_levels;           /* 152 */
    const void         *d_top_rows_y;       /* 160: the top level's resident Y half: n_total rows in top_form (64-byte symbols below LCM,
                                                    or 32-byte symbols below p_icc) */
    const void         *d_top_macs_y;       /* 168: its MAC rows, 64 bytes each */
    const void         *d_top_align_y;      /* 176: its alignment store; NULL = every alignment at infinity */
    const void         *d_prf_top_y;        /* 184: 16 raw bytes per top-level Y row, read as d_prf is read */
    void               *d_top_patch;        /* 192: scratch, n_total x n_cols x (64 or 32) bytes: the patched half */
    unsigned char      *d_row_status_top_y; /* 200: n_total status bytes */
    unsigned long long  top_step;           /* 208: the write step the rebuild that wrote the top level was given (the protocol:
                                                    write_step - t, a multiple of n_total; any value is accepted, as the rebuild calls do) */
    unsigned long long  top_y;              /* 216: 1 = try the top level's Y half; 0 = do not; anything else is refused */
} porla_extract_xyt_req;
int porla_kzg_extract_xyt_batch_device(const porla_extract_xyt_req *reqs, size_t k, size_t n_total, int top_form, void *hip_stream);
int porla_ipa_extract_xyt_batch_device(porla_fixed_base *alpha_generators_fb, porla_fixed_base *h_fb, const uint8_t alpha_be[32],
                                       const porla_extract_xyt_req *reqs, size_t k, size_t n_total, int top_form, void *hip_stream);

/* ---- top-level repair: damaged rows of a top level written back, in place, from the other half ----
 * The call above computes wt^-1 Y_j for every top-level X row that fails its check and leaves it in scratch; the store stays damaged,
 * every later audit that draws the row fails, and a second hit on the same row index in the other half loses the level.  This call
 * heals the store: one request is one file's top level, both halves with their MAC rows, alignment stores and PRF values;
 * n_total is a power of two, 2 .. 2^16; top_form is PORLA_ICC_DECODE_EXACT or PORLA_ICC_DECODE_RESIDUE32 for the whole call; n_cols is
 * the SRS size (KZG) or 128 (IPA).
 *   1. Check.  Every row of both halves gets the status of porla_*_retrieve_aligned_batch_device on that half, byte for byte, in
 *      top_form's symbol width with the half's alignment store and PRF values: d_status_x, d_status_y.  Both halves of all K files are
 *      halves of ONE pass of the row check.  The statuses are the rows' BEFORE the repair.
 *   2. Source.  Row j of a half is repairable iff its own status is 0 and row j of the other half is OK; lost iff both are 0; untouched
 *      otherwise.
 *   3. Data row.  e = reverse_bits(top_step % n_total, log2 n_total), wt = w^e.  The candidate for an X row is wt^-1 Y_j, rule 3t
 *      above.  The candidate for a Y row is wt X_j: the p_icc plane by entry e of the encode's table of w^e mod p_icc, the q plane by
 *      (w^e mod p_icc) mod q, entry e of the encode's q-plane table; in the exact form the two are joined below LCM as the encode's
 *      finish joins them, in RESIDUE32 it is the p_icc plane alone.  With e == 0 the sibling row is copied as it lies.  Any 64 (32)
 *      bytes of the sibling row are defined: they are reduced as the decode's load reduces them.  The candidate is written over the
 *      row IN PLACE; PORLA_REPAIR_DATA is set iff the stored bytes differed from it.
 *   4. MAC row.  For every repairable row the expected MAC is E_j - alpha A_j, E_j taken over the row AS REPAIRED, A_j the half's
 *      alignment row as it lies; it is written over the row's MAC bytes as canonical affine bytes, and PORLA_REPAIR_MAC is set iff the
 *      stored bytes differed.  A repairable row whose data bytes were intact therefore always gets MAC.
 *   5. Lost rows get PORLA_REPAIR_LOST in both halves; not one byte of their data or MAC is written in either half.
 *   6. Rows that are OK are never written.  Alignment stores and PRF values are never written.
 *   7. d_counts, EIGHT words: [0] X rows with status 0, [1] Y rows with status 0, [2] X data rows rewritten, [3] X MAC rows rewritten,
 *      [4] Y data rows rewritten, [5] Y MAC rows rewritten, [6] lost row indices, [7] always 0.
 *   8. After the call every row of both halves that is not lost passes the aligned retrieval's check, and a second call on the same
 *      stores writes nothing: its actions are 0 except LOST, its counts [2 .. 5] are 0.
 * The authenticity of a repaired row rests on its sibling's check and on the linearity Y_j = wt X_j of the rebuild that wrote both
 * halves: the candidate is a function of a row that passed its MAC check, and the MAC written is the one the client would have sent
 * for it.  A damaged ALIGNMENT row is not restored: the row then fails its check with intact data, and the MAC written is the one
 * that satisfies the relation with the alignment as stored.
 * Launches: one upload, one clear, the row check, ONE patch kernel for both directions and all files (a lane per symbol, 16-byte
 * accesses, plain vector stores), and one more pass of the check's expected-MAC stages over all rows of both halves whose last
 * kernel writes the selected rows' MAC bytes instead of comparing.  The sequence does not depend on K, on which rows are damaged or
 * on whether any are.  Contract: as the calls above -- asynchronous on hip_stream, no side stream, no host wait beyond the retrieval
 * calls' first-use table upload, workspaces under their locks and fences.
 * PORLA_ERR_ARG (with a message, before the device is touched): reqs NULL with k > 0; any of the four store pointers, the two PRF
 * pointers, the two status pointers or the two action pointers NULL; a store, alignment or PRF pointer not 16-byte aligned; d_counts
 * not 4-byte aligned; n_total out of range; a top_form that is neither of the two; reserved != 0; more than 65535 requests; a byte
 * size that wraps; NULL alpha_be or bases (IPA); an overlap -- the four stores, the statuses, the actions and the counts are OUTPUTS
 * in the overlap walk, so, unlike in the extraction, no two requests may share a store and a store may overlap no input of the call.
 * k = 0 returns 0; KZG without key + SRS: PORLA_ERR_STATE; valid arguments without a device: PORLA_ERR_NO_DEVICE.
 * Not in this call: the lower levels (their Y halves are no row-wise multiples of their X halves: porla_*_repair_levels_batch_device
 * below rebuilds a whole Y half from its X half); restoring alignment stores; a row
 * damaged in both halves; a host-memory form; n_total > 2^16.  tools/bench_repair_top.py times it. */
#define PORLA_REPAIR_DATA 1   /* the row's data bytes were rewritten */
#define PORLA_REPAIR_MAC  2   /* the row's MAC bytes were rewritten */
#define PORLA_REPAIR_LOST 4   /* the row index is damaged in both halves: nothing was written */
#define PORLA_REPAIR_TOP_REQ_BYTES 120   /* sizeof(porla_repair_top_req) on LP64; the library static_asserts it and each offset */
typedef struct {
    void               *d_rows_x;    /*   0: the top X half, n_total rows in top_form.  Read AND WRITTEN */
    void               *d_macs_x;    /*   8: its MAC rows, 64 bytes each.  Read and written */
    const void         *d_align_x;   /*  16: its alignment store; NULL = every alignment at infinity.  Read only */
    const void         *d_prf_x;     /*  24: 16 raw bytes per row, read as d_prf is read everywhere */
    void               *d_rows_y;    /*  32: the top Y half, likewise */
    void               *d_macs_y;    /*  40 */
    const void         *d_align_y;   /*  48 */
    const void         *d_prf_y;     /*  56 */
    unsigned char      *d_status_x;  /*  64: n_total bytes: the row's status BEFORE the repair, PORLA_RETRIEVE_ROW_OK or 0 */
    unsigned char      *d_status_y;  /*  72 */
    unsigned char      *d_action_x;  /*  80: n_total bytes: what the call did to the row, PORLA_REPAIR_* bits */
    unsigned char      *d_action_y;  /*  88 */
    unsigned int       *d_counts;    /*  96: EIGHT words or NULL, zeroed by the call */
    unsigned long long  top_step;    /* 104: the write step the rebuild that wrote the top level was given, as in porla_extract_xyt_req */
    unsigned long long  reserved;    /* 112: must be 0; anything else is refused */
} porla_repair_top_req;
int porla_kzg_repair_top_batch_device(const porla_repair_top_req *reqs, size_t k, size_t n_total, int top_form, void *hip_stream);
int porla_ipa_repair_top_batch_device(porla_fixed_base *alpha_generators_fb, porla_fixed_base *h_fb, const uint8_t alpha_be[32],
                                      const porla_repair_top_req *reqs, size_t k, size_t n_total, int top_form, void *hip_stream);

/* ---- lower-level repair: the damaged rows of a lower level's Y half written back, in place, from the level's X half ----
 * porla_*_extract_xy_batch_device reports a damaged Y row of a lower level (d_counts[4], d_row_status_y) and heals nothing: every
 * later audit that draws the row fails, and a second hit on the X half of the same level then loses up to 2^i blocks, of which a
 * clean Y half would have kept the residues mod p_icc only.  Row by row the two halves share nothing, every block having been scaled
 * by its own wt; but the WHOLE Y half is an exact function of the whole X half, byte for byte (tests/test_repair_levels_cpu.py):
 *   data rows       the resident X half of level i is the one-shot data network (porla_icc_encode_device) over the chunks of its
 *                   epoch's 2^i blocks in write order, the resident Y half the same network over the rows y_p = chunk_p * wt_p mod
 *                   p_icc, wt_p = w^reverse_bits(step_p % n_total, log2 n_total), step_p rule 3y's "entry p of level i"; level 0's
 *                   one row is the input row itself, zero-extended.  So Y half = Encode(HAdd_y(DecodeExact(X half))).
 *   alignment rows  row j of the Y alignment store is the point network over Commit(c_p), c_p = (y_p - chunk_p * wt_p) mod q.  A
 *                   point butterfly multiplies by the integer v^i mod p_icc and so does the data network's q plane: by linearity
 *                   row j = Commit(N_j mod q), N the data network over the rows c_p.  No group-element network runs.
 * One request is one file's lower levels as porla_update_req lays them out; t = write_step % n_total decides residency as in the
 * extraction, and only the levels of levels & t are NAMED.  The mask is the caller's for the reason y_levels is: the launch shapes
 * are fixed on the host.  n_total is a power of two, 2 .. 2^16; n_cols is the SRS size (KZG) or 128 (IPA).
 *   1. Check.  Every row of the X half and of the Y half of every named level gets the status of
 *      porla_*_retrieve_aligned_batch_device, byte for byte: the X halves as PORLA_ICC_DECODE_EXACT without an alignment store, the Y
 *      halves as PORLA_ICC_DECODE_RESIDUE64 with align_y; level 0's rows are included.  All halves of all files are halves of ONE
 *      pass of the row check.  d_status_x, d_status_y hold the statuses BEFORE the repair, laid out like d_row_status_y of
 *      porla_extract_xy_req; the rows of unnamed levels get PORLA_EXTRACT_ROW_NOT_TRIED.
 *   2. Verdict per named level, d_level[i], in this order: PORLA_REPAIR_LEVEL_CLEAN -- no row of either half failed;
 *      PORLA_REPAIR_LEVEL_X_DAMAGED -- some X row failed: nothing of the level is written, its Y rows included; otherwise the level
 *      is UNDER REPAIR and ends as INCONSISTENT (rule 4) or REPAIRED (rule 5).  d_level[i] of a level that is not named is 0.
 *   3. Candidates of a level under repair: the exact decode of the X half (the ragged decode's body; level 0's row as it lies, a
 *      symbol with a nonzero upper half counted as bad); per block y_p and c_p with the block's own wt; the data network over the rows
 *      y_p on both planes, joined below LCM: the candidate data rows; the network over the rows c_p on the q plane, then one
 *      commitment per row against the resident SRS (KZG) or the generators (IPA): the candidate alignment rows as canonical affine
 *      bytes, a row of zero scalars giving 64 zero bytes.  The IPA call is handed the ALPHA generators only: it scales the rows c_p by
 *      alpha^-1 mod q before the network, which is linear, so the commitment is the one against the generators; alpha = 0 mod q is
 *      refused.
 *   4. Witnesses.  A level under repair is PORLA_REPAIR_LEVEL_INCONSISTENT if any Y row with status OK holds data bytes or alignment
 *      bytes that differ from its candidate, or if the X decode counts a bad symbol.  Such a level is not written at all; the differing
 *      rows are counted in d_counts[7].  Two halves that each pass their checks and disagree mean that write_step or the stores do not
 *      belong together, and writing then would destroy an authentic copy.  A level ALL of whose Y rows failed has no witness and is
 *      repaired: what is written there rests on the X half's row check and on the write steps the caller gave alone.
 *   5. Write, for a level under repair that is not inconsistent (PORLA_REPAIR_LEVEL_REPAIRED), on each FAILED Y row only: the data
 *      bytes that differ from the candidate are overwritten and PORLA_REPAIR_DATA is set; the alignment bytes likewise,
 *      PORLA_REPAIR_ALIGN; then the expected MAC E_j - alpha A_j over the row and the alignment as they now lie is written where the
 *      stored bytes differ, PORLA_REPAIR_MAC -- the top-level repair's write pass, a per-row permit in the place of the sibling's
 *      statuses.  Rows that checked OK, the X stores and the PRF values are never written.
 *   6. d_counts, EIGHT words: [0] X rows with status 0, [1] Y rows with status 0, [2] Y data rows rewritten, [3] Y alignment rows
 *      rewritten, [4] Y MAC rows rewritten, [5] levels repaired, [6] levels left X_DAMAGED or INCONSISTENT, [7] witness rows that
 *      differ.
 *   7. After the call every Y row of a REPAIRED level passes the aligned retrieval's check, its data, alignment and MAC bytes are
 *      those the update batch wrote before the damage, and a second call reports the level CLEAN and writes nothing.
 * d_work: porla_repair_levels_work_bytes(n_total, n_cols, write_step, levels) bytes of scratch, 16-byte aligned: 200 * n_cols * m
 * with m = levels & (write_step % n_total), the number of named rows -- per named row and column 32 bytes of decoded chunk (then
 * y_p), 32 of c_p, 64 of candidate symbol and 72 of residue planes between two passes.  0 for an n_total out of range or a size that
 * overflows.  The function touches no device.
 * Launches: one upload, one fill of the rows of alignment scalars with zeros, the clear, the row check, the plan, ONE ragged exact
 * decode over the named X halves of two rows and more, the per-block HAdd, then per level SIZE named in the call (two rows and more)
 * the passes of the data network over the rows y_p and over the rows c_p, the named level in blockIdx.y; ONE commitment pass over all
 * named rows and the kernel that makes its sums affine; the compare, the write, the write pass of the row check over the Y halves,
 * and the tally of actions, counters and verdicts.  The sequence depends on which level sizes are named in the call, never on K, on
 * which rows are damaged or on whether any are.  The per-level flag: the HAdd, the data passes, the compare and the write leave at
 * once for a level that is not under repair (a work-group reads the level's state word the plan set); the row check, the X decode,
 * the commitment pass (over rows of zero scalars for such a level) and the write pass run over ALL named rows.
 * Contract: as the calls above -- asynchronous on hip_stream, no side stream, no host wait beyond the retrieval calls' first-use table
 * upload, workspaces under their locks and fences.
 * PORLA_ERR_ARG (with a message, before the device is touched): reqs NULL with k > 0; n_total out of range; more than 65535
 * requests; reserved != 0; a byte size that wraps; more than 2^18 named rows in the call (the workspace of alignment scalars stops
 * there); with t > 0 a NULL d_status_x, d_status_y or d_action_y; a NULL d_level; with named levels a NULL data_x, mac_x, data_y, mac_y
 * or align_y (the arrays), d_prf_x, d_prf_y or d_work, and a named level with a NULL entry in any of the five families (align_y
 * included: the call may write it); a level pointer, d_prf_x, d_prf_y or d_work not 16-byte aligned, d_counts not 4-byte aligned; NULL
 * alpha_be or bases, alpha = 0 mod q (IPA); an overlap -- the Y stores, the statuses, the actions, the verdicts, the counts and d_work
 * are OUTPUTS in the overlap walk, the X stores and PRF values inputs that may be shared.  k = 0 returns 0; KZG without key + SRS:
 * PORLA_ERR_STATE; valid arguments without a device: PORLA_ERR_NO_DEVICE.
 * Not in this call: healing an X half (a clean Y half gives the chunks mod p_icc only, an X row is a value mod LCM); the top level
 * (porla_*_repair_top_batch_device above); a ragged forward network (one group of data-pass launches per level size instead); a
 * host-memory form; n_total > 2^16.  tools/bench_repair_levels.py times it. */
#define PORLA_REPAIR_ALIGN 8   /* d_action_y: the row's alignment bytes were rewritten (beside PORLA_REPAIR_DATA and PORLA_REPAIR_MAC) */
#define PORLA_REPAIR_LEVEL_CLEAN        1   /* d_level: no row of either half failed */
#define PORLA_REPAIR_LEVEL_X_DAMAGED    2   /* an X row failed: nothing of the level was written */
#define PORLA_REPAIR_LEVEL_INCONSISTENT 3   /* the halves pass their checks and disagree, or the X decode met a bad symbol: nothing written */
#define PORLA_REPAIR_LEVEL_REPAIRED     4   /* every failed Y row was written back */
#define PORLA_REPAIR_LEVELS_REQ_BYTES 128   /* sizeof(porla_repair_levels_req) on LP64; the library static_asserts it and each offset */
typedef struct {
    unsigned long long  write_step;  /*   0: the server's counter; t = write_step % n_total */
    unsigned long long  levels;      /*   8: bit i = check and repair level i; only the bits of levels & t count */
    void *const        *data_x;      /*  16: HOST array of log2(n_total) DEVICE pointers, as in porla_extract_req: the X data stores.  Read only */
    void *const        *mac_x;       /*  24: the X MAC stores.  Read only */
    const void         *d_prf_x;     /*  32: 16 raw bytes per lower-level row, laid out like the lower-level part of d_prf in
                                             porla_extract_xy_req (t entries); only the entries of named levels are read */
    const void         *d_prf_y;     /*  40: the same for the Y halves */
    void *const        *data_y;      /*  48: the Y data stores.  Read AND WRITTEN */
    void *const        *mac_y;       /*  56: the Y MAC stores.  Read and written */
    void *const        *align_y;     /*  64: the Y alignment stores.  Read and written; a named level's entry must not be NULL */
    void               *d_work;      /*  72: porla_repair_levels_work_bytes(...) bytes of scratch */
    unsigned char      *d_status_x;  /*  80: t bytes: the row's status BEFORE the repair, or PORLA_EXTRACT_ROW_NOT_TRIED */
    unsigned char      *d_status_y;  /*  88 */
    unsigned char      *d_action_y;  /*  96: t bytes: what the call did to the Y row, PORLA_REPAIR_DATA | _MAC | _ALIGN */
    unsigned char      *d_level;     /* 104: 16 bytes: level i's verdict, PORLA_REPAIR_LEVEL_*, 0 = not named */
    unsigned int       *d_counts;    /* 112: EIGHT words or NULL, zeroed by the call */
    unsigned long long  reserved;    /* 120: must be 0; anything else is refused */
} porla_repair_levels_req;
size_t porla_repair_levels_work_bytes(size_t n_total, size_t n_cols, unsigned long long write_step, unsigned long long levels);
int porla_kzg_repair_levels_batch_device(const porla_repair_levels_req *reqs, size_t k, size_t n_total, void *hip_stream);
int porla_ipa_repair_levels_batch_device(porla_fixed_base *alpha_generators_fb, porla_fixed_base *h_fb, const uint8_t alpha_be[32],
                                         const porla_repair_levels_req *reqs, size_t k, size_t n_total, void *hip_stream);

/* ---- AES on the device: the MAC PRF of the client writes, the audit challenge from its seed, the client's complement scalar ----
 * These calls PRODUCE the buffers the batches above consume (d_prf; d_idx* / d_coef* / d_mac_*; the 32-byte scalars of
 * porla_kzg_complement_batch_device or of a one-point fixed base) and change none of them.  Both uses are standard AES-128
 * (FIPS-197): the reference's PRG (porla/Utils/prg.h:44-50, 84-97) and AES_encrypt under SECRET_KEY (Client.hpp:423-443).
 * Definitions, written once for host and device: porla_amd/csrc/challenge_host.hpp; INTEGRATION s3g has the flow.
 *
 * The MAC PRF.  A run names count triples: slot t is (level, index0 + t, time0 + t * time_stride), index wrapping as an int32 does,
 * and its value the 16 raw bytes of AES(key16, level int32 LE | index int32 LE | time int64 LE).  porla_mac_prf_batch_device writes
 * the values of all runs back to back in run order into d_out (device memory, 16-byte aligned, 16 * sum count bytes), asynchronously
 * on hip_stream: no host wait, no side stream.  runs is a HOST array.  One lane per AES block; the round keys are expanded on the
 * host and travel as a kernel argument; the one 1 KiB table lives in LDS.  porla_mac_prf_host is the same on the host, no device.
 * PORLA_ERR_ARG (with a message, before the device is touched): key16, runs or d_out NULL while there is something to write; d_out
 * not 16-byte aligned; more than 2^38 values in one call.  n_runs = 0 or all counts 0 returns 0; valid arguments without a device:
 * PORLA_ERR_NO_DEVICE. */
#define PORLA_PRF_RUN_BYTES 32   /* sizeof(porla_prf_run) on LP64; the library static_asserts it and each offset */
typedef struct {
    int level; int index0;                     /* offsets 0, 4 */
    unsigned long long count;                  /* 8 */
    long long time0; long long time_stride;    /* 16, 24 */
} porla_prf_run;
int porla_mac_prf_batch_device(const uint8_t key16[16], const porla_prf_run *runs, size_t n_runs, void *d_out, void *hip_stream);
int porla_mac_prf_host(const uint8_t key16[16], const porla_prf_run *runs, size_t n_runs, uint8_t *out);
/* the run list whose values are the d_prf of one request of porla_*_client_update_batch_device (PORLA_PRF_UPDATE: level + 2 runs,
 * 2^(level+2) - 1 values) or porla_*_client_rebuild_batch_device (PORLA_PRF_REBUILD: 3 runs, 3 * n_total + 1 values; level is
 * ignored), in the order those requests document.  write_step is the request's (after the ++ of Client.hpp:480).  Host only.
 *   update:  (0, block_id, W - 1); for i < level: (i, j, t_i), j < 2^(i+1), t_i = (W & ~2^level) | (2^level - 2^i); (level, j, W), j < 2^(level+1)
 *   rebuild: (0, block_id, W - 1); (0, i + 1, W - n_total + i), i < n_total; (log2 n_total, j, W), j < 2 n_total
 * PORLA_ERR_ARG: what the batches refuse (n_total not a power of two in 2 .. 2^30; update: level < 0 or 2^level > n_total / 2,
 * write_step % n_total == 0), an unknown kind, a NULL output, max_runs too small. */
#define PORLA_PRF_UPDATE  0
#define PORLA_PRF_REBUILD 1
int porla_client_prf_runs(int kind, int block_id, unsigned long long write_step, int level, size_t n_total, porla_prf_run *runs_out,
                          size_t max_runs, size_t *n_runs, size_t *n_values);

/* The audit challenge from its 16-byte seed (Server.hpp:595-732, Client.hpp:682-744).  s = the int stream of the PRG keyed with the
 * seed: int t is the little-endian int32 at byte 4t of AES(seed, counter as u64 LE | 0), counters from 0.  N = num_blocks (a power of
 * two, 2 .. 2^24), H = log2 N + 1, ws = write_step % N.  Level i (l = 2^i) is challenged iff bit i of ws is set or i = H - 1; with
 * 2l > 128 it has 128 points, index = mag(s[pos + j]) mod 2l, coef = mag(s[pos + 128 + j]), pos += 256; otherwise its 2l rows, index =
 * j, coef = mag(s[pos + j]), pos += 2l.  index >= l is row index - l of the Y half, otherwise row index of the X half.
 * mag(v) = |v| as a uint32 with mag(INT32_MIN) = 2^31: the one place the library DEFINES what the reference leaves undefined (abs).
 * levels is a HOST array of H descriptors: the row numbers at which level i's halves begin inside the caller's stores (data_*: in
 * the store the level's form names, 0 = the 64-byte rows of d_rows64, 1 = the 32-byte rows of d_rows32; mac_*: in d_mac_store /
 * d_align_store).  For point p (numbered in walk order) at level i, row r of half X / Y:
 *   d_mac_idx[p] = mac_{x|y}[i] + r, d_mac_coef[p] = coef, and the pair (data_{x|y}[i] + r, coef) is appended, in point order, to
 *   (d_idx64, d_coef64) or (d_idx32, d_coef32).
 * infos_out[k] is HOST memory, filled before the call returns (it needs the seed, write_step, num_blocks, the forms and two AES
 * blocks): the list lengths, KZG's random_point = (uint64)(int64) s[pos] (Server.hpp:907) and IPA's a = s[n_points] (:861) raw and as
 * a_value (32 bytes big-endian, a mod n: a negative a is n - |a|).  A caller fills porla_kzg_audit_req / porla_ipa_audit_req from it
 * and enqueues the audit batch right behind this call on the same stream.  The six outputs are device memory (idx 8-, coef 4-byte
 * aligned); a request with all six NULL is planned only, and a call of such requests touches no device.
 * porla_audit_challenge_host: the same with the six outputs in HOST memory; no device.
 * Asynchronous on hip_stream, no host wait, no side stream.  PORLA_ERR_ARG (with a message, before the device is touched): reqs or
 * infos_out NULL while k > 0; levels NULL; num_blocks not a power of two in 2 .. 2^24; form > 1; pad != 0; a NULL or misaligned list
 * whose count is > 0 (unless all six are NULL); more than 65535 requests.  k = 0 returns 0; valid arguments without a device:
 * PORLA_ERR_NO_DEVICE. */
#define PORLA_AUDIT_LEVEL_BYTES 40            /* sizeof(porla_audit_level) */
#define PORLA_AUDIT_CHALLENGE_REQ_BYTES 88    /* sizeof(porla_audit_challenge_req) on LP64 */
#define PORLA_AUDIT_CHALLENGE_INFO_BYTES 72   /* sizeof(porla_audit_challenge_info) */
typedef struct {
    unsigned long long data_x, data_y, mac_x, mac_y;   /* offsets 0, 8, 16, 24 */
    int form; int pad;                                 /* 32, 36 */
} porla_audit_level;
typedef struct {
    uint8_t seed[16];                                  /* 0 */
    unsigned long long write_step, num_blocks;         /* 16, 24 */
    const porla_audit_level *levels;                   /* 32 */
    uint64_t *d_idx64; uint32_t *d_coef64;             /* 40, 48 */
    uint64_t *d_idx32; uint32_t *d_coef32;             /* 56, 64 */
    uint64_t *d_mac_idx; uint32_t *d_mac_coef;         /* 72, 80 */
} porla_audit_challenge_req;
typedef struct {
    unsigned long long n64, n32, n_macs;               /* 0, 8, 16 */
    unsigned long long random_point;                   /* 24 */
    int a_raw; int pad;                                /* 32, 36 */
    uint8_t a_value[32];                               /* 40 */
} porla_audit_challenge_info;
int porla_audit_challenge_batch_device(const porla_audit_challenge_req *reqs, size_t k, porla_audit_challenge_info *infos_out,
                                       void *hip_stream);
int porla_audit_challenge_host(const porla_audit_challenge_req *reqs, size_t k, porla_audit_challenge_info *infos_out);

/* The client's side of a MAC check without a complement store.  Every complement is prf * h, so sum_p coef_p * comp[idx_p] =
 * (sum_p coef_p * val_p) * h: d_scalars[k] (device memory, 32 bytes big-endian each) is that sum for the challenge of reqs[k], val_p the
 * PRF output of (i, index, write_step & ~(2^i - 1)) -- the FULL write_step, Client.hpp:646-650 -- read as the write batches read it
 * (curve 0, KZG: a big-endian 128-bit integer; curve 1, IPA: r.d[0], r.d[1], a little-endian one).  The sum is exact: every term is
 * < 2^160 and there are fewer than 2^12 of them, so it stays below 2^172 and below either group order.  ONE point P_k = s_k * h
 * (porla_kzg_complement_batch_device, or a commit against the one-point base h_fb) then stands in for the whole store in
 * porla_*_verify_batch_device: d_comp_store = P_k, idx = [0], coef = [1], n = 1.  One work-group per request.
 * Asynchronous on hip_stream.  PORLA_ERR_ARG: key16, reqs or d_scalars NULL while k > 0; curve not 0 or 1; num_blocks as above; more
 * than 65535 requests.  k = 0 returns 0; no device: PORLA_ERR_NO_DEVICE.  _host: scalars in host memory, no device. */
#define PORLA_AUDIT_SCALAR_REQ_BYTES 32
typedef struct {
    uint8_t seed[16];
    unsigned long long write_step, num_blocks;
} porla_audit_scalar_req;
int porla_audit_complement_scalar_batch_device(const uint8_t key16[16], const porla_audit_scalar_req *reqs, size_t k, int curve,
                                               void *d_scalars, void *hip_stream);
int porla_audit_complement_scalar_host(const uint8_t key16[16], const porla_audit_scalar_req *reqs, size_t k, int curve,
                                       uint8_t *scalars);
/* diagnostic (tests): the walk of porla_audit_challenge_* over an int stream the caller wrote in place of the PRG's, on the host
 * (on_device = 0) or through the device kernel (1; blocking).  Everything is HOST memory; all six lists and info are required and
 * hold up to n_macs entries; n_ints must cover every int the walk and its tail read. */
int porla_diag_audit_walk(const int32_t *stream_ints, size_t n_ints, unsigned long long write_step, unsigned long long num_blocks,
                          const porla_audit_level *levels, int on_device, uint64_t *idx64, uint32_t *coef64, uint64_t *idx32,
                          uint32_t *coef32, uint64_t *mac_idx, uint32_t *mac_coef, porla_audit_challenge_info *info);

/* ---- audit row combine (Server::audit, Server.hpp:790-828) + the scalar part of align_MAC on the result (:531-541) ----
 * B_j = sum_i coeff_i * row_i[j] (exact integer), then aligned_j = B_j mod p_icc, c_j = (aligned_j - B_j) mod q.
 * The challenged rows are addressed inside row stores resident in HBM:
 *   d_rows64 : store of 512-bit rows, n_cols * 64 bytes per row, little-endian values < LCM (utils.h:473-517, cached levels)
 *   d_rows32 : store of 256-bit rows, n_cols * 32 bytes per row, little-endian (levels kept aligned)
 *   d_idx*   : row numbers inside the store (uint64), d_coef* : abs(int32) coefficients (Server.hpp:617-621), n* : counts
 * outputs (each may be NULL): exact 80 bytes/column LE (the unreduced B_j), aligned 32 B LE, aligned_be 32 B BE (the
 * coefficient format of create_proof / compute_digest_from_srs), scalars c_j 32 B BE.  curve selects q as for the ICC encode. */
int porla_audit_combine_device(const void *d_rows64, const uint64_t *d_idx64, const uint32_t *d_coef64, size_t n64,
                               const void *d_rows32, const uint64_t *d_idx32, const uint32_t *d_coef32, size_t n32,
                               size_t n_cols, int curve, void *d_exact_out, void *d_aligned_out, void *d_aligned_be_out,
                               void *d_scalars_out, void *hip_stream);

#ifdef __cplusplus
}
#endif
#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#endif
