// Host side of the batched MSM (kernels: msm_batch.hip.h): the work list of every launch round, built from the caller's offsets
// in one pinned buffer and uploaded with one copy, then per round a fixed sequence -- clear the arrival counters, k_batch_tiny,
// k_batch_bucket, k_batch_fold, k_fb_finish -- on the caller's stream.  Included by one translation unit per curve.
#pragma once
#include "engine.hpp"
#include "msm_batch.hip.h"
#include <vector>

namespace porla {

struct BatchRound {
    size_t e0, k;            // entries [e0, e0 + k)
    uint64_t pair0;          // the round's first pair
    uint32_t nb, nf, nq;     // bucket blocks, bucket entries, tiny quads (padding included)
    size_t words;            // offset of the round's work list in the buffer (32-bit words): entries, blk, fold, tq
};

// bucket blocks of an entry of n pairs: `lone` = what a lone k_small_msm takes (msm_impl.hip.h), else ceil(n / 64) and at least
// bmin (> the windows' count of every shape small_cfg can pick, so that every window has a block)
static inline uint32_t batch_blocks(uint64_t n, bool lone, uint32_t bmin) {
    const uint32_t cap = small_lone_blocks(n);
    if (lone) return cap;
    uint32_t b = (uint32_t)((n + 63) / 64);
    if (b < bmin) b = bmin;
    return b > cap ? cap : b;
}

// K independent MSMs (arguments checked by the C ABI: offsets non-decreasing from 0, entries <= SMALL_MAX_N, non-null pointers);
// enqueued on `stream`, results written to d_out, no host wait for this call's work.  ws->mu held.
// raw_sums != nullptr: the entries' projective sums go there instead (entry e at raw_sums[e]) and d_out is not used.
template <class C>
static int msm_batch_locked(Workspace* ws, const uint8_t* d_scalars, const uint8_t* d_points, const uint64_t* offsets, size_t k, uint8_t* d_out,
                            hipStream_t stream, XYZZ<typename C::Fp>* raw_sums = nullptr) {
    using M = typename C::Fp;
    int rc;
    const uint32_t bmin = g_use_glv == 0 ? 34u : 18u;        // windows: <= 33 over unsplit 256-bit scalars, <= 17 otherwise (c = 8)
    const int c_flags = g_small_c | (g_use_glv == 0 ? 0x100 : 0);
    // ---- cut the batch into rounds and size each one's work list
    std::vector<BatchRound> rounds;
    {
        // rounds: entries, pairs, bucket blocks (at the batch allotment) and tiny quads (padding included) within the round limits
        BatchRound cur = {0, 0, 0, 0, 0, 0, 0};
        uint32_t qfill = 0;                                  // quads used in the current block of k_batch_tiny
        for (size_t e = 0; e < k; e++) {
            const uint64_t n = offsets[e + 1] - offsets[e];
            const bool tiny = n <= BATCH_TINY_MAX;
            const uint32_t nq = tiny ? (n ? (uint32_t)n : 1u) : 0u;
            const uint32_t pad = tiny && qfill + nq > (uint32_t)BATCH_QUADS ? (uint32_t)BATCH_QUADS - qfill : 0u;
            const uint32_t nb = tiny ? 0u : batch_blocks(n, false, bmin);
            if (cur.k && (cur.k + 1 > BATCH_ROUND_ENTRIES || offsets[e + 1] - cur.pair0 > BATCH_ROUND_PAIRS ||
                          cur.nb + nb > BATCH_ROUND_BLOCKS || cur.nq + pad + nq > BATCH_ROUND_QUADS)) {
                rounds.push_back(cur);
                cur = {e, 0, offsets[e], 0, 0, 0, 0};
                qfill = 0;
                e--;
                continue;
            }
            if (tiny) {
                cur.nq += pad + nq;
                qfill = (qfill + pad + nq) % (uint32_t)BATCH_QUADS;
            } else {
                cur.nb += nb;
                cur.nf++;
            }
            cur.k++;
        }
        rounds.push_back(cur);
    }
    // the lone MSM's allotment when even that fills at most two blocks per compute unit: latency, as a lone call has it
    std::vector<char> lone(rounds.size(), 0);
    size_t words = 0;
    for (size_t ri = 0; ri < rounds.size(); ri++) {
        BatchRound& R = rounds[ri];
        uint64_t lone_blocks = 0;
        for (size_t e = R.e0; e < R.e0 + R.k; e++) {
            const uint64_t n = offsets[e + 1] - offsets[e];
            if (n > BATCH_TINY_MAX) lone_blocks += batch_blocks(n, true, bmin);
        }
        if (lone_blocks <= 2u * (uint32_t)SMALL_BLOCKS) { lone[ri] = 1; R.nb = (uint32_t)lone_blocks; }
        R.words = words;
        words += 4 * R.k + R.nb + R.nf + R.nq;
    }
    {
        // ---- the work list into pinned memory (a buffer whose previous upload is still queued is retired, not waited for)
        if ((rc = ws->batch_list_h.stage(words * 4))) return rc;
        uint32_t* h = (uint32_t*)ws->batch_list_h.h;
        for (size_t ri = 0; ri < rounds.size(); ri++) {
            BatchRound& R = rounds[ri];
            BatchEntry* ents = (BatchEntry*)(h + R.words);
            uint32_t* blk = h + R.words + 4 * R.k;
            uint32_t* fold = blk + R.nb;
            uint32_t* tq = fold + R.nf;
            uint32_t base = 0, nf = 0, nq = 0;
            for (size_t i = 0; i < R.k; i++) {
                const size_t e = R.e0 + i;
                const uint64_t n = offsets[e + 1] - offsets[e];
                BatchEntry be;
                be.off = (uint32_t)(offsets[e] - R.pair0);
                be.n = (uint32_t)n;
                be.base = 0;
                be.blocks = 0;
                if (n > BATCH_TINY_MAX) {
                    be.base = base;
                    be.blocks = batch_blocks(n, lone[ri] != 0, bmin);
                    for (uint32_t b = 0; b < be.blocks; b++) blk[base + b] = (uint32_t)i;
                    base += be.blocks;
                    fold[nf++] = (uint32_t)i;
                } else {
                    const uint32_t m = n ? (uint32_t)n : 1u;
                    const uint32_t fill = nq % (uint32_t)BATCH_QUADS;
                    if (fill + m > (uint32_t)BATCH_QUADS)
                        for (uint32_t t = fill; t < (uint32_t)BATCH_QUADS; t++) tq[nq++] = BATCH_IDLE;
                    for (uint32_t t = 0; t < m; t++) tq[nq++] = (uint32_t)i | (t << 20);
                }
                ents[i] = be;
            }
            if (base != R.nb || nf != R.nf || nq != R.nq) {
                set_last_error("porla: batched MSM work list does not match its sizing");
                return PORLA_ERR_STATE;
            }
        }
    }
    size_t list_words = 0, max_k = 0;
    uint32_t max_nb = 0;
    for (const BatchRound& R : rounds) {
        list_words = R.words + 4 * R.k + R.nb + R.nf + R.nq;
        if (R.k > max_k) max_k = R.k;
        if (R.nb > max_nb) max_nb = R.nb;
    }
    // ---- device scratch: the work list, the blocks' partial sums + window sums, the entries' sums, counters + shapes
    if ((rc = ws->batch_fence.enter(stream))) return rc;
    const size_t part_bytes = (size_t)max_nb * SMALL_MAX_C * sizeof(XYZZ<M>);
    if ((rc = ws->batch_list.ensure(list_words * 4))) return rc;
    if ((rc = ws->batch_part.ensure(2 * part_bytes + 256))) return rc;
    if ((rc = ws->batch_sums.ensure(max_k * sizeof(XYZZ<M>) + 256))) return rc;
    if ((rc = ws->batch_ctrl.ensure(((size_t)max_nb + max_k) * 4 + 256))) return rc;
    if ((rc = ws->batch_list_h.send(ws->batch_list.p, list_words * 4, stream))) return rc;
    const uint32_t* d_list = (const uint32_t*)ws->batch_list.p;
    XYZZ<M>* part = (XYZZ<M>*)ws->batch_part.p;
    XYZZ<M>* fin = (XYZZ<M>*)((uint8_t*)ws->batch_part.p + part_bytes);
    XYZZ<M>* const round_sums = (XYZZ<M>*)ws->batch_sums.p;
    uint32_t* counters = (uint32_t*)ws->batch_ctrl.p;
    uint32_t* shape = counters + max_nb;
    for (const BatchRound& R : rounds) {
        if (R.k == 0) continue;
        const BatchEntry* ents = (const BatchEntry*)(d_list + R.words);
        const uint32_t* blk = d_list + R.words + 4 * R.k;
        const uint32_t* fold = blk + R.nb;
        const uint32_t* tq = fold + R.nf;
        const uint8_t* sc = d_scalars + 32 * R.pair0;
        const uint8_t* pt = d_points + 64 * R.pair0;
        XYZZ<M>* sums = raw_sums ? raw_sums + R.e0 : round_sums;
        if (R.nq) {
            ProfScope ps("batch_tiny", stream);
            hipLaunchKernelGGL((k_batch_tiny<C>), dim3((R.nq + BATCH_QUADS - 1) / BATCH_QUADS), dim3(4 * BATCH_QUADS), 0, stream, sc, pt, ents, tq,
                               R.nq, sums);
            PORLA_HIP(hipGetLastError());
        }
        if (R.nb) {
            // the arrival counters and the shapes start at zero (a shape never written would fold as infinity, not as stale sums)
            PORLA_HIP(hipMemsetAsync(counters, 0, ((size_t)max_nb + R.k) * 4, stream));
            {
                ProfScope ps("batch_bucket", stream);
                hipLaunchKernelGGL((k_batch_bucket<C>), dim3(R.nb), dim3(SMALL_THREADS), 0, stream, sc, pt, ents, blk, c_flags, part, counters,
                                   fin, shape);
                PORLA_HIP(hipGetLastError());
            }
            ProfScope ps("batch_fold", stream);
            hipLaunchKernelGGL((k_batch_fold<C>), dim3((R.nf + BATCH_QUADS - 1) / BATCH_QUADS), dim3(4 * BATCH_QUADS), 0, stream, ents, fold, R.nf,
                               (const XYZZ<M>*)fin, (const uint32_t*)shape, sums);
            PORLA_HIP(hipGetLastError());
        }
        if (!raw_sums) {
            ProfScope ps("batch_finish", stream);
            uint8_t* out = d_out + 64 * R.e0;
            if (R.k <= 4096) hipLaunchKernelGGL((k_fb_finish<C, 1>), dim3((unsigned)((R.k + 63) / 64)), dim3(64), 0, stream, sums, (uint32_t)R.k, 1u, out);
            else hipLaunchKernelGGL((k_fb_finish<C, FB_FINISH_ROWS_MAX>), dim3((unsigned)((R.k + 64 * FB_FINISH_ROWS_MAX - 1) / (64 * FB_FINISH_ROWS_MAX))),
                                    dim3(64), 0, stream, sums, (uint32_t)R.k, 1u, out);
            PORLA_HIP(hipGetLastError());
        }
    }
    return ws->batch_fence.leave(stream);
}

template <class C>
int msm_batch_device(const uint8_t* d_scalars, const uint8_t* d_points, const uint64_t* offsets, size_t k, uint8_t* d_out, hipStream_t stream) {
    int rc = ensure_device();
    if (rc) return rc;
    if (k == 0) return PORLA_OK;
    Workspace* ws;
    if ((rc = lease_blocking_slot(&ws))) return rc;
    std::lock_guard<std::mutex> lk(ws->mu, std::adopt_lock);
    return msm_batch_locked<C>(ws, d_scalars, d_points, offsets, k, d_out, stream);
}

template <class C>
int msm_batch_sums_device(const uint8_t* d_scalars, const uint8_t* d_points, const uint64_t* offsets, size_t k, XYZZ<typename C::Fp>* d_sums,
                          hipStream_t stream) {
    int rc = ensure_device();
    if (rc) return rc;
    if (k == 0) return PORLA_OK;
    Workspace* ws;
    if ((rc = lease_blocking_slot(&ws))) return rc;
    std::lock_guard<std::mutex> lk(ws->mu, std::adopt_lock);
    return msm_batch_locked<C>(ws, d_scalars, d_points, offsets, k, nullptr, stream, d_sums);
}

// host buffers: upload to the slot's staging buffers, the batch on the slot's own stream, results back, wait
template <class C>
int msm_batch_host(const uint8_t* scalars, const uint8_t* points, const uint64_t* offsets, size_t k, uint8_t* out) {
    int rc = ensure_device();
    if (rc) return rc;
    if (k == 0) return PORLA_OK;
    Workspace* ws;
    if ((rc = lease_blocking_slot(&ws))) return rc;
    std::lock_guard<std::mutex> lk(ws->mu, std::adopt_lock);
    const size_t n = (size_t)offsets[k];
    hipStream_t s = ws->own_stream;
    if ((rc = ws->in_scalars.ensure(n * 32 + 32))) return rc;
    if ((rc = ws->in_points.ensure(n * 64 + 64))) return rc;
    if ((rc = ws->batch_out.ensure(k * 64))) return rc;
    if (n) {
        PORLA_HIP(hipMemcpyAsync(ws->in_scalars.p, scalars, n * 32, hipMemcpyHostToDevice, s));
        PORLA_HIP(hipMemcpyAsync(ws->in_points.p, points, n * 64, hipMemcpyHostToDevice, s));
    }
    if ((rc = msm_batch_locked<C>(ws, (const uint8_t*)ws->in_scalars.p, (const uint8_t*)ws->in_points.p, offsets, k, (uint8_t*)ws->batch_out.p, s)))
        return rc;
    PORLA_HIP(hipMemcpyAsync(out, ws->batch_out.p, k * 64, hipMemcpyDeviceToHost, s));
    PORLA_HIP(hipStreamSynchronize(s));
    return PORLA_OK;
}

}  // namespace porla
