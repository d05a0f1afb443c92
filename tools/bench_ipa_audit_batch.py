#!/usr/bin/env python3
"""bench_ipa_audit_batch.py -- many IPA audits per call, proofs included (porla_ipa_audit_batch_device), against the same audits
through the single-call path: per audit one porla_ipa_audit_device and six porla_fixed_base_commit_host calls of two rows (the
rounds of Server::inner_product_prove), server side, the level and its MAC arrays resident in HBM.

Setup: a level of 2^15 blocks of random 64-byte symbols, a MAC store of 2^15 secp256k1 points (commitments of random scalars), a
rotated copy of it as the alignment store; the fixed base over generators[0..127] || u.  For each K every audit has its own challenge
(--points rows, abs(int32) coefficients) and its own a_value.

Baseline time: the folding of a and b, the x_values and the transcript hash between the rounds are Python integers here (the
reference runs them in NTL and C).  Their time is NOT part of the baseline: only the seven engine calls per audit are timed
(perf_counter around each call, summed), which is the same as measuring the whole loop and subtracting the Python arithmetic.  That
favours the baseline.  `host_python_ms` reports what was left out.

Prints ONE JSON line per K in bench.py's format: value = audits/s through the batch (K / median batch time over --reps calls, the
device drained around each, after >= 0.25 s of warm-up calls); `sequential_*` = the baseline over --seq-reps passes; both spreads
(min, max); `speedup`; `kernels_ms` = time per kernel of one profiled batch call; `bit_exact` = every record equals the reply
assembled from the single-call path in the same run (points compressed, combined_align after align_MAC, the proof from the host
rounds) and every B the single call's."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NCOLS = 128
REC = 655


def profile_kernels(fn):
    from porla_amd import lib
    lib.porla_gpu_profile_enable(1)
    fn()
    out = {}
    name = ctypes.create_string_buffer(64)
    ms, n = ctypes.c_double(), ctypes.c_longlong()
    slot = 0
    while lib.porla_gpu_profile_get(slot, name, 64, ctypes.byref(ms), ctypes.byref(n)) == 0:
        out[name.value.decode()] = round(ms.value, 4)
        slot += 1
    lib.porla_gpu_profile_enable(0)
    return out


def single_path(fb, a, clock):
    """one audit through porla_ipa_audit_device and six two-row commit_host rounds -> (record, B); clock[0] += the engine calls' time,
    clock[1] += the Python arithmetic's"""
    from tests import ipa_proof_py as ipa
    N = ipa.N
    t0 = time.perf_counter()
    one = fb.ipa_audit_device(*a[:8], NCOLS, *a[8:13])
    t1 = time.perf_counter()
    clock[0] += t1 - t0
    va = [int.from_bytes(one["b"][32 * i:32 * i + 32], "big") for i in range(NCOLS)]
    vb = ipa.audit_b(a[13])
    proof = ipa.le32(sum(x * y for x, y in zip(va, vb)) % N)
    xv = [1] * NCOLS
    sha = ipa.Transcript()
    sha.write(ipa.TAG)
    sha.write(proof)
    h = sha.finalize()
    half = NCOLS // 2
    be = lambda v: v.to_bytes(32, "big")
    while half > 1:
        x = ipa.challenge(h)
        ix = ipa.inv(x)
        row_l, row_r = [0] * (NCOLS + 1), [0] * (NCOLS + 1)
        row_l[NCOLS] = sum(va[i] * vb[half + i] for i in range(half)) % N
        row_r[NCOLS] = sum(va[half + i] * vb[i] for i in range(half)) % N
        for j in range(NCOLS):
            q = j % half
            if (j // half) & 1:
                row_l[j] = va[q] * xv[j] % N
                xv[j] = xv[j] * x % N
            else:
                row_r[j] = va[half + q] * xv[j] % N
                xv[j] = xv[j] * ix % N
        rows = b"".join(be(v) for v in row_l) + b"".join(be(v) for v in row_r)
        t2 = time.perf_counter()
        clock[1] += t2 - t1
        lr = fb.commit_host(rows, 2, NCOLS + 1)
        t1 = time.perf_counter()
        clock[0] += t1 - t2
        for p in (lr[:64], lr[64:]):
            ser = ipa.compress(p)
            proof += ser
            sha.write(ser)
            h = sha.finalize()
        va = [(va[i] * x + va[i + half] * ix) % N for i in range(half)]
        vb = [(vb[i] * ix + vb[i + half] * x) % N for i in range(half)]
        half >>= 1
    for i in range(2):
        proof += ipa.le32(va[i]) + ipa.le32(vb[i])
    align = ipa.msm([(1, one["combined_align"]), (1, one["align_value"])])
    rec = ipa.compress(one["commitment"]) + ipa.compress(one["combined_mac"]) + ipa.compress(align) + proof
    clock[1] += time.perf_counter() - t1
    return rec, one["b"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,8,64,256")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seq-reps", type=int, default=5)
    ap.add_argument("--log2blocks", type=int, default=15)
    ap.add_argument("--points", type=int, default=3200)
    ap.add_argument("--window", type=int, default=0, help="window bits of the 129-point table (0: PORLA_COMMIT_TABLE_GB / PORLA_COMMIT_WINDOW)")
    ap.add_argument("--out")
    args = ap.parse_args()

    import numpy as np
    import torch
    from porla_amd import multiexp as mx
    from tests import common

    assert torch.cuda.is_available(), "bench_ipa_audit_batch.py needs a GPU (the engine has no CPU path)"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    cs = torch.cuda.current_stream()
    stream = cs.cuda_stream
    n, m = 1 << args.log2blocks, args.points
    gens_u = common.secp_bench_points(NCOLS + 1)
    fb = mx.FixedBase("secp256k1", gens_u, NCOLS + 1, args.window)
    g = torch.Generator(device=dev).manual_seed(77)
    d_x = torch.randint(0, 256, (64 * n * NCOLS,), dtype=torch.uint8, device=dev, generator=g)
    d_sc = torch.randint(0, 256, (32 * n,), dtype=torch.uint8, device=dev, generator=g)
    d_macs = torch.empty(64 * n, dtype=torch.uint8, device=dev)
    fb.commit_device(d_sc.data_ptr(), n, 1, d_macs.data_ptr(), stream)
    torch.cuda.synchronize()
    d_align = torch.roll(d_macs.view(n, 64), 1, 0).contiguous().view(-1)

    rng = np.random.Generator(np.random.PCG64(9))
    lines = []
    for k in [int(x) for x in args.ks.split(",")]:
        d_idx = torch.from_numpy(rng.integers(0, n, (k, m), dtype=np.int64)).cuda()
        d_coef = torch.from_numpy(rng.integers(0, 1 << 31, (k, m), dtype=np.int64).astype(np.uint32).view(np.int32)).cuda()
        vs = [int.from_bytes(rng.bytes(32), "big") for _ in range(k)]
        audits = [(d_x.data_ptr(), d_idx[a].data_ptr(), d_coef[a].data_ptr(), m, 0, 0, 0, 0, d_macs.data_ptr(), d_align.data_ptr(),
                   d_idx[a].data_ptr(), d_coef[a].data_ptr(), m, vs[a]) for a in range(k)]
        d_out = torch.zeros(REC * k, dtype=torch.uint8, device=dev)
        d_b = torch.zeros(32 * NCOLS * k, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()

        def batch():
            fb.ipa_audit_batch_device(audits, d_out.data_ptr(), d_b.data_ptr(), stream)

        warm, t0 = 0, time.perf_counter()
        while warm < 3 or time.perf_counter() - t0 < 0.25:
            batch()
            torch.cuda.synchronize()
            warm += 1
        times = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(cs)
            batch()
            e1.record(cs)
            e1.synchronize()
            times.append(max(e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3))
        got, got_b = bytes(d_out.cpu().numpy()), bytes(d_b.cpu().numpy())

        clock = [0.0, 0.0]
        ones = [single_path(fb, a, clock) for a in audits]       # warm-up + the reference replies
        want, want_b = b"".join(o[0] for o in ones), b"".join(o[1] for o in ones)
        seq, py = [], []
        for _ in range(args.seq_reps):
            torch.cuda.synchronize()
            clock = [0.0, 0.0]
            for a in audits:
                single_path(fb, a, clock)
            seq.append(clock[0] * 1e3)
            py.append(clock[1] * 1e3)
        kern = profile_kernels(lambda: (batch(), torch.cuda.synchronize()))
        b_ms, s_ms = statistics.median(times), statistics.median(seq)
        line = {"metric": "IPA audits/s with proofs, %d audits of %d challenged rows per batched call (2^%d-block level, device-resident)" % (k, m, args.log2blocks),
                "value": round(k * 1e3 / b_ms, 1), "unit": "audits/s", "n_gpus": 1, "steps": args.reps, "warmup": warm,
                "audits": k, "points": m, "batch_ms": round(b_ms, 4), "batch_ms_min": round(min(times), 4), "batch_ms_max": round(max(times), 4),
                "sequential_ms": round(s_ms, 3), "sequential_ms_min": round(min(seq), 3), "sequential_ms_max": round(max(seq), 3),
                "sequential_audits_per_s": round(k * 1e3 / s_ms, 1), "host_python_ms": round(statistics.median(py), 3),
                "speedup": round(s_ms / b_ms, 2), "table": fb.info(), "bit_exact": got == want and got_b == want_b, "kernels_ms": kern}
        print(json.dumps(line), flush=True)
        lines.append(json.dumps(line))
        del d_idx, d_coef, d_out, d_b
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
