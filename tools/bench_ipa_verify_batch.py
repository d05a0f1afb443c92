#!/usr/bin/env python3
"""bench_ipa_verify_batch.py -- the client's check of many IPA audit replies per call (porla_ipa_verify_batch_device) against what
the library offered before it: per reply two blocking porla_secp256k1_msm_device calls, one over the challenged complements with
the MAC check's three pairs behind them, one over the 142 pairs of the proof equation, the scalars (transcript, inversions,
x_values, decompressed points) prepared on the host beforehand and only the engine calls timed -- the convention of
profiles/r09_a_ipa_audit_batch.jsonl.

Setup: 2^--log2blocks random blocks -> per-block commitments on the generators -> data encode and MAC encode; complements
comp_i = s_i G_0 and the honest MAC store M'_i = alpha M_i + comp_i (the batched MSM, 2-pair entries); a fresh level (alignment
store at infinity).  For each K every reply has its own linked challenge of --points rows and its own a_value; the server batch
(porla_ipa_audit_batch_device) writes the K records into HBM, where the verifier reads them.

Prints ONE JSON line per K in bench.py's format: value = replies/s through the batch (K / median time of the call, the larger of
the stream's event time and the host's wall time); `sequential_replies_per_s` = the same K replies through the 2 K blocking MSM
calls; `speedup`; `kernels_ms` = the time per kernel of one profiled batch call (porla_gpu_profile_*); `statuses_ok` = every status
byte of the batch is FULL | PROOF | BVEC and every sequential MSM sums to infinity."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ALPHA = bytes.fromhex("00112233445566778899aabbccddeeff")   # SECRET_KEY, config.hpp:38
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


def proof_pairs(ipa, ipv, points, rec):
    """the 142 pairs of one reply's proof equation, summing to infinity iff Client::inner_product_verify accepts:
    (1, C), (x_r^2, L_r), (x_r^-2, R_r), (-a_(j & 1) x_values[j], G_j), (c - a0 b0 - a1 b1, u)"""
    n = ipa.N
    proof = rec[99:]
    xs = ipv.challenges(proof)
    xv = ipv.x_values(xs)
    le = lambda at: int.from_bytes(proof[at:at + 32], "little") % n
    tail = 32 + 6 * 66
    c, a0, b0, a1, b1 = le(0), le(tail), le(tail + 32), le(tail + 64), le(tail + 96)
    pairs = [(1, ipa.decompress(rec[:33]))]
    for r, x in enumerate(xs):
        x2 = x * x % n
        pairs.append((x2, ipa.decompress(proof[32 + 66 * r:65 + 66 * r])))
        pairs.append((ipa.inv(x2), ipa.decompress(proof[65 + 66 * r:98 + 66 * r])))
    for j in range(NCOLS):
        pairs.append(((n - (a1 if j & 1 else a0) * xv[j]) % n, points[j]))
    pairs.append(((c - a0 * b0 - a1 * b1) % n, points[NCOLS]))
    return b"".join(s.to_bytes(32, "big") for s, _ in pairs), b"".join(p for _, p in pairs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,8,64,256")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seq-reps", type=int, default=3)
    ap.add_argument("--log2blocks", type=int, default=15)
    ap.add_argument("--points", type=int, default=3200)
    ap.add_argument("--window", type=int, default=0, help="window bits of the 129-point table (0: PORLA_COMMIT_TABLE_GB / PORLA_COMMIT_WINDOW)")
    ap.add_argument("--out")
    args = ap.parse_args()

    import numpy as np
    import torch
    from porla_amd import icc, multiexp as mx
    from tests import common
    from tests import ipa_proof_py as ipa
    from tests import ipa_verify_py as ipv

    assert torch.cuda.is_available(), "bench_ipa_verify_batch.py needs a GPU (the engine has no CPU path)"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    cs = torch.cuda.current_stream()
    stream = cs.cuda_stream
    n, m = 1 << args.log2blocks, args.points
    gens_u = common.secp_bench_points(NCOLS + 1)
    points = ipa.split_points(gens_u, NCOLS + 1)
    fb = mx.FixedBase("secp256k1", gens_u, NCOLS + 1, args.window)
    g = torch.Generator(device=dev).manual_seed(79)
    d_blocks = torch.randint(0, 256, (n * NCOLS, 32), dtype=torch.uint8, device=dev, generator=g)
    d_coeffs_be = d_blocks.flip(1).contiguous()
    d_macs_u = torch.empty(64 * n, dtype=torch.uint8, device=dev)
    fb.commit_device(d_coeffs_be.data_ptr(), n, NCOLS, d_macs_u.data_ptr(), stream)
    d_x = torch.empty(64 * n * NCOLS, dtype=torch.uint8, device=dev)
    icc.crebuild_device(d_blocks.data_ptr(), n, NCOLS, "secp256k1", 0, 0, d_x.data_ptr(), 0, 0, stream=stream)
    d_macs = torch.empty(64 * n, dtype=torch.uint8, device=dev)
    icc.mac_crebuild_device(d_macs_u.data_ptr(), n, "secp256k1", 0, 0, d_macs.data_ptr(), stream)
    d_s = torch.randint(0, 256, (32 * n,), dtype=torch.uint8, device=dev, generator=g)
    d_comp = torch.empty(64 * n, dtype=torch.uint8, device=dev)
    fb.commit_device(d_s.data_ptr(), n, 1, d_comp.data_ptr(), stream)              # comp_i = s_i G_0
    sc = torch.frombuffer(bytearray((bytes(16) + ALPHA + (1).to_bytes(32, "big")) * n), dtype=torch.uint8).to(dev)
    pt = torch.stack([d_macs.view(n, 64), d_comp.view(n, 64)], 1).contiguous().view(-1)
    d_macs_a = torch.empty(64 * n, dtype=torch.uint8, device=dev)
    mx.msm_batch_device("secp256k1", sc.data_ptr(), pt.data_ptr(), mx.batch_offsets([2] * n), d_macs_a.data_ptr(), stream)
    d_zero = torch.zeros(64 * n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    del d_coeffs_be, d_blocks, d_macs_u, sc, pt, d_s

    rng = np.random.Generator(np.random.PCG64(11))
    alpha_i = int.from_bytes(ALPHA, "big")
    lines = []
    for k in [int(x) for x in args.ks.split(",")]:
        idx = rng.integers(0, n, (k, m), dtype=np.int64)
        coef = rng.integers(0, 1 << 31, (k, m), dtype=np.int64).astype(np.uint32)
        d_idx = torch.from_numpy(idx).cuda()
        d_coef = torch.from_numpy(coef.view(np.int32)).cuda()
        vs = [int.from_bytes(rng.bytes(32), "big") for _ in range(k)]
        audits = [(d_x.data_ptr(), d_idx[a].data_ptr(), d_coef[a].data_ptr(), m, 0, 0, 0, 0, d_macs_a.data_ptr(), d_zero.data_ptr(),
                   d_idx[a].data_ptr(), d_coef[a].data_ptr(), m, vs[a]) for a in range(k)]
        verifs = [(d_comp.data_ptr(), d_idx[a].data_ptr(), d_coef[a].data_ptr(), m, ALPHA, vs[a]) for a in range(k)]
        d_rec = torch.zeros(REC * k, dtype=torch.uint8, device=dev)
        d_status = torch.zeros(k, dtype=torch.uint8, device=dev)
        fb.ipa_audit_batch_device(audits, d_rec.data_ptr(), None, stream)
        torch.cuda.synchronize()
        recs = bytes(d_rec.cpu().numpy())

        def batch():
            fb.ipa_verify_batch_device(verifs, d_rec.data_ptr(), d_status=d_status.data_ptr(), stream=stream)

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
        got = list(bytes(d_status.cpu().numpy()))

        # what the library offered before: the pairs of both equations prepared beforehand, two blocking MSM calls per reply
        seq_in = []
        for a in range(k):
            r = recs[REC * a:REC * (a + 1)]
            c_pt, m_pt, a_pt = (ipa.decompress(r[33 * i:33 * i + 33]) for i in range(3))
            sc1 = np.zeros((m, 32), dtype=np.uint8)
            sc1[:, 28:] = coef[a].astype(">u4").view(np.uint8).reshape(m, 4)
            tail_sc = b"".join(v.to_bytes(32, "big") for v in (alpha_i, ipa.N - alpha_i, ipa.N - 1))
            d_sc1 = torch.cat([torch.from_numpy(sc1).view(-1), torch.frombuffer(bytearray(tail_sc), dtype=torch.uint8)]).cuda()
            d_pt1 = torch.cat([d_comp.view(n, 64)[d_idx[a]].view(-1),
                               torch.frombuffer(bytearray(c_pt + a_pt + m_pt), dtype=torch.uint8).cuda()])
            sc2, pt2 = proof_pairs(ipa, ipv, points, r)
            seq_in.append((d_sc1, d_pt1, torch.frombuffer(bytearray(sc2), dtype=torch.uint8).cuda(),
                           torch.frombuffer(bytearray(pt2), dtype=torch.uint8).cuda()))
        torch.cuda.synchronize()

        def sequential():
            ok = True
            for d_sc1, d_pt1, d_sc2, d_pt2 in seq_in:
                ok &= mx.msm_device("secp256k1", d_sc1.data_ptr(), d_pt1.data_ptr(), m + 3, stream) == bytes(64)
                ok &= mx.msm_device("secp256k1", d_sc2.data_ptr(), d_pt2.data_ptr(), 142, stream) == bytes(64)
            return ok

        seq_ok = sequential()                                # warm-up + the verdicts
        seq = []
        for _ in range(args.seq_reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sequential()
            seq.append((time.perf_counter() - t0) * 1e3)
        kern = profile_kernels(lambda: (batch(), torch.cuda.synchronize()))
        b_ms, s_ms = statistics.median(times), statistics.median(seq)
        line = {"metric": "IPA audit replies/s, %d replies of %d challenged complements per batched check (2^%d-block level, device-resident)" % (k, m, args.log2blocks),
                "value": round(k * 1e3 / b_ms, 1), "unit": "audits/s", "n_gpus": 1, "steps": args.reps, "warmup": warm,
                "audits": k, "points": m, "batch_ms": round(b_ms, 4), "batch_ms_min": round(min(times), 4), "batch_ms_max": round(max(times), 4),
                "sequential_ms": round(s_ms, 3), "sequential_ms_min": round(min(seq), 3), "sequential_ms_max": round(max(seq), 3),
                "sequential_replies_per_s": round(k * 1e3 / s_ms, 1), "speedup": round(s_ms / b_ms, 2), "table": fb.info(),
                "statuses_ok": bool(got == [mx.IPA_VERIFY_PASS_BOUND] * k and seq_ok), "device": torch.cuda.get_device_name(0),
                "device_ms": round(sum(kern.values()), 4), "kernels_ms": kern}
        print(json.dumps(line), flush=True)
        lines.append(json.dumps(line))
        del d_idx, d_coef, d_rec, seq_in
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
