#!/usr/bin/env python3
"""bench_audit_batch.py -- many KZG audits per call (porla_kzg_audit_batch_device) against the same audits one call at a time
(porla_kzg_audit_device), server side, the level and its MAC arrays resident in HBM.

Setup = the protocol pipeline of tools/bench_audit_flow.py: 2^15 random blocks -> per-block commitments -> data encode (64-byte code
symbols) and MAC encode; a rotated copy of the MAC array is the alignment store, so that both MSMs of every audit do real work.  For
each K every audit has its own challenge (--points rows, abs(int32) coefficients) and its own z.

Prints ONE JSON line per K in bench.py's format: value = audits/s through the batch (K / median batch time, CUDA events around the
call); `sequential_audits_per_s` = the same K audits as K sequential porla_kzg_audit_device calls; `speedup`; `kernels_ms` = time per
kernel of one profiled batch call (porla_gpu_profile_*); `bit_exact` = every record equals the single call's reply (combined_align
after align_MAC) and every B the single call's."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TAU = bytes.fromhex("ffeeddccbbaa99887766554433221100")     # TAU_KEY, config.hpp:39
ALPHA = bytes.fromhex("00112233445566778899aabbccddeeff")   # SECRET_KEY, config.hpp:38
NCOLS = 128
REC = 320


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,8,64,256")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seq-reps", type=int, default=3)
    ap.add_argument("--log2blocks", type=int, default=15)
    ap.add_argument("--points", type=int, default=3200)
    ap.add_argument("--out")
    args = ap.parse_args()

    import numpy as np
    import torch
    from porla_amd import icc, multiexp as mx

    assert torch.cuda.is_available(), "bench_audit_batch.py needs a GPU (the engine has no CPU path)"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    cs = torch.cuda.current_stream()
    stream = cs.cuda_stream
    n, m = 1 << args.log2blocks, args.points
    mx.init_key(TAU, ALPHA)
    mx.init_SRS_from_data(NCOLS, mx.init_SRS(NCOLS))
    g = torch.Generator(device=dev).manual_seed(77)
    d_blocks = torch.randint(0, 256, (n * NCOLS, 32), dtype=torch.uint8, device=dev, generator=g)
    d_coeffs_be = d_blocks.flip(1).contiguous()
    d_macs_u = torch.empty(64 * n, dtype=torch.uint8, device=dev)
    mx.kzg_commit_batch_device(d_coeffs_be.data_ptr(), n, d_macs_u.data_ptr(), stream)
    d_x = torch.empty(64 * n * NCOLS, dtype=torch.uint8, device=dev)
    icc.crebuild_device(d_blocks.data_ptr(), n, NCOLS, "bn254", 0, 0, d_x.data_ptr(), 0, 0, stream=stream)
    d_macs = torch.empty(64 * n, dtype=torch.uint8, device=dev)
    icc.mac_crebuild_device(d_macs_u.data_ptr(), n, "bn254", 0, 0, d_macs.data_ptr(), stream)
    torch.cuda.synchronize()
    del d_coeffs_be, d_blocks
    d_align = torch.roll(d_macs.view(n, 64), 1, 0).contiguous().view(-1)

    rng = np.random.Generator(np.random.PCG64(9))
    lines = []
    for k in [int(x) for x in args.ks.split(",")]:
        d_idx = torch.from_numpy(rng.integers(0, n, (k, m), dtype=np.int64)).cuda()
        d_coef = torch.from_numpy(rng.integers(0, 1 << 31, (k, m), dtype=np.int64).astype(np.uint32).view(np.int32)).cuda()
        zs = [int(v) for v in rng.integers(0, 1 << 63, k, dtype=np.int64)]
        audits = [(d_x.data_ptr(), d_idx[a].data_ptr(), d_coef[a].data_ptr(), m, 0, 0, 0, 0, d_macs.data_ptr(), d_align.data_ptr(),
                   d_idx[a].data_ptr(), d_coef[a].data_ptr(), m, zs[a]) for a in range(k)]
        d_out = torch.zeros(REC * k, dtype=torch.uint8, device=dev)
        d_b = torch.zeros(32 * NCOLS * k, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()

        def batch():
            mx.kzg_audit_batch_device(audits, d_out.data_ptr(), d_b.data_ptr(), stream)

        for _ in range(3):
            batch()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(cs)
            batch()
            e1.record(cs)
            e1.synchronize()
            times.append(max(e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3))
        got, got_b = bytes(d_out.cpu().numpy()), bytes(d_b.cpu().numpy())

        def sequential():
            return [mx.kzg_audit_device(*a, stream=stream) for a in audits]

        ones = sequential()                                  # warm-up + the reference replies
        want = b"".join(o["commitment"] + o["proof_h"] + o["point"] + o["claim"] + o["combined_mac"] +
                        mx.bn254_add(o["combined_align"], o["align_value"]) for o in ones)
        want_b = b"".join(o["b"] for o in ones)
        seq = []
        for _ in range(args.seq_reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sequential()
            torch.cuda.synchronize()
            seq.append((time.perf_counter() - t0) * 1e3)
        kern = profile_kernels(lambda: (batch(), torch.cuda.synchronize()))
        b_ms, s_ms = statistics.median(times), statistics.median(seq)
        line = {"metric": "KZG audits/s, %d audits of %d challenged rows per batched call (2^%d-block level, device-resident)" % (k, m, args.log2blocks),
                "value": round(k * 1e3 / b_ms, 1), "unit": "audits/s", "n_gpus": 1, "steps": args.reps, "warmup": 3,
                "audits": k, "points": m, "batch_ms": round(b_ms, 4), "batch_ms_min": round(min(times), 4),
                "sequential_ms": round(s_ms, 3), "sequential_audits_per_s": round(k * 1e3 / s_ms, 1), "speedup": round(s_ms / b_ms, 2),
                "bit_exact": got == want and got_b == want_b, "kernels_ms": kern}
        print(json.dumps(line), flush=True)
        lines.append(json.dumps(line))
        del d_idx, d_coef, d_out, d_b
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
