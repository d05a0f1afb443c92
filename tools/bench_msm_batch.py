#!/usr/bin/env python3
"""Batched MSM against the same entries as sequential single calls (include/porla_gpu.h: porla_*_msm_batch_device vs
porla_*_msm_device), one JSON line per shape:

  batch_ms       one batch call, HIP events around it, after warm-up: median of --reps (>= 20)
  seq_ms         the K entries as K porla_*_msm_device calls one after the other (each returns its result to the host): median of
                 --seq-reps whole loops
  speedup        seq_ms / batch_ms
  bit_exact      the K outputs of the batch equal the K single calls' byte for byte
  kernels_ms     per new kernel (porla_gpu_profile_get, one profiled batch call): where the batch's time goes

Shapes (--shapes, default all):
  audit64    BN254, 64 entries x 3 200 pairs, abs(int32) coefficients over 64-way repeated points (64 audits)
  full1024   BN254, 1 024 entries x 128 pairs, full 256-bit scalars
  ecmult1    secp256k1, 32 842 one-pair entries x G with the keys of the reference's ecmult constants test (tests.c:4738-4751)
  max8       BN254, 8 entries x 32 768 pairs (the largest entries allowed)

  --sweep N1,N2,..  instead: BN254 batches of 256 entries x N pairs (256-bit scalars), batch time only -- the cost on both sides of
                    the tiny / bucket crossover (entries of <= 64 pairs run in k_batch_tiny, larger ones in k_batch_bucket)

  python tools/bench_msm_batch.py [--shapes a,b] [--reps 20] [--seq-reps 3] [--sweep 8,16,17,32] [--out FILE]"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def shape_inputs(name):
    from tests import common
    rnd = random.Random(0x5EED)
    be = lambda x: (x % (1 << 256)).to_bytes(32, "big")
    if name == "audit64":
        k, n = 64, 3200
        base = common.synth_points(n)
        sc = b"".join(be(abs(rnd.randrange(-(1 << 31), 1 << 31))) for _ in range(k * n))
        return "bn254", sc, base * k, [n * i for i in range(k + 1)]
    if name == "full1024":
        k, n = 1024, 128
        pts = common.synth_points(k * n)
        sc = b"".join(be(rnd.getrandbits(256)) for _ in range(k * n))
        return "bn254", sc, pts, [n * i for i in range(k + 1)]
    if name == "ecmult1":
        from tests.test_reference_kats_gpu import G, b32, constants_keys
        keys = constants_keys()
        return "secp256k1", b"".join(b32(x) for x in keys), G * len(keys), list(range(len(keys) + 1))
    if name == "max8":
        k, n = 8, 32768
        pts = common.synth_points(n)
        sc = b"".join(be(rnd.getrandbits(256)) for _ in range(k * n))
        return "bn254", sc, pts * k, [n * i for i in range(k + 1)]
    raise SystemExit("unknown shape %s" % name)


def sweep_line(mx, n, reps, k=256):
    import torch
    from tests import common
    rnd = random.Random(n)
    sc = b"".join(rnd.getrandbits(256).to_bytes(32, "big") for _ in range(k * n))
    pts = common.synth_points(k * n)
    offsets = [n * i for i in range(k + 1)]
    d_sc = torch.frombuffer(bytearray(sc), dtype=torch.uint8).cuda()
    d_pt = torch.frombuffer(bytearray(pts), dtype=torch.uint8).cuda()
    d_out = torch.zeros(64 * k, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream()
    torch.cuda.synchronize()
    times = []
    for i in range(reps + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        mx.msm_batch_device("bn254", d_sc.data_ptr(), d_pt.data_ptr(), offsets, d_out.data_ptr(), stream.cuda_stream)
        e1.record(stream)
        e1.synchronize()
        if i >= 3:
            times.append(e0.elapsed_time(e1))
    return {"sweep": "bn254", "entries": k, "pairs_per_entry": n, "path": "tiny" if n <= 64 else "bucket",
            "batch_ms": round(statistics.median(times), 4), "us_per_entry": round(statistics.median(times) * 1e3 / k, 3)}


def profile_kernels(mx, fn):
    from porla_amd import lib
    import ctypes
    lib.porla_gpu_profile_enable(1)
    fn()
    out = {}
    name = ctypes.create_string_buffer(64)
    ms, n = ctypes.c_double(), ctypes.c_longlong()
    slot = 0
    while lib.porla_gpu_profile_get(slot, name, 64, ctypes.byref(ms), ctypes.byref(n)) == 0:
        if name.value.decode().startswith("batch_"):
            out[name.value.decode()] = round(ms.value, 4)
        slot += 1
    lib.porla_gpu_profile_enable(0)
    return out


def run_shape(mx, name, reps, seq_reps):
    import torch
    curve, sc, pts, offsets = shape_inputs(name)
    k = len(offsets) - 1
    d_sc = torch.frombuffer(bytearray(sc), dtype=torch.uint8).cuda()
    d_pt = torch.frombuffer(bytearray(pts), dtype=torch.uint8).cuda()
    d_out = torch.zeros(64 * k, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    torch.cuda.synchronize()

    def batch():
        mx.msm_batch_device(curve, d_sc.data_ptr(), d_pt.data_ptr(), offsets, d_out.data_ptr(), s)

    for _ in range(3):
        batch()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        batch()
        e1.record(stream)
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    got = bytes(d_out.cpu().numpy().tobytes())

    def sequential():
        return [mx.msm_device(curve, d_sc.data_ptr() + 32 * offsets[i], d_pt.data_ptr() + 64 * offsets[i], offsets[i + 1] - offsets[i], s)
                for i in range(k)]

    want = sequential()                                  # warm-up + the reference outputs
    seq = []
    for _ in range(seq_reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(stream)
        sequential()
        e1.record(stream)
        e1.synchronize()
        seq.append(max(e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3))
    kern = profile_kernels(mx, lambda: (batch(), torch.cuda.synchronize()))
    b_ms, s_ms = statistics.median(times), statistics.median(seq)
    return {"shape": name, "curve": curve, "entries": k, "pairs": offsets[-1], "batch_ms": round(b_ms, 4),
            "batch_ms_min": round(min(times), 4), "batch_reps": reps, "seq_ms": round(s_ms, 3), "seq_reps": seq_reps,
            "speedup": round(s_ms / b_ms, 2), "bit_exact": got == b"".join(want), "kernels_ms": kern}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="audit64,full1024,ecmult1,max8")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seq-reps", type=int, default=3)
    ap.add_argument("--sweep")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    from porla_amd import multiexp as mx
    lines = []
    jobs = [("sweep", int(x)) for x in a.sweep.split(",")] if a.sweep else [("shape", x) for x in a.shapes.split(",")]
    for kind, arg in jobs:
        if kind == "sweep":
            line = json.dumps(sweep_line(mx, arg, max(a.reps, 20)))
        else:
            line = json.dumps(run_shape(mx, arg, max(a.reps, 20), max(a.seq_reps, 1)))
        print(line, flush=True)
        lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
