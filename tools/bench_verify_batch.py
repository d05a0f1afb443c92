#!/usr/bin/env python3
"""bench_verify_batch.py -- the client's check of many KZG audit replies per call (porla_kzg_verify_batch_device) against the same
replies checked one at a time through the reference's 14-symbol sequence (Client.hpp:685-869: compute_multi_exp over the challenged
complements, mult_point by alpha twice, add_point twice, compare_commitment, verify_proof).

Setup: 2^15 random blocks -> per-block commitments -> data encode and MAC encode (as tools/bench_audit_batch.py); the client's
complements comp_i = s_i h_MAC (porla_kzg_complement_batch_device) and the honest MAC store M'_i = alpha M_i + comp_i (the batched MSM,
2-pair entries); a fresh level (alignment store at infinity).  For each K every reply has its own linked challenge of --points rows
and its own z; the server batch (porla_kzg_audit_batch_device) writes the K replies into HBM, where the verifier reads them.

Prints ONE JSON line per K in bench.py's format: value = replies/s through the batch (K / median wall time of the blocking call);
`sequential_audits_per_s` = the same K replies through the 14 symbols, one after another (host arrays prepared outside the clock);
`speedup`; `device_ms` = the sum of `kernels_ms`, the time per kernel of one profiled batch call (porla_gpu_profile_*); `pairing_ms`
= one host pairing check (porla_bn254_pairing_product_is_one, the folded check's cost); `statuses_equal` = every status byte equals
the reference sequence's verdicts."""
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
ALPHA32 = bytes(16) + ALPHA                                  # Client.hpp:851-853
R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
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
    ap.add_argument("--log2blocks", type=int, default=15)
    ap.add_argument("--points", type=int, default=3200)
    ap.add_argument("--out")
    args = ap.parse_args()

    import numpy as np
    import torch
    from porla_amd import icc, lib, multiexp as mx

    assert torch.cuda.is_available(), "bench_verify_batch.py needs a GPU (the engine has no CPU path)"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    cs = torch.cuda.current_stream()
    stream = cs.cuda_stream
    n, m = 1 << args.log2blocks, args.points
    mx.init_key(TAU, ALPHA)
    mx.init_SRS_from_data(NCOLS, mx.init_SRS(NCOLS))
    g = torch.Generator(device=dev).manual_seed(78)
    d_blocks = torch.randint(0, 256, (n * NCOLS, 32), dtype=torch.uint8, device=dev, generator=g)
    d_coeffs_be = d_blocks.flip(1).contiguous()
    d_macs_u = torch.empty(64 * n, dtype=torch.uint8, device=dev)
    mx.kzg_commit_batch_device(d_coeffs_be.data_ptr(), n, d_macs_u.data_ptr(), stream)
    d_x = torch.empty(64 * n * NCOLS, dtype=torch.uint8, device=dev)
    icc.crebuild_device(d_blocks.data_ptr(), n, NCOLS, "bn254", 0, 0, d_x.data_ptr(), 0, 0, stream=stream)
    d_macs = torch.empty(64 * n, dtype=torch.uint8, device=dev)
    icc.mac_crebuild_device(d_macs_u.data_ptr(), n, "bn254", 0, 0, d_macs.data_ptr(), stream)
    rng = np.random.Generator(np.random.PCG64(10))
    s = b"".join(int(v).to_bytes(32, "big") for v in rng.integers(1, 1 << 62, n, dtype=np.int64))
    d_s = torch.frombuffer(bytearray(s), dtype=torch.uint8).to(dev)
    d_comp = torch.empty(64 * n, dtype=torch.uint8, device=dev)
    mx.kzg_complement_batch_device(d_s.data_ptr(), n, d_comp.data_ptr(), stream)
    sc = torch.frombuffer(bytearray((ALPHA32 + (1).to_bytes(32, "big")) * n), dtype=torch.uint8).to(dev)
    pt = torch.stack([d_macs.view(n, 64), d_comp.view(n, 64)], 1).contiguous().view(-1)
    d_macs_a = torch.empty(64 * n, dtype=torch.uint8, device=dev)
    mx.msm_batch_device("bn254", sc.data_ptr(), pt.data_ptr(), mx.batch_offsets([2] * n), d_macs_a.data_ptr(), stream)
    d_zero = torch.zeros(64 * n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    comp_host = bytes(d_comp.cpu().numpy())
    del d_coeffs_be, d_blocks, d_macs_u, sc, pt, d_s

    lines = []
    for k in [int(x) for x in args.ks.split(",")]:
        idx = rng.integers(0, n, (k, m), dtype=np.int64)
        coef = rng.integers(0, 1 << 31, (k, m), dtype=np.int64).astype(np.uint32)
        d_idx = torch.from_numpy(idx).cuda()
        d_coef = torch.from_numpy(coef.view(np.int32)).cuda()
        zs = [int(v) for v in rng.integers(0, 1 << 63, k, dtype=np.int64)]
        audits = [(d_x.data_ptr(), d_idx[a].data_ptr(), d_coef[a].data_ptr(), m, 0, 0, 0, 0, d_macs_a.data_ptr(), d_zero.data_ptr(),
                   d_idx[a].data_ptr(), d_coef[a].data_ptr(), m, zs[a]) for a in range(k)]
        verifs = [(d_comp.data_ptr(), d_idx[a].data_ptr(), d_coef[a].data_ptr(), m, ALPHA) for a in range(k)]
        d_rec = torch.zeros(REC * k, dtype=torch.uint8, device=dev)
        mx.kzg_audit_batch_device(audits, d_rec.data_ptr(), None, stream)
        torch.cuda.synchronize()
        recs = bytes(d_rec.cpu().numpy())

        def batch():
            return mx.kzg_verify_batch_device(verifs, d_rec.data_ptr(), stream=stream)

        for _ in range(3):
            got = batch()
        times = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            batch()
            times.append((time.perf_counter() - t0) * 1e3)
        # the reference sequence: the client's arrays prepared outside the clock, then the 14 symbols per reply
        pts = [b"".join(comp_host[64 * int(i):64 * int(i) + 64] for i in idx[a]) for a in range(k)]
        scs = [b"".join(bytes(28) + int(c).to_bytes(4, "big") for c in coef[a]) for a in range(k)]

        def sequential():
            st = []
            for a in range(k):
                r = recs[REC * a:REC * (a + 1)]
                comp = mx.bn254_multi_exp(pts[a], scs[a], m)
                c = mx.bn254_add(mx.bn254_mult(r[0:64], ALPHA32), comp)
                mac = mx.bn254_add(r[192:256], mx.bn254_mult(r[256:320], ALPHA32))
                full = mx.bn254_compare(c, mac)
                proof = mx.verify_proof(r[0:64], r[64:128], r[128:160], r[160:192])
                st.append((mx.KZG_VERIFY_FULL if full else 0) | (mx.KZG_VERIFY_PROOF if proof else 0))
            return st

        want = sequential()                                  # warm-up + the reference verdicts
        t0 = time.perf_counter()
        sequential()
        s_ms = (time.perf_counter() - t0) * 1e3
        kern = profile_kernels(batch)
        g2 = [ctypes.create_string_buffer(128) for _ in range(2)]
        lib.porla_bn254_g2_mul_generator((1).to_bytes(32, "big"), g2[0])
        lib.porla_bn254_g2_mul_generator((12345).to_bytes(32, "big"), g2[1])
        pair_t = []
        for _ in range(10):
            t0 = time.perf_counter()
            lib.porla_bn254_pairing_product_is_one(recs[0:64], g2[0], recs[64:128], g2[1], 0)
            pair_t.append((time.perf_counter() - t0) * 1e3)
        b_ms = statistics.median(times)
        line = {"metric": "KZG audit replies/s, %d replies of %d challenged complements per batched check (2^%d-block level, device-resident)" % (k, m, args.log2blocks),
                "value": round(k * 1e3 / b_ms, 1), "unit": "audits/s", "n_gpus": 1, "steps": args.reps, "warmup": 3,
                "audits": k, "points": m, "batch_ms": round(b_ms, 4), "batch_ms_min": round(min(times), 4),
                "sequential_ms": round(s_ms, 3), "sequential_audits_per_s": round(k * 1e3 / s_ms, 1), "speedup": round(s_ms / b_ms, 2),
                "statuses_equal": got == want, "all_pass": all(v == mx.KZG_VERIFY_PASS for v in got),
                "device_ms": round(sum(kern.values()), 4), "pairing_ms": round(statistics.median(pair_t), 4), "kernels_ms": kern}
        print(json.dumps(line), flush=True)
        lines.append(json.dumps(line))
        del d_idx, d_coef, d_rec
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
