#!/usr/bin/env python3
"""The ICC MAC decode (porla_icc_mac_decode_batch_device) beside the encode it inverts, same rows, same run.

For (K, n_rows) in {(1, 2^15), (8, 2^15), (64, 2^10)}, per curve:
  encode   K porla_icc_mac_encode_device calls (part 0), one after the other on one stream: MAC_a -> X_a
  decode   ONE porla_icc_mac_decode_batch_device call for the K levels: X_a -> MACs
The inputs are s_i G for random s_i, made on the device by a one-point fixed-base commit.  Both are timed with device events around
the calls on a stream of their own, alternating, `--reps` times each after a warm-up; the medians are reported.  Every output byte of
the decode is compared with the encode's input.  The encode is the yardstick: the decode runs its ladder count plus one scalar
multiplication per row at the close (expected about 1 + 2 / log2 n_rows of the encode's time, an estimate, no gate).  One JSON line
per (curve, K, n_rows).

    python tools/bench_icc_mac_decode.py [--out profiles/r20_a_mac_decode.jsonl] [--reps 7] [--shapes 15:1,15:8,10:64]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GEN = {"bn254": (1, 2),
       "secp256k1": (0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798,
                     0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8)}


def event_ms(stream, fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="15:1,15:8,10:64")
    ap.add_argument("--curves", default="bn254,secp256k1")
    args = ap.parse_args()
    import torch
    from porla_amd import icc
    from porla_amd import multiexp as mx
    assert torch.cuda.is_available(), "bench_icc_mac_decode.py needs a GPU"
    out = open(args.out, "w") if args.out else None
    stream = torch.cuda.Stream()
    for curve in args.curves.split(","):
        g = GEN[curve]
        fb = mx.FixedBase(curve, g[0].to_bytes(32, "big") + g[1].to_bytes(32, "big"), 1, window_bits=8)
        for shape in args.shapes.split(","):
            log, k = (int(x) for x in shape.split(":"))
            n = 1 << log
            gen = torch.Generator(device="cuda")
            gen.manual_seed(1000 * k + log)
            macs = []
            for _ in range(k):
                sc = torch.randint(0, 256, (n * 32,), dtype=torch.uint8, device="cuda", generator=gen)
                m = torch.empty(n * 64, dtype=torch.uint8, device="cuda")
                fb.commit_device(sc.data_ptr(), n, 1, m.data_ptr())
                macs.append(m)
            x = [torch.empty(n * 64, dtype=torch.uint8, device="cuda") for _ in range(k)]
            back = [torch.full((n * 64,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(k)]
            reqs = [(x[a].data_ptr(), back[a].data_ptr(), 0, 0) for a in range(k)]
            torch.cuda.synchronize()

            def encode():
                for a in range(k):
                    icc.mac_crebuild_device(macs[a].data_ptr(), n, curve, 0, 0, x[a].data_ptr(), stream.cuda_stream)

            def decode():
                icc.mac_decode_batch_device(reqs, n, n, curve, stream.cuda_stream)

            encode()                                                              # tables, workspaces
            decode()
            stream.synchronize()
            t_enc, t_dec = [], []
            for _ in range(args.reps):
                t_enc.append(event_ms(stream, encode))
                t_dec.append(event_ms(stream, decode))
            stream.synchronize()
            for a in range(k):
                assert torch.equal(back[a], macs[a]), "request %d: the decode is not the encode's input" % a
            enc, dec = statistics.median(t_enc), statistics.median(t_dec)
            rec = {"curve": curve, "k": k, "n_rows": n, "reps": args.reps, "mac_decode_ms": round(dec, 4),
                   "mac_encode_ms": round(enc, 4), "decode_over_encode": round(dec / enc, 3),
                   "estimate": round(1 + 2 / log, 3),
                   "decode_ms_min_max": [round(min(t_dec), 4), round(max(t_dec), 4)],
                   "encode_ms_min_max": [round(min(t_enc), 4), round(max(t_enc), 4)], "outputs_checked": True}
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
            del macs, x, back
        fb.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
