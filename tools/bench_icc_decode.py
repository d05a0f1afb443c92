#!/usr/bin/env python3
"""The EXACT ICC decode (porla_icc_decode_batch_device) beside the encode it inverts, same rows, same run.

For (K, n_rows) in {(1, 2^15), (8, 2^15), (64, 2^10)} x 128 columns, per curve:
  encode   K porla_icc_encode_device calls (part 0, the 64-byte X rows only), one after the other on one stream: U_a -> X_a
  decode   ONE porla_icc_decode_batch_device call for the K levels: X_a -> blocks, with a counter per request
Both are timed with device events around the calls on a stream of their own, alternating, `--reps` times each after a warm-up; the
medians are reported.  Every output byte of the decode is compared with the encode's input and every counter must be 0.  The encode
is the yardstick: the decode runs its butterfly count with one short reduction more per butterfly, reads 64 bytes per symbol and
writes 32 where the encode does the opposite.  One JSON line per (curve, K, n_rows).

One run on one MI355X (profiles/r17_a_icc_decode.jsonl), decode ms / K encodes ms / ratio:
  bn254      K = 1, 2^15: 0.951 / 0.675 / 1.41    K = 8, 2^15: 6.43 / 4.88 / 1.32    K = 64, 2^10: 1.29 / 3.26 / 0.40
  secp256k1  K = 1, 2^15: 0.898 / 0.650 / 1.38    K = 8, 2^15: 6.46 / 4.88 / 1.32    K = 64, 2^10: 1.25 / 3.24 / 0.39

    python tools/bench_icc_decode.py [--out profiles/r17_a_icc_decode.jsonl] [--reps 9] [--shapes 15:1,15:8,10:64]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NCOLS = 128


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
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--shapes", default="15:1,15:8,10:64")
    ap.add_argument("--curves", default="bn254,secp256k1")
    args = ap.parse_args()
    import torch
    from porla_amd import icc
    assert torch.cuda.is_available(), "bench_icc_decode.py needs a GPU"
    out = open(args.out, "w") if args.out else None
    stream = torch.cuda.Stream()
    for curve in args.curves.split(","):
        for shape in args.shapes.split(","):
            log, k = (int(x) for x in shape.split(":"))
            n = 1 << log
            gen = torch.Generator(device="cuda")
            gen.manual_seed(1000 * k + log)
            u = [torch.randint(0, 256, (n * NCOLS * 32,), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(k)]
            x = [torch.empty(n * NCOLS * 64, dtype=torch.uint8, device="cuda") for _ in range(k)]
            back = [torch.full((n * NCOLS * 32,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(k)]
            bad = torch.full((k,), -1, dtype=torch.int32, device="cuda")
            reqs = [(x[a].data_ptr(), back[a].data_ptr(), 0, bad[a:].data_ptr()) for a in range(k)]
            torch.cuda.synchronize()

            def encode():
                for a in range(k):
                    icc.crebuild_device(u[a].data_ptr(), n, NCOLS, curve, 0, 0, d_x=x[a].data_ptr(), stream=stream.cuda_stream)

            def decode():
                icc.decode_batch_device(reqs, n, NCOLS, n, curve, "exact", stream.cuda_stream)

            encode()                                                              # tables, workspaces
            decode()
            stream.synchronize()
            t_enc, t_dec = [], []
            for _ in range(args.reps):
                t_enc.append(event_ms(stream, encode))
                t_dec.append(event_ms(stream, decode))
            stream.synchronize()
            for a in range(k):
                assert torch.equal(back[a], u[a]), "request %d: the decode is not the encode's input" % a
            assert int(bad.abs().sum()) == 0, "a counter is not 0"
            enc, dec = statistics.median(t_enc), statistics.median(t_dec)
            rec = {"curve": curve, "k": k, "n_rows": n, "n_cols": NCOLS, "reps": args.reps, "decode_exact_ms": round(dec, 4),
                   "encode_x_ms": round(enc, 4), "decode_over_encode": round(dec / enc, 3),
                   "decode_ms_min_max": [round(min(t_dec), 4), round(max(t_dec), 4)],
                   "encode_ms_min_max": [round(min(t_enc), 4), round(max(t_enc), 4)], "outputs_checked": True}
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
            del u, x, back
    if out:
        out.close()


if __name__ == "__main__":
    main()
