#!/usr/bin/env python3
"""The ragged ICC decode (porla_icc_decode_ragged_batch_device) beside the uniform call (porla_icc_decode_batch_device), same stores,
same run, form EXACT, 128 columns.

Cases, per curve:
  file15       the fifteen X levels of a file of 2^15 blocks (2^1 .. 2^15 rows): ONE ragged call against one uniform call per size (15)
  files64      the ten X levels (2^1 .. 2^10 rows) of 64 files of 2^10 blocks: ONE ragged call of 640 requests against one uniform
               call of 64 requests per size (10).  The files share the stores and have outputs of their own
  same_2^15    ONE level of 2^15 rows through both entry points: the same tile work, the difference is the cost of the map
  same_64x2^10 64 levels of 2^10 rows through both entry points, likewise
The levels are random blocks encoded on the device (porla_icc_encode_device, X part).  Timed, each leg as ONE window of device events
on a stream of its own, the legs alternating (the order rotates from repeat to repeat), `--reps` times after a warm-up; median and
min..max reported.  Checked: every output byte of the ragged call equals the uniform calls' and the encoded blocks, every counter is 0.
For the same_* cases the record says whether the ragged median lies inside the min..max of the uniform call's repeats.  One JSON line
per (curve, case).

    python tools/bench_icc_decode_ragged.py [--out profiles/r25_a_decode_ragged.jsonl] [--reps 9] [--curves bn254,secp256k1]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from tools.bench_retrieve import NCOLS, event_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--curves", default="bn254,secp256k1")
    ap.add_argument("--tag", default=None, help="a label copied into every record")
    args = ap.parse_args()
    import torch
    from porla_amd import icc
    assert torch.cuda.is_available(), "bench_icc_decode_ragged.py needs a GPU"
    out = open(args.out, "a" if args.append else "w") if args.out else None
    stream = torch.cuda.Stream()
    bb = NCOLS * 32
    for curve in args.curves.split(","):
        gen = torch.Generator(device="cuda")
        gen.manual_seed(2500)
        blocks, rows = {}, {}                                               # log2 n_rows -> the blocks, their X rows
        for lg in range(1, 16):
            m = 1 << lg
            blocks[lg] = torch.randint(0, 256, (m * bb,), dtype=torch.uint8, device="cuda", generator=gen)
            rows[lg] = torch.empty(m * NCOLS * 64, dtype=torch.uint8, device="cuda")
            icc.crebuild_device(blocks[lg].data_ptr(), m, NCOLS, curve, 0, 0, d_x=rows[lg].data_ptr())
        torch.cuda.synchronize()
        # (case, n_total, the requests' levels as (log2 n_rows, copies))
        cases = [("file15", 1 << 15, [(lg, 1) for lg in range(1, 16)]), ("files64", 1 << 10, [(lg, 64) for lg in range(1, 11)]),
                 ("same_2^15", 1 << 15, [(15, 1)]), ("same_64x2^10", 1 << 10, [(10, 64)])]
        for name, n_total, levels in cases:
            full = lambda size, dtype=torch.uint8: torch.full((size,), 0xA5 if dtype == torch.uint8 else -1, dtype=dtype, device="cuda")
            outs = {leg: {lg: [(full((bb << lg)), full(1, torch.int32)) for _ in range(c)] for lg, c in levels} for leg in ("ragged", "uniform")}
            rag_reqs = [(rows[lg].data_ptr(), o.data_ptr(), 0, b.data_ptr(), 1 << lg) for lg, _ in levels for o, b in outs["ragged"][lg]]
            uni_reqs = {lg: [(rows[lg].data_ptr(), o.data_ptr(), 0, b.data_ptr()) for o, b in outs["uniform"][lg]] for lg, _ in levels}

            def uniform():
                for lg, _ in levels:
                    icc.decode_batch_device(uni_reqs[lg], 1 << lg, NCOLS, n_total, curve, "exact", stream.cuda_stream)

            legs = {"ragged": lambda: icc.decode_ragged_batch_device(rag_reqs, NCOLS, n_total, curve, "exact", stream.cuda_stream),
                    "uniform": uniform}
            torch.cuda.synchronize()
            for fn in legs.values():                                        # tables, workspaces
                fn()
            stream.synchronize()
            times = {leg: [] for leg in legs}
            names = list(legs)
            for r in range(args.reps):
                for leg in names[r % len(names):] + names[:r % len(names)]:
                    times[leg].append(event_ms(stream, legs[leg]))
            stream.synchronize()
            torch.cuda.synchronize()
            for lg, c in levels:                                            # every output byte, every counter
                for (ro, rb), (uo, ub) in zip(outs["ragged"][lg], outs["uniform"][lg]):
                    assert torch.equal(ro, uo), "%s: a level of 2^%d rows differs from the uniform call's" % (name, lg)
                    assert torch.equal(ro, blocks[lg]), "%s: a level of 2^%d rows is not the encoded blocks" % (name, lg)
                    assert int(rb[0]) == 0 and int(ub[0]) == 0, "%s: a counter is not 0" % name
            med = {leg: statistics.median(v) for leg, v in times.items()}
            lo, hi = min(times["uniform"]), max(times["uniform"])
            rec = {"bench": "icc_decode_ragged", "curve": curve, "case": name, "n_total": n_total, "n_cols": NCOLS, "reps": args.reps,
                   "requests": len(rag_reqs), "uniform_calls": len(levels),
                   "ragged_ms": round(med["ragged"], 4), "ragged_ms_min_max": [round(min(times["ragged"]), 4), round(max(times["ragged"]), 4)],
                   "uniform_ms": round(med["uniform"], 4), "uniform_ms_min_max": [round(lo, 4), round(hi, 4)],
                   "uniform_over_ragged": round(med["uniform"] / med["ragged"], 4),
                   "ragged_median_inside_uniform_min_max": bool(lo <= med["ragged"] <= hi), "outputs_checked": True}
            if args.tag:
                rec["tag"] = args.tag
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
            del outs, rag_reqs, uni_reqs
        del blocks, rows
    if out:
        out.close()


if __name__ == "__main__":
    main()
