#!/usr/bin/env python3
"""The verified file extraction (porla_{kzg,ipa}_extract_batch_device) beside what a caller has without it, same stores, same run.

For (K, n_total) in {(1, 2^15), (64, 2^10)} x 128 columns, per build (KZG on BN254, IPA on secp256k1), one file with t = n_total - 1
(every lower level resident) and an exact top level, all made on the device as tools/bench_retrieve.py makes a level: random blocks
whose chunk 0 names a slot (the top level's block b names b + 1, a lower level's block a random slot), their MACs hiding the inverse
network of the PRF values, then the device encodes.  The K files of a call share the stores and have outputs of their own.  Timed, each
as ONE window of device events on a stream of its own, alternating (the order rotates from repeat to repeat), `--reps` times after a
warm-up, medians reported:
  extract    the one call
  per_level  one aligned retrieval call (form exact, with d_out) per resident level SIZE of 2 rows and more: log2(n_total) calls.
             This sequence has NO MERGE and NO LEVEL 0 (the retrieval calls refuse one row): it does less than the extraction
Checked: every status is 1 in both; every status byte of the levels both cover is equal; every decoded byte is equal -- the
extraction's d_work against the per-level calls' blocks, and the slots the top level wins in d_blocks against the top level's blocks;
every slot is FOUND and none UNSURE; level 0's block is in d_work.  One JSON line per (build, K, n_total).

    python tools/bench_extract.py [--out profiles/r23_a_extract.jsonl] [--reps 7] [--shapes 15:1,10:64]
"""
import argparse
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from tools.bench_retrieve import ALPHA, GEN, NCOLS, TAU, event_ms, inverse_network  # noqa: E402

IPA_ALPHA = 0x6a09e667f3bcc908b2fb1366ea957d3e3adec17512775099da2f590b0667322a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="15:1,10:64")
    ap.add_argument("--curves", default="bn254,secp256k1")
    args = ap.parse_args()
    import torch
    from porla_amd import icc
    from porla_amd import multiexp as mx
    assert torch.cuda.is_available(), "bench_extract.py needs a GPU"
    out = open(args.out, "w") if args.out else None
    stream = torch.cuda.Stream()
    dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    bb = NCOLS * 32
    for curve in args.curves.split(","):
        g = GEN[curve]
        if curve == "bn254":
            mx.init_key(TAU, ALPHA)
            mx.init_SRS(NCOLS)
            afb = hfb = both = None
        else:
            gfb = mx.FixedBase(curve, g[0].to_bytes(32, "big") + g[1].to_bytes(32, "big"), 1, window_bits=8)
            gen = torch.Generator(device="cuda")
            gen.manual_seed(79)
            sc = torch.randint(0, 256, ((NCOLS + 1) * 32,), dtype=torch.uint8, device="cuda", generator=gen)
            pts = torch.empty((NCOLS + 1) * 64, dtype=torch.uint8, device="cuda")
            gfb.commit_device(sc.data_ptr(), NCOLS + 1, 1, pts.data_ptr())
            torch.cuda.synchronize()
            pts = bytes(pts.cpu().numpy())
            afb = mx.FixedBase(curve, pts[:64 * NCOLS], NCOLS)
            hfb = mx.FixedBase(curve, pts[64 * NCOLS:], 1)
            both = mx.FixedBase(curve, pts, NCOLS + 1)

        def block_macs(chunks_le, scalars32, n, d_out):
            rows_be = chunks_le.reshape(-1, 32).flip(1).contiguous().reshape(-1)
            if curve == "bn254":
                mx.kzg_mac_batch_device(rows_be.data_ptr(), scalars32.data_ptr(), n, d_out.data_ptr())
            else:
                rows = torch.cat([rows_be.reshape(n, bb), scalars32.reshape(n, 32)], dim=1).contiguous().reshape(-1)
                both.commit_device(rows.data_ptr(), n, NCOLS + 1, d_out.data_ptr())
            torch.cuda.synchronize()

        def aligned(reqs, n_rows, n):
            if curve == "bn254":
                mx.kzg_retrieve_aligned_batch_device(reqs, n_rows, n, "exact", stream.cuda_stream)
            else:
                afb.ipa_retrieve_aligned_batch_device(hfb, IPA_ALPHA, reqs, n_rows, n, "exact", stream.cuda_stream)

        def extract(reqs, n):
            if curve == "bn254":
                mx.kzg_extract_batch_device(reqs, n, "exact", stream.cuda_stream)
            else:
                afb.ipa_extract_batch_device(hfb, IPA_ALPHA, reqs, n, "exact", stream.cuda_stream)

        for shape in args.shapes.split(","):
            log, k = (int(x) for x in shape.split(":"))
            n, t = 1 << log, (1 << log) - 1
            rng = random.Random(2300 * k + log)
            gen = torch.Generator(device="cuda")
            gen.manual_seed(2300 * k + log)
            order = "big" if curve == "bn254" else "little"
            # the stores: level i (2^i rows) for i < log, then the top level (n rows); d_prf's order is ascending, then the top level
            data, macs, blocks, prf_all = [], [], [], []
            for i in list(range(log)) + [log]:
                m = 1 << i
                blk = torch.randint(0, 256, (m * bb,), dtype=torch.uint8, device="cuda", generator=gen)
                idx = torch.arange(1, n + 1, dtype=torch.int64, device="cuda") if i == log else \
                    torch.randint(1, n + 1, (m,), dtype=torch.int64, device="cuda", generator=gen)
                blk.view(torch.int64).view(m, bb // 8)[:, 0] = idx          # chunk 0's low 8 bytes, little-endian: the slot's index
                s = [rng.getrandbits(128) for _ in range(m)]
                prf_all += s
                hide = dev(b"".join(v.to_bytes(32, "big") for v in (inverse_network(s, curve) if m > 1 else s)))
                bm = torch.empty(m * 64, dtype=torch.uint8, device="cuda")
                block_macs(blk, hide, m, bm)
                if m == 1:                                                  # level 0: the chunks zero-extended, the block's own MAC
                    rows_x = torch.cat([blk.reshape(NCOLS, 32), torch.zeros((NCOLS, 32), dtype=torch.uint8, device="cuda")], dim=1).contiguous().reshape(-1)
                    macs_x = bm
                else:
                    rows_x = torch.empty(m * NCOLS * 64, dtype=torch.uint8, device="cuda")
                    macs_x = torch.empty(m * 64, dtype=torch.uint8, device="cuda")
                    icc.crebuild_device(blk.data_ptr(), m, NCOLS, curve, 0, 0, d_x=rows_x.data_ptr())
                    icc.mac_crebuild_device(bm.data_ptr(), m, curve, 0, 0, macs_x.data_ptr())
                    torch.cuda.synchronize()
                data.append(rows_x)
                macs.append(macs_x)
                blocks.append(blk)
            prf = dev(b"".join(v.to_bytes(16, order) for v in prf_all))
            rows = t + n
            full = lambda size, dtype=torch.uint8: torch.full((size,), 0xA5 if dtype == torch.uint8 else -1, dtype=dtype, device="cuda")
            ex = [dict(work=full(t * bb), blocks=full(n * bb), steps=full(n, torch.int32), flags=full(n), status=full(rows),
                       counts=full(4, torch.int32)) for _ in range(k)]
            ex_reqs = [(t, [d.data_ptr() for d in data[:log]], [m.data_ptr() for m in macs[:log]], data[log].data_ptr(), macs[log].data_ptr(), 0,
                        prf.data_ptr(), e["work"].data_ptr(), e["blocks"].data_ptr(), e["steps"].data_ptr(), e["flags"].data_ptr(),
                        e["status"].data_ptr(), e["counts"].data_ptr()) for e in ex]
            pl = [dict(out=full(rows * bb), status=full(rows), counts=full(2 * (log + 1), torch.int32)) for _ in range(k)]
            off = lambda i: t if i == log else (1 << i) - 1                 # (t = 2^log - 1: level i starts at 2^i - 1)
            pl_reqs = {i: [(data[i].data_ptr(), macs[i].data_ptr(), prf.data_ptr() + 16 * off(i), 0, 0, p["out"].data_ptr() + off(i) * bb,
                            p["status"].data_ptr() + off(i), p["counts"].data_ptr() + 8 * i) for p in pl] for i in range(1, log + 1)}

            def per_level():
                for i in range(1, log + 1):
                    aligned(pl_reqs[i], 1 << i, n)

            legs = {"extract": lambda: extract(ex_reqs, n), "per_level": per_level}
            torch.cuda.synchronize()
            for fn in legs.values():                                        # tables, workspaces
                fn()
            stream.synchronize()
            times = {name: [] for name in legs}
            names = list(legs)
            for r in range(args.reps):
                for name in names[r % len(names):] + names[:r % len(names)]:
                    times[name].append(event_ms(stream, legs[name]))
            stream.synchronize()
            torch.cuda.synchronize()
            # every status byte, every decoded byte
            written = torch.cat(blocks[:log])                               # the lower levels' blocks in d_work's order
            for e, p in zip(ex, pl):
                assert bool((e["status"] == 1).all()) and bool((p["status"][1:] == 1).all()), "a status is not 1"
                assert torch.equal(e["status"][1:], p["status"][1:]), "the statuses of the levels both cover differ"
                assert torch.equal(e["work"][bb:], p["out"][bb:t * bb]), "d_work differs from the per-level calls' blocks"
                assert torch.equal(e["work"], written), "d_work is not the written blocks"
                assert e["counts"].tolist() == [0, 0, 0, 0] and bool((e["flags"] == 1).all()), "counters or flags"
                top_wins = e["steps"] == 0
                assert torch.equal(e["blocks"].view(n, bb)[top_wins], p["out"][t * bb:].view(n, bb)[top_wins]), "the top level's slots differ"
                assert bool((e["blocks"].view(torch.int64).view(n, bb // 8)[:, 0] == torch.arange(1, n + 1, device="cuda")).all()), "a slot's index"
            med = {name: statistics.median(v) for name, v in times.items()}
            rec = {"build": "kzg" if curve == "bn254" else "ipa", "curve": curve, "k": k, "n_total": n, "t": t, "n_cols": NCOLS, "reps": args.reps,
                   "extract_ms": round(med["extract"], 4), "per_level_ms": round(med["per_level"], 4), "per_level_calls": log,
                   "per_level_has_no_merge_and_no_level_0": True,
                   "extract_ms_min_max": [round(min(times["extract"]), 4), round(max(times["extract"]), 4)],
                   "per_level_ms_min_max": [round(min(times["per_level"]), 4), round(max(times["per_level"]), 4)],
                   "extract_over_per_level": round(med["extract"] / med["per_level"], 4),
                   "slots_won_by_the_top_level": int((ex[0]["steps"] == 0).sum()), "outputs_checked": True}
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
            del ex, pl, data, macs, blocks, written
    if out:
        out.close()


if __name__ == "__main__":
    main()
