#!/usr/bin/env python3
"""The lower-level repair (porla_{kzg,ipa}_repair_levels_batch_device) on clean files and on one damaged Y row, beside the scrub a
caller has today, same stores, same run.

For (K, n_total) in {(1, 2^15), (64, 2^10)} x 128 columns, per build (KZG on BN254, IPA on secp256k1), files with t = n_total - 1
(every lower level resident, no top level).  The X halves are made as tools/bench_extract.py makes them (device encodes of random
blocks below 2^248 and of their MACs; the K files share them).  The Y halves are made by the call under test itself, before anything
is timed: from Y stores of zeros every Y row fails, no level has a witness, and the call writes data, alignment and MAC rows; what
it wrote is then CHECKED by calls this tool does not time against: the scrub below finds every Y row OK and its RESIDUE64 decode of
every Y half gives the blocks back (they are below p_icc), byte for byte.  Every file has Y stores and outputs of its own.  Timed, each
as ONE window of device events on a stream of its own, alternating (the order rotates from repeat to repeat), `--reps` times after a
warm-up; medians and the spread are reported:
  a_clean    the call, every level named, on the clean files
  b_damaged  the call, every level named, one data byte of one Y row of the largest level of every file flipped before each repeat
             (the flip is outside the window)
  c_scrub    porla_*_extract_xy_batch_device with y_levels all ones on the same stores: it reports damaged Y rows and heals nothing
Checked, every output byte: a_clean -- statuses 1, actions 0, verdicts CLEAN, counters 0, the Y stores equal to their reference copies;
b_damaged -- the damaged row's status 0 and action DATA, all else 1 / 0, the largest level REPAIRED, counters [0, 1, 1, 0, 0, 1, 0, 0],
the Y stores equal to their reference copies after every repeat; c_scrub -- every status of both halves 1, counters 0, d_work and d_work_y
equal to the blocks.  No timing threshold gates anything: the figures are records.  One JSON line per (build, K, n_total).

    python tools/bench_repair_levels.py [--out profiles/r28_a_repair_levels.jsonl] [--reps 9] [--shapes 15:1,10:64]
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
ALL = (1 << 64) - 1
DATA, CLEAN, REPAIRED = 1, 1, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--shapes", default="15:1,10:64")
    ap.add_argument("--curves", default="bn254,secp256k1")
    args = ap.parse_args()
    import torch
    from porla_amd import icc
    from porla_amd import multiexp as mx
    assert torch.cuda.is_available(), "bench_repair_levels.py needs a GPU"
    out = open(args.out, "w") if args.out else None
    stream = torch.cuda.Stream()
    dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    pb = lambda p: p[0].to_bytes(32, "big") + p[1].to_bytes(32, "big")
    bb = NCOLS * 32
    for curve in args.curves.split(","):
        gfb = mx.FixedBase(curve, pb(GEN[curve]), 1, window_bits=8)
        if curve == "bn254":
            mx.init_key(TAU, ALPHA)
            mx.init_SRS(NCOLS)
            afb = hfb = both = None
        else:
            gen = torch.Generator(device="cuda")
            gen.manual_seed(80)
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

        def repair(reqs, n):
            if curve == "bn254":
                mx.kzg_repair_levels_batch_device(reqs, n, stream.cuda_stream)
            else:
                afb.ipa_repair_levels_batch_device(hfb, IPA_ALPHA, reqs, n, stream.cuda_stream)

        def extract_xy(reqs, n):
            if curve == "bn254":
                mx.kzg_extract_xy_batch_device(reqs, n, "exact", stream.cuda_stream)
            else:
                afb.ipa_extract_xy_batch_device(hfb, IPA_ALPHA, reqs, n, "exact", stream.cuda_stream)

        for shape in args.shapes.split(","):
            log, k = (int(x) for x in shape.split(":"))
            n, t = 1 << log, (1 << log) - 1
            rng = random.Random(2800 * k + log)
            gen = torch.Generator(device="cuda")
            gen.manual_seed(2800 * k + log)
            order = "big" if curve == "bn254" else "little"
            # the X stores, shared by the K files: level i (2^i rows) at rows 2^i - 1 .. of the t layout; blocks below 2^248
            data, macs, prf_all, blocks = [], [], [], []
            for i in range(log):
                m = 1 << i
                blk = torch.randint(0, 256, (m * NCOLS, 32), dtype=torch.uint8, device="cuda", generator=gen)
                blk[:, 31] = 0
                blk = blk.reshape(-1)
                s = [rng.getrandbits(128) for _ in range(m)]
                prf_all += s
                hide = dev(b"".join(v.to_bytes(32, "big") for v in (inverse_network(s, curve) if m > 1 else s)))
                bm = torch.empty(m * 64, dtype=torch.uint8, device="cuda")
                block_macs(blk, hide, m, bm)
                if m == 1:
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
            all_blocks = torch.cat(blocks)
            prf_x = dev(b"".join(v.to_bytes(16, order) for v in prf_all))
            prf_y = dev(b"".join(rng.getrandbits(128).to_bytes(16, order) for _ in range(t)))
            full = lambda size, dtype=torch.uint8: torch.full((size,), 0xA5 if dtype == torch.uint8 else -1, dtype=dtype, device="cuda")
            zeros = lambda size: torch.zeros(size, dtype=torch.uint8, device="cuda")
            work_b = mx.repair_levels_work_bytes(n, NCOLS, t, ALL)
            files = [dict(data_y=[zeros(64 * NCOLS << i) for i in range(log)], mac_y=[zeros(64 << i) for i in range(log)],
                          align_y=[zeros(64 << i) for i in range(log)], work=full(work_b), status_x=full(t), status_y=full(t), action=full(t),
                          level=full(16), counts=full(8, torch.int32)) for _ in range(k)]
            ptrs = lambda ts: [x.data_ptr() for x in ts]
            reqs = [(t, ALL, ptrs(data), ptrs(macs), prf_x.data_ptr(), prf_y.data_ptr(), ptrs(f["data_y"]), ptrs(f["mac_y"]), ptrs(f["align_y"]),
                     f["work"].data_ptr(), f["status_x"].data_ptr(), f["status_y"].data_ptr(), f["action"].data_ptr(), f["level"].data_ptr(),
                     f["counts"].data_ptr()) for f in files]
            # the Y stores: written by the call itself from stores of zeros, then checked by the scrub
            torch.cuda.synchronize()
            repair(reqs, n)
            stream.synchronize()
            for f in files:
                assert bool((f["status_x"] == 1).all()) and bool((f["status_y"] == 0).all()), "making the Y stores: the statuses"
                assert f["level"][:log].tolist() == [REPAIRED] * log and f["counts"].tolist()[5:] == [log, 0, 0], "making the Y stores: the verdicts"
            ref = [{name: [x.clone() for x in f[name]] for name in ("data_y", "mac_y", "align_y")} for f in files]
            ex = [dict(work=full(t * bb), blocks=full(n * bb), steps=full(n, torch.int32), flags=full(n), status=full(t), counts=full(6, torch.int32),
                       work_y=full(t * bb), status_y=full(t)) for _ in range(k)]
            ex_reqs = [(t, ptrs(data), ptrs(macs), 0, 0, 0, prf_x.data_ptr(), o["work"].data_ptr(), o["blocks"].data_ptr(), o["steps"].data_ptr(),
                        o["flags"].data_ptr(), o["status"].data_ptr(), o["counts"].data_ptr(), ptrs(f["data_y"]), ptrs(f["mac_y"]), ptrs(f["align_y"]),
                        prf_y.data_ptr(), o["work_y"].data_ptr(), o["status_y"].data_ptr(), ALL) for f, o in zip(files, ex)]
            big = log - 1
            off_big = (1 << big) - 1
            bad_row = (1 << big) // 3
            at = 64 * (bad_row * NCOLS + 17) + 2

            def same_stores(what):
                for f, r in zip(files, ref):
                    for name in r:
                        for i in range(log):
                            assert torch.equal(f[name][i], r[name][i]), "%s: %s of level %d differs from its reference copy" % (what, name, i)

            def check_scrub():
                for o in ex:
                    assert bool((o["status"] == 1).all()) and bool((o["status_y"] == 1).all()), "c: a status is not 1"
                    assert o["counts"].tolist()[:2] == [0, 0] and o["counts"].tolist()[4] == 0, "c: counters %s" % o["counts"].tolist()
                    assert torch.equal(o["work"], all_blocks), "c: the X decode differs from the blocks"
                    assert torch.equal(o["work_y"], all_blocks), "c: the Y decode differs from the blocks"

            def check_clean():
                for f in files:
                    assert bool((f["status_x"] == 1).all()) and bool((f["status_y"] == 1).all()) and bool((f["action"] == 0).all()), "a: statuses, actions"
                    assert f["level"].tolist() == [CLEAN] * log + [0] * (16 - log) and f["counts"].tolist() == [0] * 8, "a: verdicts, counters"
                same_stores("a")

            def check_damaged():
                for f in files:
                    sy, ac = f["status_y"].clone(), f["action"].clone()
                    assert int(sy[off_big + bad_row]) == 0 and int(ac[off_big + bad_row]) == DATA, "b: the damaged row"
                    sy[off_big + bad_row], ac[off_big + bad_row] = 1, 0
                    assert bool((f["status_x"] == 1).all()) and bool((sy == 1).all()) and bool((ac == 0).all()), "b: the other rows"
                    assert f["level"].tolist() == [CLEAN] * big + [REPAIRED] + [0] * (16 - log), "b: verdicts"
                    assert f["counts"].tolist() == [0, 1, 1, 0, 0, 1, 0, 0], "b: counters %s" % f["counts"].tolist()
                same_stores("b")

            def damage():
                with torch.cuda.stream(stream):
                    for f in files:
                        f["data_y"][big][at] ^= 0x20

            legs = {"a_clean": lambda: repair(reqs, n), "b_damaged": lambda: repair(reqs, n), "c_scrub": lambda: extract_xy(ex_reqs, n)}
            checks = {"a_clean": check_clean, "b_damaged": check_damaged, "c_scrub": check_scrub}
            times = {name: [] for name in legs}
            names = list(legs)
            for r in range(-1, args.reps):                                  # r = -1: the warm-up (tables, workspaces), checked like the rest
                for name in names[r % len(names):] + names[:r % len(names)]:
                    if name == "b_damaged":
                        damage()
                    ms = event_ms(stream, legs[name])
                    stream.synchronize()
                    checks[name]()
                    if r >= 0:
                        times[name].append(ms)
            torch.cuda.synchronize()
            med = {name: statistics.median(v) for name, v in times.items()}
            rec = {"build": "kzg" if curve == "bn254" else "ipa", "curve": curve, "k": k, "n_total": n, "t": t, "n_cols": NCOLS, "reps": args.reps,
                   "work_bytes_per_file": work_b}
            for name in names:
                rec[name + "_ms"] = round(med[name], 4)
                rec[name + "_ms_min_max"] = [round(min(times[name]), 4), round(max(times[name]), 4)]
            rec.update({"b_damaged_over_a_clean": round(med["b_damaged"] / med["a_clean"], 4), "a_clean_over_c_scrub": round(med["a_clean"] / med["c_scrub"], 4),
                        "damaged_level_rows": 1 << big, "c_scrub_heals_nothing": True, "outputs_checked": True})
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
            del files, ref, ex, data, macs, blocks, all_blocks, reqs, ex_reqs
    if out:
        out.close()


if __name__ == "__main__":
    main()
