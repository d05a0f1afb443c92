#!/usr/bin/env python3
"""The file extraction with the top level's Y half (porla_{kzg,ipa}_extract_xyt_batch_device) beside the call without it and beside
what a caller had before it, same stores, same run.

For (K, n_total) in {(1, 2^15), (64, 2^10)} x 128 columns, per build (KZG on BN254, IPA on secp256k1), one file with t = n_total - 1
(every lower level resident) and an exact top level, the X halves made as tools/bench_extract.py makes them.  The top level's Y half
is the rebuild's own: the encode's Y part of the same blocks at write step TOP_STEP (wt != 1: every patched row pays for its two
products), its MAC rows the MAC network's Y part with complements s_j h on every row.  The K files of a call share the stores and have
outputs of their own.  Timed, each as ONE window of device events on a stream of its own, alternating (the order rotates from repeat
to repeat), `--reps` times after a warm-up; medians and the spread are reported:
  a_xy       porla_*_extract_xy_batch_device, y_levels = 0                   } the same launches: the new entry's median has to lie
  a_xyt0     the new call with top_y = 0 and NULL new pointers               } inside the min .. max of a_xy's repeats (the one gate)
  b_top1     the new call with top_y = 1 on the clean file: the check of one more half and the patch pass (a copy)
  c_xyt      one top X row damaged, the new call with top_y = 1
  c_parent   what a caller had before: porla_*_extract_xy_batch_device on the damaged file plus ONE aligned retrieval (EXACT, d_out)
             of the whole top Y half, which needs that half entirely clean; nothing is unscaled or merged
Checked, every output byte: a_xyt0 against a_xy (d_work, d_blocks, d_steps, d_flags, d_row_status, six counters; counters 6, 7 zero);
b_top1 the same, every top Y status 1, d_top_patch the X half; c_xyt: d_blocks and d_steps of the CLEAN file, d_top_patch the clean X
half, the flags FOUND | FROM_Y on the top level's slots and FOUND elsewhere, counters [1, 0, 0, 0, 0, 0, 0, 1]; c_parent: one failed
row, UNSURE slots, the retrieval's statuses all 1.  One JSON line per (build, K, n_total); exit status 1 if the gate of (a) is missed.

    python tools/bench_extract_xyt.py [--out profiles/r26_a_extract_xyt.jsonl] [--reps 9] [--shapes 15:1,10:64]
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
FOUND, UNSURE, FROM_Y = 1, 2, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--shapes", default="15:1,10:64")
    ap.add_argument("--curves", default="bn254,secp256k1")
    args = ap.parse_args()
    import icc_py
    import torch
    from porla_amd import icc
    from porla_amd import multiexp as mx
    assert torch.cuda.is_available(), "bench_extract_xyt.py needs a GPU"
    out = open(args.out, "w") if args.out else None
    stream = torch.cuda.Stream()
    dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    pb = lambda p: p[0].to_bytes(32, "big") + p[1].to_bytes(32, "big")
    bb = NCOLS * 32
    gate_ok = True
    for curve in args.curves.split(","):
        g, q = GEN[curve], icc_py.Q[curve]
        if curve == "bn254":
            mx.init_key(TAU, ALPHA)
            mx.init_SRS(NCOLS)
            afb = hfb = both = None
        else:
            gfb = mx.FixedBase(curve, pb(g), 1, window_bits=8)
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

        def aligned_exact(reqs, n_rows, n):
            if curve == "bn254":
                mx.kzg_retrieve_aligned_batch_device(reqs, n_rows, n, "exact", stream.cuda_stream)
            else:
                afb.ipa_retrieve_aligned_batch_device(hfb, IPA_ALPHA, reqs, n_rows, n, "exact", stream.cuda_stream)

        def extract_xy(reqs, n):
            if curve == "bn254":
                mx.kzg_extract_xy_batch_device(reqs, n, "exact", stream.cuda_stream)
            else:
                afb.ipa_extract_xy_batch_device(hfb, IPA_ALPHA, reqs, n, "exact", stream.cuda_stream)

        def extract_xyt(reqs, n):
            if curve == "bn254":
                mx.kzg_extract_xyt_batch_device(reqs, n, "exact", stream.cuda_stream)
            else:
                afb.ipa_extract_xyt_batch_device(hfb, IPA_ALPHA, reqs, n, "exact", stream.cuda_stream)

        for shape in args.shapes.split(","):
            log, k = (int(x) for x in shape.split(":"))
            n, t = 1 << log, (1 << log) - 1
            top_step = n + 3                                                # wt = w^reverse_bits(3) != 1
            rng = random.Random(2600 * k + log)
            gen = torch.Generator(device="cuda")
            gen.manual_seed(2600 * k + log)
            order = "big" if curve == "bn254" else "little"
            # the X stores as tools/bench_extract.py makes them: level i (2^i rows) for i < log, then the top level (n rows)
            data, macs, prf_all = [], [], []
            top_y = None
            for i in list(range(log)) + [log]:
                m = 1 << i
                blk = torch.randint(0, 256, (m * bb,), dtype=torch.uint8, device="cuda", generator=gen)
                idx = torch.arange(1, n + 1, dtype=torch.int64, device="cuda") if i == log else \
                    torch.randint(1, n + 1, (m,), dtype=torch.int64, device="cuda", generator=gen)
                blk.view(torch.int64).view(m, bb // 8)[:, 0] = idx
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
                if i == log:
                    # the Y part of the same rebuild: the MAC network scales by wt first, so the block MACs carry wt^-1 times the
                    # inverse network of the Y complements
                    wt = pow(icc_py.root_w(n), icc_py.reverse_bits(top_step % n, log), icc_py.P_ICC)
                    unwt = pow(wt % q, -1, q)
                    s_y = [rng.getrandbits(128) for _ in range(m)]
                    hide_y = dev(b"".join((v * unwt % q).to_bytes(32, "big") for v in inverse_network(s_y, curve)))
                    block_macs(blk, hide_y, m, bm)
                    rows_y = torch.empty(m * NCOLS * 64, dtype=torch.uint8, device="cuda")
                    macs_y = torch.empty(m * 64, dtype=torch.uint8, device="cuda")
                    icc.crebuild_device(blk.data_ptr(), m, NCOLS, curve, top_step, 1, d_x=rows_y.data_ptr())
                    icc.mac_crebuild_device(bm.data_ptr(), m, curve, top_step, 1, macs_y.data_ptr())
                    torch.cuda.synchronize()
                    top_y = (rows_y, macs_y, dev(b"".join(v.to_bytes(16, order) for v in s_y)))
                del blk
            prf = dev(b"".join(v.to_bytes(16, order) for v in prf_all))
            damaged = data[log].clone()
            damaged[64 * (5 * NCOLS + 7) + 1] ^= 1                           # top X row 5
            rows = t + n
            full = lambda size, dtype=torch.uint8: torch.full((size,), 0xA5 if dtype == torch.uint8 else -1, dtype=dtype, device="cuda")

            def outputs(kind):
                o = dict(work=full(t * bb), blocks=full(n * bb), steps=full(n, torch.int32), flags=full(n), status=full(rows),
                         counts=full(8 if kind else 6, torch.int32))
                if kind == 2:
                    o.update(patch=full(n * NCOLS * 64), status_ty=full(n))
                return o

            def xy_req(o, top_rows):
                return (t, [d.data_ptr() for d in data[:log]], [m.data_ptr() for m in macs[:log]], top_rows.data_ptr(), macs[log].data_ptr(), 0,
                        prf.data_ptr(), o["work"].data_ptr(), o["blocks"].data_ptr(), o["steps"].data_ptr(), o["flags"].data_ptr(),
                        o["status"].data_ptr(), o["counts"].data_ptr(), None, None, None, 0, 0, 0, 0)

            def top_req(o, tried):
                if not tried:
                    return (0, 0, 0, 0, 0, 0, top_step, 0)
                return (top_y[0].data_ptr(), top_y[1].data_ptr(), 0, top_y[2].data_ptr(), o["patch"].data_ptr(), o["status_ty"].data_ptr(), top_step, 1)

            bufs = {"a_xy": [outputs(0) for _ in range(k)], "a_xyt0": [outputs(1) for _ in range(k)], "b_top1": [outputs(2) for _ in range(k)],
                    "c_xyt": [outputs(2) for _ in range(k)], "c_parent": [outputs(0) for _ in range(k)]}
            reqs = {"a_xy": [xy_req(o, data[log]) for o in bufs["a_xy"]],
                    "a_xyt0": [xy_req(o, data[log]) + top_req(o, False) for o in bufs["a_xyt0"]],
                    "b_top1": [xy_req(o, data[log]) + top_req(o, True) for o in bufs["b_top1"]],
                    "c_xyt": [xy_req(o, damaged) + top_req(o, True) for o in bufs["c_xyt"]],
                    "c_parent": [xy_req(o, damaged) for o in bufs["c_parent"]]}
            rt = [dict(out=full(n * bb), status=full(n), counts=full(2, torch.int32)) for _ in range(k)]
            rt_reqs = [(top_y[0].data_ptr(), top_y[1].data_ptr(), top_y[2].data_ptr(), 0, 0, r["out"].data_ptr(), r["status"].data_ptr(),
                        r["counts"].data_ptr()) for r in rt]

            def c_parent():
                extract_xy(reqs["c_parent"], n)
                aligned_exact(rt_reqs, n, n)

            legs = {"a_xy": lambda: extract_xy(reqs["a_xy"], n), "a_xyt0": lambda: extract_xyt(reqs["a_xyt0"], n),
                    "b_top1": lambda: extract_xyt(reqs["b_top1"], n), "c_xyt": lambda: extract_xyt(reqs["c_xyt"], n), "c_parent": c_parent}
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
            # every output byte
            same = ("work", "blocks", "steps", "flags", "status")
            for j in range(k):
                p, a0, b, c, cp = (bufs[x][j] for x in ("a_xy", "a_xyt0", "b_top1", "c_xyt", "c_parent"))
                r = rt[j]
                assert bool((p["status"] == 1).all()) and p["counts"].tolist() == [0] * 6 and bool((p["flags"] == FOUND).all()), "the clean file"
                for name in same:
                    assert torch.equal(a0[name], p[name]), "a: %s differs from the xy call" % name
                    assert torch.equal(b[name], p[name]), "b: %s differs from the xy call" % name
                assert a0["counts"].tolist() == [0] * 8 and b["counts"].tolist() == [0] * 8, "a / b: counters"
                assert bool((b["status_ty"] == 1).all()), "b: a top Y status is not 1"
                assert torch.equal(b["patch"], data[log]), "b: the patched half is not the X half"
                assert bool((r["status"] == 1).all()) and r["counts"].tolist()[0] == 0, "the retrieval of the top Y half"
                assert cp["counts"].tolist()[0] == 1 and int((cp["status"] == 0).sum()) == 1 and int(cp["status"][t + 5]) == 0, "c: one damaged row"
                assert bool((cp["flags"] & UNSURE).any()), "c_parent: the top level is failed"
                assert torch.equal(c["status"], cp["status"]) and bool((c["status_ty"] == 1).all()), "c: the statuses"
                assert torch.equal(c["patch"], data[log]), "c: the patched half is not the clean X half"
                assert torch.equal(c["blocks"], p["blocks"]) and torch.equal(c["steps"], p["steps"]) and torch.equal(c["work"], p["work"]), \
                    "c: the file differs from the clean file's"
                want = torch.where(p["steps"] == 0, torch.full_like(p["flags"], FOUND | FROM_Y), p["flags"])
                assert torch.equal(c["flags"], want) and bool((p["steps"] == 0).any()), "c: the flags"
                assert c["counts"].tolist() == [1, 0, 0, 0, 0, 0, 0, 1], "c: counters %s" % c["counts"].tolist()
            med = {name: statistics.median(v) for name, v in times.items()}
            within = min(times["a_xy"]) <= med["a_xyt0"] <= max(times["a_xy"])
            gate_ok = gate_ok and within
            rec = {"build": "kzg" if curve == "bn254" else "ipa", "curve": curve, "k": k, "n_total": n, "t": t, "n_cols": NCOLS, "reps": args.reps,
                   "top_step": top_step}
            for name in names:
                rec[name + "_ms"] = round(med[name], 4)
                rec[name + "_ms_min_max"] = [round(min(times[name]), 4), round(max(times[name]), 4)]
            rec.update({"a_xyt0_over_a_xy": round(med["a_xyt0"] / med["a_xy"], 4), "a_xyt0_median_inside_a_xy_min_max": within,
                        "b_top1_over_a_xy": round(med["b_top1"] / med["a_xy"], 4), "c_xyt_over_c_parent": round(med["c_xyt"] / med["c_parent"], 4),
                        "c_parent_unscales_and_merges_nothing": True, "outputs_checked": True})
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
            del bufs, reqs, rt, data, macs, top_y, damaged
    if out:
        out.close()
    return 0 if gate_ok else 1


if __name__ == "__main__":
    sys.exit(main())
