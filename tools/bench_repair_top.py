#!/usr/bin/env python3
"""The top-level repair (porla_{kzg,ipa}_repair_top_batch_device) beside the extraction with the top level's Y half and beside what
healed a top level before it, same stores, same run.

For (K, n_total) in {(1, 2^15), (64, 2^10)} x 128 columns, per build (KZG on BN254, IPA on secp256k1), K top-only files (t = 0) with an
exact top level made as tools/bench_extract_xyt.py makes it: the X half the encode's X part of the blocks, the Y half the Y part of
the same rebuild at write step TOP_STEP (wt != 1: every repaired symbol pays for its two products), MAC rows with complements s_j h
on every row of both halves.  Every file of a call has stores of its own (the repair writes them).  Timed, each as ONE window of device
events on a stream of its own, alternating (the order rotates from repeat to repeat), `--reps` times after a warm-up; medians and the
spread are reported:
  clean      the repair call on clean files: the scrub cost
  one_x      one top X row damaged per file, the repair call (the damage is put back before every repeat, outside the window)
  xyt        porla_*_extract_xyt_batch_device with top_y = 1 on the same damaged stores, for scale
  before     what healed a top level before: that extraction, then the client rebuild batch and the server rebuild batch of the file
             (the whole MAC network and the whole data network over the extracted blocks), on stores of their own
Checked, every output byte: clean -- statuses 1, actions 0, counters 0, the four stores as they were; one_x -- exactly one status 0,
the action DATA on that row, counters [1, 0, 1, 0, 0, 0, 0, 0], the four stores the pristine ones again; xyt -- the patched half is the
pristine X half, counters [1, 0, 0, 0, 0, 0, 0, 1].  The rebuild legs' outputs are those of their own tools and are not compared
here.  One JSON line per (build, K, n_total); exit status 1 if the repair of one damaged row is slower than `before`.

    python tools/bench_repair_top.py [--out profiles/r27_a_repair_top.jsonl] [--reps 9] [--shapes 15:1,10:64]
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
DATA = 1


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
    assert torch.cuda.is_available(), "bench_repair_top.py needs a GPU"
    out = open(args.out, "w") if args.out else None
    stream = torch.cuda.Stream()
    dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    pb = lambda p: p[0].to_bytes(32, "big") + p[1].to_bytes(32, "big")
    bb = NCOLS * 32
    ok = True
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

        def repair(reqs, n):
            if curve == "bn254":
                mx.kzg_repair_top_batch_device(reqs, n, "exact", stream.cuda_stream)
            else:
                afb.ipa_repair_top_batch_device(hfb, IPA_ALPHA, reqs, n, "exact", stream.cuda_stream)

        def extract_xyt(reqs, n):
            if curve == "bn254":
                mx.kzg_extract_xyt_batch_device(reqs, n, "exact", stream.cuda_stream)
            else:
                afb.ipa_extract_xyt_batch_device(hfb, IPA_ALPHA, reqs, n, "exact", stream.cuda_stream)

        def client_rebuild(reqs, n):
            if curve == "bn254":
                mx.kzg_client_rebuild_batch_device(reqs, n, stream.cuda_stream)
            else:
                afb.ipa_client_rebuild_batch_device(hfb, reqs, n, stream.cuda_stream)

        for shape in args.shapes.split(","):
            log, k = (int(x) for x in shape.split(":"))
            n = 1 << log
            top_step = n + 3                                                # wt = w^reverse_bits(3) != 1
            rng = random.Random(2700 * k + log)
            gen = torch.Generator(device="cuda")
            gen.manual_seed(2700 * k + log)
            order = "big" if curve == "bn254" else "little"
            # the top level of one file, both halves: tools/bench_extract_xyt.py's
            blk = torch.randint(0, 256, (n * bb,), dtype=torch.uint8, device="cuda", generator=gen)
            blk.view(torch.int64).view(n, bb // 8)[:, 0] = torch.arange(1, n + 1, dtype=torch.int64, device="cuda")
            wt = pow(icc_py.root_w(n), icc_py.reverse_bits(top_step % n, log), icc_py.P_ICC)
            unwt = pow(wt % q, -1, q)
            s_x, s_y = ([rng.getrandbits(128) for _ in range(n)] for _ in range(2))
            bm = torch.empty(n * 64, dtype=torch.uint8, device="cuda")
            half = {}
            for part, s, scale in ((0, s_x, 1), (1, s_y, unwt)):
                hide = dev(b"".join((v * scale % q).to_bytes(32, "big") for v in inverse_network(s, curve)))
                block_macs(blk, hide, n, bm)
                rows = torch.empty(n * NCOLS * 64, dtype=torch.uint8, device="cuda")
                macs = torch.empty(n * 64, dtype=torch.uint8, device="cuda")
                icc.crebuild_device(blk.data_ptr(), n, NCOLS, curve, top_step if part else 0, part, d_x=rows.data_ptr())
                icc.mac_crebuild_device(bm.data_ptr(), n, curve, top_step if part else 0, part, macs.data_ptr())
                torch.cuda.synchronize()
                half[part] = (rows, macs, dev(b"".join(v.to_bytes(16, order) for v in s)))
            damaged = half[0][0].clone()
            damaged[64 * (5 % n * NCOLS + 7) + 1] ^= 1                       # top X row 5
            full = lambda size, dtype=torch.uint8: torch.full((size,), 0xA5 if dtype == torch.uint8 else -1, dtype=dtype, device="cuda")

            def stores(rows_x):
                return dict(rows_x=rows_x.clone(), macs_x=half[0][1].clone(), rows_y=half[1][0].clone(), macs_y=half[1][1].clone(),
                            status_x=full(n), status_y=full(n), action_x=full(n), action_y=full(n), counts=full(8, torch.int32))

            def repair_req(o):
                return (o["rows_x"].data_ptr(), o["macs_x"].data_ptr(), 0, half[0][2].data_ptr(), o["rows_y"].data_ptr(), o["macs_y"].data_ptr(), 0,
                        half[1][2].data_ptr(), o["status_x"].data_ptr(), o["status_y"].data_ptr(), o["action_x"].data_ptr(),
                        o["action_y"].data_ptr(), o["counts"].data_ptr(), top_step)

            def xyt_outputs():
                return dict(blocks=full(n * bb), steps=full(n, torch.int32), flags=full(n), status=full(n), counts=full(8, torch.int32),
                            patch=full(n * NCOLS * 64), status_ty=full(n))

            def xyt_req(o):
                return (2 * n, None, None, damaged.data_ptr(), half[0][1].data_ptr(), 0, half[0][2].data_ptr(), 0, o["blocks"].data_ptr(),
                        o["steps"].data_ptr(), o["flags"].data_ptr(), o["status"].data_ptr(), o["counts"].data_ptr(), None, None, None, 0, 0, 0, 0,
                        half[1][0].data_ptr(), half[1][1].data_ptr(), 0, half[1][2].data_ptr(), o["patch"].data_ptr(), o["status_ty"].data_ptr(),
                        top_step, 1)

            clean = [stores(half[0][0]) for _ in range(k)]
            hurt = [stores(damaged) for _ in range(k)]
            xo = {name: [xyt_outputs() for _ in range(k)] for name in ("xyt", "before")}
            reqs = {"clean": [repair_req(o) for o in clean], "one_x": [repair_req(o) for o in hurt],
                    "xyt": [xyt_req(o) for o in xo["xyt"]], "before": [xyt_req(o) for o in xo["before"]]}
            # the rebuild write of the extracted file: the client's batch (MAC, complements), then the server's (both networks over U)
            prf3 = torch.randint(0, 256, (16 * (3 * n + 1),), dtype=torch.uint8, device="cuda", generator=gen)
            rb = [dict(mac=full(64), comp=full(128 * n), u_macs=half[0][1].clone(),
                       **{f: full(2 * n * (64 * NCOLS if f.startswith("data") else 64)) for f in ("data_x", "data_y", "mac_x", "mac_y", "align_x", "align_y")})
                  for _ in range(k)]
            block1 = blk[:bb].clone()                                       # the block the rebuild write itself carries (index 1)
            cr_reqs = [(block1.data_ptr(), prf3.data_ptr(), r["mac"].data_ptr(), r["comp"].data_ptr(), top_step) for r in rb]
            sr_reqs = [(block1.data_ptr(), r["mac"].data_ptr(), r["comp"].data_ptr(), o["blocks"].data_ptr(), r["u_macs"].data_ptr(),
                        r["data_x"].data_ptr(), r["data_y"].data_ptr(), r["mac_x"].data_ptr(), r["mac_y"].data_ptr(), r["align_x"].data_ptr(),
                        r["align_y"].data_ptr(), top_step, 1) for o, r in zip(xo["before"], rb)]

            def before():
                extract_xyt(reqs["before"], n)
                client_rebuild(cr_reqs, n)
                icc.server_rebuild_batch_device(sr_reqs, n, NCOLS, curve, stream.cuda_stream)

            def damage():
                for o in hurt:
                    o["rows_x"].copy_(damaged)
                torch.cuda.synchronize()

            legs = {"clean": lambda: repair(reqs["clean"], n), "one_x": lambda: repair(reqs["one_x"], n),
                    "xyt": lambda: extract_xyt(reqs["xyt"], n), "before": before}
            torch.cuda.synchronize()
            for fn in legs.values():                                        # tables, workspaces
                fn()
            stream.synchronize()
            times = {name: [] for name in legs}
            names = list(legs)
            for r in range(args.reps):
                for name in names[r % len(names):] + names[:r % len(names)]:
                    if name == "one_x":
                        damage()
                    times[name].append(event_ms(stream, legs[name]))
                    if name == "one_x":
                        stream.synchronize()
                        for o in hurt:
                            assert int((o["status_x"] == 0).sum()) == 1 and int(o["status_x"][5 % n]) == 0, "one_x: the damaged row's status"
                            assert int(o["action_x"][5 % n]) == DATA and int(o["action_x"].sum()) == DATA, "one_x: the action"
                            assert o["counts"].tolist() == [1, 0, 1, 0, 0, 0, 0, 0], "one_x: counters %s" % o["counts"].tolist()
            stream.synchronize()
            torch.cuda.synchronize()
            # every output byte
            pristine = dict(rows_x=half[0][0], macs_x=half[0][1], rows_y=half[1][0], macs_y=half[1][1])
            for j in range(k):
                c, h, x = clean[j], hurt[j], xo["xyt"][j]
                for name, want in pristine.items():
                    assert torch.equal(c[name], want), "clean: %s was written" % name
                    assert torch.equal(h[name], want), "one_x: %s is not the pristine store" % name
                assert bool((c["status_x"] == 1).all()) and bool((c["status_y"] == 1).all()), "clean: a status is not 1"
                assert not bool(c["action_x"].any()) and not bool(c["action_y"].any()) and c["counts"].tolist() == [0] * 8, "clean: actions, counters"
                assert bool((h["status_y"] == 1).all()) and not bool(h["action_y"].any()), "one_x: the Y half"
                assert torch.equal(x["patch"], half[0][0]) and x["counts"].tolist() == [1, 0, 0, 0, 0, 0, 0, 1], "xyt: the patched half"
            med = {name: statistics.median(v) for name, v in times.items()}
            faster = med["one_x"] <= med["before"]
            ok = ok and faster
            rec = {"build": "kzg" if curve == "bn254" else "ipa", "curve": curve, "k": k, "n_total": n, "n_cols": NCOLS, "form": "exact",
                   "reps": args.reps, "top_step": top_step}
            for name in names:
                rec[name + "_ms"] = round(med[name], 4)
                rec[name + "_ms_min_max"] = [round(min(times[name]), 4), round(max(times[name]), 4)]
            rec.update({"one_x_over_clean": round(med["one_x"] / med["clean"], 4), "one_x_over_xyt": round(med["one_x"] / med["xyt"], 4),
                        "one_x_over_before": round(med["one_x"] / med["before"], 4), "one_x_not_slower_than_before": faster,
                        "outputs_checked": True})
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
            del clean, hurt, xo, reqs, rb, half, damaged, blk
    if out:
        out.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
