#!/usr/bin/env python3
"""The file extraction with the Y halves (porla_{kzg,ipa}_extract_xy_batch_device) beside the call without them and beside what a
caller had before it, same stores, same run.

For (K, n_total) in {(1, 2^15), (64, 2^10)} x 128 columns, per build (KZG on BN254, IPA on secp256k1), one file with t = n_total - 1
(every lower level resident) and an exact top level, the X halves made as tools/bench_extract.py makes them.  The Y half of every lower
level is made as tools/bench_retrieve_aligned.py makes a residue half: random 64-byte symbols below 2^248, per row an alignment A_j =
a_j G and the MAC row E_j - alpha A_j -- every row of every Y half pays for the aligned compare's ladder, as the rows HAdd writes do.
Such a half checks clean and decodes (RESIDUE64, the blocks' write steps) to blocks that name no slot: the merge counts and drops them.
The K files of a call share the stores and have outputs of their own.  Timed, each as ONE window of device events on a stream of its
own, alternating (the order rotates from repeat to repeat), `--reps` times after a warm-up; medians and the spread are reported:
  a_parent   porla_*_extract_batch_device                                   } the same launches: a gap beyond the run-to-run spread
  a_xy0      the new call with y_levels = 0 and NULL Y pointers             } is a finding
  b_all      the new call with y_levels all ones on the clean file: a full scrub of both halves
  c_xy       the largest lower level damaged in one X symbol, the new call with only that level's bit
  c_parent   what a caller had before: porla_*_extract_batch_device on the damaged file plus ONE aligned retrieval (RESIDUE64, write
             steps, d_out) of that level's Y half; the merge of its blocks on the host is NOT counted
Checked, every output byte: a_xy0 against a_parent (d_work, d_blocks, d_steps, d_flags, d_row_status, four counters); b_all the same,
every Y status 1, the Y counters 0, the largest level's part of d_work_y against c_parent's retrieval; c_xy: the X statuses, d_steps and
d_blocks of c_parent's extraction, the level's Y statuses 1 and all others NOT_TRIED, its part of d_work_y against the retrieval, every
flag FOUND alone (the level is no longer failed: no UNSURE), counters [1, c_parent's bad symbols, 2^(log - 1), 0, 0, 0].  One JSON line
per (build, K, n_total).

    python tools/bench_extract_xy.py [--out profiles/r24_a_extract_xy.jsonl] [--reps 7] [--shapes 15:1,10:64]
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
NOT_TRIED = 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="15:1,10:64")
    ap.add_argument("--curves", default="bn254,secp256k1")
    args = ap.parse_args()
    import icc_py
    import torch
    from porla_amd import icc
    from porla_amd import multiexp as mx
    assert torch.cuda.is_available(), "bench_extract_xy.py needs a GPU"
    out = open(args.out, "w") if args.out else None
    stream = torch.cuda.Stream()
    dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    pb = lambda p: p[0].to_bytes(32, "big") + p[1].to_bytes(32, "big")
    bb = NCOLS * 32
    for curve in args.curves.split(","):
        g, q = GEN[curve], icc_py.Q[curve]
        gfb = mx.FixedBase(curve, pb(g), 1, window_bits=8)
        if curve == "bn254":
            mx.init_key(TAU, ALPHA)
            mx.init_SRS(NCOLS)
            afb = hfb = both = three = None
        else:
            gen = torch.Generator(device="cuda")
            gen.manual_seed(80)
            sc = torch.randint(0, 256, ((NCOLS + 1) * 32,), dtype=torch.uint8, device="cuda", generator=gen)
            pts = torch.empty((NCOLS + 1) * 64, dtype=torch.uint8, device="cuda")
            gfb.commit_device(sc.data_ptr(), NCOLS + 1, 1, pts.data_ptr())
            torch.cuda.synchronize()
            pts = bytes(pts.cpu().numpy())
            minus = icc_py.ec_neg(curve, icc_py.ec_mul(curve, g, IPA_ALPHA))
            afb = mx.FixedBase(curve, pts[:64 * NCOLS], NCOLS)
            hfb = mx.FixedBase(curve, pts[64 * NCOLS:], 1)
            both = mx.FixedBase(curve, pts, NCOLS + 1)
            three = mx.FixedBase(curve, pts + pb(minus), NCOLS + 2)

        def block_macs(chunks_le, scalars32, n, d_out):
            rows_be = chunks_le.reshape(-1, 32).flip(1).contiguous().reshape(-1)
            if curve == "bn254":
                mx.kzg_mac_batch_device(rows_be.data_ptr(), scalars32.data_ptr(), n, d_out.data_ptr())
            else:
                rows = torch.cat([rows_be.reshape(n, bb), scalars32.reshape(n, 32)], dim=1).contiguous().reshape(-1)
                both.commit_device(rows.data_ptr(), n, NCOLS + 1, d_out.data_ptr())
            torch.cuda.synchronize()

        def y_half(m, rng, gen):
            """(rows of 64-byte symbols, MAC rows E_j - alpha A_j, alignment rows A_j = a_j G, the PRF integers) of m rows"""
            lo = torch.randint(0, 256, (m * NCOLS, 32), dtype=torch.uint8, device="cuda", generator=gen)
            lo[:, 31] = 0                                                      # little-endian symbols below 2^248
            rows64 = torch.cat([lo, torch.zeros_like(lo)], dim=1).contiguous().reshape(-1)
            s = [rng.getrandbits(128) for _ in range(m)]
            a = [rng.getrandbits(128) for _ in range(m)]
            s32 = dev(b"".join(v.to_bytes(32, "big") for v in s))
            a32 = dev(b"".join(v.to_bytes(32, "big") for v in a))
            align = torch.empty(m * 64, dtype=torch.uint8, device="cuda")
            gfb.commit_device(a32.data_ptr(), m, 1, align.data_ptr())
            rows_be = lo.flip(1).reshape(m, bb).contiguous()
            macs = torch.empty(m * 64, dtype=torch.uint8, device="cuda")
            if curve == "bn254":
                # E_j - alpha a_j G1[0] is the MAC of the row with a_j taken off its constant coefficient (mod r)
                c0 = bytes(rows_be[:, :32].contiguous().reshape(-1).cpu().numpy())
                shifted = dev(b"".join(((int.from_bytes(c0[32 * j:32 * j + 32], "big") - a[j]) % q).to_bytes(32, "big") for j in range(m)))
                rows_be[:, :32] = shifted.reshape(m, 32)
                mx.kzg_mac_batch_device(rows_be.data_ptr(), s32.data_ptr(), m, macs.data_ptr())
            else:
                r3 = torch.cat([rows_be, s32.reshape(m, 32), a32.reshape(m, 32)], dim=1).contiguous()
                three.commit_device(r3.data_ptr(), m, NCOLS + 2, macs.data_ptr())
            torch.cuda.synchronize()
            return rows64, macs, align, s

        def aligned_y(reqs, n_rows, n):
            if curve == "bn254":
                mx.kzg_retrieve_aligned_batch_device(reqs, n_rows, n, "residue64", stream.cuda_stream)
            else:
                afb.ipa_retrieve_aligned_batch_device(hfb, IPA_ALPHA, reqs, n_rows, n, "residue64", stream.cuda_stream)

        def extract(reqs, n):
            if curve == "bn254":
                mx.kzg_extract_batch_device(reqs, n, "exact", stream.cuda_stream)
            else:
                afb.ipa_extract_batch_device(hfb, IPA_ALPHA, reqs, n, "exact", stream.cuda_stream)

        def extract_xy(reqs, n):
            if curve == "bn254":
                mx.kzg_extract_xy_batch_device(reqs, n, "exact", stream.cuda_stream)
            else:
                afb.ipa_extract_xy_batch_device(hfb, IPA_ALPHA, reqs, n, "exact", stream.cuda_stream)

        for shape in args.shapes.split(","):
            log, k = (int(x) for x in shape.split(":"))
            n, t = 1 << log, (1 << log) - 1
            rng = random.Random(2400 * k + log)
            gen = torch.Generator(device="cuda")
            gen.manual_seed(2400 * k + log)
            order = "big" if curve == "bn254" else "little"
            # the X stores as tools/bench_extract.py makes them: level i (2^i rows) for i < log, then the top level (n rows)
            data, macs, prf_all = [], [], []
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
                del blk
            prf = dev(b"".join(v.to_bytes(16, order) for v in prf_all))
            # the Y stores of the lower levels
            ys = [y_half(1 << i, rng, gen) for i in range(log)]
            prf_y = dev(b"".join(v.to_bytes(16, order) for y in ys for v in y[3]))
            big = log - 1                                                   # the largest lower level: rows 2^big - 1 .. t - 1, steps 1 .. 2^big
            damaged = data[big].clone()
            damaged[64 * 5 + 1] ^= 1
            rows = t + n
            full = lambda size, dtype=torch.uint8: torch.full((size,), 0xA5 if dtype == torch.uint8 else -1, dtype=dtype, device="cuda")

            def outputs(y):
                o = dict(work=full(t * bb), blocks=full(n * bb), steps=full(n, torch.int32), flags=full(n), status=full(rows),
                         counts=full(6 if y is not None else 4, torch.int32))
                if y:
                    o.update(work_y=full(t * bb), status_y=full(t))
                return o

            def x_req(o, level_data):
                return (t, [d.data_ptr() for d in level_data], [m.data_ptr() for m in macs[:log]], data[log].data_ptr(), macs[log].data_ptr(), 0,
                        prf.data_ptr(), o["work"].data_ptr(), o["blocks"].data_ptr(), o["steps"].data_ptr(), o["flags"].data_ptr(),
                        o["status"].data_ptr(), o["counts"].data_ptr())

            def y_req(o, mask):
                if not mask:
                    return (None, None, None, 0, 0, 0, 0)
                return ([y[0].data_ptr() for y in ys], [y[1].data_ptr() for y in ys], [y[2].data_ptr() for y in ys], prf_y.data_ptr(),
                        o["work_y"].data_ptr(), o["status_y"].data_ptr(), mask)

            clean_x, bad_x = data[:log], data[:big] + [damaged]
            bufs = {"a_parent": [outputs(None) for _ in range(k)], "a_xy0": [outputs(False) for _ in range(k)],
                    "b_all": [outputs(True) for _ in range(k)], "c_xy": [outputs(True) for _ in range(k)],
                    "c_parent": [outputs(None) for _ in range(k)]}
            reqs = {"a_parent": [x_req(o, clean_x) for o in bufs["a_parent"]],
                    "a_xy0": [x_req(o, clean_x) + y_req(o, 0) for o in bufs["a_xy0"]],
                    "b_all": [x_req(o, clean_x) + y_req(o, (1 << 64) - 1) for o in bufs["b_all"]],
                    "c_xy": [x_req(o, bad_x) + y_req(o, 1 << big) for o in bufs["c_xy"]],
                    "c_parent": [x_req(o, bad_x) for o in bufs["c_parent"]]}
            m_big, off_big = 1 << big, (1 << big) - 1
            steps_big = torch.arange(1, m_big + 1, dtype=torch.int64, device="cuda")
            rt = [dict(out=full(m_big * bb), status=full(m_big), counts=full(2, torch.int32)) for _ in range(k)]
            rt_reqs = [(ys[big][0].data_ptr(), ys[big][1].data_ptr(), prf_y.data_ptr() + 16 * off_big, ys[big][2].data_ptr(), steps_big.data_ptr(),
                        r["out"].data_ptr(), r["status"].data_ptr(), r["counts"].data_ptr()) for r in rt]

            def c_parent():
                extract(reqs["c_parent"], n)
                aligned_y(rt_reqs, m_big, n)

            legs = {"a_parent": lambda: extract(reqs["a_parent"], n), "a_xy0": lambda: extract_xy(reqs["a_xy0"], n),
                    "b_all": lambda: extract_xy(reqs["b_all"], n), "c_xy": lambda: extract_xy(reqs["c_xy"], n), "c_parent": c_parent}
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
            lvl = slice(off_big, off_big + m_big)
            for j in range(k):
                p, a0, b, c, cp = (bufs[x][j] for x in ("a_parent", "a_xy0", "b_all", "c_xy", "c_parent"))
                r = rt[j]
                assert bool((p["status"] == 1).all()) and p["counts"].tolist() == [0, 0, 0, 0] and bool((p["flags"] == 1).all()), "the clean file"
                for name in same:
                    assert torch.equal(a0[name], p[name]), "a: %s differs from the call without Y halves" % name
                    assert torch.equal(b[name], p[name]), "b: %s differs from the call without Y halves" % name
                assert a0["counts"].tolist() == [0] * 6 and b["counts"].tolist() == [0] * 6, "a / b: counters"
                assert bool((b["status_y"] == 1).all()), "b: a Y status is not 1"
                assert bool((r["status"] == 1).all()) and r["counts"].tolist() == [0, 0], "the retrieval of the Y half"
                assert torch.equal(b["work_y"][off_big * bb:], r["out"]), "b: d_work_y differs from the retrieval's blocks"
                assert cp["counts"].tolist()[0] == 1 and int((cp["status"] == 0).sum()) == 1, "c: one damaged row"
                for name in ("status", "steps", "blocks"):
                    assert torch.equal(c[name], cp[name]), "c: %s differs from the extraction without Y halves" % name
                assert bool((c["status_y"][lvl] == 1).all()) and int((c["status_y"] == NOT_TRIED).sum()) == t - m_big, "c: the Y statuses"
                assert torch.equal(c["work_y"][off_big * bb:], r["out"]), "c: d_work_y differs from the retrieval's blocks"
                assert bool((c["flags"] == 1).all()) and bool((cp["flags"] & 2).any()), "c: the level is no longer failed"
                # (the damaged symbol's column decodes to symbols that are no chunks: the exact decode counts them in either call)
                assert c["counts"].tolist() == [1, cp["counts"].tolist()[1], m_big, 0, 0, 0], "c: counters %s" % c["counts"].tolist()
            med = {name: statistics.median(v) for name, v in times.items()}
            rec = {"build": "kzg" if curve == "bn254" else "ipa", "curve": curve, "k": k, "n_total": n, "t": t, "n_cols": NCOLS, "reps": args.reps}
            for name in names:
                rec[name + "_ms"] = round(med[name], 4)
                rec[name + "_ms_min_max"] = [round(min(times[name]), 4), round(max(times[name]), 4)]
            rec.update({"a_xy0_over_a_parent": round(med["a_xy0"] / med["a_parent"], 4), "b_all_over_a_parent": round(med["b_all"] / med["a_parent"], 4),
                        "c_xy_over_c_parent": round(med["c_xy"] / med["c_parent"], 4), "damaged_level_rows": m_big,
                        "c_parent_has_no_merge_of_the_y_blocks": True, "outputs_checked": True})
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
            del bufs, reqs, rt, data, macs, ys, damaged
    if out:
        out.close()


if __name__ == "__main__":
    main()
