#!/usr/bin/env python3
"""The aligned verified retrieval (porla_{kzg,ipa}_retrieve_aligned_batch_device) beside the exact call, same rows, same run.

For (K, n_rows) in {(1, 2^15), (64, 2^10)} x 128 columns, per build (KZG on BN254, IPA on secp256k1), two levels, all made on the device:
an EXACT half as tools/bench_retrieve.py builds it (the device encodes of random blocks whose MACs hide the PRF values), and a residue
half of random symbols below 2^248 (so a symbol is its own residue mod p_icc and mod q, in the 64-byte and in the 32-byte width) with,
per row, an alignment A_j = a_j G, a_j random 128 bits, and the MAC row E_j - alpha A_j = E_j - a_j (alpha G), made as one more
coefficient of the commitment that makes E_j.  Timed, each as ONE window of device events on a stream of its own, alternating (the order
rotates from repeat to repeat), `--reps` times after a warm-up, medians reported, check-only and with the decode:
  a   the exact call (porla_*_retrieve_batch_device) on the exact half
  b   the aligned call, form exact, d_align = NULL, same half                  (the launches of a)
  c   the aligned call, form exact, d_align = n_rows x 64 zero bytes           (the aligned compare's block skip)
  d   the aligned call, residue64, every alignment finite, on the residue half
  e   the same on its 32-byte rows, residue32
Checked: every status is 1 and both counters are 0 in every case; the blocks of a are the input blocks; status, blocks and counters of
b and c are byte for byte those of a; the blocks of d and e are the stand-alone decode's.  Two conditions are recorded, not asserted: b inside the run-to-run spread of a, and c
nearer to a than to d.  One JSON line per (build, K, n_rows).

    python tools/bench_retrieve_aligned.py [--out profiles/r22_a_retrieve_aligned.jsonl] [--reps 7] [--shapes 15:1,10:64]
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
    import icc_py
    import torch
    from porla_amd import icc
    from porla_amd import multiexp as mx
    assert torch.cuda.is_available(), "bench_retrieve_aligned.py needs a GPU"
    out = open(args.out, "w") if args.out else None
    stream = torch.cuda.Stream()
    dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    pb = lambda p: p[0].to_bytes(32, "big") + p[1].to_bytes(32, "big")
    for curve in args.curves.split(","):
        g, q = GEN[curve], icc_py.Q[curve]
        gfb = mx.FixedBase(curve, pb(g), 1, window_bits=8)
        if curve == "bn254":
            mx.init_key(TAU, ALPHA)
            mx.init_SRS(NCOLS)
            afb = hfb = both = three = None
        else:
            gen = torch.Generator(device="cuda")
            gen.manual_seed(78)
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

        def exact(reqs, n):
            if curve == "bn254":
                mx.kzg_retrieve_batch_device(reqs, n, n, stream.cuda_stream)
            else:
                afb.ipa_retrieve_batch_device(hfb, reqs, n, n, stream.cuda_stream)

        def aligned(reqs, n, form):
            if curve == "bn254":
                mx.kzg_retrieve_aligned_batch_device(reqs, n, n, form, stream.cuda_stream)
            else:
                afb.ipa_retrieve_aligned_batch_device(hfb, IPA_ALPHA, reqs, n, n, form, stream.cuda_stream)

        for shape in args.shapes.split(","):
            log, k = (int(x) for x in shape.split(":"))
            n = 1 << log
            rng = random.Random(2200 * k + log)
            gen = torch.Generator(device="cuda")
            gen.manual_seed(2200 * k + log)
            lo = torch.randint(0, 256, (n * NCOLS, 32), dtype=torch.uint8, device="cuda", generator=gen)
            lo[:, 31] = 0                                                          # little-endian symbols below 2^248
            rows32 = lo.reshape(-1).contiguous()
            rows64 = torch.cat([lo, torch.zeros_like(lo)], dim=1).contiguous().reshape(-1)
            s = [rng.getrandbits(128) for _ in range(n)]
            a = [rng.getrandbits(128) for _ in range(n)]
            order = "big" if curve == "bn254" else "little"
            prf = dev(b"".join(v.to_bytes(16, order) for v in s))
            s32 = dev(b"".join(v.to_bytes(32, "big") for v in s))
            a32 = dev(b"".join(v.to_bytes(32, "big") for v in a))
            align = torch.empty(n * 64, dtype=torch.uint8, device="cuda")
            gfb.commit_device(a32.data_ptr(), n, 1, align.data_ptr())              # A_j = a_j G
            rows_be = lo.flip(1).reshape(n, NCOLS * 32).contiguous()
            macs_e = torch.empty(n * 64, dtype=torch.uint8, device="cuda")
            macs_a = torch.empty(n * 64, dtype=torch.uint8, device="cuda")
            if curve == "bn254":
                # E_j - alpha a_j G1[0] is the MAC of the row with a_j taken off its constant coefficient (mod r)
                mx.kzg_mac_batch_device(rows_be.data_ptr(), s32.data_ptr(), n, macs_e.data_ptr())
                c0 = bytes(rows_be[:, :32].contiguous().reshape(-1).cpu().numpy())
                shifted = dev(b"".join(((int.from_bytes(c0[32 * j:32 * j + 32], "big") - a[j]) % q).to_bytes(32, "big") for j in range(n)))
                rows_sh = rows_be.clone()
                rows_sh[:, :32] = shifted.reshape(n, 32)
                mx.kzg_mac_batch_device(rows_sh.data_ptr(), s32.data_ptr(), n, macs_a.data_ptr())
                del rows_sh
            else:
                r2 = torch.cat([rows_be, s32.reshape(n, 32)], dim=1).contiguous()
                both.commit_device(r2.data_ptr(), n, NCOLS + 1, macs_e.data_ptr())
                r3 = torch.cat([r2, a32.reshape(n, 32)], dim=1).contiguous()
                three.commit_device(r3.data_ptr(), n, NCOLS + 2, macs_a.data_ptr())
                torch.cuda.synchronize()
                del r2, r3
            torch.cuda.synchronize()
            del rows_be, macs_e
            # the exact half: the X half of the device encodes of random blocks, MAC row j hiding exactly s_j
            hide = dev(b"".join(v.to_bytes(32, "big") for v in inverse_network(s, curve)))
            blk = torch.randint(0, 256, (n * NCOLS * 32,), dtype=torch.uint8, device="cuda", generator=gen)
            blk_be = blk.reshape(-1, 32).flip(1).reshape(n, NCOLS * 32).contiguous()
            blk_macs = torch.empty(n * 64, dtype=torch.uint8, device="cuda")
            if curve == "bn254":
                mx.kzg_mac_batch_device(blk_be.data_ptr(), hide.data_ptr(), n, blk_macs.data_ptr())
            else:
                r2 = torch.cat([blk_be, hide.reshape(n, 32)], dim=1).contiguous()
                both.commit_device(r2.data_ptr(), n, NCOLS + 1, blk_macs.data_ptr())
                torch.cuda.synchronize()
                del r2
            rows_x = torch.empty(n * NCOLS * 64, dtype=torch.uint8, device="cuda")
            macs_x = torch.empty(n * 64, dtype=torch.uint8, device="cuda")
            icc.crebuild_device(blk.data_ptr(), n, NCOLS, curve, 0, 0, d_x=rows_x.data_ptr())
            icc.mac_crebuild_device(blk_macs.data_ptr(), n, curve, 0, 0, macs_x.data_ptr())
            torch.cuda.synchronize()
            del blk_be, blk_macs
            zeros = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
            cases = {"a": (None, rows_x, macs_x, None), "b": ("exact", rows_x, macs_x, None), "c": ("exact", rows_x, macs_x, zeros),
                     "d": ("residue64", rows64, macs_a, align), "e": ("residue32", rows32, macs_a, align)}
            bufs, legs = {}, {}
            for name, (form, rows, macs, al) in cases.items():
                for full in (False, True):
                    back = [torch.full((n * NCOLS * 32,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(k)] if full else [None] * k
                    st = [torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(k)]
                    cn = [torch.full((2,), -1, dtype=torch.int32, device="cuda") for _ in range(k)]
                    ptr = lambda t: t.data_ptr() if t is not None else 0
                    if form is None:
                        reqs = [(rows.data_ptr(), macs.data_ptr(), prf.data_ptr(), ptr(back[i]), st[i].data_ptr(), cn[i].data_ptr()) for i in range(k)]
                        legs[name + ("_full" if full else "_check")] = (lambda reqs=reqs: exact(reqs, n))
                    else:
                        reqs = [(rows.data_ptr(), macs.data_ptr(), prf.data_ptr(), ptr(al), 0, ptr(back[i]), st[i].data_ptr(), cn[i].data_ptr())
                                for i in range(k)]
                        legs[name + ("_full" if full else "_check")] = (lambda reqs=reqs, form=form: aligned(reqs, n, form))
                    bufs[name, full] = (back, st, cn)
            torch.cuda.synchronize()
            for fn in legs.values():                                              # tables, workspaces
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
            ref = torch.full((n * NCOLS * 32,), 0xA5, dtype=torch.uint8, device="cuda")
            for name in cases:
                for full in (False, True):
                    back, st, cn = bufs[name, full]
                    if name in "de" and full:
                        form, rows = cases[name][0], cases[name][1]
                        icc.decode_batch_device([(rows.data_ptr(), ref.data_ptr(), 0, 0)], n, NCOLS, n, curve, form)
                        torch.cuda.synchronize()
                    for i in range(k):
                        assert bool((st[i] == 1).all()), "case %s request %d: a status is not 1" % (name, i)
                        assert cn[i].tolist() == [0, 0], "case %s request %d: counters" % (name, i)
                        assert not (name == "a" and full) or torch.equal(back[i], blk), "request %d: the exact call's blocks are not the input" % i
                        if name in "bc":
                            assert torch.equal(cn[i], bufs["a", full][2][i]), "case %s: counters differ from the exact call's" % name
                            assert not full or torch.equal(back[i], bufs["a", True][0][i]), "case %s: blocks differ from the exact call's" % name
                        if name in "de" and full:
                            assert torch.equal(back[i], ref), "case %s: blocks differ from the stand-alone decode's" % name
            assert torch.equal(bufs["d", True][0][0], bufs["e", True][0][0])     # (the same residues mod p_icc in both widths)
            med = {name: statistics.median(t) for name, t in times.items()}
            rec = {"build": "kzg" if curve == "bn254" else "ipa", "curve": curve, "k": k, "n_rows": n, "n_cols": NCOLS, "reps": args.reps}
            rec.update({name + "_ms": round(v, 4) for name, v in med.items()})
            for what in ("check", "full"):
                am, bm, cm, dm = (med[c + "_" + what] for c in "abcd")
                rec["a_%s_ms_min_max" % what] = [round(min(times["a_" + what]), 4), round(max(times["a_" + what]), 4)]
                rec["b_inside_a_spread_" + what] = min(times["a_" + what]) <= bm <= max(times["a_" + what])
                rec["c_nearer_a_than_d_" + what] = abs(cm - am) < abs(dm - cm)
                rec["d_minus_a_%s_ms" % what] = round(dm - am, 4)
                rec["e_minus_a_%s_ms" % what] = round(med["e_" + what] - am, 4)
            rec["outputs_checked"] = True
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
            del bufs, legs, rows64, rows32, lo, rows_x, macs_x, blk
    if out:
        out.close()


if __name__ == "__main__":
    main()
