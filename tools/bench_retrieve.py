#!/usr/bin/env python3
"""The verified retrieval (porla_{kzg,ipa}_retrieve_batch_device) beside what it replaces, same level, same run.

For (K, n_rows) in {(1, 2^15), (8, 2^15), (64, 2^10)} x 128 columns, per build (KZG on BN254, IPA on secp256k1), K levels are built by
the device encodes (porla_icc_encode_device, porla_icc_mac_encode_device, X half) from random blocks whose MACs carry the hiding scalars
u = (inverse Z_q network)(s), so that MAC row j hides exactly the 128-bit value s_j.  Timed on that level, each as ONE window of device
events on a stream of its own, alternating, `--reps` times after a warm-up, medians reported:
  retrieve        this call with d_out (check + EXACT decode)
  check           this call with d_out = NULL
  decode          porla_icc_decode_batch_device (EXACT) alone
  mac_decode      porla_icc_mac_decode_batch_device alone
  four_call       today's documented sequence: data decode, MAC decode, the byte flip of the decoded chunks, the block MACs of the
                  decoded chunks (KZG: porla_kzg_mac_batch_device; IPA, which has no block-MAC call: one fixed-base commit over the 128
                  alpha generators and h), the comparison of the two point arrays
Checked: every status is 1 and both counters are 0, d_out equals the input blocks, and the four-call sequence's recomputed MACs equal
the decoded ones.  The comparison that matters is check against mac_decode.  One JSON line per (build, K, n_rows).

    python tools/bench_retrieve.py [--out profiles/r21_a_retrieve.jsonl] [--reps 7] [--shapes 15:1,15:8,10:64]
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

NCOLS = 128
TAU = bytes.fromhex("ffeeddccbbaa99887766554433221100")
ALPHA = bytes.fromhex("00112233445566778899aabbccddeeff")
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


def inverse_network(s, curve):
    """the inverse of the MAC network on scalars mod q (tests/retrieve_model.py: zq_network(inverse=True)) with the twiddles' inverses
    from one table: (w^e mod p_icc) mod q for e < n by a running product, inverted together (Montgomery's trick)"""
    import icc_py
    n, q, p = len(s), icc_py.Q[curve], icc_py.P_ICC
    w = icc_py.root_w(n)
    tw, x = [], 1
    for _ in range(n):
        tw.append(x % q)
        x = x * w % p
    pre, acc = [], 1
    for t in tw:
        pre.append(acc)
        acc = acc * t % q
    inv_all, inv = pow(acc, -1, q), [0] * n
    for e in range(n - 1, -1, -1):
        inv[e] = inv_all * pre[e] % q
        inv_all = inv_all * tw[e] % q
    half = pow(2, -1, q)
    x = list(s)
    for st in range(n.bit_length() - 1, 0, -1):
        m, m2 = 1 << st, 1 << (st - 1)
        for j in range(m2):
            f = half * inv[j * (n // m2)] % q                                  # (2 v^j)^-1, v^j = w^(j n / m2)
            for k in range(j, n, m):
                a, b = x[k], x[k + m2]
                x[k], x[k + m2] = (a + b) * half % q, (a - b) * f % q
    return x


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
    assert torch.cuda.is_available(), "bench_retrieve.py needs a GPU"
    out = open(args.out, "w") if args.out else None
    stream = torch.cuda.Stream()
    for curve in args.curves.split(","):
        g = GEN[curve]
        if curve == "bn254":
            mx.init_key(TAU, ALPHA)
            mx.init_SRS(NCOLS)
            afb = hfb = both = None
        else:
            # 128 alpha generators and h: random multiples of the generator, made on the device
            gfb = mx.FixedBase(curve, g[0].to_bytes(32, "big") + g[1].to_bytes(32, "big"), 1, window_bits=8)
            gen = torch.Generator(device="cuda")
            gen.manual_seed(77)
            sc = torch.randint(0, 256, ((NCOLS + 1) * 32,), dtype=torch.uint8, device="cuda", generator=gen)
            pts = torch.empty((NCOLS + 1) * 64, dtype=torch.uint8, device="cuda")
            gfb.commit_device(sc.data_ptr(), NCOLS + 1, 1, pts.data_ptr())
            torch.cuda.synchronize()
            pts = bytes(pts.cpu().numpy())
            afb = mx.FixedBase(curve, pts[:64 * NCOLS], NCOLS)
            hfb = mx.FixedBase(curve, pts[64 * NCOLS:], 1)
            both = mx.FixedBase(curve, pts, NCOLS + 1)

        def block_macs(chunks_le, scalars32, n, d_out, s=0):
            """alpha Commit(block_i) + scalar_i h for n blocks: little-endian chunks -> the commitment's big-endian rows (the byte flip)"""
            rows_be = chunks_le.reshape(-1, 32).flip(1).contiguous().reshape(-1)
            if curve == "bn254":
                mx.kzg_mac_batch_device(rows_be.data_ptr(), scalars32.data_ptr(), n, d_out.data_ptr(), s)
                return rows_be
            rows = torch.cat([rows_be.reshape(n, NCOLS * 32), scalars32.reshape(n, 32)], dim=1).contiguous().reshape(-1)
            both.commit_device(rows.data_ptr(), n, NCOLS + 1, d_out.data_ptr(), s)
            return rows

        def retrieve(reqs, n):
            if curve == "bn254":
                mx.kzg_retrieve_batch_device(reqs, n, n, stream.cuda_stream)
            else:
                afb.ipa_retrieve_batch_device(hfb, reqs, n, n, stream.cuda_stream)

        for shape in args.shapes.split(","):
            log, k = (int(x) for x in shape.split(":"))
            n = 1 << log
            rng = random.Random(1000 * k + log)
            s = [rng.getrandbits(128) for _ in range(n)]
            order = "big" if curve == "bn254" else "little"
            prf = torch.frombuffer(bytearray(b"".join(v.to_bytes(16, order) for v in s)), dtype=torch.uint8).cuda()
            hide = torch.frombuffer(bytearray(b"".join(v.to_bytes(32, "big") for v in inverse_network(s, curve))), dtype=torch.uint8).cuda()
            gen = torch.Generator(device="cuda")
            gen.manual_seed(1000 * k + log)
            u, x, mac_x = [], [], []
            for _ in range(k):
                blk = torch.randint(0, 256, (n * NCOLS * 32,), dtype=torch.uint8, device="cuda", generator=gen)
                macs = torch.empty(n * 64, dtype=torch.uint8, device="cuda")
                block_macs(blk, hide, n, macs)
                xa = torch.empty(n * NCOLS * 64, dtype=torch.uint8, device="cuda")
                ma = torch.empty(n * 64, dtype=torch.uint8, device="cuda")
                icc.crebuild_device(blk.data_ptr(), n, NCOLS, curve, 0, 0, d_x=xa.data_ptr())
                icc.mac_crebuild_device(macs.data_ptr(), n, curve, 0, 0, ma.data_ptr())
                torch.cuda.synchronize()
                u.append(blk); x.append(xa); mac_x.append(ma)
                del macs
            back = [torch.full((n * NCOLS * 32,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(k)]
            status = [torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(k)]
            status2 = [torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(k)]
            counts = [torch.full((2,), -1, dtype=torch.int32, device="cuda") for _ in range(k)]
            counts2 = [torch.full((2,), -1, dtype=torch.int32, device="cuda") for _ in range(k)]
            dec_macs = [torch.full((n * 64,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(k)]
            re_macs = torch.empty(n * 64, dtype=torch.uint8, device="cuda")
            bad = torch.zeros(k, dtype=torch.int32, device="cuda")
            ok4 = torch.zeros(k, dtype=torch.bool, device="cuda")
            full = [(x[a].data_ptr(), mac_x[a].data_ptr(), prf.data_ptr(), back[a].data_ptr(), status[a].data_ptr(), counts[a].data_ptr()) for a in range(k)]
            chk = [(x[a].data_ptr(), mac_x[a].data_ptr(), prf.data_ptr(), 0, status2[a].data_ptr(), counts2[a].data_ptr()) for a in range(k)]
            dreq = [(x[a].data_ptr(), back[a].data_ptr(), 0, bad[a:].data_ptr()) for a in range(k)]
            mreq = [(mac_x[a].data_ptr(), dec_macs[a].data_ptr(), 0, 0) for a in range(k)]
            torch.cuda.synchronize()

            def decode():
                icc.decode_batch_device(dreq, n, NCOLS, n, curve, "exact", stream.cuda_stream)

            def mac_decode():
                icc.mac_decode_batch_device(mreq, n, n, curve, stream.cuda_stream)

            def four_call():
                decode()
                mac_decode()
                with torch.cuda.stream(stream):
                    for a in range(k):
                        block_macs(back[a], hide, n, re_macs, stream.cuda_stream)
                        ok4[a] = (re_macs == dec_macs[a]).all()

            legs = {"retrieve": lambda: retrieve(full, n), "check": lambda: retrieve(chk, n), "decode": decode, "mac_decode": mac_decode,
                    "four_call": four_call}
            for fn in legs.values():                                              # tables, workspaces
                fn()
            stream.synchronize()
            times = {name: [] for name in legs}
            for _ in range(args.reps):
                for name, fn in legs.items():
                    times[name].append(event_ms(stream, fn))
            # the last writer of `back` is the four-call sequence's decode: run the call once more so that the check below is its own
            for b in back:
                b.fill_(0xA5)
            torch.cuda.synchronize()
            retrieve(full, n)
            stream.synchronize()
            torch.cuda.synchronize()
            for a in range(k):
                assert bool((status[a] == 1).all()) and bool((status2[a] == 1).all()), "request %d: a status is not 1" % a
                assert counts[a].tolist() == [0, 0] and counts2[a].tolist() == [0, 0], "request %d: counters" % a
                assert torch.equal(back[a], u[a]), "request %d: d_out is not the input blocks" % a
            assert bool(ok4.all()) and bad.tolist() == [0] * k, "the four-call sequence did not verify"
            med = {name: statistics.median(t) for name, t in times.items()}
            rec = {"build": "kzg" if curve == "bn254" else "ipa", "curve": curve, "k": k, "n_rows": n, "n_cols": NCOLS, "reps": args.reps}
            rec.update({name + "_ms": round(v, 4) for name, v in med.items()})
            rec.update({"check_over_mac_decode": round(med["check"] / med["mac_decode"], 3),
                        "retrieve_over_four_call": round(med["retrieve"] / med["four_call"], 3),
                        "check_ms_min_max": [round(min(times["check"]), 4), round(max(times["check"]), 4)],
                        "mac_decode_ms_min_max": [round(min(times["mac_decode"]), 4), round(max(times["mac_decode"]), 4)],
                        "symbol_gb_per_s_check": round(k * n * NCOLS * 64 / med["check"] / 1e6, 1), "outputs_checked": True})
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
            del u, x, mac_x, back, dec_macs
    if out:
        out.close()


if __name__ == "__main__":
    main()
