#!/usr/bin/env python3
"""Batched client update against the composition a caller had before it, same K writes, every output byte compared.

  batch     one porla_kzg_client_update_batch_device / porla_ipa_client_update_batch_device call for the K writes
  baseline  per write: the complements of all its PRF values in one porla_kzg_complement_batch_device (IPA: porla_fixed_base_commit_device
            on the hiding base) and a download; the MAC by porla_kzg_mac_batch_device (IPA: the alpha generators' fixed base and a host
            add); wt * comp0 by porla_icc_mac_scale_host; HRebuildX / HRebuildY by porla_icc_mac_hrebuild_host; the differences by host
            point adds; the upload of the MAC and the 2 * 2^level points

n_total = 2^15, K in {1, 8, 64}, two shapes: every write at step s for s = 1 .. 64 (the ruler sequence of levels a real log follows),
and every write at level 10.  One JSON line per (scheme, shape, K); writes/s of both and their ratio.

    python tools/bench_client_update_batch.py [--out profiles/r13_a_client_update_batch.jsonl] [--reps 3] [--ks 1,8,64]
"""
import argparse
import ctypes
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
N_TOTAL, NCOLS = 1 << 15, 128
TAU = bytes.fromhex("ffeeddccbbaa99887766554433221100")
ALPHA = bytes.fromhex("00112233445566778899aabbccddeeff")


def level_of(step):
    return (step & -step).bit_length() - 1


def dev(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


class Writes:
    """K writes at one level: blocks and PRF values on both sides, output buffers for the batch and for the baseline"""

    def __init__(self, k, level, seed):
        import torch
        rnd = random.Random(seed)
        self.k, self.level = k, level
        n = (4 << level) - 1
        self.block_host = [bytes(rnd.getrandbits(8) for _ in range(32 * NCOLS)) for _ in range(k)]
        self.prf_host = [rnd.getrandbits(128 * n).to_bytes(16 * n, "big") for _ in range(k)]
        self.block = [dev(b) for b in self.block_host]
        self.prf = [dev(p) for p in self.prf_host]
        self.mac = [torch.zeros(64, dtype=torch.uint8, device="cuda") for _ in range(k)]
        self.comp = [torch.zeros(64 * (2 << level), dtype=torch.uint8, device="cuda") for _ in range(k)]
        self.base_mac = [torch.zeros(64, dtype=torch.uint8, device="cuda") for _ in range(k)]
        self.base_comp = [torch.zeros(64 * (2 << level), dtype=torch.uint8, device="cuda") for _ in range(k)]

    def reqs(self, step):
        return [(self.block[a].data_ptr(), self.prf[a].data_ptr(), self.mac[a].data_ptr(), self.comp[a].data_ptr(), step, self.level)
                for a in range(self.k)]

    def check(self):
        for a in range(self.k):
            assert bytes(self.mac[a].cpu().numpy()) == bytes(self.base_mac[a].cpu().numpy()), ("MAC", a)
            assert bytes(self.comp[a].cpu().numpy()) == bytes(self.base_comp[a].cpu().numpy()), ("complements", a)


def baseline(W, step, scheme, afb, hfb):
    import icc_py
    import torch
    from porla_amd import icc, multiexp as mx
    from tests.update_model import pt_bytes, pt_tuple
    curve = "bn254" if scheme == "kzg" else "secp256k1"
    level, top = W.level, 1 << W.level
    n = (4 << level) - 1
    for a in range(W.k):
        raw = W.prf_host[a]
        vals = [raw[16 * i:16 * i + 16] for i in range(n)]
        sc = dev(b"".join((v if scheme == "kzg" else v[::-1]).rjust(32, b"\0") for v in vals))
        d_pts = torch.empty(64 * n, dtype=torch.uint8, device="cuda")
        rows = dev(b"".join(W.block_host[a][32 * i:32 * i + 32][::-1] for i in range(NCOLS)))
        d_mac = torch.empty(64, dtype=torch.uint8, device="cuda")
        if scheme == "kzg":
            mx.kzg_complement_batch_device(sc.data_ptr(), n, d_pts.data_ptr())
            mx.kzg_mac_batch_device(rows.data_ptr(), sc.data_ptr(), 1, d_mac.data_ptr())
        else:
            hfb.commit_device(sc.data_ptr(), n, 1, d_pts.data_ptr())
            afb.commit_device(rows.data_ptr(), 1, NCOLS, d_mac.data_ptr())
        pts = bytes(d_pts.cpu().numpy())
        pt = lambda i: pts[64 * i:64 * i + 64]
        mac = bytes(d_mac.cpu().numpy())
        if scheme == "ipa":
            mac = pt_bytes(icc_py.ec_add(curve, pt_tuple(mac), pt_tuple(pt(0))))
        b2 = icc.mac_scale_host(pt(0), N_TOTAL, step, curve)
        out = []
        for part, b in ((0, pt(0)), (1, b2)):
            bufs, pos = [], 1
            for i in range(level + 1):
                buf = bytearray(64 * (2 << i))
                if i < level:
                    buf[:64 << i] = pts[64 * (pos + (part << i)):64 * (pos + (part << i) + (1 << i))]
                    pos += 2 << i
                bufs.append(buf)
            slot = 1 if level else 0
            bufs[0][64 * slot:64 * slot + 64] = b
            cb = [ctypes.create_string_buffer(bytes(x), len(x)) for x in bufs]
            if level:
                icc.mac_hrebuild_host(cb, level, N_TOTAL, curve)
            t = cb[level].raw[:64 * top]
            for j in range(top):
                new, tj = pt(2 * top - 1 + part * top + j), t[64 * j:64 * j + 64]
                if scheme == "kzg":
                    out.append(mx.bn254_add(new, mx.bn254_neg(tj)))
                else:
                    out.append(pt_bytes(icc_py.ec_add(curve, pt_tuple(new), icc_py.ec_neg(curve, pt_tuple(tj)))))
        W.base_mac[a].copy_(torch.frombuffer(bytearray(mac), dtype=torch.uint8))
        W.base_comp[a].copy_(torch.frombuffer(bytearray(b"".join(out)), dtype=torch.uint8))
    torch.cuda.synchronize()


def timed(fn, reps):
    import torch
    best = float("inf")
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ks", default="1,8,64")
    ap.add_argument("--schemes", default="kzg,ipa")
    ap.add_argument("--shapes", default="ruler_1_64,level_10")
    args = ap.parse_args()
    import icc_py
    from porla_amd import multiexp as mx
    from tests import common
    from tests.update_model import pt_bytes, pt_tuple
    out = open(args.out, "w") if args.out else None
    for scheme in args.schemes.split(","):
        afb = hfb = None
        if scheme == "kzg":
            mx.init_key(TAU, ALPHA)
            mx.init_SRS_from_data(NCOLS, mx.init_SRS(NCOLS))
            call = lambda reqs: mx.kzg_client_update_batch_device(reqs, N_TOTAL, 0)
        else:
            pts = common.secp_bench_points(NCOLS + 1)
            gens = b"".join(pt_bytes(icc_py.ec_mul("secp256k1", pt_tuple(pts[64 * i:64 * i + 64]), 5)) for i in range(NCOLS))
            afb = mx.FixedBase("secp256k1", gens, NCOLS, 11)
            hfb = mx.FixedBase("secp256k1", pts[64 * NCOLS:], 1, 11)
            call = lambda reqs: afb.ipa_client_update_batch_device(hfb, reqs, N_TOTAL, 0)
        for k in [int(x) for x in args.ks.split(",")]:
            for shape in args.shapes.split(","):
                steps = list(range(1, 65)) if shape == "ruler_1_64" else [1 << 10]
                t_batch = t_base = 0.0
                for lv in sorted({level_of(s) for s in steps}):
                    at = [s for s in steps if level_of(s) == lv]
                    W = Writes(k, lv, 1000 * k + lv)
                    call(W.reqs(at[0]))                                           # tables, workspaces
                    baseline(W, at[0], scheme, afb, hfb)
                    for s in at:                                                  # (the work of a step depends on its level alone)
                        t_batch += timed(lambda: call(W.reqs(s)), args.reps)
                        t_base += timed(lambda: baseline(W, s, scheme, afb, hfb), 1)
                        W.check()
                    del W
                n = k * len(steps)
                rec = {"scheme": scheme, "shape": shape, "k": k, "n_total": N_TOTAL, "writes": n, "batch_writes_per_s": n / t_batch,
                       "batch_ms_per_call": 1e3 * t_batch / len(steps), "baseline_writes_per_s": n / t_base, "ratio": t_base / t_batch,
                       "outputs_checked": True}
                line = json.dumps(rec)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()
    if out:
        out.close()


if __name__ == "__main__":
    main()
