#!/usr/bin/env python3
"""The client's rebuild write (Client::CRebuild's step) in one call against the composition a caller had before it, same K writes,
every output byte compared.

  batch     one porla_kzg_client_rebuild_batch_device / porla_ipa_client_rebuild_batch_device call for the K writes
  baseline  per write: the complements of all 3 * n_total + 1 PRF values in one porla_kzg_complement_batch_device (IPA:
            porla_fixed_base_commit_device on the hiding base); porla_icc_mac_encode_xy_device on the old ones; the MAC by
            porla_kzg_mac_batch_device (IPA: the alpha generators' fixed base and a host add); a download; the 2 * n_total differences
            by host point subtractions.  Timed in two parts: the device calls up to the download, and the host subtractions.

n_total in {2^10, 2^15}, K in {1, 8}.  One JSON line per (scheme, n_total, K); the new call's milliseconds, both parts of the
baseline, and the ratios against the device part alone and against the whole.

    python tools/bench_client_rebuild.py [--out profiles/r14_a_client_rebuild.jsonl] [--reps 3] [--ks 1,8] [--logs 10,15]
"""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
NCOLS = 128
TAU = bytes.fromhex("ffeeddccbbaa99887766554433221100")
ALPHA = bytes.fromhex("00112233445566778899aabbccddeeff")


def dev(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def host(t):
    return bytes(t.cpu().numpy())


class Writes:
    """K rebuild writes: blocks and PRF values on both sides, output buffers for the batch, host results of the baseline"""

    def __init__(self, k, n_total, seed):
        import torch
        rnd = random.Random(seed)
        self.k, self.n = k, n_total
        m = 3 * n_total + 1
        self.block_host = [rnd.randbytes(32 * NCOLS) for _ in range(k)]
        self.prf_host = [rnd.randbytes(16 * m) for _ in range(k)]
        self.block = [dev(b) for b in self.block_host]
        self.prf = [dev(p) for p in self.prf_host]
        self.mac = [torch.zeros(64, dtype=torch.uint8, device="cuda") for _ in range(k)]
        self.comp = [torch.zeros(128 * n_total, dtype=torch.uint8, device="cuda") for _ in range(k)]
        self.base_mac, self.base_comp = [None] * k, [None] * k

    def reqs(self, step):
        return [(self.block[a].data_ptr(), self.prf[a].data_ptr(), self.mac[a].data_ptr(), self.comp[a].data_ptr(), step + a)
                for a in range(self.k)]

    def check(self):
        for a in range(self.k):
            assert host(self.mac[a]) == self.base_mac[a], ("MAC", a)
            assert host(self.comp[a]) == self.base_comp[a], ("complements", a)


def baseline(W, step, scheme, afb, hfb):
    """returns (seconds in the device calls and the download, seconds in the host subtractions)"""
    import icc_py
    import torch
    from porla_amd import icc, multiexp as mx
    from tests.update_model import pt_bytes, pt_tuple
    curve = "bn254" if scheme == "kzg" else "secp256k1"
    n, m = W.n, 3 * W.n + 1
    t_dev = t_host = 0.0
    for a in range(W.k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        raw = W.prf_host[a]
        vals = [raw[16 * i:16 * i + 16] for i in range(m)]
        sc = dev(b"".join((v if scheme == "kzg" else v[::-1]).rjust(32, b"\0") for v in vals))
        rows = dev(b"".join(W.block_host[a][32 * i:32 * i + 32][::-1] for i in range(NCOLS)))
        d_pts = torch.empty(64 * m, dtype=torch.uint8, device="cuda")
        d_xy = torch.empty(128 * n, dtype=torch.uint8, device="cuda")
        d_mac = torch.empty(64, dtype=torch.uint8, device="cuda")
        if scheme == "kzg":
            mx.kzg_complement_batch_device(sc.data_ptr(), m, d_pts.data_ptr())
            mx.kzg_mac_batch_device(rows.data_ptr(), sc.data_ptr(), 1, d_mac.data_ptr())
        else:
            hfb.commit_device(sc.data_ptr(), m, 1, d_pts.data_ptr())
            afb.commit_device(rows.data_ptr(), 1, NCOLS, d_mac.data_ptr())
        icc.mac_crebuild_xy_device(d_pts.data_ptr() + 64, n, curve, step + a, d_xy.data_ptr(), d_xy.data_ptr() + 64 * n)
        pts, t, mac = host(d_pts), host(d_xy), host(d_mac)
        t1 = time.perf_counter()
        new = pts[64 * (n + 1):]
        if scheme == "kzg":
            out = [mx.bn254_add(new[64 * g:64 * g + 64], mx.bn254_neg(t[64 * g:64 * g + 64])) for g in range(2 * n)]
        else:
            mac = pt_bytes(icc_py.ec_add(curve, pt_tuple(mac), pt_tuple(pts[:64])))
            out = [pt_bytes(icc_py.ec_add(curve, pt_tuple(new[64 * g:64 * g + 64]), icc_py.ec_neg(curve, pt_tuple(t[64 * g:64 * g + 64]))))
                   for g in range(2 * n)]
        t2 = time.perf_counter()
        W.base_mac[a], W.base_comp[a] = mac, b"".join(out)
        t_dev += t1 - t0
        t_host += t2 - t1
    return t_dev, t_host


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
    ap.add_argument("--ks", default="1,8")
    ap.add_argument("--logs", default="10,15")
    ap.add_argument("--schemes", default="kzg,ipa")
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
            call = lambda reqs, n: mx.kzg_client_rebuild_batch_device(reqs, n, 0)
        else:
            pts = common.secp_bench_points(NCOLS + 1)
            gens = b"".join(pt_bytes(icc_py.ec_mul("secp256k1", pt_tuple(pts[64 * i:64 * i + 64]), 5)) for i in range(NCOLS))
            afb = mx.FixedBase("secp256k1", gens, NCOLS, 11)
            hfb = mx.FixedBase("secp256k1", pts[64 * NCOLS:], 1, 11)
            call = lambda reqs, n: afb.ipa_client_rebuild_batch_device(hfb, reqs, n, 0)
        for log in [int(x) for x in args.logs.split(",")]:
            n_total = 1 << log
            for k in [int(x) for x in args.ks.split(",")]:
                W = Writes(k, n_total, 1000 * k + log)
                step = 3 * n_total                                                # request a: step + a -- the first is the protocol's
                call(W.reqs(step), n_total)                                       # tables, workspaces
                t_batch = timed(lambda: call(W.reqs(step), n_total), args.reps)
                if k == 1:
                    baseline(W, step, scheme, afb, hfb)                           # its tables, per n_total
                t_dev, t_host = baseline(W, step, scheme, afb, hfb)
                W.check()
                rec = {"scheme": scheme, "n_total": n_total, "k": k, "batch_ms": 1e3 * t_batch, "baseline_device_ms": 1e3 * t_dev,
                       "baseline_host_sub_ms": 1e3 * t_host, "ratio_device_only": t_dev / t_batch,
                       "ratio_whole": (t_dev + t_host) / t_batch, "outputs_checked": True}
                line = json.dumps(rec)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()
                del W
    if out:
        out.close()


if __name__ == "__main__":
    main()
