#!/usr/bin/env python3
"""Batched server update against the device-resident composition of the single-step entry points, same K writes.

  batch     one porla_kzg_update_batch_device / porla_ipa_update_batch_device call for the K files
  baseline  per file: HAdd through the host wrapper (porla_kzg_hadd_host; IPA: porla_icc_hadd_host, porla_icc_mac_scale_host and the
            generators' fixed base) and an upload of its six rows, then per step porla_server_mix_device for the X and for the Y part,
            device-to-device copies for the close, and the complements by host point adds

n_total = 2^15, K in {1, 8, 64}, two shapes: every file at write step s, averaged over s = 1 .. 64 (the ruler sequence of levels a
real log follows), and every file at level 10.  One JSON line per (scheme, shape, K); updates/s of both and their ratio.

    python tools/bench_update_batch.py [--out profiles/r11_a_update_batch.jsonl] [--reps 3] [--ks 1,8,64]
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
N_TOTAL, NCOLS = 1 << 15, 128
FAMS = ("data_x", "data_y", "mac_x", "mac_y", "align_x", "align_y")
TAU = bytes.fromhex("ffeeddccbbaa99887766554433221100")
ALPHA = bytes.fromhex("00112233445566778899aabbccddeeff")


def level_of(step):
    """the level write `step` of a fresh log lands on: the number of trailing one bits of step - 1"""
    lv, s = 0, step - 1
    while s & 1:
        lv, s = lv + 1, s >> 1
    return lv


class Files:
    """K files with levels 0 .. top allocated and filled with valid content (random symbols below LCM are not needed for timing: the
    kernels' work does not depend on the values; points must be on the curve)"""

    def __init__(self, k, top, curve, points):
        import torch
        self.k, self.curve = k, curve
        rnd = random.Random(k)
        self.t = []
        for _ in range(k):
            f = {}
            for name in FAMS:
                if name.startswith("data"):
                    f[name] = [torch.randint(0, 128, ((2 << i) * NCOLS * 64,), dtype=torch.uint8, device="cuda") for i in range(top + 1)]
                    for t in f[name]:
                        t.view(-1, 64)[:, 60:] = 0                      # < 2^480 < LCM
                else:
                    f[name] = [torch.frombuffer(bytearray(b"".join(rnd.choice(points) for _ in range(2 << i))), dtype=torch.uint8).cuda()
                               for i in range(top + 1)]
            self.t.append(f)
        self.block = [torch.randint(0, 256, (NCOLS * 32,), dtype=torch.uint8, device="cuda") for _ in range(k)]
        self.block_host = [bytes(b.cpu().numpy()) for b in self.block]
        self.mac_host = [rnd.choice(points) for _ in range(k)]
        self.mac = [torch.frombuffer(bytearray(m), dtype=torch.uint8).cuda() for m in self.mac_host]
        self.comp_host = [[rnd.choice(points) for _ in range(2 << top)] for _ in range(k)]
        self.comp = [torch.frombuffer(bytearray(b"".join(c)), dtype=torch.uint8).cuda() for c in self.comp_host]

    def reqs(self, step, level):
        return [(self.block[a].data_ptr(), self.mac[a].data_ptr(), self.comp[a].data_ptr(), step, level) +
                tuple([t.data_ptr() for t in self.t[a][f][:level + 1]] for f in FAMS) for a in range(self.k)]


def baseline(F, step, level, fb):
    """the parent's entry points, levels resident on the device"""
    import torch
    from porla_amd import icc, lib
    import ctypes
    import icc_py
    from tests.update_model import pt_bytes, pt_tuple
    vp = ctypes.c_void_p
    cid = icc.CURVE[F.curve]
    s = torch.cuda.current_stream().cuda_stream
    for a in range(F.k):
        if F.curve == "bn254":
            b2, m2, ma = icc.kzg_hadd_host(F.block_host[a], F.mac_host[a], N_TOTAL, step)
        else:
            b2, sc, _ = icc.hadd_host(F.block_host[a], N_TOTAL, step, F.curve)
            m2 = icc.mac_scale_host(F.mac_host[a], N_TOTAL, step, F.curve)
            ma = fb.commit_host(sc, 1, NCOLS)
        rows = {"data_x": b"".join(F.block_host[a][32 * i:32 * i + 32] + bytes(32) for i in range(NCOLS)),
                "data_y": b"".join(b2[32 * i:32 * i + 32] + bytes(32) for i in range(NCOLS)),
                "mac_x": F.mac_host[a], "mac_y": m2, "align_x": bytes(64), "align_y": ma}
        slot = 1 if level else 0
        for f in FAMS:
            t = F.t[a][f][0]
            r = len(rows[f])
            t[slot * r:(slot + 1) * r].copy_(torch.frombuffer(bytearray(rows[f]), dtype=torch.uint8), non_blocking=True)
        for i in range(level):
            ln = 1 << i
            for part in ("x", "y"):
                d, m, al = F.t[a]["data_" + part], F.t[a]["mac_" + part], F.t[a]["align_" + part]
                rc = lib.porla_server_mix_device(vp(d[i].data_ptr()), vp(d[i].data_ptr() + ln * NCOLS * 64), vp(m[i].data_ptr()),
                                                 vp(m[i].data_ptr() + ln * 64), vp(al[i].data_ptr()), vp(al[i].data_ptr() + ln * 64), ln, NCOLS,
                                                 N_TOTAL, cid, vp(d[i + 1].data_ptr() + 2 * ln * NCOLS * 64), vp(m[i + 1].data_ptr() + 2 * ln * 64),
                                                 vp(al[i + 1].data_ptr() + 2 * ln * 64), vp(s))
                assert rc == 0
        top = 1 << level
        if level:
            for f in FAMS:
                t = F.t[a][f][level]
                half = t.numel() // 2
                t[:half].copy_(t[half:])
        # the complements: host point adds on the resident MAC halves (there is no entry point for them)
        for part, off in (("mac_x", 0), ("mac_y", top)):
            t = F.t[a][part][level]
            cur = bytes(t[:64 * top].cpu().numpy())
            out = b"".join(pt_bytes(icc_py.ec_add(F.curve, pt_tuple(cur[64 * j:64 * j + 64]), pt_tuple(F.comp_host[a][off + j])))
                           for j in range(top))
            t[:64 * top].copy_(torch.frombuffer(bytearray(out), dtype=torch.uint8))
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
    ap.add_argument("--baseline-max-k", type=int, default=64)
    args = ap.parse_args()
    from porla_amd import icc, multiexp as mx
    from tests import common
    out = open(args.out, "w") if args.out else None
    for scheme in args.schemes.split(","):
        curve = "bn254" if scheme == "kzg" else "secp256k1"
        if scheme == "kzg":
            mx.init_key(TAU, ALPHA)
            mx.init_SRS_from_data(NCOLS, mx.init_SRS(NCOLS))
            raw, fb = common.synth_points(32), None
            call = lambda reqs: icc.kzg_update_batch_device(reqs, N_TOTAL, 0)
        else:
            pts = common.secp_bench_points(NCOLS + 32)
            fb = mx.FixedBase("secp256k1", pts[:64 * NCOLS], NCOLS, 11)
            raw = pts[64 * NCOLS:]
            call = lambda reqs: fb.ipa_update_batch_device(reqs, N_TOTAL, 0)
        points = [raw[64 * i:64 * i + 64] for i in range(32)]
        for k in [int(x) for x in args.ks.split(",")]:
            for shape in ("ruler_1_64", "level_10"):
                steps = list(range(1, 65)) if shape == "ruler_1_64" else [1 << 10]
                top = max(level_of(s) for s in steps)
                F = Files(k, top, curve, points)
                call(F.reqs(steps[-1], level_of(steps[-1])))                   # tables, workspaces
                t_batch = sum(timed(lambda: call(F.reqs(s, level_of(s))), args.reps) for s in steps)
                if k <= args.baseline_max_k:
                    baseline(F, steps[-1], level_of(steps[-1]), fb)
                    t_base = sum(timed(lambda: baseline(F, s, level_of(s), fb), 1 if shape == "level_10" and k > 8 else args.reps) for s in steps)
                else:
                    t_base = None
                n = k * len(steps)
                rec = {"scheme": scheme, "shape": shape, "k": k, "n_total": N_TOTAL, "updates": n, "batch_updates_per_s": n / t_batch,
                       "batch_ms_per_call": 1e3 * t_batch / len(steps),
                       "baseline_updates_per_s": n / t_base if t_base else None, "ratio": t_base / t_batch if t_base else None}
                line = json.dumps(rec)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()
                del F
    if out:
        out.close()


if __name__ == "__main__":
    main()
