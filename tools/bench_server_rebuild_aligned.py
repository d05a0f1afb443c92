#!/usr/bin/env python3
"""The server's rebuild write in the CRebuild_No_Cached form (rows mod p_icc, an alignment commitment per row) in one call against
what a caller had before it, same K files, every output byte compared.

  batch     one porla_kzg_server_rebuild_aligned_batch_device / porla_ipa_server_rebuild_aligned_batch_device call for the K files
  baseline  per file, one after the other: device copies of the block into U and of the MAC into MAC_U; then
              KZG  porla_kzg_crebuild_stage_device (both parts' encode, alignment scalars and commitments, the MAC network beside
                   them on its side stream) straight into the resident halves;
              IPA  porla_icc_encode_xy_device (rows mod p_icc and scalars of both parts) + porla_fixed_base_commit_device on the 2 n
                   rows of scalars + porla_icc_mac_encode_xy_device;
            then the complement adds.  No existing device entry point adds two arrays of points, so the cheapest existing route for the
            2 * n_total adds is a download, host point additions (the library's bn254_add; Python for secp256k1) and an upload.  Timed
            in two parts: the device calls, and the complement adds with their transfers (a column of its own).

K in {1, 8, 64} at n_total = 2^10, K in {1, 8} at n_total = 2^15, both curves, 128 columns.  One JSON line per (curve, n_total, K): the
new call's milliseconds, both parts of the baseline, and the ratios against the device part alone and against the whole.

    python tools/bench_server_rebuild_aligned.py [--out profiles/r16_a_server_rebuild_aligned.jsonl] [--reps 3]
                                                 [--shapes 10:1,10:8,10:64,15:1,15:8] [--curves bn254,secp256k1]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
NCOLS = 128
FAMILIES = ("data_x", "data_y", "mac_x", "mac_y", "align_x", "align_y")
TAU = bytes.fromhex("ffeeddccbbaa99887766554433221100")
ALPHA = bytes.fromhex("00112233445566778899aabbccddeeff")


def host(t):
    return bytes(t.cpu().numpy())


class Files:
    """K files on the device, twice (one set per side): the stores before the write, the top level of the six families (data rows: 32
    bytes a symbol), the write"""

    def __init__(self, k, n_total, curve, seed):
        import torch
        from tests import common
        self.k, self.n, self.curve = k, n_total, curve
        gen = torch.Generator(device="cuda")
        gen.manual_seed(seed)
        pts = common.synth_points(40) if curve == "bn254" else common.secp_bench_points(40)
        table = torch.frombuffer(bytearray(pts + bytes(64)), dtype=torch.uint8).cuda().view(41, 64)      # entry 40: infinity
        rand = lambda nbytes: torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda", generator=gen)
        draw = lambda cnt: table[torch.randint(0, 41, (cnt,), device="cuda", generator=gen)].reshape(-1).contiguous()
        self.block = [rand(32 * NCOLS) for _ in range(k)]
        self.mac = [draw(1) for _ in range(k)]
        self.comp = [draw(2 * n_total) for _ in range(k)]
        self.index = [1 + (a * 37) % n_total for a in range(k)]
        u, um = [rand(32 * NCOLS * n_total) for _ in range(k)], [draw(n_total) for _ in range(k)]
        self.sides = []
        for _ in range(2):
            side = {"u_blocks": [t.clone() for t in u], "u_macs": [t.clone() for t in um]}
            for f in FAMILIES:
                size = 2 * n_total * (32 * NCOLS if f.startswith("data") else 64)
                side[f] = [torch.full((size,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(k)]
            self.sides.append(side)
        # the single-file calls' scratch: both parts' scalars and commitments of one file
        self.scalars = torch.empty(2 * n_total * NCOLS * 32, dtype=torch.uint8, device="cuda")
        self.commits = torch.empty(2 * n_total * 64, dtype=torch.uint8, device="cuda")

    def reqs(self, step):
        s = self.sides[0]
        return [(self.block[a].data_ptr(), self.mac[a].data_ptr(), self.comp[a].data_ptr(), s["u_blocks"][a].data_ptr(),
                 s["u_macs"][a].data_ptr()) + tuple(s[f][a].data_ptr() for f in FAMILIES) + (step + a, self.index[a])
                for a in range(self.k)]

    def check(self):
        import torch
        for f in FAMILIES + ("u_blocks", "u_macs"):
            for a in range(self.k):
                assert torch.equal(self.sides[0][f][a], self.sides[1][f][a]), (f, a)


def baseline(F, fb, step):
    """returns (seconds in the device calls, seconds in the complement adds with their transfers)"""
    import icc_py
    import torch
    from porla_amd import icc, multiexp as mx
    from tests.update_model import pt_bytes, pt_tuple
    s, n, curve = F.sides[1], F.n, F.curve
    t_dev = t_add = 0.0
    for a in range(F.k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        i = F.index[a] - 1
        s["u_blocks"][a][i * 32 * NCOLS:(i + 1) * 32 * NCOLS].copy_(F.block[a])
        s["u_macs"][a][64 * i:64 * i + 64].copy_(F.mac[a])
        if curve == "bn254":
            icc.kzg_crebuild_stage_device(s["u_blocks"][a].data_ptr(), n, step + a, s["data_x"][a].data_ptr(), s["data_y"][a].data_ptr(),
                                          F.scalars.data_ptr(), F.commits.data_ptr(), s["u_macs"][a].data_ptr(), s["mac_x"][a].data_ptr(),
                                          s["mac_y"][a].data_ptr())
        else:
            icc.crebuild_xy_device(s["u_blocks"][a].data_ptr(), n, NCOLS, curve, step + a, d_aligned=s["data_x"][a].data_ptr(),
                                   d_scalars=F.scalars.data_ptr(), d_y_aligned=s["data_y"][a].data_ptr(),
                                   d_y_scalars=F.scalars.data_ptr() + n * NCOLS * 32)
            fb.commit_device(F.scalars.data_ptr(), 2 * n, NCOLS, F.commits.data_ptr())
            icc.mac_crebuild_xy_device(s["u_macs"][a].data_ptr(), n, curve, step + a, s["mac_x"][a].data_ptr(), s["mac_y"][a].data_ptr())
        s["align_x"][a][:64 * n].copy_(F.commits[:64 * n])
        s["align_y"][a][:64 * n].copy_(F.commits[64 * n:])
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        comp = host(F.comp[a])
        for part, f in enumerate(("mac_x", "mac_y")):
            cur = host(s[f][a][:64 * n])
            if curve == "bn254":
                out = [mx.bn254_add(cur[64 * j:64 * j + 64], comp[64 * (part * n + j):64 * (part * n + j) + 64]) for j in range(n)]
            else:
                out = [pt_bytes(icc_py.ec_add(curve, pt_tuple(cur[64 * j:64 * j + 64]), pt_tuple(comp[64 * (part * n + j):64 * (part * n + j) + 64])))
                       for j in range(n)]
            s[f][a][:64 * n].copy_(torch.frombuffer(bytearray(b"".join(out)), dtype=torch.uint8))
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        t_dev += t1 - t0
        t_add += t2 - t1
    return t_dev, t_add


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
    ap.add_argument("--shapes", default="10:1,10:8,10:64,15:1,15:8")
    ap.add_argument("--curves", default="bn254,secp256k1")
    args = ap.parse_args()
    from porla_amd import icc, multiexp as mx
    from tests import common
    out = open(args.out, "w") if args.out else None
    for curve in args.curves.split(","):
        fb = None
        if curve == "bn254":
            mx.init_key(TAU, ALPHA)
            mx.init_SRS_from_data(NCOLS, mx.init_SRS(NCOLS))
        else:
            fb = mx.FixedBase("secp256k1", common.secp_bench_points(NCOLS + 40)[:64 * NCOLS], NCOLS, 11)
        for shape in args.shapes.split(","):
            log, k = (int(x) for x in shape.split(":"))
            n_total = 1 << log
            F = Files(k, n_total, curve, 1000 * k + log)
            step = 3 * n_total                                                    # request a: step + a -- the first is the protocol's
            if curve == "bn254":
                call = lambda: icc.kzg_server_rebuild_aligned_batch_device(F.reqs(step), n_total, 0)
            else:
                call = lambda: fb.ipa_server_rebuild_aligned_batch_device(F.reqs(step), n_total, 0)
            call()                                                                # tables, workspaces (the call is idempotent on its stores)
            t_batch = timed(call, args.reps)
            if k == 1:
                baseline(F, fb, step)                                             # its tables, per n_total
            t_dev, t_add = baseline(F, fb, step)
            F.check()
            rec = {"curve": curve, "n_total": n_total, "k": k, "batch_ms": 1e3 * t_batch, "baseline_device_ms": 1e3 * t_dev,
                   "baseline_complement_adds_ms": 1e3 * t_add, "ratio_device_only": t_dev / t_batch,
                   "ratio_whole": (t_dev + t_add) / t_batch, "outputs_checked": True}
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
