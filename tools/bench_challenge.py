#!/usr/bin/env python3
"""AES on the device (porla_mac_prf_batch_device, porla_audit_challenge_batch_device, porla_audit_complement_scalar_batch_device),
timed with HIP events on the stream the calls are enqueued on; one JSON line per measurement.

  prf        one run of 2^16, 2^20, 2^22 PRF values: values/s and the bytes/s written
  rebuild    the d_prf of K rebuild writes (64 at n_total = 2^10, 8 at 2^15) in ONE call over the 3 K runs of porla_client_prf_runs,
             beside porla_kzg_client_rebuild_batch_device on those very buffers
  challenge  K = 64 challenges at num_blocks = 2^15, write_step = 2^15 - 1 (every level challenged), mixed forms
  scalar     K = 64 complement scalars at the same shape, beside porla_kzg_complement_batch_device over the 2^16 complements per audit
             that Client::audit recomputes (Client.hpp:639-654)

Every timed call is warmed up first and repeated inside one event pair; the outputs of the first and last repetition are compared
with the host forms on a sample.  Nothing of the parent commit does this work on the device, so no ratio is an acceptance figure.

    python tools/bench_challenge.py [--out profiles/r18_a_challenge.jsonl] [--reps 20]
"""
import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NCOLS = 128
TAU = bytes.fromhex("ffeeddccbbaa99887766554433221100")
KEY = bytes.fromhex("00112233445566778899aabbccddeeff")


def event_ms(fn, reps, stream):
    """milliseconds per call: calls between two events on `stream`, after two warm-up calls.  A first window of `reps` calls sizes
    the count so that a window lasts about a quarter of a second (at most 4000 calls); the median of three such windows is returned"""
    import torch

    def window(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(n):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / n
    for _ in range(2):
        fn()
    stream.synchronize()
    first = window(reps)
    n = max(reps, min(4000, int(250.0 / max(first, 1e-3))))
    return sorted(window(n) for _ in range(3))[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_challenge.py needs a GPU"
    from porla_amd import challenge as ch, multiexp as mx
    out = open(args.out, "w") if args.out else None
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    rnd = random.Random(18)

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    def sample_ok(d, runs, n):
        raw = bytes(d.cpu().numpy())
        for r0 in (0, n // 2, n - 64):
            lo = max(0, min(r0, n - 64))
            level, index0, _, time0, stride = runs[0]
            want = ch.mac_prf_host(KEY, [(level, index0 + lo, 64, time0 + lo * stride, stride)])
            if raw[16 * lo:16 * lo + 1024] != want:
                return False
        return True

    with torch.cuda.stream(stream):
        # ---- PRF throughput
        for log in (16, 20, 22):
            n = 1 << log
            d = torch.zeros(16 * n, dtype=torch.uint8, device="cuda")
            runs = [(3, 0, n, 1 << 33, 1)]
            ms = event_ms(lambda: ch.mac_prf_batch_device(KEY, runs, d.data_ptr(), stream=st), args.reps, stream)
            emit({"what": "prf", "values": n, "ms": ms, "values_per_s": n / (ms * 1e-3), "written_GBps": 16 * n / (ms * 1e-3) / 1e9,
                  "outputs_checked": sample_ok(d, runs, n)})
            del d

        # ---- the d_prf of K rebuild writes beside the write itself
        mx.init_key(TAU, KEY)
        mx.init_SRS_from_data(NCOLS, mx.init_SRS(NCOLS))
        for log, k in ((10, 64), (15, 8)):
            n_total = 1 << log
            m = 3 * n_total + 1
            runs = []
            for a in range(k):
                r, nv = ch.client_prf_runs("rebuild", 7 + a, 3 * n_total, n_total)
                assert nv == m
                runs += r
            d_prf = torch.zeros(16 * m * k, dtype=torch.uint8, device="cuda")
            blocks = [torch.frombuffer(bytearray(rnd.randbytes(32 * NCOLS)), dtype=torch.uint8).cuda() for _ in range(k)]
            macs = torch.zeros(64 * k, dtype=torch.uint8, device="cuda")
            comp = torch.zeros(128 * n_total * k, dtype=torch.uint8, device="cuda")
            reqs = [(blocks[a].data_ptr(), d_prf.data_ptr() + 16 * m * a, macs.data_ptr() + 64 * a, comp.data_ptr() + 128 * n_total * a,
                     3 * n_total) for a in range(k)]
            prf_ms = event_ms(lambda: ch.mac_prf_batch_device(KEY, runs, d_prf.data_ptr(), stream=st), args.reps, stream)
            write_ms = event_ms(lambda: mx.kzg_client_rebuild_batch_device(reqs, n_total, st), max(2, args.reps // 4), stream)
            both_ms = event_ms(lambda: (ch.mac_prf_batch_device(KEY, runs, d_prf.data_ptr(), stream=st),
                                        mx.kzg_client_rebuild_batch_device(reqs, n_total, st)), max(2, args.reps // 4), stream)
            raw = bytes(d_prf[:16 * m].cpu().numpy())
            emit({"what": "rebuild", "n_total": n_total, "k": k, "prf_values": m * k, "prf_ms": prf_ms, "client_rebuild_batch_ms": write_ms,
                  "prf_then_rebuild_ms": both_ms, "prf_share_of_write": prf_ms / write_ms,
                  "outputs_checked": raw == ch.mac_prf_host(KEY, runs[:3])})
            del d_prf, blocks, macs, comp

        # ---- K = 64 challenges and complement scalars
        k, nb, ws = 64, 1 << 15, (1 << 15) - 1
        levels = [(0, 1 << i, (2 << i) - 2, (2 << i) - 2 + (1 << i), 1 if i > 10 else 0) for i in range(16)]
        seeds = [rnd.randbytes(16) for _ in range(k)]
        plan = ch.audit_challenge_plan([(s, ws, nb, levels) for s in seeds])
        bufs, reqs = [], []
        for s, info in zip(seeds, plan):
            t = [torch.zeros(max(info[c], 1), dtype=torch.int64 if j % 2 == 0 else torch.int32, device="cuda")
                 for j, c in enumerate(("n64", "n64", "n32", "n32", "n_macs", "n_macs"))]
            bufs.append(t)
            reqs.append((s, ws, nb, levels, [x.data_ptr() for x in t]))
        ms = event_ms(lambda: ch.audit_challenge_batch_device(reqs, stream=st), args.reps, stream)
        _, want = ch.audit_challenge_host(seeds[-1], ws, nb, levels)
        got = [int(v) for v in bufs[-1][4].cpu().numpy().view("uint64")]
        emit({"what": "challenge", "k": k, "num_blocks": nb, "write_step": ws, "points_per_audit": plan[0]["n_macs"], "ms": ms,
              "outputs_checked": got == want["mac_idx"]})

        sreqs = [(s, ws, nb) for s in seeds]
        d_s = torch.zeros(32 * k, dtype=torch.uint8, device="cuda")
        ms = event_ms(lambda: ch.audit_complement_scalar_batch_device(KEY, sreqs, "bn254", d_s.data_ptr(), stream=st), args.reps, stream)
        raw = bytes(d_s.cpu().numpy())
        ok = [int.from_bytes(raw[32 * i:32 * i + 32], "big") for i in (0, k - 1)] == ch.audit_complement_scalar_host(KEY, [sreqs[0], sreqs[-1]], "bn254")
        d_p = torch.zeros(64 * k, dtype=torch.uint8, device="cuda")
        point_ms = event_ms(lambda: mx.kzg_complement_batch_device(d_s.data_ptr(), k, d_p.data_ptr(), stream=st), args.reps, stream)
        n_comp = k << 16
        d_sc = torch.zeros((n_comp, 32), dtype=torch.uint8, device="cuda")
        d_sc[:, 16:] = torch.randint(0, 256, (n_comp, 16), dtype=torch.uint8, device="cuda")
        d_c = torch.zeros(64 * n_comp, dtype=torch.uint8, device="cuda")
        store_ms = event_ms(lambda: mx.kzg_complement_batch_device(d_sc.data_ptr(), n_comp, d_c.data_ptr(), stream=st), 3, stream)
        emit({"what": "scalar", "k": k, "num_blocks": nb, "write_step": ws, "scalar_ms": ms, "one_point_per_audit_ms": point_ms,
              "complement_store_ms": store_ms, "store_complements": n_comp, "store_over_seeded": store_ms / (ms + point_ms),
              "outputs_checked": ok})
    if out:
        out.close()


if __name__ == "__main__":
    main()
