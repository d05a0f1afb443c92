"""GPU: the batched MSM (porla_*_msm_batch_device / _host) -- every entry equals the oracle and, byte for byte, porla_*_msm_device on
the same pairs; edge scalars and points; the reference's ecmult constants KAT (tests.c:4694-4751) through one batch; an audit-like
batch; the stream contract; the host form; concurrent callers; an oversized entry."""
import random
import threading

import pytest

from tests import common

pytestmark = pytest.mark.gpu

R = {"bn254": 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001,
     "secp256k1": 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141}
P = {"bn254": 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47,
     "secp256k1": 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEFFFFFC2F}
CURVES = ("bn254", "secp256k1")
INF = bytes(64)


@pytest.fixture(scope="module")
def mx():
    import torch
    torch.cuda.set_device(0)
    from porla_amd import multiexp
    return multiexp


def points_for(curve, n):
    if curve == "bn254":
        return bytes(common.synth_points(n))
    return bytes(common.secp_bench_points(n))


def oracle(curve, scalars, points, n):
    if n == 0:
        return INF
    if curve == "bn254":
        return common.oracle_msm(scalars, points, n)
    return common.oracle_secp_msm(scalars, points, n)


def dev(data):
    import torch
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda() if data else torch.zeros(64, dtype=torch.uint8).cuda()


def run_batch(mx, curve, scalars, points, offsets, stream=None):
    import torch
    k = len(offsets) - 1
    d_sc, d_pt = dev(scalars), dev(points)
    d_out = torch.zeros(max(64 * k, 64), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    mx.msm_batch_device(curve, d_sc.data_ptr(), d_pt.data_ptr(), offsets, d_out.data_ptr(), s)
    torch.cuda.synchronize()
    raw = bytes(d_out.cpu().numpy().tobytes())
    return mx.split_outputs(raw, k), (d_sc, d_pt)


def singles(mx, curve, d_sc, d_pt, offsets):
    import torch
    s = torch.cuda.current_stream().cuda_stream
    return [mx.msm_device(curve, d_sc.data_ptr() + 32 * offsets[i], d_pt.data_ptr() + 64 * offsets[i], offsets[i + 1] - offsets[i], s)
            for i in range(len(offsets) - 1)]


def be(x):
    return (x % (1 << 256)).to_bytes(32, "big")


@pytest.mark.parametrize("curve", CURVES)
def test_mixed_sizes_against_the_oracle_and_single_calls(mx, curve):
    rnd = random.Random(0xBA7C)
    sizes = [0, 1, 2, 3, 17, 64, 65, 128, 1408, 3200, 4096, 32768]
    rnd.shuffle(sizes)
    offsets = mx.batch_offsets(sizes)
    n = offsets[-1]
    # full-length scalars in most entries, abs(int32) in a few: both shapes in one batch
    sc = b"".join(be(rnd.getrandbits(256)) if (i // 7) % 3 else be(rnd.getrandbits(31)) for i in range(n))
    pts = points_for(curve, n)
    got, (d_sc, d_pt) = run_batch(mx, curve, sc, pts, offsets)
    ones = singles(mx, curve, d_sc, d_pt, offsets)
    for i, size in enumerate(sizes):
        lo, hi = offsets[i], offsets[i + 1]
        want = oracle(curve, sc[32 * lo:32 * hi], pts[64 * lo:64 * hi], size)
        assert got[i] == want, "entry %d (%d pairs)" % (i, size)
        assert got[i] == ones[i], "entry %d (%d pairs) differs from the single call" % (i, size)


@pytest.mark.parametrize("curve", CURVES)
def test_edge_values(mx, curve):
    r = R[curve]
    base = points_for(curve, 100)
    p0 = base[:64]
    neg_p0 = p0[:32] + ((P[curve] - int.from_bytes(p0[32:], "big")) % P[curve]).to_bytes(32, "big")
    edge = [0, 1, r - 1, r, r + 1, (1 << 256) - 1]
    entries = []                                    # (scalars, points)
    for s in edge:                                  # one-pair entries of each edge scalar
        entries.append(([s], [p0]))
    entries.append((edge, [base[64 * i:64 * i + 64] for i in range(6)]))   # all of them in one entry
    entries.append(([5, 7, 9], [INF, base[64:128], INF]))                   # infinity points
    entries.append(([12345, 12345], [p0, neg_p0]))                         # P and -P, equal scalars: infinity
    entries.append(([77] * 10 + [42] * 10, [p0] * 10 + [neg_p0] * 10))     # a sum that does not cancel
    s = random.Random(5).randrange(1, r)
    entries.append(([s, r - s], [p0, p0]))                                  # s P + (r - s) P = infinity (tiny path)
    entries.append(([s] * 40 + [r - s] * 40, [p0] * 80))                   # ... through the bucket path (> 64 pairs)
    entries.append(([random.Random(i).getrandbits(31) for i in range(100)], [base[64 * i:64 * i + 64] for i in range(100)]))  # short: no split
    entries.append(([random.Random(i).getrandbits(256) for i in range(100)], [base[64 * i:64 * i + 64] for i in range(100)]))  # split
    entries.append(([1, 2], [INF, INF]))
    entries.append(([random.Random(i).getrandbits(256) for i in range(64)], [base[64 * i:64 * i + 64] for i in range(64)]))   # the largest tiny entry
    entries.append(([random.Random(i).getrandbits(31) for i in range(40)], [base[64 * i:64 * i + 64] for i in range(40)]))    # tiny, short scalars
    sc = b"".join(be(x) for e in entries for x in e[0])
    pts = b"".join(p for e in entries for p in e[1])
    offsets = mx.batch_offsets([len(e[0]) for e in entries])
    got, (d_sc, d_pt) = run_batch(mx, curve, sc, pts, offsets)
    ones = singles(mx, curve, d_sc, d_pt, offsets)
    for i in range(len(entries)):
        lo, hi = offsets[i], offsets[i + 1]
        assert got[i] == oracle(curve, sc[32 * lo:32 * hi], pts[64 * lo:64 * hi], hi - lo), "entry %d" % i
        assert got[i] == ones[i], "entry %d" % i
    assert got[0] == INF and got[3] == INF                      # scalars 0 and r
    assert got[1] == p0 and got[4] == p0                        # 1 and r + 1
    assert got[2] == neg_p0                                     # r - 1
    assert got[8] == INF and got[10] == INF and got[11] == INF and got[14] == INF


@pytest.mark.parametrize("curve", CURVES)
def test_scalars_built_from_their_endomorphism_halves(mx, curve):
    """the public path by which user scalars reach quad30.hip.h:macq_ladder: the scalar families of tests/ladder_vectors.py (edge
    values, halves built from digit patterns with every sign pair, a set 33rd window, NAF shapes) as one-pair tiny entries over one
    point, then the same scalars eight to an entry over eight points -- against the oracle and the single calls"""
    from tests import ec_vectors as ev
    from tests import ladder_vectors as lv
    C = ev.CURVES[curve]
    fam = lv.families(C, "abcd")
    counts = {f: sum(1 for g, _ in fam if g == f) for f in "abcd"}
    assert counts["b"] >= 1000 and counts["c"] == (32 if curve == "secp256k1" else 0) and counts["d"] == 12 and lv.order(C) == R[curve]
    ks = [k for _, k in fam]
    ks += ks[:-len(ks) % 8]                                         # whole entries of eight
    base = points_for(curve, 8)
    pts8 = [base[64 * i:64 * i + 64] for i in range(8)]
    entries = [([k], [pts8[0]]) for k in ks] + [(ks[i:i + 8], pts8) for i in range(0, len(ks), 8)]
    sc = b"".join(be(x) for e in entries for x in e[0])
    pts = b"".join(p for e in entries for p in e[1])
    offsets = mx.batch_offsets([len(e[0]) for e in entries])
    got, (d_sc, d_pt) = run_batch(mx, curve, sc, pts, offsets)
    ones = singles(mx, curve, d_sc, d_pt, offsets)
    checked = 0
    for i, e in enumerate(entries):
        lo, hi = offsets[i], offsets[i + 1]
        assert got[i] == oracle(curve, sc[32 * lo:32 * hi], pts[64 * lo:64 * hi], hi - lo), "entry %d: scalars %s" % (i, [hex(x) for x in e[0]])
        assert got[i] == ones[i], "entry %d differs from the single call" % i
        checked += 1
    assert checked == len(entries) and len(ks) >= sum(counts.values()) > 1200 and len(ks) % 8 == 0


def test_reference_constants_kat_through_one_batch(mx):
    """tests.c:4738-4751: the 32 842 keys as one-pair secp256k1 entries over G in ONE batch call, hashed with tests.c's
    accumulate; no oracle in between"""
    from tests.test_reference_kats_gpu import EXPECTED_CONSTANTS_HASH, G, accumulate, b32, constants_keys
    keys = constants_keys()
    sc = b"".join(b32(k) for k in keys)
    got, _ = run_batch(mx, "secp256k1", sc, G * len(keys), list(range(len(keys) + 1)))
    assert got[0] == INF and got[1] == INF and got[2] == G
    assert accumulate(got) == EXPECTED_CONSTANTS_HASH


def test_audit_like_batch(mx):
    """64 audits: 3 200 abs(int32) coefficients each over points repeated 64 ways, BN254, against the oracle"""
    rnd = random.Random(64)
    k, n = 64, 3200
    base = points_for("bn254", n)
    sc = b"".join(be(abs(rnd.randrange(-(1 << 31), 1 << 31))) for _ in range(k * n))
    pts = base * k
    offsets = [n * i for i in range(k + 1)]
    got, _ = run_batch(mx, "bn254", sc, pts, offsets)
    for i in range(k):
        assert got[i] == oracle("bn254", sc[32 * n * i:32 * n * (i + 1)], base, n), "audit %d" % i


@pytest.mark.parametrize("curve", CURVES)
def test_stream_contract(mx, curve):
    """inputs uploaded asynchronously on a non-default stream, the call on that stream, one sync of it, then d_out; the bytes
    after k * 64 stay untouched"""
    import torch
    rnd = random.Random(11)
    sizes = [1, 20, 300, 0, 5]
    offsets = mx.batch_offsets(sizes)
    n = offsets[-1]
    sc = b"".join(be(rnd.getrandbits(256)) for _ in range(n))
    pts = points_for(curve, n)
    h_sc = torch.frombuffer(bytearray(sc), dtype=torch.uint8).pin_memory()
    h_pt = torch.frombuffer(bytearray(pts), dtype=torch.uint8).pin_memory()
    d_sc = torch.empty(len(sc), dtype=torch.uint8, device="cuda")
    d_pt = torch.empty(len(pts), dtype=torch.uint8, device="cuda")
    d_out = torch.full((64 * len(sizes) + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_sc.copy_(h_sc, non_blocking=True)
        d_pt.copy_(h_pt, non_blocking=True)
    mx.msm_batch_device(curve, d_sc.data_ptr(), d_pt.data_ptr(), offsets, d_out.data_ptr(), s.cuda_stream)
    s.synchronize()
    raw = bytes(d_out.cpu().numpy().tobytes())
    assert raw[64 * len(sizes):] == b"\xa5" * 256
    got = mx.split_outputs(raw, len(sizes))
    for i in range(len(sizes)):
        lo, hi = offsets[i], offsets[i + 1]
        assert got[i] == oracle(curve, sc[32 * lo:32 * hi], pts[64 * lo:64 * hi], hi - lo), "entry %d" % i


@pytest.mark.parametrize("curve", CURVES)
def test_host_form_equals_device_form_and_repeats(mx, curve):
    rnd = random.Random(23)
    sizes = [4, 0, 700, 1, 33]
    offsets = mx.batch_offsets(sizes)
    n = offsets[-1]
    sc = b"".join(be(rnd.getrandbits(256)) for _ in range(n))
    pts = points_for(curve, n)
    got_dev, _ = run_batch(mx, curve, sc, pts, offsets)
    h1 = mx.msm_batch_host(curve, sc, pts, offsets)
    h2 = mx.msm_batch_host(curve, sc, pts, offsets)
    assert h1 == got_dev and h2 == h1


def test_concurrent_callers(mx):
    """8 host threads, each its own batch (both curves, different sizes) at once: every result is right"""
    import torch
    jobs = []
    for t in range(8):
        curve = CURVES[t % 2]
        rnd = random.Random(100 + t)
        sizes = [rnd.choice([1, 2, 9, 40, 200, 1500]) for _ in range(6 + t)]
        offsets = mx.batch_offsets(sizes)
        n = offsets[-1]
        sc = b"".join(be(rnd.getrandbits(256)) for _ in range(n))
        pts = points_for(curve, n)
        want = [oracle(curve, sc[32 * offsets[i]:32 * offsets[i + 1]], pts[64 * offsets[i]:64 * offsets[i + 1]], sizes[i])
                for i in range(len(sizes))]
        jobs.append((curve, sc, pts, offsets, want))
    results = [None] * len(jobs)
    errors = []

    def work(i):
        try:
            torch.cuda.set_device(0)
            curve, sc, pts, offsets, _ = jobs[i]
            k = len(offsets) - 1
            d_sc, d_pt = dev(sc), dev(pts)
            d_out = torch.zeros(64 * k, dtype=torch.uint8, device="cuda")
            s = torch.cuda.Stream()
            torch.cuda.synchronize()
            for _ in range(3):
                mx.msm_batch_device(curve, d_sc.data_ptr(), d_pt.data_ptr(), offsets, d_out.data_ptr(), s.cuda_stream)
            s.synchronize()
            results[i] = mx.split_outputs(bytes(d_out.cpu().numpy().tobytes()), k)
        except Exception as e:          # reported below
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(len(jobs))]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for i, job in enumerate(jobs):
        assert results[i] == job[4], "thread %d" % i


@pytest.mark.parametrize("curve", CURVES)
def test_oversized_entry_is_refused_and_leaves_the_output(mx, curve):
    import torch
    offsets = [0, 3, 3 + 32769]
    n = offsets[-1]
    d_sc = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
    d_pt = torch.zeros(64 * n, dtype=torch.uint8, device="cuda")
    d_out = torch.full((128,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="porla_%s_msm_device" % curve):
        mx.msm_batch_device(curve, d_sc.data_ptr(), d_pt.data_ptr(), offsets, d_out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bytes(d_out.cpu().numpy().tobytes()) == b"\x5a" * 128


def test_a_batch_of_several_launch_rounds(mx):
    """2 000 bucket-path entries of 65 .. 80 pairs (18 blocks each: more than the 32 768 bucket blocks of one round) with tiny and empty
    entries between them -- the batch runs as two rounds (the profile counts the bucket kernel's launches); every output equals the
    single call on its entry"""
    import ctypes
    import torch
    from porla_amd import lib
    rnd = random.Random(0x2201)
    sizes = []
    for i in range(2000):
        sizes.append(rnd.randrange(65, 81))
        if i % 50 == 0:
            sizes.append(rnd.choice([0, 1, 5, 64]))
    offsets = mx.batch_offsets(sizes)
    n = offsets[-1]
    sc = b"".join(be(rnd.getrandbits(256)) for _ in range(n))
    pts = points_for("bn254", n)
    lib.porla_gpu_profile_enable(1)
    try:
        got, (d_sc, d_pt) = run_batch(mx, "bn254", sc, pts, offsets)
        launches = {}
        name, ms, cnt = ctypes.create_string_buffer(64), ctypes.c_double(), ctypes.c_longlong()
        slot = 0
        while lib.porla_gpu_profile_get(slot, name, 64, ctypes.byref(ms), ctypes.byref(cnt)) == 0:
            launches[name.value.decode()] = cnt.value
            slot += 1
    finally:
        lib.porla_gpu_profile_enable(0)
    assert launches.get("batch_bucket") == 2 and launches.get("batch_finish") == 2, launches
    ones = singles(mx, "bn254", d_sc, d_pt, offsets)
    bad = [i for i in range(len(sizes)) if got[i] != ones[i]]
    assert not bad, "entries %s differ from the single calls" % bad[:10]
    # and a sample against the oracle, from both rounds
    for i in (0, 1, len(sizes) // 2, len(sizes) - 2, len(sizes) - 1):
        lo, hi = offsets[i], offsets[i + 1]
        assert got[i] == oracle("bn254", sc[32 * lo:32 * hi], pts[64 * lo:64 * hi], hi - lo), "entry %d" % i
