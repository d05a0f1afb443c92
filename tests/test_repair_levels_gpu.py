"""GPU box: the lower-level repair (porla_{kzg,ipa}_repair_levels_batch_device) -- the failed rows of a lower level's Y half are
rebuilt from the level's X half and written back in place: data row, alignment row, MAC row.  The stores are the ones
tests/test_extract_xy_gpu.py builds (XyFlow: a top level left by a rebuild write, then seven writes through the client and server update
batches, n_total = 8, 128 columns; t = 7 holds levels of 1, 2 and 4 rows, t = 1 level 0 alone), the synthetic file of n_total = 64
with the Y halves of tests/repair_levels_model.py, and one level of 2^10 rows made by the single-file encodes.  The expected bytes of
a repaired store are the PRISTINE bytes: what the update batch wrote before the damage.  Every comparison is byte equality; every
store the call may write and every output lies in front of a 256-byte sentinel guard that must survive, and the X stores are compared
with what they were.  No test damages anything but copies of its own buffers.

The KZG build draws its hiding base anew at every init_SRS, so every test builds its own file and installs no key after that."""
import functools
import types

import pytest

from tests import common  # noqa: F401  (puts oracle/ on the path)
import icc_py
from tests import extract_model as em
from tests import repair_levels_model as rl
from tests import retrieve_model as model
from tests import test_extract_gpu as te
from tests import test_extract_xy_gpu as txy
from tests import test_retrieve_aligned_gpu as ta
from tests import test_retrieve_gpu as tr

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "secp256k1"]
SENTINEL, GUARD = tr.SENTINEL, tr.GUARD
_dev, _host = tr._dev, tr._host
N, NCOLS = te.N, te.NCOLS
ALL = (1 << 64) - 1
DATA, MAC, ALIGN = rl.DATA, rl.MAC, rl.ALIGN
flipped, with_lower = txy.flipped, txy.with_lower
ROW = 64 * NCOLS


def levels_call_of(curve, afb=None, hfb=None, alpha=None):
    from porla_amd import multiexp as mx
    if curve == "bn254":
        return lambda reqs, n, s=0: mx.kzg_repair_levels_batch_device(reqs, n, s)
    return lambda reqs, n, s=0: afb.ipa_repair_levels_batch_device(hfb, alpha, reqs, n, s)


def flow(curve):
    import torch
    F = txy.XyFlow(curve, torch.cuda.Stream())
    F.levels = levels_call_of(curve) if curve == "bn254" else levels_call_of(curve, F.C.afb, F.C.hfb, F.C.alpha)
    return F


def offsets(t, n):
    return rl.offsets(t, n)


def run_levels(F, files, masks, n=N, stream=None, work=None, reserved=None):
    """one call on working copies of the files' Y stores (or on `work`, the copies of an earlier call, in place).  files: txy's
    dictionaries.  Returns a function giving (per file the outputs and {"y": {level: (data, MAC, alignment bytes)}}; the working
    copies); the guards are checked, and the X stores are as they were"""
    import torch
    from porla_amd import multiexp as mx
    logn = n.bit_length() - 1
    full = lambda size: torch.full((size + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    works, reqs, keep, xs = [], [], [], []
    for a, (f, mask) in enumerate(zip(files, masks)):
        t = f["write_step"] % n
        lv = sorted(f["lower"])
        assert lv == [i for i, _, _ in em.resident_levels(t, n)]
        sizes = {"status_x": t, "status_y": t, "action_y": t, "level": 16, "counts": 32, "work": mx.repair_levels_work_bytes(n, NCOLS, t, mask)}
        wk = dict(work[a]) if work else {}
        for name, size in sizes.items():
            wk[name] = full(size)
        for i in lv:
            dy, my, py, ay = f["y"][i]
            for name, src, size in (("data_y", dy, ROW << i), ("mac_y", my, 64 << i), ("align_y", ay, 64 << i)):
                sizes[(name, i)] = size
                if not work:
                    wk[(name, i)] = full(size)
                    wk[(name, i)][:size] = src[:size]
        wk["sizes"] = sizes
        prf_x = _dev(ta.raw_prf(F.curve, [v for i in lv for v in f["lower"][i][2]])) if t else None
        prf_y = _dev(ta.raw_prf(F.curve, [v for i in lv for v in f["y"][i][2]])) if t else None
        ptr = lambda x: x.data_ptr() if x is not None else 0
        fam_x = lambda k: [ptr(f["lower"][i][k]) if i in f["lower"] else 0 for i in range(logn)]
        fam_y = lambda name: [ptr(wk[(name, i)]) if i in f["lower"] else 0 for i in range(logn)]
        req = (f["write_step"], mask, fam_x(0), fam_x(1), ptr(prf_x), ptr(prf_y), fam_y("data_y"), fam_y("mac_y"), fam_y("align_y"),
               ptr(wk["work"]) if sizes["work"] else 0, ptr(wk["status_x"]), ptr(wk["status_y"]), ptr(wk["action_y"]), ptr(wk["level"]),
               ptr(wk["counts"]))
        reqs.append(req if reserved is None else req + (reserved,))
        works.append(wk)
        keep += [prf_x, prf_y]
        xs.append([(f["lower"][i][k], _host(f["lower"][i][k])) for i in lv for k in (0, 1)])
    torch.cuda.synchronize()
    F.levels(reqs, n, stream.cuda_stream if stream is not None else 0)

    def done():
        if stream is not None:
            stream.synchronize()
        torch.cuda.synchronize()
        res = []
        for a, wk in enumerate(works):
            for name, size in wk["sizes"].items():
                assert bool(torch.all(wk[name][size:] == SENTINEL)), "file %d: the guard behind %s changed" % (a, name)
            for tns, before in xs[a]:
                assert _host(tns) == before, "file %d: an X store was written" % a
            got = {name: _host(wk[name][:wk["sizes"][name]]) for name in ("status_x", "status_y", "action_y", "level")}
            got["counts"] = wk["counts"][:32].cpu().view(torch.int32).tolist()
            got["y"] = {i: tuple(_host(wk[(name, i)][:wk["sizes"][(name, i)]]) for name in ("data_y", "mac_y", "align_y"))
                        for i in sorted(files[a]["lower"])}
            res.append(got)
        del keep[:]
        return res, works
    return done


def stores_of(f):
    """the resident Y halves of a file as bytes: {level: (data, MAC, alignment)}"""
    return {i: (_host(dy[:ROW << i]), _host(my[:64 << i]), _host(ay[:64 << i])) for i, (dy, my, py, ay) in f["y"].items()}


def verdicts(named):
    return bytes(named.get(i, 0) for i in range(16))


def repair_and_settle(F, f, pristine, mask=ALL, n=N, repaired=(), stream=None):
    """one damaged file through the call; then what holds for every call that repairs: the Y stores are the pristine ones, every Y row
    passes the aligned retrieval's check, and a second call on the repaired stores reports the levels CLEAN and writes nothing"""
    stream = stream or F.stream
    (got,), works = run_levels(F, [f], [mask], n, stream)()
    t = f["write_step"] % n
    named = [i for i in sorted(f["lower"]) if mask >> i & 1]
    assert got["y"] == pristine
    for i in named:
        assert got["level"][i] == (rl.REPAIRED if i in repaired else rl.CLEAN), "level %d" % i
    (again,), _ = run_levels(F, [f], [mask], n, stream, work=works)()
    off = offsets(t, n)
    want_st = bytes(1 if any(off[i] <= r < off[i] + (1 << i) for i in named) else rl.NOT_TRIED for r in range(t))
    assert again["status_x"] == again["status_y"] == want_st
    assert again["action_y"] == bytes(t) and again["counts"] == [0] * 8 and again["y"] == pristine
    assert again["level"] == verdicts({i: rl.CLEAN for i in named})
    return got


# ---- 1. a clean file is left alone
@pytest.mark.parametrize("curve", CURVES)
def test_a_clean_file_is_left_alone(curve):
    F = flow(curve)
    for t in (7, 1, 6):
        f = F.file(t)
        (got,), _ = run_levels(F, [f], [ALL], stream=F.stream)()
        assert got["status_x"] == got["status_y"] == bytes([1] * t) and got["action_y"] == bytes(t) and got["counts"] == [0] * 8, "t = %d" % t
        assert got["level"] == verdicts({i: rl.CLEAN for i in f["lower"]}) and got["y"] == stores_of(f), "t = %d" % t


# ---- 2. per level, one flipped Y data byte comes back
@pytest.mark.parametrize("curve", CURVES)
def test_a_flipped_y_data_byte_comes_back(curve):
    F = flow(curve)
    for t, level, row in ((7, 0, 0), (7, 1, 1), (7, 2, 2), (1, 0, 0)):
        what = "t = %d level %d" % (t, level)
        f = F.file(t)
        g = with_lower(f, level, data_y=flipped(f["y"][level][0], 64 * (row * NCOLS + 77) + 3))
        got = repair_and_settle(F, g, stores_of(f), repaired={level})
        r = offsets(t, N)[level] + row
        assert got["status_x"] == bytes([1] * t) and got["status_y"] == bytes(0 if j == r else 1 for j in range(t)), what
        assert got["action_y"] == bytes(DATA if j == r else 0 for j in range(t)), what
        assert got["counts"] == [0, 1, 1, 0, 0, 1, 0, 0], what


# ---- 3. a MAC byte, an alignment byte, and all three in one row
@pytest.mark.parametrize("curve", CURVES)
def test_mac_alignment_and_all_three(curve):
    F = flow(curve)
    f = F.file(7)
    dy, my, py, ay = f["y"][2]
    cases = [(3, dict(macs_y=flipped(my, 64 * 3 + 40, 0x80)), MAC), (0, dict(align_y=flipped(ay, 63, 2)), ALIGN),
             (1, dict(data_y=flipped(dy, 64 * (NCOLS + 5) + 9), macs_y=flipped(my, 64 + 1), align_y=flipped(ay, 64 + 33, 0x10)), DATA | MAC | ALIGN)]
    for row, change, bits in cases:
        what = "row %d %s" % (row, sorted(change))
        got = repair_and_settle(F, with_lower(f, 2, **change), stores_of(f), repaired={2})
        assert got["status_y"] == bytes(0 if j == 3 + row else 1 for j in range(7)), what
        assert got["action_y"] == bytes(bits if j == 3 + row else 0 for j in range(7)), what
        assert got["counts"] == [0, 1, bits & DATA, (bits & ALIGN) >> 3, (bits & MAC) >> 1, 1, 0, 0], what


# ---- 4. every row of a Y half damaged: no witness, repaired all the same
@pytest.mark.parametrize("curve", CURVES)
def test_a_y_half_without_a_witness_is_repaired(curve):
    F = flow(curve)
    f = F.file(7)
    dy = f["y"][2][0].clone()
    for row in range(4):
        dy[64 * (row * NCOLS + 11 * row) + row] ^= 1 << row
    got = repair_and_settle(F, with_lower(f, 2, data_y=dy), stores_of(f), repaired={2})
    assert got["status_y"] == bytes([1, 1, 1, 0, 0, 0, 0]) and got["action_y"] == bytes([0, 0, 0] + [DATA] * 4)
    assert got["counts"] == [0, 4, 4, 0, 0, 1, 0, 0]


# ---- 5. an X row damaged beside a damaged Y row
@pytest.mark.parametrize("curve", CURVES)
def test_a_damaged_x_half_leaves_the_level_alone(curve):
    F = flow(curve)
    f = F.file(7)
    g = with_lower(f, 2, data=flipped(f["lower"][2][0], 64 * (2 * NCOLS + 9) + 1), data_y=flipped(f["y"][2][0], 64 * (NCOLS + 5) + 9))
    (got,), _ = run_levels(F, [g], [ALL], stream=F.stream)()
    assert got["status_x"] == bytes(0 if j == 5 else 1 for j in range(7)) and got["status_y"] == bytes(0 if j == 4 else 1 for j in range(7))
    assert got["level"] == verdicts({0: rl.CLEAN, 1: rl.CLEAN, 2: rl.X_DAMAGED}) and got["action_y"] == bytes(7)
    assert got["counts"] == [1, 1, 0, 0, 0, 0, 1, 0] and got["y"] == stores_of(g)


# ---- 6. two halves that pass their checks and do not belong together
@pytest.mark.parametrize("curve", CURVES)
def test_inconsistent_halves_are_not_written(curve):
    """level 1's X half from the snapshot at t = 7 (steps 5, 6) with level 1's Y stores, MACs, PRF values and alignments from the
    snapshot at t = 3 (steps 1, 2) of the same flow; one Y row damaged: the other is a witness that differs"""
    F = flow(curve)
    f7, f3 = F.file(7), F.file(3)
    dy, my, py, ay = f3["y"][1]
    g = with_lower(f7, 1, data_y=dy, macs_y=my, prf_y=py, align_y=ay)
    (got,), _ = run_levels(F, [g], [ALL], stream=F.stream)()
    assert got["status_x"] == got["status_y"] == bytes([1] * 7) and got["counts"] == [0] * 8      # both halves pass their checks
    h = with_lower(g, 1, data_y=flipped(dy, 64 * 3 + 2))
    (got,), _ = run_levels(F, [h], [ALL], stream=F.stream)()
    assert got["status_y"] == bytes(0 if j == 1 else 1 for j in range(7)) and got["action_y"] == bytes(7)
    assert got["level"] == verdicts({0: rl.CLEAN, 1: rl.INCONSISTENT, 2: rl.CLEAN})
    assert got["counts"] == [0, 1, 0, 0, 0, 0, 1, 1] and got["counts"][7] > 0 and got["y"] == stores_of(h)


# ---- 7. an unnamed damaged level
@pytest.mark.parametrize("curve", CURVES)
def test_an_unnamed_level_is_untouched(curve):
    F = flow(curve)
    f = F.file(7)
    g = with_lower(f, 1, data_y=flipped(f["y"][1][0], 64 * 3 + 2))
    (got,), _ = run_levels(F, [g], [ALL & ~2], stream=F.stream)()
    st = bytes([1, rl.NOT_TRIED, rl.NOT_TRIED, 1, 1, 1, 1])
    assert got["status_x"] == got["status_y"] == st and got["action_y"] == bytes(7) and got["counts"] == [0] * 8
    assert got["level"] == verdicts({0: rl.CLEAN, 2: rl.CLEAN}) and got["y"] == stores_of(g)


# ---- 8. three files in one call equal three calls; the launch count
@pytest.mark.parametrize("curve", CURVES)
def test_three_files_equal_three_calls_and_the_launch_count(curve):
    import torch
    from porla_amd import multiexp as mx
    F = flow(curve)
    f7 = F.file(7)
    files = [with_lower(f7, 1, data_y=flipped(f7["y"][1][0], 64 * 9 + 1)), F.file(5, top=False, write_step=5),
             with_lower(f7, 2, macs_y=flipped(f7["y"][2][1], 64 * 2 + 7), data=flipped(f7["lower"][2][0], 5))]
    masks = [ALL, 1, ALL]
    got, _ = run_levels(F, files, masks, stream=F.stream)()
    for a, (f, mask) in enumerate(zip(files, masks)):
        assert got[a] == run_levels(F, [f], [mask], stream=F.stream)()[0][0], "file %d against its single call" % a
    assert got[0]["level"] == verdicts({0: rl.CLEAN, 1: rl.REPAIRED, 2: rl.CLEAN}) and got[0]["y"] == stores_of(f7)
    assert got[1]["level"] == verdicts({0: rl.CLEAN}) and got[1]["status_y"] == bytes([1, rl.NOT_TRIED, rl.NOT_TRIED, rl.NOT_TRIED, rl.NOT_TRIED])
    assert got[2]["level"] == verdicts({0: rl.CLEAN, 1: rl.CLEAN, 2: rl.X_DAMAGED})

    def launches(fs, ms):
        torch.cuda.synchronize()
        before = sum(c for _, _, c in mx.profile_get())
        run_levels(F, fs, ms)()
        return sum(c for _, _, c in mx.profile_get()) - before

    mx.profile_enable(1)
    try:
        clean1, clean3 = launches([f7], [ALL]), launches([f7] * 3, [ALL] * 3)
        bad1, bad3 = launches([files[0]], [ALL]), launches([files[0], f7, files[2]], [ALL] * 3)
        fewer = launches([f7], [1])
    finally:
        mx.profile_enable(0)
    assert clean1 == clean3 == bad1 == bad3 and fewer < clean1


# ---- 9. the seams of the check's blocks: the synthetic file of n_total = 64 at t = 63
@functools.lru_cache(maxsize=None)
def synthetic_y(curve, n=64):
    """the Y halves of te.synthetic's levels by the model: data rows, the logarithms of the alignment rows Commit(N_j mod q), the rows'
    alpha-commitments and PRF values: computed once, shared, left unchanged"""
    import random
    _, blocks, _, _, _ = te.synthetic(curve)
    rnd = random.Random(6600)
    key = tr.commit_key(curve)
    q = icc_py.Q[curve]
    out = {}
    for i, lo, hi in em.resident_levels(n - 1, n):
        chunks, steps = [blocks[s] for s in range(lo, hi + 1)], rl.level_steps(2 * n + n - 1, n, i)
        assert [s % n for s in steps] == list(range(lo, hi + 1))
        rows = rl.y_half(chunks, steps, n, curve)
        if curve == "bn254":
            logs = [sum(c * pow(key["tau"], k, q) for k, c in enumerate(r)) % q for r in rl.align_scalars(chunks, steps, n, curve)]
        else:
            inv = pow(ta.IPA_ALPHA, -1, q)
            logs = [sum(c * d for c, d in zip(r, key["dlogs"])) * inv % q for r in rl.align_scalars(chunks, steps, n, curve)]
        out[i] = (rows, [model.alpha_commit(r, key) for r in rows], [rnd.getrandbits(128) for _ in rows], logs)
    return out


@pytest.mark.parametrize("curve", CURVES)
def test_126_rows_across_the_block_seams(curve):
    """levels 0 .. 5 in both halves: 63 X rows, then 63 Y rows in the one pass of the check, the seam between them at row 63, the
    levels' seams inside the 32-row evaluation blocks and the 64-row compare blocks.  Clean; then the last Y row of level 5 (row 125
    of the pass), level 0's Y row (row 63) and a row of level 3 damaged in data, MAC and alignment: they come back"""
    import torch
    mdm = ta.mdm
    n = 64
    S = ta.Setup(curve)
    _, _, levels, commits, prf = te.synthetic(curve)
    ys = synthetic_y(curve)
    if curve == "bn254":
        call = levels_call_of(curve)
    else:
        _, afb, hfb = tr.ipa_bases()
        call = levels_call_of(curve, afb, hfb, ta.IPA_ALPHA)
    F = types.SimpleNamespace(curve=curve, levels=call, stream=torch.cuda.Stream())
    dev = {i: (_dev(model.rows_bytes(levels[i])), _dev(model.points_to_bytes(S.expected(commits[i], prf[i]))), prf[i]) for i in range(6)}
    dev_y = {}
    for i, (rows, cm, pv, logs) in ys.items():
        align_b = model.points_to_bytes([icc_py.ec_mul(curve, mdm.GEN[curve], a) if a else None for a in logs])
        dev_y[i] = (_dev(model.rows_bytes(rows)), _dev(model.points_to_bytes(S.expected_aligned(cm, pv, logs))), pv, _dev(align_b))
    f = {"write_step": 2 * n + 63, "lower": dev, "y": dev_y, "top": None}
    (got,), _ = run_levels(F, [f], [ALL], n, F.stream)()
    assert got["status_x"] == got["status_y"] == bytes([1] * 63) and got["counts"] == [0] * 8 and got["y"] == stores_of(f)
    assert got["level"] == verdicts({i: rl.CLEAN for i in range(6)})
    g = with_lower(f, 5, data_y=flipped(dev_y[5][0], 64 * (31 * NCOLS + 100) + 2, 4))
    g = with_lower(g, 0, macs_y=flipped(dev_y[0][1], 33))
    g = with_lower(g, 3, data_y=flipped(dev_y[3][0], 64 * (2 * NCOLS + 1)), macs_y=flipped(dev_y[3][1], 64 * 2 + 5), align_y=flipped(dev_y[3][3], 64 * 2 + 60))
    got = repair_and_settle(F, g, stores_of(f), n=n, repaired={0, 3, 5})
    bad = {0: MAC, 7 + 2: DATA | MAC | ALIGN, 31 + 31: DATA}
    assert got["status_y"] == bytes(0 if r in bad else 1 for r in range(63)) and got["status_x"] == bytes([1] * 63)
    assert got["action_y"] == bytes(bad.get(r, 0) for r in range(63)) and got["counts"] == [0, 3, 2, 1, 2, 3, 0, 0]


# ---- 10. one level of 2^10 rows: the smallest that takes two data passes
@functools.lru_cache(maxsize=None)
def g_table(curve):
    """d 256^w G for d < 256, w < 32: a multiple of the generator is 32 additions"""
    base, tab = ta.mdm.GEN[curve], []
    for _ in range(32):
        row, acc = [None], None
        for _ in range(255):
            acc = icc_py.ec_add(curve, acc, base)
            row.append(acc)
        tab.append(row)
        base = icc_py.ec_add(curve, acc, base)
    return tab


def g_mul(curve, e):
    acc = None
    for w, row in enumerate(g_table(curve)):
        acc = icc_py.ec_add(curve, acc, row[e >> (8 * w) & 255])
    return acc


@pytest.mark.parametrize("curve", CURVES)
def test_a_level_of_two_data_passes(curve):
    """n_total = 2^11, t = 2^10: level 10 alone.  Its stores come from entry points this call shares no pass kernel with: the X half
    is the single-file encode of the chunks, the pristine Y data rows the single-file encode of the rows y_p; the X MAC rows are the
    model's.  The Y MAC and alignment stores are zeros, so every Y row fails and there is no witness; three Y data rows are damaged.
    The data rows come back as the encode's bytes, sampled alignment rows are the model's Commit(N_j mod q), and a second call finds
    every row clean under the MACs and alignments the first wrote"""
    import random
    import torch
    from porla_amd import icc
    n, lg, rows = 2048, 10, 1024
    S = ta.Setup(curve)
    if curve == "bn254":
        call = levels_call_of(curve)
    else:
        _, afb, hfb = tr.ipa_bases()
        call = levels_call_of(curve, afb, hfb, ta.IPA_ALPHA)
    F = types.SimpleNamespace(curve=curve, levels=call, stream=torch.cuda.Stream())
    q, key = icc_py.Q[curve], S.key
    rnd = random.Random(6700)
    chunks = [[rnd.getrandbits(256) for _ in range(NCOLS)] for _ in range(rows)]
    write_step = 3 * n + rows
    steps = rl.level_steps(write_step, n, lg)
    ys, cs = rl.hadd_rows(chunks, steps, n, curve)

    def encode(rws):
        d_in, d_out = _dev(ta.chunk_bytes(rws)), torch.empty(rows * ROW, dtype=torch.uint8, device="cuda")
        icc.crebuild_device(d_in.data_ptr(), rows, NCOLS, curve, 0, 0, d_x=d_out.data_ptr())
        torch.cuda.synchronize()
        return d_out

    def rows_mod_q(t, js):
        b = _host(t)
        return [[int.from_bytes(b[64 * (j * NCOLS + c):64 * (j * NCOLS + c + 1)], "little") % q for c in range(NCOLS)] for j in js]

    d_x, d_y, d_c = encode(chunks), encode(ys), encode(cs)
    if curve == "bn254":
        gen = [pow(key["tau"], c, q) for c in range(NCOLS)]                                  # Commit = sum c_i gen_i G
        agen = [key["alpha"] * g % q for g in gen]
    else:
        agen = key["dlogs"]
        gen = [d * pow(ta.IPA_ALPHA, -1, q) % q for d in agen]
    dot = lambda row, wts: sum(v * w for v, w in zip(row, wts)) % q
    macs_x = model.points_to_bytes([g_mul(curve, dot(r, agen)) for r in rows_mod_q(d_x, range(rows))])
    damaged = d_y.clone()
    bad_rows = (0, 517, 1023)
    for j in bad_rows:
        damaged[64 * (j * NCOLS + j % NCOLS) + 5] ^= 0x40
    zeros = lambda size: torch.zeros(size, dtype=torch.uint8, device="cuda")
    f = {"write_step": write_step, "lower": {lg: (d_x, _dev(macs_x), [0] * rows)}, "y": {lg: (damaged, zeros(64 * rows), [0] * rows, zeros(64 * rows))},
         "top": None}
    (got,), works = run_levels(F, [f], [ALL], n, F.stream)()
    assert got["status_x"] == bytes([1] * rows) and got["status_y"] == bytes(rows) and got["level"] == verdicts({lg: rl.REPAIRED})
    data, macs, align = got["y"][lg]
    assert data == _host(d_y)
    sample = (0, 1, 511, 1023)
    for j, r in zip(sample, rows_mod_q(d_c, sample)):
        assert align[64 * j:64 * j + 64] == model.point_bytes(g_mul(curve, dot(r, gen))), "alignment row %d" % j
    finite = sum(1 for j in range(rows) if align[64 * j:64 * j + 64] != bytes(64))
    assert finite > rows // 2 and got["counts"] == [0, rows, 3, finite, rows, 1, 0, 0]
    assert got["action_y"] == bytes((DATA if j in bad_rows else 0) | MAC | (ALIGN if align[64 * j:64 * j + 64] != bytes(64) else 0) for j in range(rows))
    (again,), _ = run_levels(F, [f], [ALL], n, F.stream, work=works)()
    assert again["status_x"] == again["status_y"] == bytes([1] * rows) and again["counts"] == [0] * 8 and again["y"] == got["y"]
    assert again["level"] == verdicts({lg: rl.CLEAN}) and again["action_y"] == bytes(rows)


# ---- 11. after a repair the scrub a caller has today finds nothing
@pytest.mark.parametrize("curve", CURVES)
def test_after_a_repair_the_extraction_finds_every_y_row_clean(curve):
    F = flow(curve)
    f = F.file(7)
    g = with_lower(with_lower(f, 2, data_y=flipped(f["y"][2][0], 64 * (3 * NCOLS + 1) + 7)), 1, macs_y=flipped(f["y"][1][1], 3))
    before, = txy.extract_xy(F, [g], [ALL], stream=F.stream)
    assert before["counts"][4] == 2
    (got,), works = run_levels(F, [g], [ALL], stream=F.stream)()
    assert got["counts"] == [0, 2, 1, 0, 1, 2, 0, 0]
    wk = works[0]
    healed = dict(g, y={i: (wk[("data_y", i)], wk[("mac_y", i)], g["y"][i][2], wk[("align_y", i)]) for i in g["y"]})
    after, = txy.extract_xy(F, [healed], [ALL], stream=F.stream)
    assert after["counts"] == [0] * 6 and after["row_status_y"] == bytes([1] * 7)
    assert after == txy.extract_xy(F, [f], [ALL], stream=F.stream)[0]


# ---- 12. a second call on another stream while the first is in flight
@pytest.mark.parametrize("curve", CURVES)
def test_a_second_call_on_another_stream_while_the_first_is_in_flight(curve):
    import torch
    F = flow(curve)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    f7 = F.file(7)
    g = with_lower(f7, 2, data_y=flipped(f7["y"][2][0], 64 * 5 + 1))
    (one,), _ = run_levels(F, [g], [ALL], stream=F.stream)()
    first = run_levels(F, [g for _ in range(6)], [ALL] * 6, stream=s1)
    second = run_levels(F, [F.file(t) for t in (5, 1, 6)], [ALL, ALL, 2], stream=s2)
    third = run_levels(F, [g], [4], stream=s1)
    assert one["counts"] == [0, 1, 1, 0, 0, 1, 0, 0] and one["y"] == stores_of(f7)
    for got in first()[0]:
        assert got == one
    for got, t in zip(second()[0], (5, 1, 6)):
        assert got["counts"] == [0] * 8 and got["action_y"] == bytes(t) and got["y"] == stores_of(F.file(t))
    got, = third()[0]
    assert got["y"] == stores_of(f7) and got["level"] == verdicts({2: rl.REPAIRED}) and got["status_y"][:3] == bytes([rl.NOT_TRIED] * 3)
