"""GPU box: the ragged ICC decode (porla_icc_decode_ragged_batch_device) -- levels of unequal sizes in one call -- bit-exact against the
Python model tests/icc_decode_model.py and against the uniform call (porla_icc_decode_batch_device) on each request alone: mixed sizes
in the three forms, the order of the requests, tampered requests among intact ones, the launch count, two streams.  No tolerance
anywhere; a sentinel guard behind every output."""
import functools
import random

import pytest

import icc_py
from tests import icc_decode_model as model
from tests import test_icc_decode_gpu as uniform
from tests.test_icc_decode_gpu import BAD_PRESET, GUARD, SENTINEL, _dev, _host, chunks_with_edges, first_diff

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "secp256k1"]
P = icc_py.P_ICC
# 2: one radix-2 round; 4: a radix-4 round that is also the last; 8: an odd stage count; 512: a full one-pass tile (cc_log = 1 from
# two columns on); 1024: two equal passes; 2048: two unequal passes
SIZES = (2, 4, 8, 512, 1024, 2048)
N_TOTAL = 2048
FORMS = ("exact", "residue64", "residue32")


class Prepared:
    """one ragged call, its buffers on the device.  items: (input bytes or tensor, n_rows, write steps or None, wants a counter)"""

    def __init__(self, form, items, n_cols, n_total, curve):
        import torch
        self.form, self.n_cols, self.n_total, self.curve = form, n_cols, n_total, curve
        self.out_b = [n * n_cols * 32 for _, n, _, _ in items]
        self.ins = [x if hasattr(x, "is_cuda") else _dev(x) for x, _, _, _ in items]
        self.outs = [torch.full((b + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda") for b in self.out_b]
        self.steps = [None if s is None else torch.tensor(s, dtype=torch.int64).cuda() for _, _, s, _ in items]
        self.bad = [torch.tensor([BAD_PRESET - (1 << 32)], dtype=torch.int32).cuda() if w else None for _, _, _, w in items]
        self.reqs = [(self.ins[a].data_ptr(), self.outs[a].data_ptr(), 0 if self.steps[a] is None else self.steps[a].data_ptr(),
                      0 if self.bad[a] is None else self.bad[a].data_ptr(), items[a][1]) for a in range(len(items))]
        torch.cuda.synchronize()

    def issue(self, stream=None):
        from porla_amd import icc
        icc.decode_ragged_batch_device(self.reqs, self.n_cols, self.n_total, self.curve, self.form,
                                       stream.cuda_stream if stream is not None else 0)

    def collect(self):
        """([output bytes], [counter or None]) after a synchronize; the guard behind every output is checked here"""
        import torch
        torch.cuda.synchronize()
        for a, (o, b) in enumerate(zip(self.outs, self.out_b)):
            assert bool(torch.all(o[b:] == SENTINEL)), "request %d: the guard behind the output changed" % a
        return ([_host(o[:b]) for o, b in zip(self.outs, self.out_b)],
                [None if b is None else int(b.cpu()[0]) & 0xffffffff for b in self.bad])


def ragged(form, items, n_cols, n_total, curve, stream=None):
    call = Prepared(form, items, n_cols, n_total, curve)
    call.issue(stream)
    return call.collect()


def steps_of(n):
    return [5 + n + 7 * i for i in range(n)]


@functools.lru_cache(maxsize=None)
def level(curve, n, n_cols, n_total=N_TOTAL):
    """a level of n rows, computed once and never changed: its inputs in both widths, its write steps, and per form what the model
    (decode_bytes) and the uniform call on this request alone give"""
    rows = chunks_with_edges(n, n_cols, curve, 97 * n + n_cols)
    X, _ = icc_py.crebuild(rows, curve)
    x64 = model.rows_to_bytes(X, 64)
    x32 = model.rows_to_bytes([[v % P for v in r] for r in X], 32)
    steps = steps_of(n)
    L = {"x": {"exact": x64, "residue64": x64, "residue32": x32}, "steps": steps, "want": {}}
    for form in FORMS:
        for st in ((None, steps) if form == "residue64" else (None,)):
            want, want_bad = model.decode_bytes(form, L["x"][form], n, n_cols, n_total, curve, st)
            (got,), (bad,) = uniform.decode(form, [L["x"][form]], n, n_cols, n_total, curve, steps=[st], want_bad=[form == "exact"])
            assert got == want and bad == want_bad, "the uniform call and the model differ: %s n = %d" % (form, n)
            L["want"][form, st is not None] = (want, want_bad)
    assert L["want"]["exact", False] == (model.rows_to_bytes(rows, 32), 0)
    return L


def items_of(curve, form, sizes, n_cols, with_steps, n_total=N_TOTAL):
    """(items of one call, what each request must give)"""
    items, want = [], []
    for n in sizes:
        L = level(curve, n, n_cols, n_total)
        st = L["steps"] if with_steps else None
        items.append((L["x"][form], n, st, form == "exact"))
        want.append(L["want"][form, with_steps])
    return items, want


def assert_equal(got, bad, want, what=""):
    for a, (w, wb) in enumerate(want):
        assert got[a] == w, "%s request %d: first differing byte %s" % (what, a, first_diff(got[a], w))
        assert bad[a] == wb, "%s request %d: counter %s, want %s" % (what, a, bad[a], wb)


# ---- 1. mixed sizes in one call, the three forms; n_cols 1: cc_log = 0, 3: masked columns, 5: several column tiles
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n_cols", [1, 3, 5])
def test_mixed_sizes(curve, n_cols):
    for form, with_steps in (("exact", False), ("residue64", False), ("residue64", True), ("residue32", False)):
        items, want = items_of(curve, form, SIZES, n_cols, with_steps)
        got, bad = ragged(form, items, n_cols, N_TOTAL, curve)
        assert_equal(got, bad, want, "%s%s:" % (form, " with write steps" if with_steps else ""))
    # write steps on some requests only
    items, want = items_of(curve, "residue64", SIZES, n_cols, True)
    plain, want_plain = items_of(curve, "residue64", SIZES, n_cols, False)
    for a in (1, 4):
        items[a], want[a] = plain[a], want_plain[a]
    got, bad = ragged("residue64", items, n_cols, N_TOTAL, curve)
    assert_equal(got, bad, want, "residue64, steps on some:")


# ---- 2. the outputs do not depend on the order of the requests, on repeats, or on K
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("form", FORMS)
def test_request_order(curve, form):
    n_cols, with_steps = 3, form == "residue64"
    shuffled = list(SIZES)
    random.Random(5).shuffle(shuffled)
    assert shuffled != list(SIZES) and shuffled != list(reversed(SIZES))
    for sizes in (tuple(reversed(SIZES)), tuple(shuffled), (8, 1024, 8, 2, 1024, 8, 2048, 2048)):
        items, want = items_of(curve, form, sizes, n_cols, with_steps)
        got, bad = ragged(form, items, n_cols, N_TOTAL, curve)
        assert_equal(got, bad, want, "%s:" % (sizes,))
    for n in SIZES:                                               # K = 1
        items, want = items_of(curve, form, (n,), n_cols, with_steps)
        got, bad = ragged(form, items, n_cols, N_TOTAL, curve)
        assert_equal(got, bad, want, "K = 1, n = %d:" % n)
    items, want = items_of(curve, form, (16,), n_cols, with_steps, n_total=16)          # n_total = n_rows
    got, bad = ragged(form, items, n_cols, 16, curve)
    assert_equal(got, bad, want, "n_total = n_rows = 16:")


# ---- 3. one altered symbol in the 8-row and in the 1024-row request: exactly their counters move, by what the uniform call counts
@pytest.mark.parametrize("curve", CURVES)
def test_tampered_requests_among_intact_ones(curve):
    n_cols = 3
    lcm = icc_py.LCM[curve]
    items, want = items_of(curve, "exact", SIZES, n_cols, False)
    for n, (tr, tc) in ((8, (5, 2)), (1024, (700, 1))):
        a = SIZES.index(n)
        x = bytearray(items[a][0])
        at = 64 * (tr * n_cols + tc)
        x[at:at + 64] = ((int.from_bytes(x[at:at + 64], "little") + 1) % lcm).to_bytes(64, "little")
        (u_out,), (u_bad,) = uniform.decode("exact", [bytes(x)], n, n_cols, N_TOTAL, curve, want_bad=[True])
        assert u_bad == n                                         # (the column of the altered symbol)
        assert (u_out, u_bad) == model.decode_bytes("exact", bytes(x), n, n_cols, N_TOTAL, curve)
        items[a] = (bytes(x), n, None, True)
        want[a] = (u_out, u_bad)
    # a request without a counter among them: an intact one, and (second call) a tampered one
    for no_counter in (SIZES.index(512), SIZES.index(1024)):
        its, wnt = list(items), list(want)
        its[no_counter] = its[no_counter][:3] + (False,)
        wnt[no_counter] = (wnt[no_counter][0], None)
        got, bad = ragged("exact", its, n_cols, N_TOTAL, curve)
        assert_equal(got, bad, wnt, "no counter on request %d:" % no_counter)
        assert [a for a, b in enumerate(bad) if b] == [a for a in (SIZES.index(8), SIZES.index(1024)) if a != no_counter]


# ---- 4. the launches depend on the pass classes present, not on K and not on the sizes
def test_launch_count():
    import torch
    from porla_amd import multiexp as mx
    n_cols, curve = 3, "bn254"
    zeros = torch.zeros(2048 * n_cols * 64, dtype=torch.uint8, device="cuda")

    def launches(sizes):
        call = Prepared("exact", [(zeros, n, None, True) for n in sizes], n_cols, N_TOTAL, curve)
        before = sum(c for _, _, c in mx.profile_get())
        call.issue()
        got, bad = call.collect()
        assert all(g == bytes(len(g)) for g in got) and bad == [0] * len(sizes)
        return sum(c for _, _, c in mx.profile_get()) - before

    launches((2, 1024))                                           # warm-up: the tables and the workspace exist
    mx.profile_enable(1)
    try:
        rnd = random.Random(40)
        one = [launches((2,)), launches((2, 4, 8, 512)), launches([rnd.choice((2, 4, 8, 16, 64, 512)) for _ in range(40)])]
        two = [launches((1024,)), launches((1024, 2048, 2048))]
        both = launches((2, 1024, 8, 2048, 512))
    finally:
        mx.profile_enable(0)
    assert one[0] >= 1 and one == [one[0]] * 3, one
    assert two[0] >= 2 and two == [two[0]] * 2, two
    assert both <= one[0] + two[0], (both, one, two)


# ---- 5. a second call on another stream while the first is in flight
@pytest.mark.parametrize("curve", CURVES)
def test_two_streams(curve):
    import torch
    n_cols = 3
    items_a, want_a = items_of(curve, "exact", (1024, 8, 2048), n_cols, False)
    items_b, want_b = items_of(curve, "residue64", (2048, 2, 512, 1024, 1024), n_cols, True)
    a, b = Prepared("exact", items_a, n_cols, N_TOTAL, curve), Prepared("residue64", items_b, n_cols, N_TOTAL, curve)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    ballast = torch.empty(1 << 26, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        for _ in range(4):
            ballast.normal_()                       # a few milliseconds ahead of A on its stream: A is in flight when B comes
    a.issue(s1)
    b.issue(s2)
    assert_equal(*a.collect(), want_a, "the first call:")
    assert_equal(*b.collect(), want_b, "the second call:")
