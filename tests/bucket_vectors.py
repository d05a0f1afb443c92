"""Bucket lists and expected values for the bucket accumulation driven entry by entry (tools/bucket_sum_check.hip): shared by
tests/test_bucket_sum_gpu.py and tests/test_bucket_vectors_cpu.py.

Everything is computed IN THE EXPONENT: every table point is k G for a known k (index 0 is the point at infinity, k = 0), an entry's
value is +-k, or +-lambda k for the endomorphism's image in the doubled table, and a bucket's expected sum is (sum of its entries'
values mod the group order) G.  The value an item's accumulator holds before position j is known the same way, so an entry can be
made equal to it (the doubling branch) or to its negative (the accumulator goes to infinity inside the item and the item goes on).
The group law, the curve constants and the bound tables are tests/ec_vectors.py's, the order, lambda and the fixed-base multiple
tests/ladder_vectors.py's.  Generation is deterministic (fixed seeds) and reads nothing outside the repository.

A FILE is one driver run: a table, a list of cases (one bucket each, in bucket order) and their entries for every pass.  Pass 0
fills the bucket array, every later pass accumulates into it.
"""
import functools
import os
import random
import subprocess
import tempfile

import numpy as np

from tests import common
from tests import ec_vectors as ev
from tests import ladder_vectors as lv

EXE = os.path.join(common.ROOT, "porla_amd", "bucket_sum_check")
MAGIC, HDR = 0x4d55534b, 8
CHUNK, CTRL_WORDS, NO_CHUNK = 128, 4 + 128, 0xffffffff        # msm.hip.h
COMBINE_BLOCKS = 2048                                          # msm_launch: the grid of k_bucket_combine
SIGN = 1 << 31
SMALL = 1500                                                   # ordinary entries are +-k G, 1 <= k <= SMALL
FORMS = ["plain", "signbit"]                                   # the point itself | its negative in the table and the sign bit set

POSITION_L = [1, 2, 3, 4, 5, 64, 127, 128, 129, 130, 255, 256, 257, 385]
POSITION_KINDS = ["inf", "prev", "negprev", "runsum", "negrunsum"]
ITEMS_KINDS = ([k % (128 * m + d) for m in (1, 2, 3) for d, k in enumerate(("full_%d", "full_plus_one_%d"))] +
               ["equal_sums", "equal_sums_copy", "opposite_sums", "opposite_sums_copy", "inf_item_between", "inf_item_between_plus_one",
                "all_inf_1", "all_inf_2", "all_inf_129"])
ACC_KINDS2 = ["empty|Q", "P|empty", "P,-P|Q", "P|P", "P|-P", "P|-P,Q,R", "P,Q|P,Q", "P|Q,-Q,-P", "P|Q", "P|Q,R", "P,Q|R", "P,Q|R,P",
              "P|inf", "P|inf,inf,inf", "P|multi_inf", "multi|inf", "multi|S", "multi|-S", "P|multi_total_P", "P|multi_total_-P",
              "P|multi_item0_P", "P|multi_item0_-P", "multi|multi", "multi|multi_inf", "multi|multi_total_-S"]
ACC_KINDS3 = ["P|-P|Q", "multi|P|multi", "P|Q|R", "P|empty|Q", "empty|empty|Q", "P|multi_total_-P|Q"]
ACC_KINDS = ACC_KINDS2 + ["late:" + k for k in ACC_KINDS2] + ACC_KINDS3
GLV_KINDS = ["P,-phiP", "phiP,phiP", "phiP,-phiP,Q", "P,phiP", "phi_runsum", "phi_negrunsum", "mixed_multi", "all_inf", "mixed"]
N_HEAVY, N_TEMPLATES, N_FILL, N_GLV_MIXED, HEAVY_SUM0 = 2100, 67, 300, 120, 1000000


def position_js(L):
    """{0, 1, 2, 3, L/2, L-2, L-1} and both sides of the item boundary, where the bucket reaches them"""
    return sorted(j for j in {0, 1, 2, 3, L // 2, L - 2, L - 1, 126, 127, 128, 129} if 0 <= j < L)


def position_cases():
    """(kind, L, j, form): every kind at every position in both forms; only a point at infinity can stand at position 0 (there
    is no previous entry and no running sum there)"""
    return [(kind, L, j, form) for L in POSITION_L for j in position_js(L) for kind in POSITION_KINDS if kind == "inf" or j > 0
            for form in FORMS]


# ---------------------------------------------------------------- multiples of G
@functools.lru_cache(maxsize=None)
def _small(C):
    t = [None]
    for _ in range(SMALL):
        t.append(ev.ec_add(C, t[-1], C.g))
    return t


def mul(C, k):
    n = lv.order(C)
    k %= n
    if k <= SMALL:
        return _small(C)[k]
    if n - k <= SMALL:
        return ev.ec_neg(C, _small(C)[n - k])
    return lv.mul_g(C, k)


class Table:
    """the points of one file: exponent -> index; index 0 is the point at infinity.  With glv the file's entries address the
    doubled table the conversion kernel writes: 2 i the point, 2 i + 1 its image (x, y) -> (beta x, y) = lambda (the point)"""

    def __init__(self, C, glv=False):
        self.C, self.glv, self.n, self.lam = C, glv, lv.order(C), lv.lam(C)
        self.exps, self.index = [0], {0: 0}

    def idx(self, k):
        k %= self.n
        if k not in self.index:
            self.index[k] = len(self.exps)
            self.exps.append(k)
        return self.index[k]

    def word(self, k, form="plain", phi=False):
        """the entry whose value is k G (phi: lambda k G, read from the odd slot of k G)"""
        i, s = (self.idx(-k), SIGN) if form == "signbit" else (self.idx(k), 0)
        return s | ((2 * i + (1 if phi else 0)) if self.glv else i)

    def split(self, w):
        i = w & (SIGN - 1)
        phi = bool(self.glv and (i & 1))
        return (i >> 1 if self.glv else i), phi, bool(w & SIGN)

    def value(self, w):
        i, phi, neg = self.split(w)
        k = self.exps[i] * (self.lam if phi else 1) % self.n
        return (-k) % self.n if neg else k

    def point(self, w):
        """the entry's point through the group law of ec_vectors, not through the exponent"""
        i, phi, neg = self.split(w)
        P = mul(self.C, self.exps[i])
        if phi:
            P = ev.ec_phi(self.C, P)
        return ev.ec_neg(self.C, P) if neg else P

    def size(self):
        return len(self.exps) * (2 if self.glv else 1)

    def wire(self):
        raw = b"".join(bytes(64) if P is None else P[0].to_bytes(32, "big") + P[1].to_bytes(32, "big")
                       for P in (mul(self.C, k) for k in self.exps))
        return np.frombuffer(raw, dtype="<u4")


class Seq:
    """the entries of one bucket in one pass, built in order.  acc() is the exponent of what the item's accumulator holds before
    the next entry: an item starts from infinity (or from `stored`, the single item of an accumulating pass)"""

    def __init__(self, T, rng, stored=0):
        self.T, self.rng, self.n = T, rng, T.n
        self.words, self.run, self.total, self.used = [], stored % T.n, 0, set()

    def acc(self):
        return 0 if (self.words and len(self.words) % CHUNK == 0) else self.run

    def push(self, w):
        self.run = (self.acc() + self.T.value(w)) % self.n
        self.total = (self.total + self.T.value(w)) % self.n
        self.words.append(w)
        return self

    def entry(self, k, form=None, phi=False):
        return self.push(self.T.word(k, form or self.rng.choice(FORMS), phi))

    def ordinary(self, count=1):
        """distinct multiples that meet the accumulator in no exceptional case: not equal to it, not its negative"""
        for _ in range(count):
            while True:
                k = self.rng.randrange(1, SMALL + 1)
                if k in self.used:
                    continue
                k *= self.rng.choice([1, -1])
                phi = bool(self.T.glv and self.rng.random() < 0.5)
                v = k * (self.T.lam if phi else 1) % self.n
                a = self.acc()
                if a and ((a - v) % self.n == 0 or (a + v) % self.n == 0):
                    continue
                break
            self.used.add(abs(k))
            self.entry(k, None, phi)
        return self

    def item_to(self, size, target):
        """`size` entries that close the item: ordinary ones, then the one that makes the accumulator `target` G"""
        self.ordinary(size - 1)
        return self.entry(target - self.acc())


def case(family, kind, passes, L=None, j=None, form=None):
    return dict(family=family, kind=kind, L=len(passes[0]) if L is None else L, j=j, form=form, passes=passes)


class File:
    def __init__(self, C, glv, n_passes):
        self.C, self.T, self.n_passes, self.cases = C, Table(C, glv), n_passes, []

    def add(self, c):
        assert len(c["passes"]) <= self.n_passes
        c["passes"] = [list(p) for p in c["passes"]] + [[] for _ in range(self.n_passes - len(c["passes"]))]
        self.cases.append(c)

    def counts(self, p):
        return [len(c["passes"][p]) for c in self.cases]

    def words(self):
        T = self.T
        parts = [np.array([MAGIC, len(T.exps), int(T.glv), len(self.cases), self.n_passes, 0, 0, 0], dtype="<u4"), T.wire()]
        for p in range(self.n_passes):
            counts = self.counts(p)
            parts.append(np.array([sum(counts)] + counts, dtype="<u4"))
            parts.append(np.array([w for c in self.cases for w in c["passes"][p]], dtype="<u4"))
        return np.concatenate(parts)


# ---------------------------------------------------------------- the families
def position_bucket(T, rng, kind, L, j, form):
    s = Seq(T, rng)
    for i in range(L):
        if i != j:
            s.ordinary()
        elif kind == "inf":
            s.entry(0, form)
        else:
            prev = T.value(s.words[-1])
            # the first entry of an item meets an accumulator at infinity: there the bucket's sum so far stands in for it
            acc = s.acc() or s.total
            k = {"prev": prev, "negprev": -prev, "runsum": acc, "negrunsum": -acc}[kind] % T.n
            assert k != 0
            s.entry(k, form)
    return s.words


def items_cases(T, rng):
    out = []
    for m in (1, 2, 3):
        out.append(case("items", "full_%d" % (128 * m), [Seq(T, rng).ordinary(128 * m).words]))
        out.append(case("items", "full_plus_one_%d" % (128 * m + 1), [Seq(T, rng).ordinary(128 * m + 1).words]))
    for name, sign in (("equal_sums", 1), ("opposite_sums", -1)):
        s = Seq(T, rng).ordinary(128)
        out.append(case("items", name, [s.item_to(128, sign * s.total).words]))
        s = Seq(T, rng).ordinary(128)
        out.append(case("items", name + "_copy", [s.entry(sign * s.total).words]))      # the remainder item is that one entry
    out.append(case("items", "inf_item_between", [Seq(T, rng).ordinary(128).item_to(128, 0).ordinary(128).words]))
    out.append(case("items", "inf_item_between_plus_one", [Seq(T, rng).ordinary(128).item_to(128, 0).ordinary(129).words]))
    for L in (1, 2, 129):
        out.append(case("items", "all_inf_%d" % L, [[T.word(0, FORMS[i % 2]) for i in range(L)]]))
    return out


def heavy_cases(T, rng):
    """N_HEAVY buckets of 129 entries: one of N_TEMPLATES full items (a prime count, so the buckets a combine block meets on its
    first and second trip differ) and a remainder entry that makes bucket h's sum (HEAVY_SUM0 + h) G, its own; single-item and empty buckets between"""
    templates = [Seq(T, rng).ordinary(128) for _ in range(N_TEMPLATES)]
    out = []
    for h in range(N_HEAVY):
        t = templates[h % N_TEMPLATES]
        out.append(case("heavy_stride", "heavy", [t.words + [T.word(HEAVY_SUM0 + h - t.total, FORMS[h % 2])]]))
        out.append(case("heavy_stride", "single", [Seq(T, rng).ordinary(rng.randint(1, 40)).words]))
        if h % 3 == 0:
            out.append(case("heavy_stride", "empty", [[]]))
    return out


def fill_cases(T, rng):
    """ordinary traffic over the table as it stands (build these last): whatever meets whatever, infinity included"""
    size = len(T.exps)
    return [case("fill", "fill", [[rng.randrange(size) * (2 if T.glv else 1) | (SIGN if rng.random() < 0.5 else 0)
                                   for _ in range(rng.randint(0, 40))]]) for _ in range(N_FILL)]


@functools.lru_cache(maxsize=None)
def single_pass_file(name, seed=20261):
    """position, items, heavy_stride and fill in one pass"""
    C = ev.CURVES[name]
    rng = random.Random(seed)
    F = File(C, False, 1)
    for kind, L, j, form in position_cases():
        F.add(case("position", kind, [position_bucket(F.T, rng, kind, L, j, form)], L, j, form))
    for c in items_cases(F.T, rng) + heavy_cases(F.T, rng) + fill_cases(F.T, rng):
        F.add(c)
    return F


def accumulate_compositions(T, rng):
    """[(kind, [entries of pass 0, entries of pass 1, ...])]: what earlier passes left | what this pass brings"""
    n = T.n

    def fresh(count):
        ks = rng.sample(range(1, SMALL + 1), count)
        return [k * rng.choice([1, -1]) for k in ks]

    def ws(*ks):
        return [T.word(k, rng.choice(FORMS)) for k in ks]

    def multi(size=129):
        return Seq(T, rng).ordinary(size)

    out = []
    for kind in ACC_KINDS2 + ACC_KINDS3:
        P, Q, R = fresh(3)
        simple = {"empty|Q": [[], [Q]], "P|empty": [[P], []], "P,-P|Q": [[P, -P], [Q]], "P|P": [[P], [P]], "P|-P": [[P], [-P]],
                  "P|-P,Q,R": [[P], [-P, Q, R]], "P,Q|P,Q": [[P, Q], [P, Q]], "P|Q,-Q,-P": [[P], [Q, -Q, -P]],
                  # an odd and an even number of additions in either pass: the stored Y of an odd count is the 4p - Y form
                  "P|Q": [[P], [Q]], "P|Q,R": [[P], [Q, R]], "P,Q|R": [[P, Q], [R]], "P,Q|R,P": [[P, Q], [R, P]],
                  "P|inf": [[P], [0]], "P|inf,inf,inf": [[P], [0, 0, 0]],
                  "P|-P|Q": [[P], [-P], [Q]], "P|Q|R": [[P], [Q], [R]], "P|empty|Q": [[P], [], [Q]], "empty|empty|Q": [[], [], [Q]]}
        if kind in simple:
            passes = [ws(*p) for p in simple[kind]]
        elif kind == "P|multi_inf":
            passes = [ws(P), ws(*[0] * 129)]
        elif kind == "multi|inf":
            passes = [multi().words, ws(0, 0)]
        elif kind in ("multi|S", "multi|-S"):
            m = multi()
            passes = [m.words, ws(m.total if kind == "multi|S" else -m.total)]
        elif kind in ("P|multi_total_P", "P|multi_total_-P", "P|multi_total_-P|Q"):
            m = multi(128)                                        # the remainder entry sets the bucket's total
            passes = [ws(P), m.entry((-P if "-P" in kind else P) - m.total).words] + ([ws(Q)] if kind.endswith("|Q") else [])
        elif kind in ("P|multi_item0_P", "P|multi_item0_-P"):
            # lane 0 of the combine adds its item to the stored sum first: that addition doubles, or gives infinity and the fold goes on
            passes = [ws(P), Seq(T, rng).item_to(128, P if kind.endswith("_P") else -P).ordinary(2).words]
        elif kind == "multi|multi":
            passes = [multi().words, multi(257).words]
        elif kind == "multi|multi_inf":
            passes = [multi().words, ws(*[0] * 130)]
        elif kind == "multi|multi_total_-S":
            m, m2 = multi(300), multi(128)
            passes = [m.words, m2.entry(-m.total - m2.total).words]
        elif kind == "multi|P|multi":
            passes = [multi().words, ws(P), multi(256).words]
        out.append((kind, passes))
    return out


@functools.lru_cache(maxsize=None)
def accumulate_file(name, seed=20262):
    """three passes: every two-pass composition in passes 0, 1 (pass 2 leaves it alone) and again in passes 1, 2 behind an empty
    pass 0 (a stored infinity), and the three-pass chains"""
    C = ev.CURVES[name]
    rng = random.Random(seed)
    F = File(C, False, 3)
    for kind, passes in accumulate_compositions(F.T, rng):
        F.add(case("accumulate", kind, passes))
    for kind, passes in accumulate_compositions(F.T, rng):
        if len(passes) == 2:
            F.add(case("accumulate", "late:" + kind, [[]] + passes))
    return F


@functools.lru_cache(maxsize=None)
def glv_file(name, seed=20263):
    """one pass over the doubled table"""
    C = ev.CURVES[name]
    rng = random.Random(seed)
    F = File(C, True, 1)
    T = F.T
    for form in FORMS:
        for other in FORMS:
            P, Q = [k * rng.choice([1, -1]) for k in rng.sample(range(1, SMALL + 1), 2)]
            two = lambda a, b: [T.word(a[0], form, a[1]), T.word(b[0], other, b[1])]
            F.add(case("glv", "P,-phiP", [two((P, False), (-P, True))], form=form))
            F.add(case("glv", "phiP,phiP", [two((P, True), (P, True))], form=form))
            F.add(case("glv", "phiP,-phiP,Q", [two((P, True), (-P, True)) + [T.word(Q, form, rng.random() < 0.5)]], form=form))
            F.add(case("glv", "P,phiP", [two((P, False), (P, True))], form=form))
        for kind, sign in (("phi_runsum", 1), ("phi_negrunsum", -1)):
            for L in (3, 9, 131):
                s = Seq(T, rng).ordinary(L - 2)
                # the accumulator's value as a table point of its own, taken through its odd slot: lambda (acc / lambda)
                k = sign * s.acc() * pow(T.lam, -1, T.n)
                F.add(case("glv", kind, [s.entry(k, form, True).ordinary(1).words], form=form))
    F.add(case("glv", "mixed_multi", [Seq(T, rng).ordinary(300).words]))
    F.add(case("glv", "all_inf", [[T.word(0, "plain", True), T.word(0, "signbit", False), T.word(0, "signbit", True)]]))
    for _ in range(N_GLV_MIXED):
        F.add(case("glv", "mixed", [Seq(T, rng).ordinary(rng.randint(1, 40)).words]))
    size = T.size()
    for _ in range(60):                                           # any slot with any sign, infinity's two slots included
        F.add(case("glv", "fill", [[rng.randrange(size) | (SIGN if rng.random() < 0.5 else 0) for _ in range(rng.randint(0, 40))]]))
    return F


FILES = {"single": single_pass_file, "accumulate": accumulate_file, "glv": glv_file}


# ---------------------------------------------------------------- expectations
def combine_model(n, stored, items):
    """k_bucket_combine in the exponent: lane k holds item k (lane 0 behind the stored sum when accumulating), the lanes fold
    32, 16, .. 1.  -> (exponent, bound key): "add" when the stored value came out of an addition or a doubling (a doubling's
    bound lies inside an addition's), "operand" when one item's sum passed through additions with infinity only"""
    assert len(items) <= 64
    lanes = [(0, None)] * 64

    def add(a, b):
        if b[0] == 0:
            return a
        if a[0] == 0:
            return b
        s = (a[0] + b[0]) % n
        return (s, "add") if s else (0, None)
    if stored:
        lanes[0] = (stored, "operand")
    for k, it in enumerate(items):
        lanes[k] = add(lanes[k], (it, "operand") if it else (0, None))
    m = 32
    while m >= 1:
        for t in range(m):
            lanes[t] = add(lanes[t], lanes[t + m])
        m >>= 1
    return lanes[0]


def expected(F):
    """per pass, per bucket: dict(exp = the sum's exponent, key = the bound key of ec_vectors.BOUNDS, same = bit-identical to
    what the previous pass left)"""
    T, n = F.T, F.T.n
    out = []
    prev = [dict(exp=0, key=None, same=False) for _ in F.cases]
    for p in range(F.n_passes):
        cur = []
        for b, c in enumerate(F.cases):
            vals = [T.value(w) for w in c["passes"][p]]
            stored = prev[b]["exp"] if p else 0
            if not vals:                                          # pass 0 writes infinity; later passes leave the bucket alone
                e = dict(exp=stored, key=prev[b]["key"], same=p > 0)
            elif p and not any(vals):                             # only points at infinity: the stored sum comes back unchanged
                e = dict(exp=stored, key=prev[b]["key"], same=True)
            elif len(vals) <= CHUNK:                              # one item: k_bucket_sum30 stores the bucket
                e = dict(exp=(stored + sum(vals)) % n, key="flip_finish", same=False)
            else:
                items = [sum(vals[i:i + CHUNK]) % n for i in range(0, len(vals), CHUNK)]
                exp, key = combine_model(n, stored, items)
                assert exp == (stored + sum(vals)) % n
                e = dict(exp=exp, key=key, same=False)
            cur.append(e)
        out.append(cur)
        prev = cur
    return out


_CHUNK_SUMS = {}


def sum_one_by_one(F, words):
    """the entries' points added one after the other with ec_vectors.ec_add (a full item that stands in many buckets, the
    templates of heavy_stride, is added up once)"""
    C, total = F.C, None
    for i in range(0, len(words), CHUNK):
        chunk = tuple(words[i:i + CHUNK])
        key = (C.name, id(F.T), chunk)
        if key in _CHUNK_SUMS:
            acc = _CHUNK_SUMS[key]
        else:
            acc = None
            for w in chunk:
                acc = ev.ec_add(C, acc, F.T.point(w))
            if len(chunk) == CHUNK:
                _CHUNK_SUMS[key] = acc
        total = ev.ec_add(C, total, acc)
    return total


# ---------------------------------------------------------------- running the driver
def run(F, timeout=60):
    """-> per pass dict(buckets [nb, 32], ctrl, order [items, 2], chunk_base, heavy)"""
    nb = len(F.cases)
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in"), os.path.join(d, "out")
        F.words().tofile(fin)
        r = subprocess.run([EXE, F.C.name, fin, fout], capture_output=True, text=True, timeout=timeout)
        assert r.returncode == 0, "bucket_sum_check failed (%d): %s%s" % (r.returncode, r.stdout, r.stderr)
        raw = np.fromfile(fout, dtype="<u4")
    return parse(F, raw)


def parse(F, raw):
    """the driver's output file, pass by pass"""
    nb = len(F.cases)
    out, at = [], 0
    for _ in range(F.n_passes):
        buckets = raw[at:at + 32 * nb].reshape(nb, 32)
        at += 32 * nb
        ctrl = raw[at:at + CTRL_WORDS]
        at += CTRL_WORDS
        n_items, n_heavy = int(ctrl[3]), int(ctrl[2])
        order = raw[at:at + 2 * n_items].reshape(n_items, 2)
        at += 2 * n_items
        chunk_base = raw[at:at + nb]
        at += nb
        heavy = raw[at:at + n_heavy]
        at += n_heavy
        out.append(dict(buckets=buckets, ctrl=ctrl, order=order, chunk_base=chunk_base, heavy=heavy))
    assert at == raw.size, "the output holds %d words, %d were read" % (raw.size, at)
    return out
