"""Bucket arrays, expected nodes and the layout model for the bucket reduction tree driven node by node (tools/tree_check.hip):
shared by tests/test_tree_gpu.py and tests/test_tree_vectors_cpu.py.

Everything is computed IN THE EXPONENT: bucket b of a window holds e_b G for a known e_b (0: the point at infinity), so
  S^l[i]       = sum of e_b over b in [i 2^(l+1), (i+1) 2^(l+1))
  fin[w][0]    = sum of all of the window's e_b
  fin[w][1+k]  = sum of e_b over the b whose index has bit k set
and an addition's operands can be made equal, opposite or infinite by adjusting one bucket.  The node POINTS are built bottom-up with
ec_vectors.ec_add; the roots and every M_k are compared with bucket_vectors.mul(C, exponent) by the CPU module.  Generation is
deterministic (fixed seeds) and reads nothing outside the repository.

A CASE is one window (the windows of a tree are independent).  A SECTION is one header of the driver's input -- (c, W, lone, option
overrides) -- with its runs of W cases each; a FILE is one driver run: a list of sections.
"""
import functools
import os
import random
import subprocess
import tempfile

import numpy as np

from tests import bucket_vectors as bv
from tests import common
from tests import ec_vectors as ev
from tests import ladder_vectors as lv

EXE = os.path.join(common.ROOT, "porla_amd", "tree_check")
MAGIC, HDR, DEFAULT, FILL = 0x54524545, 12, 0xffffffff, 0xA5A5A5A5
MAX_C, MAX_BUCKETS = 17, 1 << 18
ALL_QUAD, NO_QUAD = 1 << 30, 0                        # quad_max_tasks: every non-tail level as level_quad | as level

KINDS = ["equal", "opposite", "left_inf", "right_inf", "both_inf"]
ORIGINS = ["empty", "cancel"]                         # how an infinite operand comes about: empty buckets | sums that cancel
POSITIONS = ["first", "last", "last_of_last_window"]
SLOT_C = 5                                            # the slot family's window: 16 buckets, levels 0 .. 3
BALLOT_C = 6                                          # 16 nodes per window at level 0: node j is quad j of its wave
BALLOT_NODES = [0, 7, 8, 15]                          # quads of a wave whose ballot shifts are 0, 28, 32, 60
SHAPE_C, SHAPE_W = [2, 3, 4, 8, 9, 10, 11, 12], [1, 2, 3, 5]
L0_BY_C = {2: 0, 3: 0, 4: 0, 8: 0, 9: 0, 10: 3, 11: 5, 12: 6}
PLAN_C, PLAN_W = list(range(2, 18)), [1, 2, 3, 4, 5, 8, 15, 16, 17]


# ---------------------------------------------------------------- cases
class Case:
    """one window: exps[b] = the exponent of bucket b; top: every bucket at the top of the operand bound (BN254)"""

    def __init__(self, family, kind, exps, top=False, **meta):
        self.family, self.kind, self.exps, self.top, self.meta = family, kind, list(exps), top, meta
        self.B = len(self.exps)
        self.c = self.B.bit_length()
        assert self.B == 1 << (self.c - 1) and self.c >= 2

    def __repr__(self):
        return "%s/%s c=%d %s" % (self.family, self.kind, self.c, self.meta)


def ordinary(rng, B, n, density=1.0):
    """pairwise distinct non-zero multiples +-k, k <= bv.SMALL where the window is small enough for that (their sums are then
    ordinary too, up to chance -- the expected values follow the group law whatever meets); a larger window draws them with repetition"""
    if B <= bv.SMALL // 2:
        ks = rng.sample(range(1, bv.SMALL + 1), B)
    else:
        ks = [rng.randrange(1, bv.SMALL + 1) for _ in range(B)]
    return [(k * rng.choice([1, -1])) % n if rng.random() < density else 0 for k in ks]


def operand_sets(l, s, i):
    """the buckets under the two operands of the addition at level l, slot s, node i of a window: the S addition (s = l) adds the
    node's two halves, slot s < l the buckets of either half whose index has bit s set (s = l - 1: the aliased slot, read from
    S^(l-2)[4i + 1] and [4i + 3])"""
    lo, half = i << (l + 1), 1 << l
    pick = lambda r: [b for b in r if s == l or (b >> s) & 1]
    return pick(range(lo, lo + half)), pick(range(lo + half, lo + 2 * half))


def slot_case(rng, n, c, l, s, pos, kind, origin):
    """all buckets random, then the operands of (l, s, node) made `kind`: infinite operands by emptying their buckets or by
    adjusting one of them so that the sum cancels, equal / opposite by adjusting one bucket of the right-hand side"""
    B = 1 << (c - 1)
    node = 0 if pos == "first" else (B >> (l + 1)) - 1
    L, R = operand_sets(l, s, node)
    while True:
        e = ordinary(rng, B, n)
        for side, name in ((L, "left_inf"), (R, "right_inf")):
            if kind in (name, "both_inf"):
                if origin == "empty":
                    for b in side:
                        e[b] = 0
                else:
                    assert len(side) >= 2
                    e[side[-1]] = (-sum(e[b] for b in side[:-1])) % n
        sl, sr = sum(e[b] for b in L) % n, sum(e[b] for b in R) % n
        if kind in ("equal", "opposite"):
            e[R[-1]] = (e[R[-1]] + (sl if kind == "equal" else -sl) - sr) % n
            if e[R[-1]] == 0 or sl == 0:
                continue
        elif (kind == "left_inf" and sr == 0) or (kind == "right_inf" and sl == 0):
            continue
        return Case("slot", kind, e, l=l, s=s, pos=pos, node=node, origin=origin if kind.endswith("_inf") else None)


def slot_grid(c=SLOT_C):
    """(l, s, pos, kind, origin): every level, every slot s <= l, the three node positions, the five operand kinds; infinite
    operands once by empty buckets and, where an operand covers more than one bucket, once by sums that cancel"""
    out = []
    for l in range(c - 1):
        for s in range(l + 1):
            cancel = len(operand_sets(l, s, 0)[0]) >= 2
            for pos in POSITIONS:
                for kind in KINDS:
                    for origin in (ORIGINS if kind.endswith("_inf") and cancel else ORIGINS[:1]):
                        out.append((l, s, pos, kind, origin))
    return out


def ballot_case(rng, n, c, node, kind):
    """level 0, node `node` of the window: with 16 nodes per window at c = 6 the node's quad is quad `node` of its wave, in the
    level kernels (task = global node index, 16 per window) and in the tail (task = the window's node index)"""
    e = ordinary(rng, 1 << (c - 1), n)
    a, b = 2 * node, 2 * node + 1
    if kind == "equal":
        e[b] = e[a]
    elif kind == "opposite":
        e[b] = (-e[a]) % n
    if kind in ("left_inf", "both_inf"):
        e[a] = 0
    if kind in ("right_inf", "both_inf"):
        e[b] = 0
    return Case("slot", kind, e, l=0, s=0, pos="ballot", node=node, origin="empty" if kind.endswith("_inf") else None)


# ---------------------------------------------------------------- sections and files
class Section:
    def __init__(self, c, W, lone, runs, parts=None, front2=None, quad_max=None, l0=None, label=""):
        self.c, self.W, self.lone, self.runs, self.label = c, W, lone, runs, label
        self.opts = (parts, front2, quad_max, l0)
        assert all(len(r) == W and all(k.c == c for k in r) for r in runs) and runs
        assert c <= MAX_C and (W << (c - 1)) <= MAX_BUCKETS

    def group(self):
        return (self.c, self.W, self.lone) + self.opts

    def header(self):
        o = [DEFAULT if v is None else v for v in self.opts]
        return np.array([MAGIC, self.c, self.W, self.lone] + o + [len(self.runs), 0, 0, 0], dtype="<u4")

    def default_plan(self):
        return self.opts == (None, None, None, None)


class File:
    def __init__(self, C, name, sections):
        self.C, self.name, self.sections = C, name, sections

    def words(self):
        parts = []
        for sc in self.sections:
            parts.append(sc.header())
            for r in sc.runs:
                parts += [case_words(self.C, k) for k in r]
        return np.concatenate([p.reshape(-1) for p in parts])

    def cases(self):
        return [k for sc in self.sections for r in sc.runs for k in r]


def pack_runs(cases, W, last=None):
    """runs of W windows; `last`: cases that must stand as the last window of their run (one per run, the others fill up)"""
    last = list(last or [])
    cases = list(cases)
    runs = []
    while cases or last:
        tail = [last.pop(0)] if last else []
        head = cases[:W - len(tail)]
        cases = cases[W - len(tail):]
        run = head + tail
        while len(run) < W:                                   # fill up with a window that is already there
            run.insert(0, (runs[0] if runs else run)[0])
        runs.append(run)
    return runs


_WORDS, _EXPECT = {}, {}


def case_words(C, k):
    """[B, 32] words of the window's buckets in the lazy memory form: a random l per bucket, BN254's free multiples of p random
    within the operand bound (top: as many as fit, Y up to 4p, and for every other bucket a residue just under a multiple of p)"""
    key = (C.name, id(k))
    if key not in _WORDS:
        rng = random.Random("%s %s %d %d" % (k.family, k.kind, k.c, sum(k.exps[:16]) & 0xffff))
        out = np.zeros((k.B, 32), dtype="<u4")
        for b, e in enumerate(k.exps):
            P = bv.mul(C, e)
            if P is None:
                continue
            if k.top and C is ev.BN254:
                l = ev.find_l_high(C, P, (b >> 1) % 4, rng) if b % 2 else rng.randrange(1, C.p)
                vals = ev.rep_mem(C, P, l, mult="top", y_max=4 * C.p)
            else:
                vals = ev.rep_mem(C, P, rng.randrange(1, C.p), rng=rng)
            out[b] = [w for v in vals for w in ev.words(v)]
        _WORDS[key] = (k, out)                                 # (the case is kept alive: its id is the key)
    return _WORDS[key][1]


# ---------------------------------------------------------------- expectations
def combine(C, n, a, b):
    """(exponent, point, bound key of ec_vectors.BOUNDS) of a + b: an addition, a doubling, or the other operand passing through"""
    if b[0] == 0:
        return a
    if a[0] == 0:
        return b
    e = (a[0] + b[0]) % n
    if e == 0:
        return (0, None, None)
    return (e, ev.ec_add(C, a[1], b[1]), "double" if a[0] == b[0] else "add")


def expected(C, k):
    """dict(S = [S^0, .., S^(nlev-1)] as lists of (exponent, point, key), fin = [(exponent, point)] * c): the tree as the kernels
    run it -- the S additions, slot l - 1 from the odd entries of S^(l-2), the other slots from their own halves"""
    key = (C.name, id(k))
    if key in _EXPECT:
        return _EXPECT[key][1]
    n, nlev = lv.order(C), k.c - 1
    inf = (0, None, None)
    Ss = [[(e % n, bv.mul(C, e), "operand") if e % n else inf for e in k.exps]]
    M = []
    for l in range(nlev):
        nw = k.B >> (l + 1)
        prev = Ss[-1]
        newM = []
        for s in range(l):
            if s == l - 1:
                src = Ss[l - 1]
                newM.append([combine(C, n, src[4 * i + 1], src[4 * i + 3]) for i in range(nw)])
            else:
                newM.append([combine(C, n, M[s][2 * i], M[s][2 * i + 1]) for i in range(nw)])
        Ss.append([combine(C, n, prev[2 * i], prev[2 * i + 1]) for i in range(nw)])
        M = newM
    fin = [Ss[-1][0]] + [m[0] for m in M] + [Ss[nlev - 1][1]]
    assert len(fin) == k.c
    out = dict(S=Ss[1:], fin=[(e, P) for e, P, _ in fin])
    _EXPECT[key] = (k, out)
    return out


def fin_exponents(k, n):
    """the defining sums, straight from the bucket list"""
    return [sum(k.exps) % n] + [sum(e for b, e in enumerate(k.exps) if (b >> j) & 1) % n for j in range(k.c - 1)]


# ---------------------------------------------------------------- the families
def _rng(name, tag):
    return random.Random("%s %s" % (name, tag))


@functools.lru_cache(maxsize=None)
def slot_cases(name):
    C = ev.CURVES[name]
    n, rng = lv.order(C), _rng(name, "slot")
    grid = [slot_case(rng, n, SLOT_C, *g) for g in slot_grid()]
    ballots = [ballot_case(rng, n, BALLOT_C, node, kind) for node in BALLOT_NODES for kind in KINDS]
    return grid, ballots


def forced_plans(c):
    """(label, options) for a window size whose own plan is the tail alone: that plan, the tail from the middle level, and every
    non-tail level as k_tree_level / as k_tree_level_quad, without and with k_tree_front2 in front"""
    top = c - 2                                       # nlev - 1: the tail runs the last level only
    return [("default", {}),
            ("l0_%d" % (c // 2), dict(l0=c // 2)),
            ("all_level", dict(l0=top, quad_max=NO_QUAD)),
            ("all_level_quad", dict(l0=top, quad_max=ALL_QUAD)),
            ("front2_level", dict(l0=top, quad_max=NO_QUAD, front2=1)),
            ("front2_level_quad", dict(l0=top, quad_max=ALL_QUAD, front2=1))]


FORCED_SLOT, FORCED_6 = forced_plans(SLOT_C), forced_plans(6)


@functools.lru_cache(maxsize=None)
def slot_file(name):
    """the slot family at c = 5, W = 3 and its ballot cases at c = 6, W = 3, once per plan of forced_plans.  The last window of
    every run of the c = 5 sections is a last_of_last_window case: its last node's S task is the launch's last task, beside the
    padding quads"""
    grid, ballots = slot_cases(name)
    last = [k for k in grid if k.meta["pos"] == "last_of_last_window"]
    rest = [k for k in grid if k.meta["pos"] != "last_of_last_window"]
    runs = pack_runs(rest, 3, last)
    secs = [Section(SLOT_C, 3, 0, runs, label=label, **o) for label, o in FORCED_SLOT]
    secs += [Section(BALLOT_C, 3, 0, pack_runs(ballots, 3), label="ballot_" + label, **o) for label, o in FORCED_6]
    return File(ev.CURVES[name], "slot", secs)


@functools.lru_cache(maxsize=None)
def copy_file(name):
    """the last level's copy task fin[w][c-1] = S^(nlev-2)[2w+1] with that node ordinary, empty and cancelled; c = 2, where the
    tree is one addition and one copy of a bucket, with every operand kind"""
    C = ev.CURVES[name]
    n, rng = lv.order(C), _rng(name, "copy")
    secs = []
    two = []
    for kind in ["ordinary", "copy_inf"] + KINDS:
        a, b = ordinary(rng, 2, n)
        e = {"ordinary": [a, b], "copy_inf": [a, 0], "equal": [a, a], "opposite": [a, (-a) % n], "left_inf": [0, b],
             "right_inf": [a, 0], "both_inf": [0, 0]}[kind]
        two.append(Case("copy", kind, e))
    secs.append(Section(2, len(two), 0, [two], label="c2"))
    secs.append(Section(2, len(two), 1, [two], label="c2_lone"))
    secs.append(Section(2, 1, 0, [[k] for k in two[:3]], label="c2_W1"))
    for c in (3, 6, 10):
        B = 1 << (c - 1)
        cs = []
        for kind in ("ordinary", "copy_inf_empty", "copy_inf_cancel"):
            e = ordinary(rng, B, n)
            if kind == "copy_inf_empty":
                e[B // 2:] = [0] * (B // 2)
            elif kind == "copy_inf_cancel":
                e[B - 1] = (-sum(e[B // 2:B - 1])) % n
            cs.append(Case("copy", kind, e))
        secs.append(Section(c, 3, 0, [cs], label="c%d" % c))
    return File(C, "copy", secs)


@functools.lru_cache(maxsize=None)
def sparse_file(name):
    """all buckets empty; one non-empty bucket at index 0, B - 1 and each power of two; all buckets P (doublings at every level
    and slot); alternating P and -P -- under the product's plan (c = 6: the tail) and with every level as level / level_quad / front2"""
    C = ev.CURVES[name]
    n, rng = lv.order(C), _rng(name, "sparse")
    c, B = 6, 32
    cs = [Case("sparse", "all_empty", [0] * B)]
    for at in sorted({0, B - 1} | {1 << j for j in range(c - 1)}):
        e = [0] * B
        e[at] = rng.randrange(1, bv.SMALL)
        cs.append(Case("sparse", "single", e, at=at))
    P = rng.randrange(1, bv.SMALL)
    cs.append(Case("sparse", "all_equal", [P] * B))
    cs.append(Case("sparse", "alternating", [P if b % 2 == 0 else (-P) % n for b in range(B)]))
    cs.append(Case("sparse", "alternating_pairs", [P if b % 4 < 2 else (-P) % n for b in range(B)]))
    runs = pack_runs(cs, 3)
    return File(C, "sparse", [Section(c, 3, 0, runs, label=label, **o) for label, o in FORCED_6])


@functools.lru_cache(maxsize=None)
def shape_windows(name, c):
    C = ev.CURVES[name]
    n, rng = lv.order(C), _rng(name, "shape%d" % c)
    return [Case("shape", "ordinary", ordinary(rng, 1 << (c - 1), n), w=w) for w in range(max(SHAPE_W))]


@functools.lru_cache(maxsize=None)
def shape_file(name):
    """the product's own plan, lone and not lone, c in SHAPE_C x W in SHAPE_W: tail only up to c = 9, level kernels plus tail from
    c = 10.  The W windows of a shape are the first W of five per c, so every plan of a (c, W) sees the same buckets"""
    secs = []
    for c in SHAPE_C:
        for W in SHAPE_W:
            for lone in (0, 1):
                secs.append(Section(c, W, lone, [shape_windows(name, c)[:W]], label="c%d_W%d_lone%d" % (c, W, lone)))
    return File(ev.CURVES[name], "shape", secs)


@functools.lru_cache(maxsize=None)
def forced_file(name):
    """forced plans at the smallest shapes that reach the path: c = 6, W = 3 with l0 = 3 and l0 = nlev - 1 (every non-tail level
    once as level and once as level_quad, front2 followed by either at level 2); parts = 2 with W in {2, 3, 5}, under the tail
    alone and under level kernels; every tail start l0 = 0 .. nlev - 1 at c = 7 (each handover from m_global to the m_tail halves);
    each preceded by the product's own plan over the same buckets"""
    C = ev.CURVES[name]
    secs = []
    w6 = shape_windows_any(name, 6)
    for W in (2, 3, 5):
        secs.append(Section(6, W, 0, [w6[:W]], label="c6_W%d_default" % W))
        for label, o in FORCED_6[1:]:
            if W == 3:
                secs.append(Section(6, W, 0, [w6[:W]], label="c6_W3_" + label, **o))
        secs.append(Section(6, W, 1, [w6[:W]], parts=2, label="c6_W%d_parts2" % W))
        for label, o in FORCED_6[2:]:
            secs.append(Section(6, W, 0, [w6[:W]], parts=2, label="c6_W%d_parts2_%s" % (W, label), **o))
    w7 = shape_windows_any(name, 7)
    secs.append(Section(7, 3, 0, [w7[:3]], label="c7_W3_default"))
    for l0 in range(6):
        for q, qn in ((NO_QUAD, "level"), (ALL_QUAD, "level_quad")):
            secs.append(Section(7, 3, 0, [w7[:3]], l0=l0, quad_max=q, label="c7_W3_l0_%d_%s" % (l0, qn)))
    return File(C, "forced", secs)


@functools.lru_cache(maxsize=None)
def shape_windows_any(name, c):
    C = ev.CURVES[name]
    n, rng = lv.order(C), _rng(name, "forced%d" % c)
    return [Case("forced", "ordinary", ordinary(rng, 1 << (c - 1), n), w=w) for w in range(5)]


DEEP_C = 16


@functools.lru_cache(maxsize=None)
def bounds_file(name):
    """BN254: every bucket at the top of the operand bound (X 5p, Y 4p, ZZ / ZZZ p + eps; every other bucket with a residue just
    under a multiple of p): dense windows at c = 6 under every plan of forced_plans(6), and one deep window, c = 16, W = 1 -- mostly
    empty, with a few dense subtrees whose sums are re-added on every level up to the root"""
    C = ev.CURVES[name]
    assert C is ev.BN254
    n, rng = lv.order(C), _rng(name, "bounds")
    B = 32
    dense = [Case("bounds", "dense", ordinary(rng, B, n), top=True, w=w) for w in range(3)]
    dense.append(Case("bounds", "all_equal", [7] * B, top=True))
    dense.append(Case("bounds", "half_empty", ordinary(rng, B, n, 0.5), top=True))
    dense.append(Case("bounds", "dense", ordinary(rng, B, n), top=True, w=3))
    secs = [Section(6, 3, 0, pack_runs(dense, 3), label=label, **o) for label, o in FORCED_6]
    Bd = 1 << (DEEP_C - 1)
    e = [0] * Bd
    for lo, size in ((0, 64), (Bd // 2 - 32, 64), (Bd - 16, 16), (12345 & ~7, 8)):     # dense subtrees, one across the middle
        e[lo:lo + size] = ordinary(rng, size, n)
    for b in rng.sample(range(Bd), 40):                                                 # and lone buckets on the way up
        e[b] = e[b] or rng.randrange(1, bv.SMALL)
    deep = Case("bounds", "deep", e, top=True)
    for lone in (0, 1):
        secs.append(Section(DEEP_C, 1, lone, [[deep]], label="deep_lone%d" % lone))
    secs.append(Section(DEEP_C, 1, 0, [[deep]], quad_max=NO_QUAD, label="deep_level"))
    secs.append(Section(DEEP_C, 1, 0, [[deep]], quad_max=NO_QUAD, front2=1, label="deep_front2"))
    return File(C, "bounds", secs)


FILES = {"slot": slot_file, "copy": copy_file, "sparse": sparse_file, "shape": shape_file, "forced": forced_file, "bounds": bounds_file}
FILE_NAMES = {"bn254": ["slot", "copy", "sparse", "shape", "forced", "bounds"], "secp256k1": ["slot", "copy", "sparse", "shape", "forced"]}


# ---------------------------------------------------------------- the plan: the driver's text and a restatement of the rules
def parse_plans(text):
    plans = []
    for line in text.splitlines():
        head, _, rest = line.partition(" ")
        d = {}
        for kv in rest.split():
            k, v = kv.split("=")
            d[k] = v if k == "kind" else ([int(x) for x in v.split(",")] if k == "s_lev" else int(v))
        if head == "plan":
            d["parts_info"], d["launches"] = [], []
            plans.append(d)
        elif head == "part":
            plans[-1]["parts_info"].append(d)
        else:
            assert head == "launch", line
            plans[-1]["launches"].append(d)
    return plans


def plan_args(groups):
    return [("-" if v is None else str(v)) for g in groups for v in g]


def dump_plans(curve, groups):
    """tree_check --plan for (c, W, lone, parts, front2, quad_max_tasks, l0) groups (None = the product's default); no device needed"""
    out = []
    for at in range(0, len(groups), 64):
        r = subprocess.run([EXE, "--plan", curve] + plan_args(groups[at:at + 64]), capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, "tree_check --plan failed (%d): %s%s" % (r.returncode, r.stdout, r.stderr)
        out += parse_plans(r.stdout)
    assert len(out) == len(groups)
    return out


@functools.lru_cache(maxsize=None)
def file_plans(curve, name):
    return dump_plans(curve, [sc.group() for sc in FILES[name](curve).sections])


TAIL_THREADS, QUAD_MAX, QUAD_MAX_LONE = 512, 16384, 65536


def tail_start(B, nlev):
    """the tail takes over at the first level whose additions per window, four lanes each, fit one pass of its block"""
    l = 0
    while l + 1 < nlev and (l + 1) * (B >> (l + 1)) > TAIL_THREADS // 4:
        l += 1
    return l


def model_plan(c, W, lone):
    """the product's default plan restated from the comments of msm_tree.hip.h, in the shape parse_plans gives:
      sizes    S nb + 2, M 2 (nb / 4) + 6, tail 2 W (B / 4 + 1) + 4 entries
      parts    two halves (W / 2 and the rest) for a lone caller with W >= 4 and at least 2^18 buckets
      l0       tail_start
      front2   not lone, l0 >= 2, the part's bucket count divisible by 4 and more than 16 384 additions at level 0
      quad     a non-tail level of up to 16 384 (lone: 65 536) additions runs four lanes per addition
      layout   per part: S level l behind nbp - (nbp >> l) entries; M halves nbp / 4 + 1 apart, level l writes half l & 1;
               the tail's halves Wp (B / 4 + 1) + 1 apart; the parts' areas follow each other with one entry of slack per half"""
    B, nlev = 1 << (c - 1), c - 1
    nb = W * B
    parts = 2 if (lone and W >= 4 and nb >= 1 << 18) else 1
    l0 = tail_start(B, nlev)
    quad_max = QUAD_MAX_LONE if lone else QUAD_MAX
    plan = dict(c=c, W=W, lone=lone, parts=parts, nlev=nlev, B=B, s_entries=nb + 2, m_entries=2 * (nb // 4) + 6,
                mt_entries=2 * W * (B // 4 + 1) + 4, fin_entries=W * c, tail_threads=TAIL_THREADS, parts_info=[], launches=[])
    s_off = m_off = mt_off = w0 = 0
    for part in range(parts):
        Wp = W if parts == 1 else (W // 2 if part == 0 else W - W // 2)
        nbp = Wp * B
        half = [m_off, m_off + nbp // 4 + 1]
        s_level = lambda l: s_off + nbp - (nbp >> l)
        front2 = (not lone) and l0 >= 2 and nbp % 4 == 0 and nbp // 2 > QUAD_MAX
        plan["parts_info"].append(dict(part=part, w0=w0, Wp=Wp, l0=l0, front2=int(front2), quad_max=quad_max))
        first = 0
        if front2:
            n = nbp // 4
            plan["launches"].append(dict(part=part, kind="front2", l=1, n=n, grid=(n + 255) // 256, block=256, bk=w0 * B, s_prev_bk=1, s_prev=0,
                                         s_prev2_bk=1, s_prev2=0, s_out=s_level(0), s1_out=s_level(1), m_prev=half[0], m_out=half[1],
                                         m_prev_stride=0, m_out_stride=n, nb=nbp, nlev=nlev))
            first = 2
        for l in range(first, l0):
            n = nbp >> (l + 1)
            tasks = (l + 1) * n
            quad = tasks <= quad_max
            plan["launches"].append(dict(part=part, kind="level_quad" if quad else "level", l=l, n=n,
                                         grid=((4 if quad else 1) * tasks + 255) // 256, block=256, bk=w0 * B,
                                         s_prev_bk=int(l == 0), s_prev=s_level(l - 1) if l else 0, s_prev2_bk=int(l < 2),
                                         s_prev2=s_level(l - 2) if l >= 2 else 0, s_out=s_level(l), s1_out=0, m_prev=half[(l + 1) & 1],
                                         m_out=half[l & 1], m_prev_stride=2 * n, m_out_stride=n, nb=nbp, nlev=nlev))
        pw = B // 4 + 1
        threads = min(TAIL_THREADS, max(64, ((l0 + 2) * (B >> (l0 + 1)) * 4 + 63) // 64 * 64))
        plan["launches"].append(dict(part=part, kind="tail", l=l0, n=Wp, grid=Wp, block=threads, bk=w0 * B, m_global=half[(l0 + 1) & 1],
                                     m_tail0=mt_off, m_tail1=mt_off + Wp * pw + 1, per_window=pw, fin=w0 * c, nb=nbp, B=B, nlev=nlev,
                                     s_lev=[s_level(l) for l in range(nlev)]))
        s_off += nbp + 1
        m_off += 2 * (nbp // 4) + 2
        mt_off += 2 * Wp * pw + 2
        w0 += Wp
    return plan


# ---------------------------------------------------------------- what a plan's launches read and write
class Layout:
    """runs a plan's launches over tag arrays (0 = never written, else 1 + the level that wrote the entry) and asserts on the way:
    every access inside the stated sizes; every entry read was written by the level the reader means, in an earlier launch of the
    same part (or earlier in the same window of the tail) or is a bucket; within a launch no read range overlaps a write range;
    the tail's windows touch only their own entries.  Afterwards: written[area] = the entries the plan writes"""

    def __init__(self, plan):
        self.plan = plan
        self.size = dict(S=plan["s_entries"], M=plan["m_entries"], T=plan["mt_entries"], F=plan["fin_entries"], B=plan["W"] * plan["B"])
        self.tag = {a: np.zeros(self.size[a], dtype=np.int16) for a in "SMTF"}
        self.owner = {a: np.full(self.size[a], -1, dtype=np.int32) for a in "SMTF"}        # part * 2^16 + window (tail), part (levels)
        self.s_nodes = {}                                                              # (part, l) -> first entry of S^l
        for q in plan["launches"]:
            self.reads, self.writes = [], []
            (self.tail if q["kind"] == "tail" else self.front2 if q["kind"] == "front2" else self.level)(q)
        self.written = {a: self.tag[a] != 0 for a in "SMTF"}

    def where(self, q):
        p = self.plan
        return "c=%d W=%d lone=%d part %d %s l=%d" % (p["c"], p["W"], p["lone"], q["part"], q["kind"], q["l"])

    def rd(self, q, area, idx, level, who):
        """entries idx of `area` are read as the values level `level` wrote (B: buckets)"""
        idx = np.asarray(idx, dtype=np.int64)
        if idx.size == 0:
            return
        assert idx.min() >= 0 and idx.max() < self.size[area], "%s: reads %s[%d..%d] of %d" % (self.where(q), area, idx.min(), idx.max(), self.size[area])
        if area == "B":
            lo, n = q["bk"], q["nb"]
            assert idx.min() >= lo and idx.max() < lo + n, self.where(q) + ": reads another part's buckets"
            return
        assert np.all(self.tag[area][idx] == level + 1), "%s: reads %s entries that level %d did not write" % (self.where(q), area, level)
        own = self.owner[area][idx]
        assert np.all((own == who) | (own == q["part"] << 16 | 0xffff)), self.where(q) + ": reads another part's or window's entries"
        self.reads.append((area, int(idx.min()), int(idx.max())))

    def wr(self, q, area, idx, level, who):
        idx = np.asarray(idx, dtype=np.int64)
        if idx.size == 0:
            return
        assert idx.min() >= 0 and idx.max() < self.size[area], "%s: writes %s[%d..%d] of %d" % (self.where(q), area, idx.min(), idx.max(), self.size[area])
        assert len(np.unique(idx)) == idx.size, self.where(q) + ": writes an entry twice"
        own = self.owner[area][idx]
        assert np.all((own == -1) | (own == who) | (own == q["part"] << 16 | 0xffff)), self.where(q) + ": writes another part's or window's entries"
        if area in "SF":
            assert np.all(self.tag[area][idx] == 0), self.where(q) + ": writes an S or fin entry a second time"
        self.pending.append((area, idx, level + 1, who))
        self.writes.append((area, int(idx.min()), int(idx.max())))

    def commit(self, q):
        for area, lo, hi in self.reads:
            for a2, lo2, hi2 in self.writes:
                assert a2 != area or hi < lo2 or hi2 < lo, "%s: reads %s[%d..%d] and writes [%d..%d]" % (self.where(q), area, lo, hi, lo2, hi2)
        for area, idx, tag, who in self.pending:
            self.tag[area][idx] = tag
            self.owner[area][idx] = who
        self.pending, self.reads, self.writes = [], [], []

    def front2(self, q):
        self.pending = []
        who = q["part"] << 16 | 0xffff
        n, i = q["n"], np.arange(q["n"])
        assert q["s_prev_bk"] and q["l"] == 1 and q["grid"] * q["block"] >= n
        self.rd(q, "B", q["bk"] + np.arange(4 * n), -1, who)
        self.wr(q, "S", q["s_out"] + 2 * i + 1, 0, who)               # the odd entries of S^0; the even ones stay in registers
        self.wr(q, "S", q["s1_out"] + i, 1, who)
        self.wr(q, "M", q["m_out"] + i, 1, who)
        self.s_nodes[(q["part"], 0)], self.s_nodes[(q["part"], 1)] = q["s_out"], q["s1_out"]
        self.commit(q)

    def level_ops(self, q, l, n, i, jp, jo, a, who, last):
        """the additions of one level over the nodes i (tree_op): a = the level's arguments"""
        src = lambda bk, off, idx: ("B", q["bk"] + idx) if bk else ("S", off + idx)
        self.rd(q, *src(a["s_prev_bk"], a["s_prev"], np.concatenate([2 * i, 2 * i + 1])), l - 1, who)
        if l >= 1:
            self.rd(q, *src(a["s_prev2_bk"], a["s_prev2"], np.concatenate([4 * i + 1, 4 * i + 3])), l - 2, who)
        for s in range(l - 1):
            self.rd(q, a["m_area_prev"], a["m_prev"] + s * a["m_prev_stride"] + np.concatenate([2 * jp, 2 * jp + 1]), l - 1, who)
        if last:
            c = self.plan["c"]
            self.wr(q, "F", np.concatenate([a["fin"] + i * c + k for k in range(c)]), l, who)
            return
        self.wr(q, "S", a["s_out"] + i, l, who)
        for s in range(l):
            self.wr(q, a["m_area_out"], a["m_out"] + s * a["m_out_stride"] + jo, l, who)

    def level(self, q):
        self.pending = []
        who = q["part"] << 16 | 0xffff
        l, n = q["l"], q["n"]
        tasks = (l + 1) * n
        assert q["grid"] * q["block"] >= tasks * (4 if q["kind"] == "level_quad" else 1) and n == q["nb"] >> (l + 1)
        i = np.arange(n)
        self.level_ops(q, l, n, i, i, i, dict(q, m_area_prev="M", m_area_out="M"), who, False)
        self.s_nodes[(q["part"], l)] = q["s_out"]
        self.commit(q)

    def tail(self, q):
        """window by window, level by level: the blocks run at their own pace, so a window may touch only its own entries"""
        l0, nlev, B, pw = q["l"], q["nlev"], q["B"], q["per_window"]
        assert q["grid"] == q["n"] and q["block"] % 64 == 0 and 64 <= q["block"] <= self.plan["tail_threads"] and q["nb"] == q["n"] * B
        for l in range(nlev):
            self.s_nodes[(q["part"], l)] = q["s_lev"][l]
        for w in range(q["n"]):
            who = q["part"] << 16 | w
            for l in range(l0, nlev):
                self.pending = []
                nw = B >> (l + 1)
                first = l == l0
                j = np.arange(nw)
                i = w * nw + j
                n = q["nb"] >> (l + 1)
                a = dict(s_prev_bk=int(l == 0), s_prev=q["s_lev"][l - 1] if l else 0, s_prev2_bk=int(l < 2),
                         s_prev2=q["s_lev"][l - 2] if l >= 2 else 0, s_out=q["s_lev"][l],
                         m_area_prev="M" if first else "T", m_prev=q["m_global"] if first else q["m_tail%d" % ((l + 1) & 1)] + w * pw,
                         m_prev_stride=2 * n if first else 2 * nw, m_area_out="T", m_out=q["m_tail%d" % (l & 1)] + w * pw, m_out_stride=nw,
                         fin=q["fin"])
                self.level_ops(q, l, n, i, i if first else j, j, a, who, l + 1 == nlev)
                self.commit(q)

    def s_entry(self, part, l, node):
        """the S-area entry of node `node` (counted over the part's windows) of level l"""
        return self.s_nodes[(part, l)] + node


def part_of(plan, w):
    for i, p in enumerate(plan["parts_info"]):
        if p["w0"] <= w < p["w0"] + p["Wp"]:
            return i, p
    raise AssertionError(w)


# ---------------------------------------------------------------- running the driver
def run(F, timeout=60):
    """-> per section, per run: dict(fin [W * c, 32], S, M, T [entries, 32])"""
    plans = file_plans(F.C.name, F.name)
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in"), os.path.join(d, "out")
        F.words().tofile(fin)
        r = subprocess.run([EXE, F.C.name, fin, fout], capture_output=True, text=True, timeout=timeout)
        assert r.returncode == 0, "tree_check failed (%d): %s%s" % (r.returncode, r.stdout, r.stderr)
        raw = np.fromfile(fout, dtype="<u4")
    out, at = [], 0
    for sc, plan in zip(F.sections, plans):
        runs = []
        for _ in sc.runs:
            o = {}
            for area, key in (("fin", "fin_entries"), ("S", "s_entries"), ("M", "m_entries"), ("T", "mt_entries")):
                o[area] = raw[at:at + 32 * plan[key]].reshape(plan[key], 32)
                at += 32 * plan[key]
            runs.append(o)
        out.append(runs)
    assert at == raw.size, "the output holds %d words, %d were read" % (raw.size, at)
    return out
