"""Chosen operands and scalars for the per-form checks of the MAC decode's inverse stage kernels (tools/ladder_check.hip: istage_quad,
istage_quad_uniform, istage1_quad -> icc_mac_decode.hip.h: k_imd_stage_quad, k_imd_stage1_quad), with the expected outputs
(A, B) -> (A + B, s (A - B)) on Python integers (tests/ec_vectors.py's group law).  Built on tests/ladder_vectors.py: the same launch
files, shapes (which butterfly reads which table entry) and memory-form representations.

Operands: a generic pair, A == B (a doubling in the sum, infinity in the difference), A == -B (infinity in the sum, a doubling in the
difference), A or B or both at infinity, and B in the representations at the top of the memory form's bounds (the stage records'
counterpart of a byte string with x >= p: noncanonical_bytes below is that byte string, for the load step).  Scalars: 1, q - 1, one
with each endomorphism half zero, and real inverse twiddles of the table of 2^16."""
import functools
import random

import numpy as np

from tests import common  # noqa: F401  (puts oracle/ on the path)
from tests import ec_vectors as ev
from tests import ladder_vectors as lv
from tests import mac_decode_model as model

CASES = ("generic", "equal", "opposite", "a_inf", "b_inf", "both_inf", "b_top")
N_TOTAL = 1 << 16


@functools.lru_cache(maxsize=None)
def scalars(C):
    """[(label, k)]: eight scalars -- the wave-uniform shape below reads eight table entries"""
    q = lv.order(C)
    a = (1 << 100) + 0x1234567
    b = (1 << 99) + 0x7654321
    k_a, k_b = lv.from_halves(C, a, 0, 0, 0), lv.from_halves(C, 0, 0, b, 0)
    assert lv.halves_match(C, k_a, a, 0, 0, 0) and lv.halves_match(C, k_b, 0, 0, b, 0)
    out = [("one", 1), ("minus_one", q - 1), ("second_half_zero", k_a), ("first_half_zero", k_b)]
    for e in (N_TOTAL // 4, 3 * N_TOTAL // 8 + 32, 12345, N_TOTAL - 1):
        k = model.inverse_twiddle(e, N_TOTAL, C.name)
        assert k * (model.twiddle(e, N_TOTAL) % q) % q == 1
        out.append(("inverse_twiddle_%d" % e, k))
    return tuple(out)


def passes_through(C, k, uniform):
    """does the ladder hand a table entry through (possibly negated: the operand's bound, not an addition's)?  One non-zero digit in
    both halves together, at position 0"""
    if uniform:
        return lv.by_value_key(C, k) == "operand"
    digits = [d for m, _ in lv.split(C, k) for d in lv.signed_digits(m)]
    return sum(1 for d in digits if d) == 1 and (digits[0] != 0 or digits[33] != 0)


class Pair:
    """one inverse butterfly: A (rows[k]), B (rows[k + m2]), scalar k -> sum = A + B, prod = k (A - B)"""
    def __init__(self, C, label, k, case, idx, uniform, stage1=False):
        G = ev.multiples(C)
        rng = random.Random(0x1d3c + 16 * idx + CASES.index(case))
        self.k, self.label, self.case = k, label, case
        a, b = G[5 + idx % 9], G[17 + (3 * idx) % 11]
        self.A, self.B = {"generic": (a, b), "equal": (b, b), "opposite": (ev.ec_neg(C, b), b), "a_inf": (None, b), "b_inf": (a, None),
                          "both_inf": (None, None), "b_top": (a, b)}[case]
        kinds = lv.KINDS
        a_kind = kinds[idx % 4]
        b_kind = ("xmax", "top", "zmax")[idx % 3] if case == "b_top" else kinds[(idx // 4 + 1) % 4]
        # B is negated (4p - Y) on the way into the difference, and A is the difference itself when B is infinity -- the ladder's
        # operand, which negates it: both within the bound of a Y that is negated (what every stored sum and product keeps)
        self.a_words = np.array(lv.point_words(lv.shaped_mem(C, self.A, a_kind, rng, C.in_y_neg)), dtype=np.uint32)
        self.b_words = np.array(lv.point_words(lv.shaped_mem(C, self.B, b_kind, rng, C.in_y_neg)), dtype=np.uint32)
        self.sum = ev.ec_add(C, self.A, self.B)
        dif = ev.ec_add(C, self.A, ev.ec_neg(C, self.B))
        self.prod = None if dif is None else ev.ec_mul(C, k, dif)
        self.sum_key = "add" if self.A is not None and self.B is not None else "operand"
        if stage1:
            self.prod_key = self.sum_key                                  # A - B itself: no ladder
        else:
            self.prod_key = "operand" if passes_through(C, k, uniform) else "add"
        self.where = "%s %s (A %s, B %s)" % (label, case, a_kind, b_kind)


def launch(C, shape, tables, pairs, total=None, table=None):
    """one launch file: `tables` tables of shape.n rows end to end, butterfly t < total on the rows shape.bf[t % per_table] of table
    t // per_table; pairs: {t: Pair}; table: {entry: k} (the scalar table, in place of the inverse twiddles).  Rows no live butterfly
    owns and entries none reads hold the sentinel."""
    per_table = shape.n // 2
    total = tables * per_table if total is None else total
    rows = np.full((tables * shape.n, 32), lv.SENTINEL, dtype=np.uint32)
    tws = np.full((shape.n, 8), lv.SENTINEL, dtype=np.uint32)
    for t in range(total):
        k, m2, e = rows_of(shape, t)
        p = pairs[t]
        assert table is None or table[e] == p.k
        rows[k], rows[k + m2] = p.a_words, p.b_words
    for e, k in (table or {}).items():
        tws[e] = ev.words(k)
    h = np.zeros(lv.HDR, dtype=np.uint32)
    h[[lv.H_MAGIC, lv.H_N, lv.H_S, lv.H_TOTAL, lv.H_ROWS, lv.H_ENTRIES]] = [lv.MAGIC, shape.n, shape.s, total, tables * shape.n, shape.n]
    return np.concatenate([h, rows.reshape(-1), tws.reshape(-1)]), rows


def rows_of(shape, t):
    """butterfly t of a work array of several tables: mac_stage_index on t finds the pair in table t // (n / 2) because n is a multiple
    of every stage's block (checked against lv.stage_index on the whole work array)"""
    per_table = shape.n // 2
    k, m2, e = shape.bf[t % per_table]
    k += (t // per_table) * shape.n
    assert (k, m2, e) == lv.stage_index(t, shape.n, shape.s, shape.share)
    return k, m2, e


def check(C, work, rows_in, shape, total, pairs):
    """every live butterfly's two outputs as group elements with form and value bounds; every other row bit-identical"""
    owned = set()
    for t in range(total):
        k, m2, _ = rows_of(shape, t)
        p = pairs[t]
        owned |= {k, k + m2}
        ev.check_point_mem(C, work[k], p.sum, p.sum_key, "%s: sum" % p.where)
        ev.check_point_mem(C, work[k + m2], p.prod, p.prod_key, "%s: product" % p.where)
    for r in range(len(rows_in)):
        if r not in owned:
            assert (work[r] == rows_in[r]).all(), "row %d belongs to no live butterfly and changed" % r
    return total


def noncanonical_bytes(C):
    """(64 bytes, the point): a point of the curve whose byte string holds x + p and, where it fits 256 bits, y + p -- what SetBytes
    reduces.  BN254: the generator (1, 2); secp256k1: p is 2^32 + 977 below 2^256, so x must be that small -- the first such x on
    the curve, y left canonical"""
    if C is ev.BN254:
        pt = C.g
        return (pt[0] + C.p).to_bytes(32, "big") + (pt[1] + C.p).to_bytes(32, "big"), pt
    for x in range(1, 1000):
        y = ev.sqrt_mod(C, (x ** 3 + C.b) % C.p)
        if y and ev.on_curve(C, (x, y)):
            return (x + C.p).to_bytes(32, "big") + y.to_bytes(32, "big"), (x, y)
    raise AssertionError("no small x on the curve")
