"""CPU: what tests/test_icc30_gpu.py leans on.  The static bounds of the ICC stream (tools/check_fe30_bounds.py: the borrow-free
subtraction tables at the call sites' operand bounds and the symbol bound chain) hold and are the numbers the vectors feed; the
vectors' own expectations agree with oracle/icc_py.py (finish step and mix), so the GPU test's reference is itself pinned; the named
operand families are generated whatever the seed."""
import os
import random
import sys

import pytest

from tests import common
from tests import icc_vectors as iv

sys.path.insert(0, os.path.join(common.ROOT, "tools"))

import icc_py  # noqa: E402


def test_icc_bound_chain_and_subtraction_tables():
    import check_fe30_bounds as cb
    assert cb.check_sub_tables() and cb.check_icc_chain()
    assert all(cb.check("icc:" + n, p, 23, 17) for n, p in cb.ICC_MODULI.items())
    assert not cb.check_icc_chain(stages=200)                                # ... and the chain check can fail
    assert cb.ICC_MODULI == iv.MODULI and cb.ICC_STAGES == iv.STAGES
    assert (1 << cb.ICC_A_BITS) - 1 == iv.A_MAX and (1 << cb.ICC_W_BITS) - 1 == iv.W_MAX
    for name, p in iv.MODULI.items():
        assert cb.icc_product_top(p) - 1 == iv.product_top(p) == iv.product_bound(p, iv.A_MAX, iv.W_MAX) - 1
        assert cb.icc_load_top(p) - 1 == iv.load_top(p)
        for K, b_max in cb.icc_sub_operands(p).items():
            assert iv.sub_b_tops(p, K)[-1] == b_max and all(iv.borrow_free(p, K, b) for b in iv.sub_b_tops(p, K))
        assert not iv.borrow_free(p, 2, 2 * p) and not iv.borrow_free(p, 2, iv.CHUNK_MAX if name == "bn254_r" else 2 * p)
        assert iv.mu(p) < 1 << 32 and iv.A_MAX // p == iv.K_COUNT[name]


def test_the_comments_state_the_numbers_the_vectors_feed():
    csrc = os.path.join(common.ROOT, "porla_amd", "csrc")
    icc30 = open(os.path.join(csrc, "icc30.hip.h")).read()
    split = open(os.path.join(csrc, "icc30_split.hip.h")).read()
    fe30 = open(os.path.join(csrc, "fe30.hip.h")).read()
    assert "p + 2^250" in icc30 and "p + 2^250" in split and "p + 2^242" in icc30
    assert "p + 2^248" in split and "2^263" in icc30 and "2^263" in split
    assert "icc30_sub" in fe30


@pytest.mark.parametrize("name", ["bn254_r", "secp256k1_n"])
def test_finish_and_mix_expectations_agree_with_the_oracle(name):
    q, curve = iv.MODULI[name], iv.CURVE_OF[name]
    lcm = icc_py.LCM[curve]
    assert lcm == iv.P_ICC * q and q == icc_py.Q[curve]
    rng = random.Random(41)
    syms = [v % lcm for _, v in iv.symbol_families(q)] + [rng.randrange(lcm) for _ in range(300)]
    mods, cs = icc_py.align(syms, curve)
    for A, al, c in zip(syms, mods, cs):
        vp = A % iv.P_ICC + rng.randint(0, (iv.A_MAX - iv.P_ICC) // iv.P_ICC) * iv.P_ICC     # unreduced, as the stream holds them
        vq = A % q + rng.randint(0, (iv.A_MAX - q) // q) * q
        assert iv.finish(vp, vq, q) == (A, al, c, A % q)
        for mod in (iv.P_ICC, q):                                              # the symbol load keeps the residue, below 2^258
            assert iv.load_symbol(A, mod) % mod == A % mod and iv.load_symbol(A, mod) < 1 << 258
    # the mix: row i of a level of MIX_N rows takes the twiddle v^i = w^i (Server::mix with length = N)
    n = iv.MIX_N
    rows = sorted({e for _, e in iv.TWIDDLE_ROWS} | {rng.randrange(n) for _ in range(200)})
    a0 = [[rng.randrange(lcm)] for _ in range(n)]
    a1 = [[rng.randrange(lcm)] for _ in range(n)]
    for k, (_, v) in enumerate(iv.symbol_families(q)):
        a0[k][0], a1[(k * 3) % 7][0] = v % lcm, v % lcm
    want = icc_py.mix(a0, a1, n, curve)
    for e in rows:
        assert iv.mix(a0[e][0], a1[e][0], iv.twiddle_of_row(e), q) == (want[e][0], want[e + n][0])
        # the table entry the driver is handed is the twiddle in the 2^270 form: icc30_from_elem of the 2^256 form gives that residue
        vi = iv.twiddle_of_row(e)
        for mod, slot in zip((iv.P_ICC, q), iv.twiddle_slot(vi, q)):
            got = iv.mont((vi % mod) * (1 << 256) % mod, iv.c284(mod), mod)
            assert got % mod == slot and got <= iv.tw_top(mod)
    assert iv.twiddle_of_row(0) == 1 and iv.twiddle_slot(1, q) == (iv.unit(iv.P_ICC), iv.unit(q))


def test_product_expectation_is_the_montgomery_quotient():
    """mont() against the digit-by-digit reduction fe30.hip.h:f30_mul_portable runs, on the operand maxima and a sweep"""
    rng = random.Random(7)
    for name, p in iv.MODULI.items():
        inv = (-pow(p, -1, 1 << 30)) % (1 << 30)
        cases = [(iv.A_MAX, iv.W_MAX), (iv.W_MAX, iv.A_MAX), (0, 0), (p, p), (iv.A_MAX, iv.unit(p))]
        cases += [(iv.rand_value(rng, p, iv.A_MAX), iv.rand_twiddle(rng, p)) for _ in range(200)]
        for a, b in cases:
            t = a * b
            for _ in range(9):
                t = (t + ((t & iv.MASK30) * inv & iv.MASK30) * p) >> 30
            assert t == iv.mont(a, b, p) < iv.product_bound(p, iv.A_MAX, iv.W_MAX)


@pytest.mark.parametrize("name", list(iv.MODULI))
def test_named_families_are_generated_whatever_the_seed(name):
    for op in iv.ops_of(name):
        for seed in (1, 2):
            recs, metas = iv.gen(name, op, random.Random(seed), 8)
            iv.assert_families_present(name, op, metas)
            assert recs.shape == (len(metas), iv.REC)
