"""CPU: the launch decision of the single-launch MSM (porla_msm_small_shape: host execution of msm_small.hip.h's small_cfg, small_fits
and small_decide, the code the kernels and msm_pair_locked run) against a restatement of small_cfg in Python (tests/small_vectors.py:
restated_cfg, float32 step by step as the C++ evaluates it).  The grid: both curves, lone and pair, split on and off, every forced
width, the scalar lengths around every threshold of the shape function, and every n at which a block count, a slice count or a slice
size can change.

What must hold: a shape that is launched fits its blocks and its block's LDS; the pairs that do NOT fit -- two families on secp256k1,
which small_cfg's unchecked fallback would launch all the same -- are exactly the ones that are not launched (such a pair runs as two
lone single launches instead); nothing else is turned away.  No device is touched."""
import ctypes
import itertools

import numpy as np
import pytest

from tests.small_vectors import (ANY, HDR_BYTES, HINT, LONE, NO_SPLIT, PAIR, SMALL_DONE_SLOT, SMALL_MAX_C, SMALL_MAX_N, SMALL_MAX_S,
                                 SMALL_MAX_SUB, SMALL_PAIR_STRIDE, XYZZ_BYTES, blocks_of, restated_cfg)

ERR_ARG = -3
USED_BITS = [0, 1, 31, 32, 33, 64, 127, 128, 129, 200, 249, 250, 254, 256]
NS = sorted(set(list(range(1, 65)) +
                [m + d for m in range(256, 32769, 256) for d in (-1, 0, 1) if m + d <= SMALL_MAX_N] +
                [4096, 4097, 8192, 8193, 24576, 24577, 28672, 28673, 32768]))


def combos():
    return list(itertools.product((0, 1), (LONE, PAIR), (0, NO_SPLIT), range(0, SMALL_MAX_C + 1), USED_BITS))


def build_grid(recheck_fallback=True):
    """inputs (curve, n, used_bits, c_flags, form) and the restated answers (fits, blocks, glv, c, W, S), plus n_sub, one row per element"""
    ins, outs, subs = [], [], []
    n = np.array(NS, dtype=np.int64)
    for curve, form, split, c, bits in combos():
        blocks = blocks_of(form, n)
        glv, cc, W, S, n_sub, fits = restated_cfg(curve, n, bits, c | split, blocks, recheck_fallback)
        k = len(n)
        ins.append(np.stack([np.full(k, curve), n, np.full(k, bits), np.full(k, c | split), np.full(k, form)], axis=1))
        outs.append(np.stack([fits.astype(np.int64), blocks, glv, cc, W, S], axis=1))
        subs.append(n_sub)
    return np.concatenate(ins), np.concatenate(outs), np.concatenate(subs)


@pytest.fixture(scope="module")
def grid():
    return build_grid()


@pytest.fixture(scope="module")
def exported(grid):
    from porla_amd import multiexp as mx
    ins, _, _ = grid
    return mx.msm_small_shape(ins[:, 0], ins[:, 1], ins[:, 2], ins[:, 3], ins[:, 4]).astype(np.int64)


def in_the_two_families(ins):
    """secp256k1 pairs: the split on, scalars over 128 bits, more than 28 672 pairs; the split off, scalars of 250 bits and more, more
    than 24 576 pairs"""
    curve, n, bits, flags, form = ins.T
    split_off = (flags & NO_SPLIT) != 0
    return (curve == 1) & (form != LONE) & ((~split_off & (bits > 128) & (n >= 28673)) | (split_off & (bits >= 250) & (n >= 24577)))


def test_the_symbol_is_exported_and_mirrored():
    from porla_amd import lib, multiexp as mx
    assert hasattr(lib, "porla_msm_small_shape")
    assert mx.SMALL_FORMS == {"lone": LONE, "pair": PAIR, "hint": HINT, "any": ANY}
    assert mx.msm_small_shape([], [], [], [], []).shape == (0, 6)


def test_the_grid_is_the_stated_one():
    assert set(range(1, 65)) <= set(NS) and {4096, 4097, 8192, 8193, 24576, 24577, 28672, 28673, 32768} <= set(NS)
    assert all(m + d in NS for m in range(256, 32768, 256) for d in (-1, 0, 1)) and 32767 in NS and max(NS) == SMALL_MAX_N
    assert len(combos()) == 2 * 2 * 2 * 9 * len(USED_BITS) and len(USED_BITS) == 14


def test_the_export_equals_the_restatement(grid, exported):
    ins, want, _ = grid
    assert exported.shape == want.shape == (len(NS) * len(combos()), 6)
    bad = np.nonzero((exported != want).any(axis=1))[0]
    assert len(bad) == 0, "%d of %d elements differ, the first: in %s export %s restated %s" % (
        len(bad), len(want), ins[bad[0]], exported[bad[0]], want[bad[0]])


def check_launched_shapes(ins, out, n_sub):
    """the rows (by index) among those reported single-launch that break one of the bounds a launched shape must keep"""
    fits, blocks, glv, c, W, S = out.T
    slice_ = (n_sub + S - 1) // S
    good = (W >= 1) & (W <= blocks) & (W * S <= blocks) & (S >= 1) & (S <= SMALL_MAX_S) & (slice_ <= SMALL_MAX_SUB) & \
           (W * c * XYZZ_BYTES + HDR_BYTES <= SMALL_PAIR_STRIDE) & (c >= 1) & (c <= SMALL_MAX_C) & (W < SMALL_DONE_SLOT)
    return np.nonzero((fits == 1) & ~good)[0]


def test_every_launched_shape_fits_its_blocks_and_its_lds(grid, exported):
    ins, _, n_sub = grid
    bad = check_launched_shapes(ins, exported, n_sub)
    assert len(bad) == 0, "launched but unfit: in %s shape %s" % (ins[bad[0]], exported[bad[0]])
    assert (exported[:, 0] == 1).sum() > 0.9 * len(exported)


def test_exactly_the_two_families_are_not_launched(grid, exported):
    ins, _, _ = grid
    refused = exported[:, 0] == 0
    fam = in_the_two_families(ins)
    assert fam.sum() > 0 and (refused == fam).all(), "not launched but outside the families: %s; inside but launched: %s" % (
        ins[refused & ~fam][:4], ins[~refused & fam][:4])
    # both families are the fallback shapes the issue's table names
    on = fam & ((ins[:, 3] & NO_SPLIT) == 0)
    off = fam & ((ins[:, 3] & NO_SPLIT) != 0)
    assert (exported[on][:, 1:] == [128, 1, 8, 17, 7]).all() and (exported[off][:, 1:] == [128, 0, 8, 33, 3]).all()
    # the boundary elements stay: 28 672 pairs with the split on, 24 576 with it off (slices of exactly 8 192)
    curve, n, bits, flags, form = ins.T
    edge_on = (curve == 1) & (form == PAIR) & ((flags & NO_SPLIT) == 0) & (bits > 128) & (n == 28672)
    edge_off = (curve == 1) & (form == PAIR) & ((flags & NO_SPLIT) != 0) & (bits >= 250) & (n == 24576)
    assert edge_on.sum() == 9 * 6 and edge_off.sum() == 9 * 3      # forced widths x lengths over 128 bits | of 250 bits and more
    assert (exported[edge_on][:, 0] == 1).all() and (exported[edge_off][:, 0] == 1).all()


def test_every_bn254_and_every_lone_element_stays_single_launch(grid, exported):
    ins, _, n_sub = grid
    stays = (ins[:, 0] == 0) | (ins[:, 4] == LONE)
    assert stays.sum() == 3 * len(exported) // 4 and (exported[stays][:, 0] == 1).all()
    full = (ins[:, 0] == 0) & (ins[:, 4] == PAIR) & (ins[:, 1] == 32768) & (ins[:, 2] == 256) & (ins[:, 3] == 0)
    assert full.sum() == 1 and n_sub[full][0] // exported[full][0, 5] == SMALL_MAX_SUB      # BN254 pair at 32 768: a slice of exactly 8 192


def test_the_rule_before_the_check_launches_exactly_the_two_families_unfit():
    """small_cfg as it stood -- the fallback taken on trust, every shape admitted -- restated: the bounds break at the two families and
    nowhere else"""
    ins, out, n_sub = build_grid(recheck_fallback=False)
    assert (out[:, 0] == 1).all()
    bad = np.zeros(len(ins), dtype=bool)
    bad[check_launched_shapes(ins, out, n_sub)] = True
    assert (bad == in_the_two_families(ins)).all()
    S = out[:, 5]
    slices = (n_sub + S - 1) // S
    on = bad & ((ins[:, 3] & NO_SPLIT) == 0)
    off = bad & ((ins[:, 3] & NO_SPLIT) != 0)
    assert slices[on].min() == 8193 and slices[on].max() == 9363 and slices[off].min() == 8193 and slices[off].max() == 10923


def test_a_hint_decides_as_the_scan_would_and_no_hint_needs_every_length(grid, exported):
    from porla_amd import multiexp as mx
    ins, _, _ = grid
    pair = (ins[:, 4] == PAIR) & (ins[:, 2] >= 1)
    sub = ins[pair]
    hint = mx.msm_small_shape(sub[:, 0], sub[:, 1], sub[:, 2], sub[:, 3], np.full(len(sub), HINT))
    assert (hint == exported[pair]).all()
    # the host's decision without a bound = the AND over every bit length 0 .. 256 of what the kernel would derive
    # (small_decide asks the longest length of each split class only: it must agree with all 257)
    ns = np.array([1, 2, 7, 8, 9, 63, 64, 255, 256, 257, 1000, 4095, 4096, 4097, 8191, 8192, 8193, 12288, 12289, 16384, 16385, 20000, 24575,
                   24576, 24577, 26000, 28671, 28672, 28673, 30000, 32767, 32768])
    for curve, flags in itertools.product((0, 1), [c | s for c in range(9) for s in (0, NO_SPLIT)]):
        k = len(ns)
        any_ = mx.msm_small_shape(np.full(k, curve), ns, np.zeros(k), np.full(k, flags), np.full(k, ANY))
        every = np.ones(k, dtype=bool)
        for bits in range(257):
            every &= restated_cfg(curve, ns, bits, flags, blocks_of(PAIR, ns))[5]
        assert (any_[:, 0] == every).all(), (curve, flags)
        limit = SMALL_MAX_N if curve == 0 else (24576 if flags & NO_SPLIT else 28672)
        assert (every == (ns <= limit)).all(), (curve, flags)


@pytest.mark.parametrize("bad", [
    dict(curve=2), dict(curve=-1), dict(n=0), dict(n=SMALL_MAX_N + 1), dict(used_bits=-1), dict(used_bits=257),
    dict(c_flags=9), dict(c_flags=0x200), dict(form=-1), dict(form=4), dict(form=HINT, used_bits=0),
])
def test_an_element_out_of_range_is_refused_and_nothing_is_written(bad):
    from porla_amd import lib
    el = dict(curve=1, n=100, used_bits=256, c_flags=0, form=PAIR)
    rows = [dict(el), dict(el, **bad)]
    arr = lambda key, t: (t * 2)(*[r[key] for r in rows])
    out = (ctypes.c_int32 * 12)(*([-7] * 12))
    rc = lib.porla_msm_small_shape(2, arr("curve", ctypes.c_int32), arr("n", ctypes.c_uint32), arr("used_bits", ctypes.c_int32),
                                   arr("c_flags", ctypes.c_int32), arr("form", ctypes.c_int32), out)
    assert rc == ERR_ARG and list(out) == [-7] * 12
    assert "element 1" in lib.porla_gpu_last_error().decode()
    assert lib.porla_msm_small_shape(1, None, None, None, None, None, out) == ERR_ARG
