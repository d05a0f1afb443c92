"""CPU: the vectors of tests/inv_vectors.py hold what tests/test_inv_gpu.py relies on.  The table of moduli against the other places
the same numbers live; for every generated record the limb model (32- and 64-bit ranges asserted inside it) at the round count of
the record's wave AND at every count from the input's own exit up to 25: normal limbs, a value in (0, 4 p), the inverse modulo p
against pow(V, -1, p) -- the idle-round claim of inv30.hip.h on all four moduli; the families hold what their names say; and a mixed
wave really gives a lane other limbs than its uniform wave does, or the GPU test could not see a wrong vote."""
import os
import re

import pytest

from oracle import bn254_py
from tests import common
from tests import ec_vectors as ev
from tests import inv_vectors as iv
import icc_py


def header_modulus(header, struct):
    """the integer of `struct`'s P[8] in a header of porla_amd/csrc"""
    text = open(os.path.join(common.ROOT, "porla_amd", "csrc", header)).read()
    m = re.search(r"struct %s \{.*?P\[8\]\s*=\s*\{([^}]*)\}" % struct, text, re.S)
    assert m, (header, struct)
    ws = [int(w.strip().rstrip("u"), 16 if "x" in w else 10) for w in m.group(1).split(",")]
    assert len(ws) == 8
    return iv.words_value(ws)


def test_moduli_table():
    assert iv.NAMES == ["bn254_fp", "secp256k1_fp", "icc_bn254_fr", "icc_secp256k1_fn"] and iv.FE_NAMES == iv.NAMES[:2]
    assert iv.MODULI["bn254_fp"].p == bn254_py.P == ev.BN254.p == icc_py.CURVE_P["bn254"]
    assert iv.MODULI["secp256k1_fp"].p == ev.SECP.p == icc_py.CURVE_P["secp256k1"]
    assert iv.MODULI["icc_bn254_fr"].p == icc_py.Q_BN254 == bn254_py.R
    assert iv.MODULI["icc_secp256k1_fn"].p == icc_py.Q_SECP256K1 == common.SECP_N
    for name, (value, header, struct) in iv.SOURCES.items():
        p = iv.MODULI[name].p
        assert p == value == header_modulus(header, struct), name
        # fe30.hip.h:P30<M>::limb(i) is bits [30 i, 30 i + 30) of P; the model's limbs are the same split, and P30::INV = -p^-1 mod 2^30
        assert iv.val(iv.limbs_signed(p)) == p and all(0 <= l <= iv.M30 for l in iv.limbs_signed(p)[:8]) and p >> 240 < 1 << 16
        assert (iv.run_of(1, p).INV * p + 1) % (1 << 30) == 0
    # the Fe form of the two base fields: fe.hip.h R1 = radix mod p
    assert ev.BN254.r32 == iv.MODULI["bn254_fp"].fe_radix % ev.BN254.p and ev.SECP.r32 == iv.MODULI["secp256k1_fp"].fe_radix == 1


def check_limbs(limbs, V, p, where):
    assert len(limbs) == 9 and all(0 <= l < 1 << 30 for l in limbs[:8]) and limbs[8] >= 0, where
    x = iv.val(limbs)
    assert 0 < x < 4 * p, where
    assert x % p == pow(V, -1, p), where


@pytest.mark.parametrize("name", iv.NAMES)
def test_every_record_at_every_round_count(name):
    p = iv.MODULI[name].p
    generated = checked = 0
    seen = {}                                                   # V -> rounds already modelled from its exit to 25
    moved = 0
    for job in iv.jobs(name):
        assert job.block in (64, 256) and job.policy in ("leave", "stay") and (len(job.waves) * iv.WAVE) % job.block == 0
        if job.op == "fe":
            assert name in iv.FE_NAMES
        for w, lane, V, active, rounds in iv.expected_records(name, job):
            generated += 1
            assert 0 < V < 1 << 256 and V % p != 0
            own = iv.rounds_needed(V, p)
            assert 9 <= own <= iv.MAX_ROUNDS and 9 <= rounds <= iv.MAX_ROUNDS
            if active:
                assert own <= rounds, (job.name, w.label, lane)
                check_limbs(iv.raw_limbs(V, p, rounds), V, p, (job.name, w.label, lane))
            if V not in seen:
                run = iv.run_of(V, p)
                at_exit = iv.raw_limbs(V, p, own)               # (the limb model reaches g = 0 in the round the integers say)
                assert min(run.out) == own, (hex(V), own)
                for r in range(own, iv.MAX_ROUNDS + 1):
                    check_limbs(iv.raw_limbs(V, p, r), V, p, (hex(V), r))
                seen[V] = True
                moved += iv.raw_limbs(V, p, iv.MAX_ROUNDS) != at_exit
            checked += 1
    print("%s: %d records, %d distinct values, %d of them return another integer after 25 rounds than at their own exit"
          % (name, checked, len(seen), moved))
    assert checked == generated > 6000
    assert moved * 2 > len(seen)                                # the raw result does depend on the rounds: for most inputs
    assert iv.rounds_needed(iv.DUMMY, p) == 18                  # what a lane without work costs its wave under `stay`


@pytest.mark.parametrize("name", iv.NAMES)
def test_families(name):
    p = iv.MODULI[name].p
    edge = iv.edge_values(p)
    assert len(edge) == (19 if p < 1 << 255 else 15)            # 2 p -+ 1 and the top multiple -+ 1 exist below 2^256 only for p < 2^255
    assert {1, 2, 3, p - 1, p + 1, (1 << 256) - 1} <= set(edge) and ((2 * p + 1 in edge) == (p < 1 << 255))
    assert sum(v < p for v in edge) >= 9 and sum(v > p for v in edge) >= (6 if p < 1 << 255 else 2)
    assert all(iv.rounds_needed(v, p) in (17, 18, 19) for v in edge)
    fast, slow, drawn = iv.speed_families(name)
    assert len(fast) == len(slow) == iv.PER_SPEED and drawn <= iv.DRAW_CAP, drawn
    assert all(iv.rounds_needed(v, p) == 17 for v in fast) and all(iv.rounds_needed(v, p) == 19 for v in slow)
    assert len(set(fast + slow)) == 16
    # the pinned 20-round inputs: their step counts recomputed
    assert set(iv.SLOWEST) == set(iv.NAMES) and len(iv.SLOWEST["icc_bn254_fr"]) == 1
    for v in iv.SLOWEST[name]:
        assert 0 < v < 1 << 256 and v % p and iv.divsteps_needed(v, p) >= 571 and iv.rounds_needed(v, p) == iv.SLOWEST_ROUNDS
    rnd = iv.random_values(name)
    assert len(rnd) == len(set(rnd)) == 2048 and all(0 < v < 1 << 256 and v % p for v in rnd)
    assert sum(v < p for v in rnd) >= 256 and sum(v >= p for v in rnd) >= 256
    shares = {r: sum(iv.rounds_needed(v, p) == r for v in rnd) for r in range(9, 26)}
    print("%s: %d candidates for the speed families; rounds of the random values %s" % (name, drawn, {r: n for r, n in shares.items() if n}))
    assert shares[18] > 1024 and shares[19] > 0 and sum(shares.values()) == 2048


@pytest.mark.parametrize("name", iv.NAMES)
def test_layouts(name):
    p = iv.MODULI[name].p
    fast, slow, _ = iv.speed_families(name)
    js = {j.name: j for j in iv.jobs(name)}
    n_waves = sum(len(j.waves) for j in js.values())
    assert 95 <= n_waves <= 190, n_waves                        # (about 100 for an ICC modulus, 165 with the fe jobs of a base field)
    uni = {w.values[0]: w for w in js["raw uniform"].waves}
    assert all(len(set(w.values)) == 1 and all(w.active) for w in uni.values()) and len(uni) == len(iv.edge_values(p)) + 16 + len(iv.SLOWEST[name])
    # mixed waves: the slow lane where the name says, and a wave round count of 19 that the fast lanes alone would not have
    mixed = js["raw mixed"].waves
    for w, lane in zip(mixed[:4], iv.SLOW_LANES):
        assert [i for i, v in enumerate(w.values) if v in slow] == [lane] and w.rounds(p, "leave") == 19
    assert [i for i, v in enumerate(mixed[4].values) if v in fast] == [iv.FAST_LANE] and mixed[4].rounds(p, "leave") == 19
    assert all((v in fast) == (i % 2 == 0) for i, v in enumerate(mixed[5].values))
    assert len(mixed) == 6 + len(iv.SLOWEST[name])
    for w, v in zip(mixed[6:], iv.SLOWEST[name]):
        assert w.values[iv.SLOWEST_LANE] == v and w.values.count(v) == 1 and w.rounds(p, "leave") == iv.SLOWEST_ROUNDS
    # at least one mixed wave holds a lane whose expected limbs differ from those of its uniform wave: a wrong vote is visible
    differ = 0
    for w in mixed:
        r = w.rounds(p, "leave")
        for v in w.values:
            differ += iv.raw_limbs(v, p, r) != iv.raw_limbs(v, p, uni[v].rounds(p, "leave"))
    assert differ > 0
    # masks: the rounds under `leave` are those of the active lanes alone, under `stay` the dummy's 18 joins in
    masked = js["raw masks leave"].waves
    assert [w.label for w in masked] == [w.label for w in js["raw masks stay"].waves] and len(masked) == 2 * len(iv.MASKS) + 1
    counts = sorted(sum(w.active) for w in masked)
    assert counts == sorted([1, 1, 1, 1, 1, 63, 63, 32, 32, 32, 32])
    seen_by_policy = 0
    for w in masked:
        lr, sr = w.rounds(p, "leave"), w.rounds(p, "stay")
        act = [v for v, a in zip(w.values, w.active) if a]
        if "fast active" in w.label:
            assert all(v in fast for v in act) and (lr, sr) == (17, 18), w.label
            assert all(v in slow for v, a in zip(w.values, w.active) if not a)
        else:
            assert all(v in slow for v in act) and (lr, sr) == (19, 19), w.label
            assert all(v in fast for v, a in zip(w.values, w.active) if not a)
        seen_by_policy += sum(iv.raw_limbs(v, p, lr) != iv.raw_limbs(v, p, sr) for v in act)
    assert seen_by_policy > 0                                   # the two policies give some active lane different limbs
    # the block of 256: four waves with three different round counts side by side
    b = js["raw block256 leave"].waves
    assert len(b) == 4 and [w.rounds(p, "leave") for w in b] == [17, 19, 19, 17] and [w.rounds(p, "stay") for w in b] == [17, 19, 19, 18]
    if name in iv.FE_NAMES:
        below = sum(v < p for j in js.values() if j.op == "fe" for w in j.waves for v in w.values)
        above = sum(v >= p for j in js.values() if j.op == "fe" for w in j.waves for v in w.values)
        assert below > 500 and above >= 256
        m = iv.MODULI[name]
        for v in (1, 2, p - 1, p + 1, (1 << 256) - 1):          # A 2^r -> A^-1 2^r: a out = R1 under the field's product a b / R
            out = iv.fe_inverse(v, m)
            assert out < p and v * out * pow(m.fe_radix, -1, p) % p == m.fe_radix % p
    else:
        assert not any(j.op == "fe" for j in js.values())
    # the records of a job: V, the active bit, the sentinel
    recs = iv.records(js["raw masks stay"])
    assert recs.shape == (len(masked) * 64, iv.REC) and (recs[:, iv.O0:] == iv.SENTINEL).all()
    assert iv.words_value(recs[0, :8]) == masked[0].values[0] and int(recs[1, iv.FLAGS]) == 0 and int(recs[0, iv.FLAGS]) == 1
