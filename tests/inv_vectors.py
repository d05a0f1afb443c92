"""Vectors and expected values for the check of the division-step inversion (porla_amd/csrc/inv30.hip.h) through tools/inv_check.hip.

The inversion is the one hot-path primitive with a data-dependent trip count: its loop of 30-step rounds ends when a wave-wide vote
finds g = 0 in every lane that runs the call.  A round after a lane's own g = 0 leaves d alone modulo p but maps a negative d to
d + p, so the INTEGER f30_inv_safegcd_raw returns depends on how many rounds the lane's wave ran.  Everything here is built on that:

  rounds_needed(V, p)      division steps on Python integers until g = 0, in rounds of 30
  raw_limbs(V, p, rounds)  the limb-level model of tools/safegcd_model.py (32- and 64-bit ranges asserted) run for `rounds` rounds:
                           the nine limbs the device returns
  Wave / expected_rounds   a wave of 64 (V, active) lanes; the rounds it runs are the maximum of rounds_needed over the lanes that
                           EXECUTE the call -- the active lanes under `leave`, every lane under `stay`, an inactive one as the value 1

Families per modulus: edge values (below, at and above p, never 0 mod p), `fast` (17 rounds) and `slow` (19 rounds) values drawn with
a fixed seed, `slowest` (20 rounds: pinned constants, where a search found one), 2048 random 256-bit values.  Layouts: see jobs()."""
import collections
import functools
import os
import random
import subprocess
import tempfile

import numpy as np

from tests import common
from tests import ec_vectors as ev
import icc_py

EXE = os.path.join(common.ROOT, "porla_amd", "inv_check")

# records of tools/inv_check.hip
REC, V0, FLAGS, O0, F_ACTIVE = 24, 0, 8, 12, 1
SENTINEL = 0xA5A5A5A5
M30 = (1 << 30) - 1
WAVE = 64
MAX_ROUNDS = 25                # inv30.hip.h: the loop's bound
DUMMY = 1                      # what a lane without work inverts under `stay`

Modulus = collections.namedtuple("Modulus", "name p fe_radix")
# fe_radix: the integer an Fe holds is (residue * fe_radix) mod p; None where fe_inv_safegcd does not exist (no INV_OUT_30)
MODULI = {m.name: m for m in (
    Modulus("bn254_fp", 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47, 1 << 256),
    Modulus("secp256k1_fp", 2**256 - 2**32 - 977, 1),
    Modulus("icc_bn254_fr", 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001, None),
    Modulus("icc_secp256k1_fn", 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141, None),
)}
NAMES = list(MODULI)
FE_NAMES = [n for n in NAMES if MODULI[n].fe_radix is not None]
# where the same numbers live elsewhere: (python value, header, struct) -- cross-checked by tests/test_inv_vectors_cpu.py
SOURCES = {
    "bn254_fp": (ev.BN254.p, "fe.hip.h", "Bn254Fp"),
    "secp256k1_fp": (ev.SECP.p, "fe.hip.h", "Secp256k1Fp"),
    "icc_bn254_fr": (icc_py.Q_BN254, "icc.hip.h", "IccBn254Fr"),
    "icc_secp256k1_fn": (icc_py.Q_SECP256K1, "icc.hip.h", "IccSecp256k1Fn"),
}


# ---------------------------------------------------------------- division steps on Python integers
def divsteps_needed(V, p):
    """steps of (delta, f, g) <- divstep(delta, f, g) from (1, p, V) until g = 0"""
    delta, f, g, n = 1, p, V, 0
    while g:
        if g & 1:
            if delta > 0:
                delta, f, g = 1 - delta, g, (g - f) >> 1
            else:
                delta, g = 1 + delta, (g + f) >> 1
        else:
            delta, g = 1 + delta, g >> 1
        n += 1
    assert f in (1, -1), (V, p)
    return n


@functools.lru_cache(maxsize=None)
def rounds_needed(V, p):
    return -(-divsteps_needed(V, p) // 30)


# ---------------------------------------------------------------- the limb-level model (tools/safegcd_model.py, made importable)
B31, B63 = 1 << 31, 1 << 63


def limbs_signed(x):
    """nine limbs, 0..7 in [0, 2^30), limb 8 signed"""
    return [(x >> (30 * i)) & M30 for i in range(8)] + [x >> 240]


def val(l):
    return sum(v << (30 * i) for i, v in enumerate(l))


def i32(x):
    assert -B31 <= x < B31, x
    return x


def i64(x):
    assert -B63 <= x < B63, x
    return x


class Run:
    """f30_inv_safegcd_raw on (p, V), round by round: the state after `done` rounds, every value the device keeps in a 32- or 64-bit
    register asserted to fit"""

    def __init__(self, V, p):
        assert 0 < V < 1 << 256
        self.V, self.p = V, p
        self.INV = (-pow(p, -1, 1 << 30)) % (1 << 30)          # -p^-1 mod 2^30
        self.P = limbs_signed(p)
        self.f, self.g = limbs_signed(p), limbs_signed(V)
        self.d, self.e = [0] * 9, [1] + [0] * 8
        self.delta, self.done = 1, 0
        self.out = {}                                          # rounds -> limbs

    def g_is_zero(self):
        return not any(self.g)

    def round(self):
        f, g, d, e, P, INV, delta = self.f, self.g, self.d, self.e, self.P, self.INV, self.delta
        f0 = (f[0] | (f[1] << 30)) & 0xffffffff
        g0 = (g[0] | (g[1] << 30)) & 0xffffffff
        u, v, q, r = 1, 0, 0, 1
        for _ in range(30):
            godd = g0 & 1
            if godd and delta > 0:
                delta = -delta
                f0, g0, u, v, q, r = g0, (-f0) & 0xffffffff, q, r, -u, -v
            if godd:
                g0 = (g0 + f0) & 0xffffffff
                q += u
                r += v
            delta += 1
            g0 >>= 1
            u *= 2
            v *= 2
            assert -B31 <= u < B31 and -B31 <= v < B31 and -B31 <= q < B31 and -B31 <= r < B31, (u, v, q, r)
        i32(delta)
        # (f, g) <- [[u, v], [q, r]] (f, g) / 2^30
        cf = i64(u * f[0] + v * g[0])
        cg = i64(q * f[0] + r * g[0])
        assert cf & M30 == 0 and cg & M30 == 0
        cf >>= 30
        cg >>= 30
        nf, ng = [0] * 9, [0] * 9
        for i in range(1, 9):
            cf = i64(cf + u * f[i] + v * g[i])
            cg = i64(cg + q * f[i] + r * g[i])
            nf[i - 1] = cf & M30
            cf >>= 30
            ng[i - 1] = cg & M30
            cg >>= 30
        nf[8], ng[8] = i32(cf), i32(cg)
        # (d, e) <- the same matrix times (d, e), divided by 2^30 modulo p
        sd, se = d[8] < 0, e[8] < 0
        md = (u if sd else 0) + (v if se else 0)
        me = (q if sd else 0) + (r if se else 0)
        i32(md)
        i32(me)
        cd = i64(u * d[0] + v * e[0])
        ce = i64(q * d[0] + r * e[0])
        md -= (-(((cd + md * P[0]) & M30) * INV)) & M30
        me -= (-(((ce + me * P[0]) & M30) * INV)) & M30
        i32(md)
        i32(me)
        cd = i64(cd + md * P[0])
        ce = i64(ce + me * P[0])
        assert cd & M30 == 0 and ce & M30 == 0
        cd >>= 30
        ce >>= 30
        nd, ne = [0] * 9, [0] * 9
        for i in range(1, 9):
            cd = i64(cd + u * d[i] + v * e[i] + md * P[i])
            ce = i64(ce + q * d[i] + r * e[i] + me * P[i])
            nd[i - 1] = cd & M30
            cd >>= 30
            ne[i - 1] = ce & M30
            ce >>= 30
        nd[8], ne[8] = i32(cd), i32(ce)
        self.f, self.g, self.d, self.e, self.delta = nf, ng, nd, ne, delta
        self.done += 1
        assert -2 * self.p < val(nd) < self.p and -2 * self.p < val(ne) < self.p

    def result(self):
        """the function's closing step on the present state: +-d + 2 p, limb by limb as the device adds them"""
        assert self.g_is_zero() and val(self.f) in (1, -1), (hex(self.V), self.done)
        neg = self.f[8] < 0
        x, c = [0] * 9, 0
        for i in range(9):
            t = i64((-self.d[i] if neg else self.d[i]) + 2 * self.P[i] + c)
            if i < 8:
                x[i], c = t & M30, t >> 30
            else:
                assert 0 <= t < 1 << 32, t
                x[i] = t
        return tuple(x)

    def limbs(self, rounds):
        assert rounds_needed(self.V, self.p) <= rounds <= MAX_ROUNDS, (hex(self.V), rounds)
        while self.done < rounds:
            self.round()
            if self.g_is_zero():
                self.out[self.done] = self.result()
        return self.out[rounds]


@functools.lru_cache(maxsize=None)
def run_of(V, p):
    return Run(V, p)


def raw_limbs(V, p, rounds):
    """the nine limbs of f30_inv_safegcd_raw(V) in a wave that runs `rounds` rounds (at least the input's own, at most 25)"""
    return run_of(V, p).limbs(rounds)


def fe_inverse(V, m):
    """the eight words' value of fe_inv_safegcd(V): V holds A * radix, the result is A^-1 * radix (fe.hip.h: INV_OUT_30), canonical"""
    return pow(V, -1, m.p) * m.fe_radix * m.fe_radix % m.p


# ---------------------------------------------------------------- families
def edge_values(p):
    vs = [1, 2, 3, (1 << 30) - 1, 1 << 30, (1 << 30) + 1, 1 << 60, 1 << 240, 1 << 255, (1 << 256) - 1, p - 1, p - 2, (p - 1) // 2,
          (p + 1) // 2, p + 1]
    if p < 1 << 255:                                           # (above 2^255 neither 2 p -+ 1 nor a further multiple is a 256-bit value)
        top = ((1 << 256) - 1) // p * p                        # the largest multiple of p below 2^256
        vs += [2 * p - 1, 2 * p + 1, top - 1, top + 1]
    assert all(0 < v < 1 << 256 and v % p for v in vs) and len(set(vs)) == len(vs)
    return vs


DRAW_CAP = 20000               # candidates per modulus; the rarest case (17 rounds, 0.4 - 0.7 %) needs about 2 500 for 8 values
FAST_ROUNDS, SLOW_ROUNDS, PER_SPEED = 17, 19, 8


@functools.lru_cache(maxsize=None)
def speed_families(name):
    """(fast values, slow values, candidates drawn)"""
    p = MODULI[name].p
    rnd = random.Random("inv speed " + name)
    fast, slow, drawn = [], [], 0
    while (len(fast) < PER_SPEED or len(slow) < PER_SPEED) and drawn < DRAW_CAP:
        V = rnd.randrange(1, 1 << 256)
        drawn += 1
        if V % p == 0:
            continue
        r = rounds_needed(V, p)
        if r == FAST_ROUNDS and len(fast) < PER_SPEED:
            fast.append(V)
        elif r == SLOW_ROUNDS and len(slow) < PER_SPEED:
            slow.append(V)
    return tuple(fast), tuple(slow), drawn


# `slowest`: inputs that need 20 rounds (571 division steps or more), found by an offline search over uniform 256-bit draws: one for
# BN254's group order in 1.2 million draws, none for the other three moduli in 1.8 - 2.1 million draws each (their most: 569 steps)
SLOWEST_ROUNDS = 20
SLOWEST = {
    "bn254_fp": (),
    "secp256k1_fp": (),
    "icc_bn254_fr": (0xe8bf4871e4e5e705e4a1c256cce4e930341b34ae99ab057ef13535fe2bbbc13f,),
    "icc_secp256k1_fn": (),
}
SLOWEST_LANE = 7

N_RANDOM, N_ABOVE = 2048, 512


@functools.lru_cache(maxsize=None)
def random_values(name):
    """2048 values of [1, 2^256), not 0 mod p, drawn uniformly.  A modulus within 2^129 of 2^256 (the two of secp256k1) never sees a
    uniform draw at or above itself, so there the last 512 values come uniformly from (p, 2^256) instead: every modulus gets at
    least 256 inputs on either side of p."""
    p = MODULI[name].p
    rnd = random.Random("inv random " + name)
    out = []
    while len(out) < N_RANDOM:
        V = rnd.randrange(1, 1 << 256)
        if V % p:
            out.append(V)
    if sum(v >= p for v in out) < 256:
        above = set()
        while len(above) < N_ABOVE:
            above.add(rnd.randrange(p + 1, 1 << 256))
        out[N_RANDOM - N_ABOVE:] = sorted(above, key=lambda v: (v * 0x9e3779b97f4a7c15) & 0xffffffff)
    return tuple(out)


# ---------------------------------------------------------------- waves
class Wave:
    """64 lanes of (V, active) with a label; `uniform` marks a wave of one value in every lane"""

    def __init__(self, label, values, active=None):
        assert len(values) == WAVE
        self.label, self.values = label, list(values)
        self.active = [True] * WAVE if active is None else list(active)
        assert len(self.active) == WAVE and any(self.active)

    def executing(self, policy):
        """the values of the lanes that run the call"""
        if policy == "leave":
            return [v for v, a in zip(self.values, self.active) if a]
        assert policy == "stay"
        return [v if a else DUMMY for v, a in zip(self.values, self.active)]

    def rounds(self, p, policy):
        return max(rounds_needed(v, p) for v in self.executing(policy))


def cycle(vals, n=WAVE, start=0):
    return [vals[(start + i) % len(vals)] for i in range(n)]


def mask(name):
    return {"lane0": [i == 0 for i in range(WAVE)], "lane63": [i == 63 for i in range(WAVE)], "lane31": [i == 31 for i in range(WAVE)],
            "63lanes": [i != 5 for i in range(WAVE)], "lower32": [i < 32 for i in range(WAVE)], "odd": [i % 2 == 1 for i in range(WAVE)]}[name]


MASKS = ["lane0", "lane63", "63lanes", "lower32", "odd"]
SLOW_LANES = [0, 31, 32, 63]
FAST_LANE = 17


def uniform_waves(name):
    p = MODULI[name].p
    fast, slow, _ = speed_families(name)
    named = [("edge%d" % i, v) for i, v in enumerate(edge_values(p))] + [("fast%d" % i, v) for i, v in enumerate(fast)] \
        + [("slow%d" % i, v) for i, v in enumerate(slow)] + [("slowest%d" % i, v) for i, v in enumerate(SLOWEST[name])]
    return [Wave("uniform " + n, [v] * WAVE) for n, v in named]


def mixed_waves(name):
    fast, slow, _ = speed_families(name)
    ws = []
    for j, lane in enumerate(SLOW_LANES):
        vals = cycle(fast, start=j)
        vals[lane] = slow[j]
        ws.append(Wave("slow lane %d among fast" % lane, vals))
    vals = cycle(slow)
    vals[FAST_LANE] = fast[0]
    ws.append(Wave("fast lane %d among slow" % FAST_LANE, vals))
    ws.append(Wave("alternating", [fast[(i // 2) % len(fast)] if i % 2 == 0 else slow[(i // 2) % len(slow)] for i in range(WAVE)]))
    for j, v in enumerate(SLOWEST[name]):                      # (behind the six waves every modulus has)
        vals = cycle(fast + slow, start=j)
        vals[SLOWEST_LANE] = v
        ws.append(Wave("slowest lane %d among fast and slow" % SLOWEST_LANE, vals))
    return ws


def random_waves(name, ends=None):
    """the random values in waves as drawn; ends = k: only the first and the last k waves (the last hold the values above a modulus
    close to 2^256)"""
    vs = random_values(name)
    n = len(vs) // WAVE
    return [Wave("random %d" % w, vs[w * WAVE:(w + 1) * WAVE]) for w in range(n) if ends is None or w < ends or w >= n - ends]


def masked_waves(name):
    """per mask: the active lanes fast among inactive slow ones (a vote that counted the inactive lanes, or a dummy that is not 1, runs
    too long), and the active lanes slow among inactive fast ones; then the lone slow lane 31 among inactive fast lanes"""
    fast, slow, _ = speed_families(name)
    ws = []
    for m in MASKS:
        act = mask(m)
        ws.append(Wave("mask %s fast active" % m, [f if a else s for f, s, a in zip(cycle(fast), cycle(slow), act)], act))
        ws.append(Wave("mask %s slow active" % m, [s if a else f for f, s, a in zip(cycle(fast), cycle(slow), act)], act))
    act = mask("lane31")
    ws.append(Wave("only the slow lane active", [slow[3] if a else f for f, a in zip(cycle(fast, start=3), act)], act))
    return ws


def block256_waves(name):
    """one block of 256: all-fast, all-slow, mixed, half-masked (fast active below 32, slow inactive above)"""
    fast, slow, _ = speed_families(name)
    act = mask("lower32")
    return [Wave("block256 all fast", cycle(fast, start=1)), Wave("block256 all slow", cycle(slow, start=1)),
            Wave("block256 mixed", [slow[5] if i == 40 else fast[i % len(fast)] for i in range(WAVE)]),
            Wave("block256 half masked", [f if a else s for f, s, a in zip(cycle(fast, start=2), cycle(slow, start=2), act)], act)]


Job = collections.namedtuple("Job", "name op block policy waves")
FE_RANDOM_ENDS = 4


def jobs(name):
    """every job of one modulus: the driver's arguments and the waves, in launch order"""
    js = [Job("raw uniform", "raw", 64, "leave", uniform_waves(name)),
          Job("raw mixed", "raw", 64, "leave", mixed_waves(name)),
          Job("raw random", "raw", 64, "leave", random_waves(name)),
          Job("raw masks leave", "raw", 64, "leave", masked_waves(name)),
          Job("raw masks stay", "raw", 64, "stay", masked_waves(name)),
          Job("raw block256 leave", "raw", 256, "leave", block256_waves(name)),
          Job("raw block256 stay", "raw", 256, "stay", block256_waves(name))]
    if MODULI[name].fe_radix is not None:
        js += [Job("fe uniform", "fe", 64, "leave", uniform_waves(name)),
               Job("fe mixed", "fe", 64, "leave", mixed_waves(name)),
               Job("fe random", "fe", 64, "leave", random_waves(name, FE_RANDOM_ENDS)),
               Job("fe masks stay", "fe", 64, "stay", masked_waves(name)),
               Job("fe block256 leave", "fe", 256, "leave", block256_waves(name))]
    return js


def expected_records(name, job):
    """[(wave, lane, V, active, rounds of the wave)] in record order"""
    p = MODULI[name].p
    out = []
    for w in job.waves:
        r = w.rounds(p, job.policy)
        out += [(w, lane, v, a, r) for lane, (v, a) in enumerate(zip(w.values, w.active))]
    return out


def words(x, n=8):
    return [(x >> (32 * i)) & 0xffffffff for i in range(n)]


def words_value(ws):
    return sum(int(w) << (32 * i) for i, w in enumerate(ws))


def records(job):
    """the input file of a job; the result area holds the sentinel (the driver fills it again)"""
    n = len(job.waves) * WAVE
    assert n % job.block == 0
    recs = np.zeros((n, REC), dtype=np.uint32)
    recs[:, O0:] = SENTINEL
    i = 0
    for w in job.waves:
        for v, a in zip(w.values, w.active):
            recs[i, V0:V0 + 8] = words(v)
            recs[i, FLAGS] = F_ACTIVE if a else 0
            i += 1
    return recs


# ---------------------------------------------------------------- running the driver
RUN_TIMEOUT = 120              # seconds, per driver process


def run(name, js):
    """[Job] -> [output records], one process for all of them"""
    with tempfile.TemporaryDirectory() as d:
        cmd = [EXE, name]
        ins = []
        for i, j in enumerate(js):
            recs = records(j)
            recs.tofile(os.path.join(d, "in%d" % i))
            ins.append(recs)
            cmd += [j.op, str(j.block), j.policy, os.path.join(d, "in%d" % i), os.path.join(d, "out%d" % i)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=RUN_TIMEOUT)
        assert r.returncode == 0, "inv_check failed (%d): %s%s" % (r.returncode, r.stdout, r.stderr)
        return [(recs, np.fromfile(os.path.join(d, "out%d" % i), dtype=np.uint32).reshape(-1, REC)) for i, recs in enumerate(ins)]
