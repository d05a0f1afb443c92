"""A catalogue of mutations of an audit reply, for the two batched verifiers (porla_ipa_verify_batch_device,
porla_kzg_verify_batch_device): every field of a record, and of the client's side of the request, changed in every way that a
verifier could overlook.  Pure Python on integers: no device, no library, nothing imported from the package or the oracles.

Every entry carries the LITERAL status an otherwise honest reply must get once the mutation is applied, written out here from the
equations the verifier checks and not computed from any oracle.  A test asserts a status against the oracle AND against this
literal (the rule of tests/test_ipa_verify_batch_gpu.py), so that a catalogue entry whose construction is wrong fails instead of
agreeing with itself.  Where the literal is None only the oracle decides: these are the encodings of a scalar at or above the group
order, which the verifiers reduce, and whether the reduced value happens to be the honest one is not known here.

  ipa_mutations(rec)                (group, name, mutated 655-byte record, expected)      groups: cma, l, r, rounds, scalars
  ipa_request_mutations(a_value)    (name, {field of the verify tuple: value}, expected)
  kzg_mutations(rec, other)         (group, name, mutated 320-byte record, expected)      groups: points, scalars
  kzg_request_mutations()           (name, {"alpha": value}, expected)
  challenge_shapes(nblk, zero_at)   (name, idx, coef): challenges an honest reply to which must stay honest

An honest record here has all its points finite (a challenge of a few rows on real data gives that); the functions refuse any other,
because a parity flip or a negation of infinity is no mutation.

Why the IPA literals are what they are.  With the honest status FULL | PROOF | BVEC:
  C   stands in the MAC equation and in the proof's equation, and is not hashed           -> BVEC alone
  M, A stand in the MAC equation only                                                      -> PROOF | BVEC
  L_r stands in the proof's equation; its hash is finalised into a state that the transcript then zeroes, so no challenge moves
                                                                                           -> FULL | BVEC
  R_r, r < 5, also feeds x_(r+1), which moves x_values and so the two BVEC sums           -> FULL
  R_5 is hashed into a challenge nobody reads                                              -> FULL | BVEC
  c   stands in the proof's equation and feeds x_0, a factor of every x_values[j]           -> FULL
  a0, a1 stand in the proof's equation only                                                -> FULL | BVEC
  b0, b1 stand in the proof's equation (a0 b0 + a1 b1) and ARE the BVEC claim              -> FULL
A point replaced by a valid point, by its negative (the parity byte) or by infinity (33 zero bytes) is well-formed and clears the
bits above; a point that breaks secp256k1_eckey_pubkey_parse's rules gives MALFORMED alone, whatever else the record holds."""

SECP_P = 2 ** 256 - 2 ** 32 - 977
SECP_N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
SECP_G = (0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798,
          0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8)
BN_P = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47
BN_R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
BN_G = (1, 2)
TOP = 2 ** 256 - 1

IPA_FULL, IPA_PROOF, IPA_MALFORMED, IPA_BVEC = 1, 2, 4, 8
IPA_BOUND = IPA_FULL | IPA_PROOF | IPA_BVEC
KZG_FULL, KZG_PROOF, KZG_MALFORMED = 1, 2, 4
KZG_PASS = KZG_FULL | KZG_PROOF

IPA_REC, KZG_REC = 655, 320
IPA_ROUNDS = 6
IPA_C_AT = 99                                   # the proof's c; the rounds follow, then a0 b0 a1 b1
IPA_TAIL_AT = 99 + 32 + 66 * IPA_ROUNDS
IPA_SCALARS = (("c", IPA_C_AT), ("a0", IPA_TAIL_AT), ("b0", IPA_TAIL_AT + 32), ("a1", IPA_TAIL_AT + 64), ("b1", IPA_TAIL_AT + 96))
KZG_POINTS = (("C", 0), ("H", 64), ("M", 192), ("A", 256))
KZG_Z_AT, KZG_Y_AT = 128, 160


# ---- affine arithmetic on y^2 = x^3 + b over F_p, enough for small multiples of a generator
def _add(p, a, b):
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0]:
        if (a[1] + b[1]) % p == 0:
            return None
        lam = 3 * a[0] * a[0] * pow(2 * a[1], p - 2, p) % p
    else:
        lam = (b[1] - a[1]) * pow(b[0] - a[0], p - 2, p) % p
    x = (lam * lam - a[0] - b[0]) % p
    return x, (lam * (a[0] - x) - a[1]) % p


def small_multiple(p, g, m):
    """m g for a small m > 0, by repeated addition"""
    acc = None
    for _ in range(m):
        acc = _add(p, acc, g)
    return acc


def secp_compressed(pt):
    return bytes([2 | (pt[1] & 1)]) + pt[0].to_bytes(32, "big")


def bn_marshal(pt):
    return pt[0].to_bytes(32, "big") + pt[1].to_bytes(32, "big")


def _is_square(p, v):
    v %= p
    return v == 0 or pow(v, (p - 1) // 2, p) == 1


def _patched(rec, at, data):
    return rec[:at] + bytes(data) + rec[at + len(data):]


# ---------------------------------------------------------------- IPA
def ipa_point_offsets():
    """(name, offset) of the fifteen compressed points: C, M, A, L_0, R_0, ..., L_5, R_5"""
    out = [("C", 0), ("M", 33), ("A", 66)]
    for r in range(IPA_ROUNDS):
        out += [("L%d" % r, IPA_C_AT + 32 + 66 * r), ("R%d" % r, IPA_C_AT + 32 + 66 * r + 33)]
    return out


def ipa_point_expected(name):
    """the status after this point was replaced by another well-formed point (see the module's text)"""
    if name == "C":
        return IPA_BVEC
    if name in ("M", "A"):
        return IPA_PROOF | IPA_BVEC
    if name[0] == "L" or name == "R%d" % (IPA_ROUNDS - 1):
        return IPA_FULL | IPA_BVEC
    return IPA_FULL


def ipa_point_mutations(rec, name, at, salt):
    """the nine mutations of the compressed point at `at`: three well-formed, six malformed"""
    c = rec[at:at + 33]
    if c[0] not in (2, 3):
        raise ValueError("reply_mutations: point %s of the honest record is not a finite compressed point" % name)
    x = int.from_bytes(c[1:], "big")
    well = ipa_point_expected(name)
    other = secp_compressed(small_multiple(SECP_P, SECP_G, 2 + salt))
    nonres = x + 1
    while _is_square(SECP_P, nonres ** 3 + 7):
        nonres += 1
    if nonres >= SECP_P:
        raise ValueError("reply_mutations: no non-residue X above point %s" % name)
    return [
        ("parity", bytes([c[0] ^ 1]) + c[1:], well),
        ("other_point", other, well),
        ("infinity", bytes(33), well),
        ("prefix_0", b"\x00" + c[1:], IPA_MALFORMED),
        ("prefix_4", b"\x04" + c[1:], IPA_MALFORMED),
        ("prefix_ff", b"\xff" + c[1:], IPA_MALFORMED),
        ("x_is_p", c[:1] + SECP_P.to_bytes(32, "big"), IPA_MALFORMED),
        ("x_is_top", c[:1] + TOP.to_bytes(32, "big"), IPA_MALFORMED),
        ("x_nonresidue", c[:1] + nonres.to_bytes(32, "big"), IPA_MALFORMED),
    ]


def ipa_mutations(rec):
    """every record-side mutation of one honest 655-byte reply: a list of (group, name, mutated record, expected status or None)"""
    rec = bytes(rec)
    if len(rec) != IPA_REC:
        raise ValueError("reply_mutations: an IPA record is %d bytes" % IPA_REC)
    out = []
    for i, (name, at) in enumerate(ipa_point_offsets()):
        group = "cma" if i < 3 else name[0].lower()
        for kind, data, expected in ipa_point_mutations(rec, name, at, i):
            out.append((group, "%s:%s" % (name, kind), _patched(rec, at, data), expected))
    # ---- whole points moved about.  L_r <-> R_r puts another point into R_r's place: like a changed R_r
    rnd_at = lambda r: IPA_C_AT + 32 + 66 * r
    for r in range(IPA_ROUNDS):
        at = rnd_at(r)
        swapped = rec[at + 33:at + 66] + rec[at:at + 33]
        out.append(("rounds", "L%d<->R%d" % (r, r), _patched(rec, at, swapped), ipa_point_expected("R%d" % r)))
    first, last = rec[rnd_at(0):rnd_at(0) + 66], rec[rnd_at(5):rnd_at(5) + 66]
    out.append(("rounds", "round0<->round5", _patched(_patched(rec, rnd_at(0), last), rnd_at(5), first), IPA_FULL))      # R_0 moved
    t = IPA_TAIL_AT
    a0, b0, a1, b1 = (rec[t + 32 * i:t + 32 * i + 32] for i in range(4))
    out.append(("rounds", "a0<->a1", _patched(rec, t, a1 + b0 + a0 + b1), IPA_FULL | IPA_BVEC))     # s_j = a_(j & 1) x_values[j] moves
    out.append(("rounds", "b0<->b1", _patched(rec, t, a0 + b1 + a1 + b0), IPA_FULL))                # a0 b1 + a1 b0, and the claim
    # ---- the five scalars.  + 1 has a literal; 0, n, n + 1 and 2^256 - 1 are reduced mod n by the verifier, and ONLY THE ORACLE
    # DECIDES what they give (0 or 1 may coincide with the honest value).  None of them touches the MAC equation.
    plus = dict(c=IPA_FULL, a0=IPA_FULL | IPA_BVEC, a1=IPA_FULL | IPA_BVEC, b0=IPA_FULL, b1=IPA_FULL)
    for name, at in IPA_SCALARS:
        v = int.from_bytes(rec[at:at + 32], "little")
        out.append(("scalars", "%s:+1" % name, _patched(rec, at, ((v + 1) % SECP_N).to_bytes(32, "little")), plus[name]))
        for kind, value in (("0", 0), ("n", SECP_N), ("n+1", SECP_N + 1), ("top", TOP)):
            out.append(("scalars", "%s:%s" % (name, kind), _patched(rec, at, value.to_bytes(32, "little")), None))
    return out


def ipa_request_mutations(a_value):
    """the client's side: (name, fields of the verify tuple to override, expected).  alpha is taken mod n and multiplies C and A in
    the MAC equation alone; a_value is the BVEC claim's v alone.  `a_value`: the honest one, which 0 and n - 1 must differ from"""
    if a_value % SECP_N in (0, SECP_N - 1):
        raise ValueError("reply_mutations: the honest a_value is one of the mutations")
    out = [("alpha:%s" % k, dict(alpha=v), IPA_PROOF | IPA_BVEC) for k, v in (("0", 0), ("1", 1), ("n", SECP_N), ("top", TOP))]
    out += [("a_value:0", dict(a_value=0), IPA_FULL | IPA_PROOF), ("a_value:n-1", dict(a_value=SECP_N - 1), IPA_FULL | IPA_PROOF)]
    return out


# ---------------------------------------------------------------- KZG
def _bn_on_curve(x, y):
    return (y * y - x * x * x - 3) % BN_P == 0


def kzg_point_expected(name):
    """C stands in both checks, H in the opening, M and A in the MAC equation"""
    return {"C": 0, "H": KZG_FULL, "M": KZG_PROOF, "A": KZG_PROOF}[name]


def kzg_point_mutations(rec, other, name, at, salt):
    b = rec[at:at + 64]
    x, y = int.from_bytes(b[:32], "big"), int.from_bytes(b[32:], "big")
    if (x == 0 and y == 0) or x >= BN_P or y >= BN_P or not _bn_on_curve(x, y):
        raise ValueError("reply_mutations: point %s of the honest record is not a finite curve point" % name)
    if _bn_on_curve(0, y):
        raise ValueError("reply_mutations: (0, y) is on the curve for point %s" % name)
    well = kzg_point_expected(name)
    off = x + 1
    while _bn_on_curve(off, y):
        off += 1
    if off >= BN_P:
        raise ValueError("reply_mutations: no x off the curve above point %s" % name)
    out = [
        ("negated", b[:32] + (BN_P - y).to_bytes(32, "big"), well),               # y != 0: the group's order is odd
        ("other_record", other[at:at + 64], well),
        ("infinity", bytes(64), well),
        ("x_is_p", BN_P.to_bytes(32, "big") + b[32:], KZG_MALFORMED),
        ("y_is_p", b[:32] + BN_P.to_bytes(32, "big"), KZG_MALFORMED),
        ("x_off_curve", off.to_bytes(32, "big") + b[32:], KZG_MALFORMED),
        ("x_is_0", bytes(32) + b[32:], KZG_MALFORMED),                            # (0, y) is on the curve only for y^2 = 3
    ]
    if name in ("M", "A"):
        out.insert(2, ("multiple_of_g", bn_marshal(small_multiple(BN_P, BN_G, 2 + salt)), well))
    return out


def kzg_mutations(rec, other):
    """every record-side mutation of one honest 320-byte reply (C | H | z | y | M | A); `other`: another honest record, whose points
    replace this one's role by role.  A list of (group, name, mutated record, expected status or None)"""
    rec, other = bytes(rec), bytes(other)
    if len(rec) != KZG_REC or len(other) != KZG_REC:
        raise ValueError("reply_mutations: a KZG record is %d bytes" % KZG_REC)
    out = []
    for i, (name, at) in enumerate(KZG_POINTS):
        for kind, data, expected in kzg_point_mutations(rec, other, name, at, i):
            out.append(("points", "%s:%s" % (name, kind), _patched(rec, at, data), expected))
    # ---- z and y stand in the opening alone.  v + r and v + 2 r always fit (v < r < 2^254) and are the same residue, as
    # verify_proof's SetBytes reduces them; 2^256 - 1 is some other residue unless the oracle says otherwise.
    for name, at in (("z", KZG_Z_AT), ("y", KZG_Y_AT)):
        v = int.from_bytes(rec[at:at + 32], "big")
        if v >= BN_R:
            raise ValueError("reply_mutations: the honest %s is not reduced" % name)
        for kind, value, expected in (("+1", (v + 1) % BN_R, KZG_FULL), ("+r", v + BN_R, KZG_PASS), ("+2r", v + 2 * BN_R, KZG_PASS),
                                      ("0", 0, KZG_FULL), ("top", TOP, None)):
            out.append(("scalars", "%s:%s" % (name, kind), _patched(rec, at, value.to_bytes(32, "big")), expected))
    out.append(("scalars", "z<->y", _patched(rec, KZG_Z_AT, rec[KZG_Y_AT:KZG_Y_AT + 32] + rec[KZG_Z_AT:KZG_Z_AT + 32]), KZG_FULL))
    return out


def kzg_request_mutations():
    """alpha is taken mod r and stands in the MAC equation alone"""
    return [("alpha:%s" % k, dict(alpha=v), KZG_PROOF) for k, v in (("0", 0), ("1", 1), ("r", BN_R), ("top", TOP))]


# ---------------------------------------------------------------- challenges
def challenge_shapes(nblk, zero_at):
    """(name, idx, coef) of the challenges that an honest reply must survive unchanged (the server is given the same challenge):
    a zero coefficient, the largest coefficient, one index eight times, a row whose complement is infinity (the caller's store has 64
    zero bytes at `zero_at`), and the empty challenge"""
    spread = [(5 * j + 1) % nblk for j in range(8)]
    coefs = [(0x1234567 * (j + 1)) & 0x7fffffff for j in range(8)]
    return [
        ("n1_coef0", [3 % nblk], [0]),
        ("n1_coef_max", [3 % nblk], [2 ** 31 - 1]),
        ("all_idx_equal", [7 % nblk] * 8, coefs),
        ("zero_complement", [zero_at] + [i for i in spread if i != zero_at][:7], coefs),
        ("n0", [], []),
    ]


# entries per list and group: the CPU check and the device sweep both tally what they asserted against this
COUNTS = {"ipa:cma": 27, "ipa:l": 54, "ipa:r": 54, "ipa:rounds": 9, "ipa:scalars": 25, "ipa:request": 6,
          "kzg:points": 30, "kzg:scalars": 11, "kzg:request": 4, "shapes": 5}


def tally(prefix, entries):
    """{prefix:group: count} of a list whose entries begin with their group"""
    out = {}
    for e in entries:
        out[prefix + ":" + e[0]] = out.get(prefix + ":" + e[0], 0) + 1
    return out
