"""A Python restatement of Server::update's H path for ONE file (porla/Server/Server.hpp:401-476): HAdd (:1388-1477), HRebuildX /
HRebuildY (:1329-1386) and the complement adds (:449-469), built from oracle/icc_py.py (hadd, hrebuild, ec_add) and the oracle's
commitment (tests/common.py: oracle_commit_batch).  The six level families are kept as bytes in the layout the engine's level stores
have (porla_icc_hrebuild_host): family[i] = 2 * 2^i rows, resident half then incoming half; a data row = n_cols 64-byte little-endian
symbols, a point row = 64 bytes big-endian affine (zeros = infinity).  Only the rows the reference writes are written, so a buffer
pre-filled with a sentinel keeps it everywhere else.  A helper of tests/test_update_batch_*.py, not a test module."""
import icc_py

from tests import common

FAMILIES = ("data_x", "data_y", "mac_x", "mac_y", "align_x", "align_y")
CURVE_ID = {"bn254": 0, "secp256k1": 1}


def pt_bytes(p):
    return bytes(64) if p is None else p[0].to_bytes(32, "big") + p[1].to_bytes(32, "big")


def pt_tuple(b):
    b = bytes(b)
    return None if b == bytes(64) else (int.from_bytes(b[:32], "big"), int.from_bytes(b[32:], "big"))


def row_bytes(vals):
    return b"".join(v.to_bytes(64, "little") for v in vals)


def row_vals(b):
    return [int.from_bytes(b[i:i + 64], "little") for i in range(0, len(b), 64)]


class FileModel:
    def __init__(self, n_total, n_cols, curve, base, fill=0):
        """base: the n_cols commitment base points (the SRS for KZG, the generators for IPA), 64 bytes each; fill: the byte every
        level buffer starts with"""
        self.n_total, self.n_cols, self.curve, self.base = n_total, n_cols, curve, bytes(base)
        self.height = icc_py.height_of(n_total)
        self.write_step = 0
        self.empty = [True] * self.height
        self.fam = {}
        for f in FAMILIES:
            row = 64 * n_cols if f.startswith("data") else 64
            self.fam[f] = [bytearray([fill]) * ((2 << i) * row) for i in range(self.height)]

    def _row(self, f):
        return 64 * self.n_cols if f.startswith("data") else 64

    def next_level(self):
        """the level the NEXT write lands on (HAdd's bookkeeping), None when it is CRebuild's step"""
        if (self.write_step + 1) % self.n_total == 0:
            return None
        if self.empty[0]:
            return 0
        level = 1
        while not self.empty[level]:
            level += 1
        return level

    def commit(self, scalars):
        rows = b"".join(c.to_bytes(32, "big") for c in scalars)
        return pt_tuple(common.oracle_commit_batch(self.curve, rows, 1, self.n_cols, self.base))

    def update(self, chunks, mac, complements=None):
        """chunks: n_cols ints < 2^256; mac: affine tuple or None; complements: 2 * 2^level affine tuples / None (X part, then Y), or
        None for no complements.  Returns (write_step, level) of the write."""
        level = self.next_level()
        assert level is not None, "CRebuild's step"
        self.write_step += 1
        mods, cs, mac_b2, _ = icc_py.hadd(chunks, mac, self.n_total, self.write_step, self.curve)
        new = {"data_x": row_bytes(chunks), "data_y": row_bytes(mods), "mac_x": pt_bytes(mac), "mac_y": pt_bytes(mac_b2),
               "align_x": bytes(64), "align_y": pt_bytes(self.commit(cs))}
        slot = 0 if level == 0 else 1
        for f in FAMILIES:
            r = self._row(f)
            self.fam[f][0][slot * r:(slot + 1) * r] = new[f]
        if level > 0:
            for f in FAMILIES:
                self._hrebuild(f, level)
            for i in range(level):
                self.empty[i] = True
        self.empty[level] = False
        if complements is not None:
            top = 1 << level
            assert len(complements) == 2 * top
            for j in range(2 * top):
                buf = self.fam["mac_x" if j < top else "mac_y"][level]
                o = 64 * (j % top)
                buf[o:o + 64] = pt_bytes(icc_py.ec_add(self.curve, pt_tuple(buf[o:o + 64]), complements[j]))
        return self.write_step, level

    def _hrebuild(self, f, level):
        """icc_py.hrebuild on the rows it reads (the resident halves below `level`, level 0's incoming row), written back where it
        writes: the incoming halves of levels 1 .. level and the resident half of `level`"""
        r = self._row(f)
        point = not f.startswith("data")
        parse = (lambda b: pt_tuple(b)) if point else (lambda b: row_vals(b))
        pack = (lambda v: pt_bytes(v)) if point else (lambda v: row_bytes(v))
        levels = []
        for i in range(level + 1):
            buf = self.fam[f][i]
            rows = [None] * (2 << i)
            live = range(2) if i == 0 else (range(1 << i) if i < level else ())
            for j in live:
                rows[j] = parse(bytes(buf[j * r:(j + 1) * r]))
            levels.append(rows)
        if point:
            # (a None row is infinity to mac_mix: every row it reads was parsed above or is written by the step before)
            icc_py.hrebuild(levels, level, self.n_total, self.curve, mac=True)
        else:
            icc_py.hrebuild(levels, level, self.n_total, self.curve)
        for i in range(1, level + 1):
            buf = self.fam[f][i]
            lo = 0 if i == level else (1 << i)
            for j in range(lo, 2 << i):
                buf[j * r:(j + 1) * r] = pack(levels[i][j])

    def family_bytes(self):
        """{family: [bytes of level 0, level 1, ...]}"""
        return {f: [bytes(b) for b in self.fam[f]] for f in FAMILIES}
