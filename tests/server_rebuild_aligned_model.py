"""A Python restatement of the write on which Server::update calls CRebuild in its CRebuild_No_Cached form (porla/Server/Server.hpp:413-469
with :1835-2255) for ONE file, built on tests/server_rebuild_model.py's RebuildFileModel.  What differs from the cached form:

  * the TOP level's data rows are kept in the 256-bit row format: 2 * n_total rows of n_cols 32-byte little-endian symbols below p_icc
    (the lower levels keep 64 bytes per symbol);
  * rebuild() ends each part's network in align_MAC (:531-541, :1977-1980, :2061-2064): icc_py.align on every row of icc_py.crebuild's
    X and Y gives the row mod p_icc and the scalars c = (A mod p_icc - A) mod q;
  * the alignment of a row is the commitment of its scalars (FileModel.commit: the oracle's commitment against the base points), the
    whole value because B starts at infinity (:1882-1890); a row of zero scalars gives infinity.

The stores, the MAC network, the complement adds and the bookkeeping are RebuildFileModel's.  A helper of
tests/test_server_rebuild_aligned_batch_*.py, not a test module."""
import icc_py

from tests.server_rebuild_model import RebuildFileModel
from tests.update_model import pt_bytes


def row32_bytes(vals):
    return b"".join(v.to_bytes(32, "little") for v in vals)


def row32_vals(b):
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


class AlignedRebuildFileModel(RebuildFileModel):
    def __init__(self, n_total, n_cols, curve, base, fill=0):
        super().__init__(n_total, n_cols, curve, base, fill)
        top = self.height - 1
        for f in ("data_x", "data_y"):
            self.fam[f][top] = bytearray([fill]) * (2 * n_total * 32 * n_cols)
        self.scalars = {"x": None, "y": None}          # the rows of alignment scalars of the last rebuild, for the tests

    def aligned_parts(self, write_step):
        """((rows mod p_icc, rows of scalars) of the X part, the same of the Y part) of the network over U as it stands"""
        X, Y = icc_py.crebuild(self.u_rows(), self.curve, write_step)
        out = []
        for part in (X, Y):
            pairs = [icc_py.align(row, self.curve) for row in part]
            out.append(([p[0] for p in pairs], [p[1] for p in pairs]))
        return tuple(out)

    def rebuild(self, chunks, mac, index, complements=None, write_step=None):
        n, top = self.n_total, self.height - 1
        self.write_step = self.write_step + 1 if write_step is None else write_step
        self.store(index, chunks, mac)                                                  # 1
        (ax, cx), (ay, cy) = self.aligned_parts(self.write_step)                        # 2
        r = 32 * self.n_cols
        self.fam["data_x"][top][:n * r] = b"".join(row32_bytes(row) for row in ax)
        self.fam["data_y"][top][:n * r] = b"".join(row32_bytes(row) for row in ay)
        self.scalars = {"x": cx, "y": cy}
        MX, MY = self.mac_network(self.write_step)                                      # 3
        if complements is not None:                                                     # 5
            assert len(complements) == 2 * n
            MX = [icc_py.ec_add(self.curve, p, c) for p, c in zip(MX, complements[:n])]
            MY = [icc_py.ec_add(self.curve, p, c) for p, c in zip(MY, complements[n:])]
        self.fam["mac_x"][top][:64 * n] = b"".join(pt_bytes(p) for p in MX)
        self.fam["mac_y"][top][:64 * n] = b"".join(pt_bytes(p) for p in MY)
        self.fam["align_x"][top][:64 * n] = b"".join(pt_bytes(self.commit(cs)) for cs in cx)   # 4
        self.fam["align_y"][top][:64 * n] = b"".join(pt_bytes(self.commit(cs)) for cs in cy)
        for i in range(top):                                                            # clear_H_data / clear_H_MAC: flags only
            self.empty[i] = True
        self.empty[top] = False
        return self.write_step, top
