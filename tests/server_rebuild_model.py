"""A Python restatement of the write on which Server::update calls CRebuild (porla/Server/Server.hpp:413-469 with CRebuild_Cached
:1487-1833) for ONE file, built from oracle/icc_py.py (crebuild, mac_crebuild, ec_add) on the byte layout of tests/update_model.py's
FileModel, which it extends by the two raw stores (U: n_total x n_cols x 32 bytes little-endian; MAC_U: n_total x 64 bytes big-endian
affine) so that update() no longer asserts on CRebuild's step:

  1. U[index-1] = block, MAC_U[index-1] = mac                                                     (:413-427)
  2. data X / data Y of the top level, resident half = crebuild(U)                                 (:1548-1687, :1691-1830)
  3. MAC X / MAC Y of the top level, resident half = mac_crebuild(MAC_U)                           (:1523-1536 and the stage loops)
  4. align X / align Y of the top level, resident half = infinity                                  (:1527-1535)
  5. mac_x[j] += comp[j], mac_y[j] += comp[n_total + j]                                            (:449-469, updated_level = height-1)

Every buffer starts filled with `fill`; only the rows the reference writes are written.  A helper of tests/test_server_rebuild_batch_*.py,
not a test module."""
import icc_py

from tests.update_model import FileModel, pt_bytes, pt_tuple, row_bytes


_MAC_NETWORKS = {}                  # (curve, MAC_U bytes, write_step) -> mac_crebuild's result: a test may ask for it before the write


class RebuildFileModel(FileModel):
    def __init__(self, n_total, n_cols, curve, base, fill=0):
        super().__init__(n_total, n_cols, curve, base, fill)
        self.u_blocks = bytearray([fill]) * (n_total * n_cols * 32)
        self.u_macs = bytearray([fill]) * (n_total * 64)

    # ---- the raw stores
    def store(self, index, chunks, mac):
        """U[index-1] = block, MAC_U[index-1] = mac; index is the block id 1 .. n_total"""
        assert 1 <= index <= self.n_total
        r = 32 * self.n_cols
        self.u_blocks[(index - 1) * r:index * r] = b"".join(c.to_bytes(32, "little") for c in chunks)
        self.u_macs[(index - 1) * 64:index * 64] = pt_bytes(mac)

    def u_rows(self):
        r = 32 * self.n_cols
        return [[int.from_bytes(self.u_blocks[i * r + 32 * c:i * r + 32 * c + 32], "little") for c in range(self.n_cols)]
                for i in range(self.n_total)]

    def u_mac_points(self):
        return [pt_tuple(self.u_macs[64 * i:64 * i + 64]) for i in range(self.n_total)]

    def mac_network(self, write_step):
        """icc_py.mac_crebuild on MAC_U as it stands: (X part, Y part) before the complements"""
        key = (self.curve, bytes(self.u_macs), write_step)
        if key not in _MAC_NETWORKS:
            _MAC_NETWORKS[key] = icc_py.mac_crebuild(self.u_mac_points(), self.curve, write_step)
        return tuple(list(part) for part in _MAC_NETWORKS[key])

    # ---- a write
    def update(self, chunks, mac, complements=None, index=None, write_step=None):
        """FileModel.update for an H step (the block also goes to U when `index` is given); CRebuild's step otherwise, where `index`
        is required.  write_step overrides the counter's next value on CRebuild's step (the call accepts any value).  Returns
        (write_step, level)."""
        if self.next_level() is not None and write_step is None:
            if index is not None:
                self.store(index, chunks, mac)
            return super().update(chunks, mac, complements)
        assert index is not None, "CRebuild's step needs the block id"
        return self.rebuild(chunks, mac, index, complements, write_step)

    def rebuild(self, chunks, mac, index, complements=None, write_step=None):
        n, top = self.n_total, self.height - 1
        self.write_step = self.write_step + 1 if write_step is None else write_step
        self.store(index, chunks, mac)                                                  # 1
        X, Y = icc_py.crebuild(self.u_rows(), self.curve, self.write_step)              # 2
        r = 64 * self.n_cols
        self.fam["data_x"][top][:n * r] = b"".join(row_bytes(row) for row in X)
        self.fam["data_y"][top][:n * r] = b"".join(row_bytes(row) for row in Y)
        MX, MY = self.mac_network(self.write_step)                                      # 3
        if complements is not None:                                                     # 5
            assert len(complements) == 2 * n
            MX = [icc_py.ec_add(self.curve, p, c) for p, c in zip(MX, complements[:n])]
            MY = [icc_py.ec_add(self.curve, p, c) for p, c in zip(MY, complements[n:])]
        self.fam["mac_x"][top][:64 * n] = b"".join(pt_bytes(p) for p in MX)
        self.fam["mac_y"][top][:64 * n] = b"".join(pt_bytes(p) for p in MY)
        self.fam["align_x"][top][:64 * n] = bytes(64 * n)                               # 4
        self.fam["align_y"][top][:64 * n] = bytes(64 * n)
        for i in range(top):                                                            # clear_H_data / clear_H_MAC: flags only
            self.empty[i] = True
        self.empty[top] = False
        return self.write_step, top

    def top_bytes(self):
        """{family: bytes of the top level}, plus the two stores"""
        out = {f: bytes(self.fam[f][self.height - 1]) for f in self.fam}
        out["u_blocks"], out["u_macs"] = bytes(self.u_blocks), bytes(self.u_macs)
        return out
