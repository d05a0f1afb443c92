"""Host-side mirror of the ICC encode step of the reference's Server (CRebuild_Cached data part,
porla/Server/Server.hpp:1487-1833, and the scalar part of align_MAC, Server.hpp:531-541) over the engine's
C ABI (include/porla_gpu.h: porla_icc_encode_*).  Rows are in the reference's own formats: 32-byte
little-endian chunks in (utils.h:353-364), 64-byte little-endian values mod LCM out (utils.h:473-517)."""
import ctypes

from .loader import IccDecodeRaggedReq, IccDecodeReq, IccMacDecodeReq, ServerRebuildReq, UpdateReq, lib

CURVE = {"bn254": 0, "secp256k1": 1}
NUM_CHUNKS = 128  # config.hpp:22


def _check(rc):
    if rc != 0:
        raise RuntimeError("porla engine error %d: %s" % (rc, lib.porla_gpu_last_error().decode()))


def crebuild_host(rows, n_rows, n_cols=NUM_CHUNKS, curve="bn254", write_step=0, part=0, want_x=True,
                  want_aligned=True, want_scalars=True, scalar_le=False):
    """rows: n_rows*n_cols*32 bytes.  Returns (x_rows, aligned_rows, scalars) as bytes (or None)."""
    total = n_rows * n_cols
    x = ctypes.create_string_buffer(64 * total) if want_x else None
    al = ctypes.create_string_buffer(32 * total) if want_aligned else None
    sc = ctypes.create_string_buffer(32 * total) if want_scalars else None
    _check(lib.porla_icc_encode_host(bytes(rows), n_rows, n_cols, CURVE[curve], write_step, part,
                                     ctypes.cast(x, ctypes.c_void_p) if x else None,
                                     ctypes.cast(al, ctypes.c_void_p) if al else None,
                                     ctypes.cast(sc, ctypes.c_void_p) if sc else None, 1 if scalar_le else 0))
    return (x.raw if x else None, al.raw if al else None, sc.raw if sc else None)


def crebuild_cols_host(rows, n_rows, n_cols, col_begin, col_end, x, aligned, scalars, curve="bn254", write_step=0, part=0,
                       scalar_le=False):
    """column sharding: encode columns [col_begin, col_end) of the row-major `rows` into the same columns of the caller's
    full-width ctypes buffers x / aligned / scalars (each may be None)"""
    vp = ctypes.c_void_p
    _check(lib.porla_icc_encode_cols_host(bytes(rows), n_rows, n_cols, col_begin, col_end, CURVE[curve], write_step, part,
                                          ctypes.cast(x, vp) if x else None, ctypes.cast(aligned, vp) if aligned else None,
                                          ctypes.cast(scalars, vp) if scalars else None, 1 if scalar_le else 0))


def crebuild_host_multi(rows, n_rows, n_cols=NUM_CHUNKS, curve="bn254", write_step=0, part=0, devices=0, scalar_le=False):
    """the whole encode with the columns split over `devices` GPUs of this process (0 = every visible one)"""
    total = n_rows * n_cols
    x, al, sc = (ctypes.create_string_buffer(64 * total), ctypes.create_string_buffer(32 * total), ctypes.create_string_buffer(32 * total))
    vp = ctypes.c_void_p
    _check(lib.porla_icc_encode_host_multi(bytes(rows), n_rows, n_cols, CURVE[curve], write_step, part, ctypes.cast(x, vp),
                                           ctypes.cast(al, vp), ctypes.cast(sc, vp), 1 if scalar_le else 0, devices))
    return x.raw, al.raw, sc.raw


def crebuild_device(d_rows, n_rows, n_cols, curve, write_step, part, d_x=0, d_aligned=0, d_scalars=0, scalar_le=False,
                    stream=0):
    """device-pointer form (integers, e.g. torch tensor .data_ptr()); asynchronous on `stream`."""
    _check(lib.porla_icc_encode_device(ctypes.c_void_p(d_rows), n_rows, n_cols, CURVE[curve], write_step, part,
                                       ctypes.c_void_p(d_x or None), ctypes.c_void_p(d_aligned or None),
                                       ctypes.c_void_p(d_scalars or None), 1 if scalar_le else 0, ctypes.c_void_p(stream)))


def crebuild_xy_device(d_rows, n_rows, n_cols, curve, write_step, d_x=0, d_aligned=0, d_scalars=0, d_y_x=0, d_y_aligned=0,
                       d_y_scalars=0, scalar_le=False, stream=0):
    """X and Y parts from one run of the network (Y_k = wt X_k mod LCM); device pointers, any output may be 0"""
    vp = ctypes.c_void_p
    _check(lib.porla_icc_encode_xy_device(vp(d_rows), n_rows, n_cols, CURVE[curve], write_step, vp(d_x or None), vp(d_aligned or None),
                                          vp(d_scalars or None), vp(d_y_x or None), vp(d_y_aligned or None), vp(d_y_scalars or None),
                                          1 if scalar_le else 0, vp(stream)))


def mac_crebuild_host(macs, n_rows, curve="bn254", write_step=0, part=0):
    """MAC halves of CRebuild_Cached (Server.hpp:1523-1536, 1590-1609, 1658-1676): n_rows 64-byte affine MACs in/out."""
    out = ctypes.create_string_buffer(64 * n_rows)
    _check(lib.porla_icc_mac_encode_host(bytes(macs), n_rows, CURVE[curve], write_step, part, out))
    return out.raw


def mac_crebuild_xy_host(macs, n_rows, curve="bn254", write_step=0):
    """both MAC halves of CRebuild_Cached from one butterfly network (Y_k = wt * X_k): (X part, Y part)"""
    ox, oy = ctypes.create_string_buffer(64 * n_rows), ctypes.create_string_buffer(64 * n_rows)
    _check(lib.porla_icc_mac_encode_xy_host(bytes(macs), n_rows, CURVE[curve], write_step, ox, oy))
    return ox.raw, oy.raw


def mac_crebuild_xy_device(d_macs, n_rows, curve, write_step, d_out_x, d_out_y, stream=0):
    _check(lib.porla_icc_mac_encode_xy_device(ctypes.c_void_p(d_macs), n_rows, CURVE[curve], write_step, ctypes.c_void_p(d_out_x),
                                              ctypes.c_void_p(d_out_y), ctypes.c_void_p(stream)))


def kzg_crebuild_stage_device(d_rows, n_rows, write_step, d_aligned_x, d_aligned_y, d_scalars_xy, d_commits_xy, d_macs, d_macs_x,
                              d_macs_y, stream=0):
    """the last encode stage of a CRebuild (KZG build) in one call: both parts' encode + alignment scalars + commitments and, beside
    them on a second stream inside, both MAC encodes (include/porla_gpu.h: porla_kzg_crebuild_stage_device)"""
    vp = ctypes.c_void_p
    _check(lib.porla_kzg_crebuild_stage_device(vp(d_rows), n_rows, ctypes.c_ulonglong(write_step), vp(d_aligned_x or None),
                                               vp(d_aligned_y or None), vp(d_scalars_xy), vp(d_commits_xy), vp(d_macs), vp(d_macs_x),
                                               vp(d_macs_y), vp(stream)))


def mac_crebuild_device(d_macs, n_rows, curve, write_step, part, d_out, stream=0):
    _check(lib.porla_icc_mac_encode_device(ctypes.c_void_p(d_macs), n_rows, CURVE[curve], write_step, part,
                                           ctypes.c_void_p(d_out), ctypes.c_void_p(stream)))


def audit_combine_device(d_rows64, d_idx64, d_coef64, n64, d_rows32, d_idx32, d_coef32, n32, n_cols, curve,
                         d_exact=0, d_aligned=0, d_aligned_be=0, d_scalars=0, stream=0):
    """Server::audit row combine + align_MAC scalar part (Server.hpp:790-828, 531-541); all arguments device addresses."""
    vp = ctypes.c_void_p
    _check(lib.porla_audit_combine_device(vp(d_rows64 or None), vp(d_idx64 or None), vp(d_coef64 or None), n64,
                                          vp(d_rows32 or None), vp(d_idx32 or None), vp(d_coef32 or None), n32, n_cols,
                                          CURVE[curve], vp(d_exact or None), vp(d_aligned or None), vp(d_aligned_be or None),
                                          vp(d_scalars or None), vp(stream)))


def mix_host(a0, a1, length, n_cols, n_total, curve="bn254"):
    """Server::mix data part (Server.hpp:1269-1278): two blocks of `length` rows of 64-byte symbols -> 2*length rows."""
    out = ctypes.create_string_buffer(2 * length * n_cols * 64)
    _check(lib.porla_icc_mix_host(bytes(a0), bytes(a1), length, n_cols, n_total, CURVE[curve], out))
    return out.raw


def mac_mix_host(a0, a1, length, n_total, curve="bn254"):
    """Server::mix MAC part (Server.hpp:1281-1318): two blocks of `length` 64-byte affine MACs -> 2*length MACs."""
    out = ctypes.create_string_buffer(2 * length * 64)
    _check(lib.porla_icc_mac_mix_host(bytes(a0), bytes(a1), length, n_total, CURVE[curve], out))
    return out.raw


# ---- Server::HAdd / Client::HAdd and the HRebuild chains (Server.hpp:1388-1477, 1329-1386; Client.hpp:978-1038) ----
def hadd_host(data, n_total, write_step, curve="bn254", n_cols=NUM_CHUNKS, scalar_le=False):
    """data side of HAdd on one block: (data_B2 aligned mod p_icc [32-B LE each], alignment scalars, wt as 32-byte BE scalar)"""
    b2, sc, wt = ctypes.create_string_buffer(32 * n_cols), ctypes.create_string_buffer(32 * n_cols), ctypes.create_string_buffer(32)
    _check(lib.porla_icc_hadd_host(bytes(data), n_cols, n_total, write_step, CURVE[curve], b2, sc, 1 if scalar_le else 0, wt))
    return b2.raw, sc.raw, wt.raw


def mac_scale_host(mac, n_total, write_step, curve="bn254"):
    """MAC_B2 = wt * MAC (Server.hpp:1400-1417; Client::HAdd, Client.hpp:996-1014)"""
    out = ctypes.create_string_buffer(64)
    _check(lib.porla_icc_mac_scale_host(bytes(mac), n_total, write_step, CURVE[curve], out))
    return out.raw


def kzg_hadd_host(data, mac, n_total, write_step, n_cols=NUM_CHUNKS):
    """Server::HAdd for the KZG build: (data_B2, MAC_B2, MAC_align_B2)"""
    b2, m2, ma = ctypes.create_string_buffer(32 * n_cols), ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
    _check(lib.porla_kzg_hadd_host(bytes(data), bytes(mac), n_total, write_step, b2, m2, ma))
    return b2.raw, m2.raw, ma.raw


def _level_ptrs(bufs):
    arr = (ctypes.c_void_p * len(bufs))()
    for i, b in enumerate(bufs):
        arr[i] = ctypes.cast(b, ctypes.c_void_p)
    return arr


def hrebuild_host(level_bufs, level, n_total, curve="bn254", n_cols=NUM_CHUNKS):
    """level_bufs[i]: ctypes buffer of 2 * 2^i rows x n_cols x 64 bytes (resident half, incoming half); rebuilt in place"""
    _check(lib.porla_icc_hrebuild_host(_level_ptrs(level_bufs), level, n_cols, n_total, CURVE[curve]))


def mac_hrebuild_host(level_bufs, level, n_total, curve="bn254"):
    """the same for 64-byte affine points (MAC commitments, MAC alignments, the client's complements)"""
    _check(lib.porla_icc_mac_hrebuild_host(_level_ptrs(level_bufs), level, n_total, CURVE[curve]))


# ---- Server::update's H path for K files in one asynchronous call (include/porla_gpu.h: porla_*_update_batch_device) ----
UPDATE_FAMILIES = ("data_x", "data_y", "mac_x", "mac_y", "align_x", "align_y")


def update_requests(reqs):
    """a ctypes array of porla_update_req from per-write tuples (d_block, d_mac, d_complements or 0, write_step, level, data_x, data_y,
    mac_x, mac_y, align_x, align_y): device addresses as integers, each family a sequence of level + 1 of them (None: a NULL family
    array).  The array keeps the pointer arrays it refers to alive (arr._keep)."""
    arr = (UpdateReq * max(len(reqs), 1))()
    keep = []
    for i, r in enumerate(reqs):
        if len(r) != 11:
            raise ValueError("update_batch_device: request %d has %d fields, want 11" % (i, len(r)))
        fams = []
        for f in r[5:]:
            if f is None:
                fams.append(None)
                continue
            a = (ctypes.c_void_p * max(len(f), 1))(*[(x or None) for x in f])
            keep.append(a)
            fams.append(ctypes.cast(a, ctypes.POINTER(ctypes.c_void_p)))
        arr[i] = UpdateReq(r[0] or None, r[1] or None, r[2] or None, r[3], r[4], 0, *fams)
    arr._keep = keep
    return arr


def kzg_update_batch_device(reqs, n_total, stream=0):
    """Server::update's H path (HAdd, HRebuildX / Y, the complement adds) of len(reqs) independent files in ONE asynchronous call on
    `stream`, KZG build: the level stores named by the requests are rewritten in place on the device.  `reqs`: tuples as update_requests
    takes them."""
    arr = update_requests(reqs)
    _check(lib.porla_kzg_update_batch_device(arr, len(reqs), n_total, ctypes.c_void_p(stream)))


# ---- the server's rebuild write for K files in one asynchronous call (include/porla_gpu.h: porla_server_rebuild_batch_device) ----
SERVER_REBUILD_FIELDS = ("d_block", "d_mac", "d_complements", "d_u_blocks", "d_u_macs", "d_data_x", "d_data_y", "d_mac_x", "d_mac_y",
                         "d_align_x", "d_align_y", "write_step", "index")


def server_rebuild_requests(reqs):
    """a ctypes array of porla_server_rebuild_req from per-write tuples in the order of SERVER_REBUILD_FIELDS: eleven device addresses
    as integers (0 = NULL; the top-level buffers are what the update batch takes as family[log2 n_total]), write_step and index"""
    arr = (ServerRebuildReq * max(len(reqs), 1))()
    for i, r in enumerate(reqs):
        if len(r) != 13:
            raise ValueError("server_rebuild_batch_device: request %d has %d fields, want 13" % (i, len(r)))
        arr[i] = ServerRebuildReq(*[(x or None) for x in r[:11]], r[11], r[12])
    return arr


def server_rebuild_batch_device(reqs, n_total, n_cols, curve, stream=0):
    """the write on which Server::update calls CRebuild (the store, both networks over U and MAC_U into the resident halves of the top
    level, the alignments to infinity, the complement adds) for len(reqs) independent files in ONE asynchronous call on `stream`.
    `reqs`: tuples as server_rebuild_requests takes them; curve: "bn254" or "secp256k1"."""
    arr = server_rebuild_requests(reqs)
    _check(lib.porla_server_rebuild_batch_device(arr, len(reqs), n_total, n_cols, CURVE[curve], ctypes.c_void_p(stream)))


def kzg_server_rebuild_aligned_batch_device(reqs, n_total, stream=0):
    """the same write in the CRebuild_No_Cached form, KZG build (porla_kzg_server_rebuild_aligned_batch_device): the top-level data rows
    mod p_icc in the 256-bit row format (2 * n_total rows of porla_kzg_row_coefficients 32-byte symbols, what the audits take as
    d_rows32) and, per row, the commitment of its alignment scalars against the resident SRS.  `reqs`: tuples as
    server_rebuild_requests takes them.  The IPA twin is FixedBase.ipa_server_rebuild_aligned_batch_device."""
    arr = server_rebuild_requests(reqs)
    _check(lib.porla_kzg_server_rebuild_aligned_batch_device(arr, len(reqs), n_total, ctypes.c_void_p(stream)))


# ---- the ICC decode: the rows of K levels back to their blocks in one asynchronous call (include/porla_gpu.h:
# porla_icc_decode_batch_device) ----
DECODE_FORM = {"exact": 0, "residue64": 1, "residue32": 2}


def decode_requests(reqs):
    """a ctypes array of porla_icc_decode_req from per-level tuples (d_rows, d_out, d_write_steps or 0, d_bad or 0): device addresses
    as integers"""
    arr = (IccDecodeReq * max(len(reqs), 1))()
    for i, r in enumerate(reqs):
        if len(r) != 4:
            raise ValueError("decode_batch_device: request %d has %d fields, want 4" % (i, len(r)))
        arr[i] = IccDecodeReq(*[(x or None) for x in r])
    return arr


def decode_batch_device(reqs, n_rows, n_cols, n_total, curve, form, stream=0):
    """the inverse of the data network on len(reqs) levels of n_rows rows in ONE asynchronous call on `stream`: output row i is input i
    of the network whose output is d_rows.  form: "exact" (64-byte rows -> the 256-bit chunks; a symbol that cannot be a chunk is
    counted in d_bad), "residue64" / "residue32" (64- / 32-byte rows -> chunk mod p_icc; with d_write_steps position i is unscaled by
    wt_i^-1).  `reqs`: tuples as decode_requests takes them; curve: "bn254" or "secp256k1"."""
    arr = decode_requests(reqs)
    _check(lib.porla_icc_decode_batch_device(arr, len(reqs), n_rows, n_cols, n_total, CURVE[curve], DECODE_FORM[form],
                                             ctypes.c_void_p(stream)))


def decode_ragged_requests(reqs):
    """a ctypes array of porla_icc_decode_ragged_req from per-level tuples (d_rows, d_out, d_write_steps or 0, d_bad or 0, n_rows):
    device addresses as integers, then the level's own row count"""
    arr = (IccDecodeRaggedReq * max(len(reqs), 1))()
    for i, r in enumerate(reqs):
        if len(r) != 5:
            raise ValueError("decode_ragged_batch_device: request %d has %d fields, want 5" % (i, len(r)))
        arr[i] = IccDecodeRaggedReq(*[(x or None) for x in r[:4]], r[4])
    return arr


def decode_ragged_batch_device(reqs, n_cols, n_total, curve, form, stream=0):
    """decode_batch_device for levels of unequal sizes in ONE asynchronous call on `stream`: every request brings its own n_rows (a
    power of two, 2 .. n_total) and gets the bytes decode_batch_device writes for it alone; the launches depend on whether levels of up
    to 2^9 rows and larger ones are present, not on how many or which.  `reqs`: tuples as decode_ragged_requests takes them."""
    arr = decode_ragged_requests(reqs)
    _check(lib.porla_icc_decode_ragged_batch_device(arr, len(reqs), n_cols, n_total, CURVE[curve], DECODE_FORM[form],
                                                    ctypes.c_void_p(stream)))


def decode_host(rows, n_rows, n_cols, n_total, curve="bn254", form="exact", write_steps=None, want_bad=None):
    """one level from host memory.  Returns (out, bad): n_rows * n_cols * 32 bytes, and the count of symbols that cannot be chunks
    ("exact"; None for the residue forms unless want_bad is forced, which the library refuses)."""
    out = ctypes.create_string_buffer(32 * n_rows * n_cols)
    if want_bad is None:
        want_bad = form == "exact"
    bad = ctypes.c_uint(0xffffffff) if want_bad else None
    steps = (ctypes.c_ulonglong * n_rows)(*write_steps) if write_steps is not None else None
    _check(lib.porla_icc_decode_host(bytes(rows), n_rows, n_cols, n_total, CURVE[curve], DECODE_FORM[form], steps,
                                     ctypes.cast(out, ctypes.c_void_p), ctypes.byref(bad) if want_bad else None))
    return out.raw, (bad.value if want_bad else None)


# ---- the ICC MAC decode: the coded MAC rows of K levels back to their per-block MACs in one asynchronous call (include/porla_gpu.h:
# porla_icc_mac_decode_batch_device) ----
def mac_decode_requests(reqs):
    """a ctypes array of porla_icc_mac_decode_req from per-level tuples (d_macs, d_out, d_write_steps or 0, d_sub or 0): device
    addresses as integers"""
    arr = (IccMacDecodeReq * max(len(reqs), 1))()
    for i, r in enumerate(reqs):
        if len(r) != 4:
            raise ValueError("mac_decode_batch_device: request %d has %d fields, want 4" % (i, len(r)))
        arr[i] = IccMacDecodeReq(*[(x or None) for x in r])
    return arr


def mac_decode_batch_device(reqs, n_rows, n_total, curve, stream=0):
    """the inverse of the MAC network on len(reqs) levels of n_rows 64-byte affine points in ONE asynchronous call on `stream`: output
    row i is input i of the network whose output is d_macs - d_sub; with d_write_steps position i is also multiplied by wt_i^-1 mod q.
    `reqs`: tuples as mac_decode_requests takes them; curve: "bn254" or "secp256k1"."""
    arr = mac_decode_requests(reqs)
    _check(lib.porla_icc_mac_decode_batch_device(arr, len(reqs), n_rows, n_total, CURVE[curve], ctypes.c_void_p(stream)))


def mac_decode_host(macs, n_rows, n_total, curve="bn254", write_steps=None, sub=None):
    """one level from host memory: n_rows 64-byte affine points in (and optionally n_rows to subtract), n_rows out"""
    out = ctypes.create_string_buffer(64 * n_rows)
    steps = (ctypes.c_ulonglong * n_rows)(*write_steps) if write_steps is not None else None
    _check(lib.porla_icc_mac_decode_host(bytes(macs), n_rows, n_total, CURVE[curve], steps, bytes(sub) if sub is not None else None,
                                         ctypes.cast(out, ctypes.c_void_p)))
    return out.raw
