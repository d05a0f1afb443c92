"""Host-side mirror of the reference's KZG wrapper layer (porla/Utils/utils.h:235-305) over libmultiexp.so.

Same names and argument meaning as the C++ wrappers the reference's Server/Client call:
  bn254_add / bn254_mult / bn254_neg / bn254_set_infinity      utils.h:235-269
  bn254_scalar_set_int                                          utils.h:271-275
  bn254_multi_exp                                               utils.h:277-292
  bn254_compare                                                 utils.h:294-305
plus the direct GoSlice calls (init_key, init_SRS, ... Client.hpp:159-167,348-354,411-419,445-453,1637-1662;
Server.hpp:183-188,365-397,550-558).  Buffers are Python bytes/bytearray; results are returned as bytes.
"""
import ctypes

from .loader import GoSlice, IpaAuditReq, IpaVerifyReq, KzgAuditReq, KzgVerifyReq, lib

MAC_SIZE = 64       # COMMITMENT_MAC_SIZE with ENABLE_KZG, config.hpp:26
SCALAR_SIZE = 32    # bn254_scalar = uint32_t[8], utils.h:64


def _slice(buf):
    """GoSlice over a mutable ctypes buffer."""
    return GoSlice(ctypes.cast(buf, ctypes.c_void_p), len(buf), len(buf))


def _buf(data):
    return ctypes.create_string_buffer(bytes(data), len(data))


def _check(rc):
    if rc != 0:
        raise RuntimeError("porla engine error %d: %s" % (rc, lib.porla_gpu_last_error().decode()))


# ---- utils.h wrappers ---------------------------------------------------------------------------
def bn254_add(a, b):
    """utils.h:235-244 -> add_point (in place on a; returned here)."""
    ba, bb = _buf(a), _buf(b)
    sa, sb = _slice(ba), _slice(bb)
    lib.add_point(ctypes.byref(sa), ctypes.byref(sb))
    return ba.raw


def bn254_mult(a, scalar):
    """utils.h:246-255 -> mult_point."""
    ba, bs = _buf(a), _buf(scalar)
    sa, ss = _slice(ba), _slice(bs)
    lib.mult_point(ctypes.byref(sa), ctypes.byref(ss))
    return ba.raw


def bn254_neg(a):
    """utils.h:257-262 -> neg_point."""
    ba = _buf(a)
    sa = _slice(ba)
    lib.neg_point(ctypes.byref(sa))
    return ba.raw


def bn254_set_infinity():
    """utils.h:264-269 -> set_inf_point."""
    ba = _buf(b"\xff" * MAC_SIZE)
    sa = _slice(ba)
    lib.set_inf_point(ctypes.byref(sa))
    return ba.raw


def bn254_scalar_set_int(v):
    """utils.h:271-275: 28 zero bytes then v big-endian."""
    return bytes(28) + int(v & 0xffffffff).to_bytes(4, "big")


def bn254_multi_exp(points, scalars, n):
    """utils.h:277-292 -> compute_multi_exp(scalars, points, n, result)."""
    bs, bp, out = _buf(scalars), _buf(points), _buf(bytes(MAC_SIZE))
    ss, sp, so = _slice(bs), _slice(bp), _slice(out)
    lib.compute_multi_exp(ctypes.byref(ss), ctypes.byref(sp), n, ctypes.byref(so))
    return out.raw


def bn254_compare(a, b):
    """utils.h:294-305 -> compare_commitment."""
    ba, bb = _buf(a), _buf(b)
    sa, sb = _slice(ba), _slice(bb)
    return bool(lib.compare_commitment(ctypes.byref(sa), ctypes.byref(sb)))


# ---- direct cgo calls ---------------------------------------------------------------------------
def init_key(tau, alpha):
    bt, ba = _buf(tau), _buf(alpha)
    st, sa = _slice(bt), _slice(ba)
    lib.init_key(ctypes.byref(st), ctypes.byref(sa))


def init_SRS(n):
    """Client.hpp:348-354: returns the 32n+132-byte wire blob."""
    out = _buf(bytes(32 * n + 132 + 64))
    so = _slice(out)
    ln = ctypes.c_longlong(0)
    lib.init_SRS(n, ctypes.byref(so), ctypes.byref(ln))
    return out.raw[:ln.value]


def init_SRS_from_data(n, blob):
    bb = _buf(blob)
    sb = _slice(bb)
    lib.init_SRS_from_data(n, ctypes.byref(sb))


def _in_out(fn, data, out_len):
    bi, bo = _buf(data), _buf(bytes(out_len))
    si, so = _slice(bi), _slice(bo)
    fn(ctypes.byref(si), ctypes.byref(so))
    return bo.raw


def compute_digest(data):
    return _in_out(lib.compute_digest, data, MAC_SIZE)


def compute_digest_complement(data):
    return _in_out(lib.compute_digest_complement, data, MAC_SIZE)


def compute_digest_from_srs(data):
    return _in_out(lib.compute_digest_from_srs, data, MAC_SIZE)


def create_proof(random_point, data):
    """Server.hpp:363-398: returns (commitment 64, H 64, point 32, claim 32)."""
    bi = _buf(data)
    outs = [_buf(bytes(64)), _buf(bytes(64)), _buf(bytes(32)), _buf(bytes(32))]
    si = _slice(bi)
    so = [_slice(o) for o in outs]
    lib.create_proof(random_point, ctypes.byref(si), *[ctypes.byref(s) for s in so])
    return tuple(o.raw for o in outs)


def verify_proof(commitment, proof_h, point, claim):
    bufs = [_buf(commitment), _buf(proof_h), _buf(point), _buf(claim)]
    sl = [_slice(b) for b in bufs]
    return bool(lib.verify_proof(*[ctypes.byref(s) for s in sl]))


# ---- device-pointer API (include/porla_gpu.h) -------------------------------------------------------
def msm_device(curve, d_scalars, d_points, n, stream=0, partial=False):
    """d_scalars / d_points: integer device addresses (e.g. torch tensor .data_ptr())."""
    out = ctypes.create_string_buffer(96 if partial else 64)
    fn = getattr(lib, "porla_%s_msm_device%s" % (curve, "_partial" if partial else ""))
    _check(fn(ctypes.c_void_p(d_scalars), ctypes.c_void_p(d_points), n, out, ctypes.c_void_p(stream)))
    return out.raw


def msm_begin(slot, d_scalars, d_points, n, stream=0, curve="bn254"):
    """two-phase MSM: enqueue on `stream` into workspace slot 1..3 (include/porla_gpu.h)"""
    fn = getattr(lib, "porla_%s_msm_device_begin" % curve)
    _check(fn(slot, ctypes.c_void_p(d_scalars), ctypes.c_void_p(d_points), n, ctypes.c_void_p(stream)))


def msm_end(slot, partial=False, curve="bn254"):
    out = ctypes.create_string_buffer(96 if partial else 64)
    _check(getattr(lib, "porla_%s_msm_device_end" % curve)(slot, out, 1 if partial else 0))
    return out.raw


def msm_host(curve, scalars, points, n):
    out = ctypes.create_string_buffer(64)
    _check(getattr(lib, "porla_%s_msm_host" % curve)(bytes(scalars), bytes(points), n, out))
    return out.raw


def msm_pair_device(curve, d_scalars, d_points_a, d_points_b, n, stream=0):
    """the audit's two MSMs over one scalar array (Server.hpp:900-901 / :842-848) in one call: (sum s_i A_i, sum s_i B_i)"""
    oa, ob = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
    _check(getattr(lib, "porla_%s_msm_pair_device" % curve)(ctypes.c_void_p(d_scalars), ctypes.c_void_p(d_points_a), ctypes.c_void_p(d_points_b),
                                                            n, oa, ob, ctypes.c_void_p(stream)))
    return oa.raw, ob.raw


def audit_msm_pair_device(curve, d_store_a, d_store_b, d_idx, d_coef, n, stream=0):
    """the audit's two MSMs from resident MAC arrays: (sum coef_i store_a[idx_i], sum coef_i store_b[idx_i]); idx int64, coef abs(int32)"""
    oa, ob = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
    vp = ctypes.c_void_p
    _check(getattr(lib, "porla_%s_audit_msm_pair_device" % curve)(vp(d_store_a), vp(d_store_b), vp(d_idx), vp(d_coef), n, oa, ob, vp(stream)))
    return oa.raw, ob.raw


def audit_msm_pair_begin(slot, curve, d_store_a, d_store_b, d_idx, d_coef, n, stream=0):
    vp = ctypes.c_void_p
    _check(getattr(lib, "porla_%s_audit_msm_pair_begin" % curve)(slot, vp(d_store_a), vp(d_store_b), vp(d_idx), vp(d_coef), n, vp(stream)))


def audit_msm_pair_end(slot, curve):
    oa, ob = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
    _check(getattr(lib, "porla_%s_audit_msm_pair_end" % curve)(slot, oa, ob))
    return oa.raw, ob.raw


def msm_pair_host(curve, scalars, points_a, points_b, n):
    oa, ob = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
    _check(getattr(lib, "porla_%s_msm_pair_host" % curve)(bytes(scalars), bytes(points_a), bytes(points_b), n, oa, ob))
    return oa.raw, ob.raw


def batch_offsets(sizes):
    """the offsets array of a batched MSM from its entries' sizes: [0, s0, s0 + s1, ...]"""
    offs = [0]
    for s in sizes:
        if s < 0:
            raise ValueError("a batched MSM entry cannot have %d pairs" % s)
        offs.append(offs[-1] + int(s))
    return offs


def _offsets_array(offsets):
    import array
    a = array.array("Q", offsets)           # one C-level conversion (a batch of 32 842 entries: well under a millisecond)
    if not len(a):
        raise ValueError("offsets holds k + 1 values (at least [0])")
    return (ctypes.c_uint64 * len(a)).from_buffer(a), len(a) - 1


def split_outputs(raw, k):
    """k 64-byte affine outputs from one k * 64-byte buffer"""
    raw = bytes(raw)
    if len(raw) < 64 * k:
        raise ValueError("%d bytes hold fewer than %d outputs" % (len(raw), k))
    return [raw[64 * i:64 * (i + 1)] for i in range(k)]


def msm_batch_device(curve, d_scalars, d_points, offsets, d_out, stream=0):
    """K independent MSMs in one call (include/porla_gpu.h): entry k = pairs [offsets[k], offsets[k+1]) of the device arrays,
    its 64-byte affine result written to d_out + 64 k.  Asynchronous on `stream`: d_out is complete when the stream is."""
    arr, k = _offsets_array(offsets)
    _check(getattr(lib, "porla_%s_msm_batch_device" % curve)(ctypes.c_void_p(d_scalars), ctypes.c_void_p(d_points), arr, k,
                                                             ctypes.c_void_p(d_out), ctypes.c_void_p(stream)))


def msm_batch_host(curve, scalars, points, offsets):
    """the same from host bytes, blocking: a list of k 64-byte outputs"""
    arr, k = _offsets_array(offsets)
    out = ctypes.create_string_buffer(64 * k if k else 1)
    _check(getattr(lib, "porla_%s_msm_batch_host" % curve)(bytes(scalars), bytes(points), arr, k, out))
    return split_outputs(out.raw, k)


def msm_host_multi(curve, scalars, points, n, shards=0, devices=0):
    """range-sharded over `shards` pair ranges and `devices` GPUs of this process (0 = automatic), behind the C ABI"""
    out = ctypes.create_string_buffer(64)
    _check(getattr(lib, "porla_%s_msm_host_multi" % curve)(bytes(scalars), bytes(points), n, shards, devices, out))
    return out.raw


def last_msm_multi():
    """(ranges, devices) the most recent msm_host_multi used"""
    s, d = ctypes.c_int(0), ctypes.c_int(0)
    lib.porla_gpu_last_msm_multi(ctypes.byref(s), ctypes.byref(d))
    return s.value, d.value


# ---- one process per GPU: RCCL all-gather of the 96-byte partials, issued from C++ (include/porla_gpu.h) ----
def dist_unique_id():
    out = ctypes.create_string_buffer(128)
    _check(lib.porla_dist_unique_id(out))
    return out.raw


def dist_init(unique_id, rank, world):
    _check(lib.porla_dist_init(bytes(unique_id), rank, world))


def dist_info():
    r, w = ctypes.c_int(0), ctypes.c_int(0)
    lib.porla_dist_info(ctypes.byref(r), ctypes.byref(w))
    return r.value, w.value


def dist_finalize():
    _check(lib.porla_dist_finalize())


def dist_allgather_partials(partial, world):
    out = ctypes.create_string_buffer(96 * world)
    _check(lib.porla_dist_allgather_partials(bytes(partial), out))
    return out.raw


def dist_fold(curve, partial):
    """all ranks' 96-byte partials through one ncclAllGather, folded: the whole job's 64-byte result"""
    out = ctypes.create_string_buffer(64)
    _check(getattr(lib, "porla_%s_dist_fold" % curve)(bytes(partial), out))
    return out.raw


def msm_device_dist(curve, d_scalars, d_points, n_local, stream=0):
    out = ctypes.create_string_buffer(64)
    _check(getattr(lib, "porla_%s_msm_device_dist" % curve)(ctypes.c_void_p(d_scalars), ctypes.c_void_p(d_points), n_local, out,
                                                            ctypes.c_void_p(stream)))
    return out.raw


def jac_sum(curve, jacobians, count):
    out = ctypes.create_string_buffer(64)
    _check(getattr(lib, "porla_%s_jac_sum" % curve)(bytes(jacobians), count, out))
    return out.raw


# ---- Client::update's preprocessing for K writes in one asynchronous call (include/porla_gpu.h: porla_*_client_update_batch_device) ----
def client_update_requests(reqs):
    """a ctypes array of porla_client_update_req from per-write tuples (d_block, d_prf, d_mac_out, d_complements_out, write_step,
    level): device addresses as integers"""
    from .loader import ClientUpdateReq
    arr = (ClientUpdateReq * max(len(reqs), 1))()
    for i, r in enumerate(reqs):
        if len(r) != 6:
            raise ValueError("client_update_batch_device: request %d has %d fields, want 6" % (i, len(r)))
        arr[i] = ClientUpdateReq(r[0] or None, r[1] or None, r[2] or None, r[3] or None, r[4], r[5], 0)
    return arr


def kzg_client_update_batch_device(reqs, n_total, stream=0):
    """Client::update's preprocessing (the block's MAC, the complements below the write's level through HAdd / HRebuildX / HRebuildY,
    the differences that go on the wire) of len(reqs) independent writes in ONE asynchronous call on `stream`, KZG build: d_mac_out
    and d_complements_out of every request are what icc.kzg_update_batch_device takes as d_mac and d_complements.  `reqs`: tuples as
    client_update_requests takes them."""
    arr = client_update_requests(reqs)
    _check(lib.porla_kzg_client_update_batch_device(arr, len(reqs), n_total, ctypes.c_void_p(stream)))


# ---- the client's rebuild write (Client::CRebuild's step) for K writes in one call (include/porla_gpu.h: porla_*_client_rebuild_batch_device) ----
CLIENT_REBUILD_TILE = 1024      # client_rebuild_batch.hip.h:CR_TILE -- the network's stages up to this many symbols run on one LDS tile


def client_rebuild_requests(reqs):
    """a ctypes array of porla_client_rebuild_req from per-write tuples (d_block, d_prf, d_mac_out, d_complements_out, write_step):
    device addresses as integers"""
    from .loader import ClientRebuildReq
    arr = (ClientRebuildReq * max(len(reqs), 1))()
    for i, r in enumerate(reqs):
        if len(r) != 5:
            raise ValueError("client_rebuild_batch_device: request %d has %d fields, want 5" % (i, len(r)))
        arr[i] = ClientRebuildReq(r[0] or None, r[1] or None, r[2] or None, r[3] or None, r[4])
    return arr


def kzg_client_rebuild_batch_device(reqs, n_total, stream=0):
    """The client's side of the write on which the reference calls Client::CRebuild -- the block's MAC, all n_total complements through
    the whole MAC-side network (X and Y part), the 2 * n_total differences that go on the wire -- of len(reqs) independent writes in
    ONE asynchronous call on `stream`, KZG build.  d_prf holds 3 * n_total + 1 PRF outputs per request.  `reqs`: tuples as
    client_rebuild_requests takes them."""
    arr = client_rebuild_requests(reqs)
    _check(lib.porla_kzg_client_rebuild_batch_device(arr, len(reqs), n_total, ctypes.c_void_p(stream)))


# ---- verified retrieval: a level's coded rows checked against its MAC rows, then decoded (include/porla_gpu.h: porla_*_retrieve_*) ----
def retrieve_requests(reqs):
    """a ctypes array of porla_retrieve_req from per-half tuples (d_rows, d_macs, d_prf, d_out or 0, d_status, d_counts or 0): device
    addresses as integers"""
    from .loader import RetrieveReq
    arr = (RetrieveReq * max(len(reqs), 1))()
    for i, r in enumerate(reqs):
        if len(r) != 6:
            raise ValueError("retrieve_batch_device: request %d has %d fields, want 6" % (i, len(r)))
        arr[i] = RetrieveReq(*(x or None for x in r))
    return arr


def _retrieve_host(call, rows, macs, prf, n_rows, n_cols, want_blocks):
    """(status bytes, [failed rows, the decode's bad count], blocks or None) of one level from host memory"""
    for name, buf, want in (("rows", rows, 64 * n_rows * n_cols), ("macs", macs, 64 * n_rows), ("prf", prf, 16 * n_rows)):
        if n_cols and len(buf) != want:                     # the library reads exactly these sizes (no SRS yet: it refuses the call)
            raise ValueError("retrieve_host: %s holds %d bytes, the call reads %d" % (name, len(buf), want))
    out = ctypes.create_string_buffer(32 * n_rows * n_cols) if want_blocks else None
    status = ctypes.create_string_buffer(n_rows)
    counts = (ctypes.c_uint * 2)()
    _check(call(bytes(rows), bytes(macs), bytes(prf), out, status, counts))
    return status.raw, [counts[0], counts[1]], out.raw if want_blocks else None


def kzg_retrieve_batch_device(reqs, n_rows, n_total, stream=0):
    """The coded rows of len(reqs) exact halves checked row by row against their stored MAC rows in the coded domain (status byte 1 iff
    the stored MAC row equals alpha f(tau) G1[0] + prf h_MAC of the row's symbols mod r), then decoded (d_out; 0 = check only), in ONE
    asynchronous call on `stream`, KZG build; n_cols is the SRS size.  `reqs`: tuples as retrieve_requests takes them."""
    arr = retrieve_requests(reqs)
    _check(lib.porla_kzg_retrieve_batch_device(arr, len(reqs), n_rows, n_total, ctypes.c_void_p(stream)))


def kzg_retrieve_host(rows, macs, prf, n_rows, n_total, want_blocks=True):
    """one level from host memory (porla_kzg_retrieve_host; it waits) -> (status bytes, [failed rows, the decode's bad count], blocks
    or None)"""
    n_cols = kzg_row_coefficients()                        # the resident SRS size: what the library reads per row
    return _retrieve_host(lambda r, m, p, out, st, cn: lib.porla_kzg_retrieve_host(r, m, p, n_rows, n_total, out, st, cn),
                          rows, macs, prf, n_rows, n_cols, want_blocks)


# ---- verified retrieval of any half: the alignment store joins the relation (include/porla_gpu.h: porla_*_retrieve_aligned_*) ----
RETRIEVE_FORM = {"exact": 0, "residue64": 1, "residue32": 2}        # icc.DECODE_FORM: the decode's constants
RETRIEVE_SYMBOL_BYTES = {"exact": 64, "residue64": 64, "residue32": 32}


def retrieve_aligned_requests(reqs):
    """a ctypes array of porla_retrieve_aligned_req from per-half tuples (d_rows, d_macs, d_prf, d_align or 0, d_write_steps or 0, d_out
    or 0, d_status, d_counts or 0): device addresses as integers"""
    from .loader import RetrieveAlignedReq
    arr = (RetrieveAlignedReq * max(len(reqs), 1))()
    for i, r in enumerate(reqs):
        if len(r) != 8:
            raise ValueError("retrieve_aligned_batch_device: request %d has %d fields, want 8" % (i, len(r)))
        arr[i] = RetrieveAlignedReq(*(x or None for x in r))
    return arr


def _retrieve_aligned_host(call, rows, macs, prf, align, write_steps, n_rows, n_cols, form, want_blocks):
    """(status bytes, [failed rows, the decode's bad count], blocks or None) of one level from host memory"""
    sizes = [("rows", rows, RETRIEVE_SYMBOL_BYTES[form] * n_rows * n_cols), ("macs", macs, 64 * n_rows), ("prf", prf, 16 * n_rows)]
    if align is not None:
        sizes.append(("align", align, 64 * n_rows))
    for name, buf, want in sizes:
        if n_cols and len(buf) != want:                     # the library reads exactly these sizes (no SRS yet: it refuses the call)
            raise ValueError("retrieve_aligned_host: %s holds %d bytes, the call reads %d" % (name, len(buf), want))
    if write_steps is not None and len(write_steps) != n_rows:
        raise ValueError("retrieve_aligned_host: %d write steps, want %d" % (len(write_steps), n_rows))
    steps = (ctypes.c_ulonglong * n_rows)(*write_steps) if write_steps is not None else None
    out = ctypes.create_string_buffer(32 * n_rows * n_cols) if want_blocks else None
    status = ctypes.create_string_buffer(n_rows)
    counts = (ctypes.c_uint * 2)()
    _check(call(bytes(rows), bytes(macs), bytes(prf), bytes(align) if align is not None else None, steps, out, status, counts))
    return status.raw, [counts[0], counts[1]], out.raw if want_blocks else None


def kzg_retrieve_aligned_batch_device(reqs, n_rows, n_total, form, stream=0):
    """kzg_retrieve_batch_device for ANY half: status byte 1 iff the stored MAC row equals E_j - alpha A_j, E_j that call's expected MAC
    and A_j the half's alignment row (d_align; 0 = all at infinity, which is that call).  form: "exact" / "residue64" (64-byte rows) or
    "residue32" (32-byte rows below p_icc): the row width the check reads and the decode that fills d_out (with d_write_steps, the
    residue forms' unscale of a Y half).  `reqs`: tuples as retrieve_aligned_requests takes them."""
    arr = retrieve_aligned_requests(reqs)
    _check(lib.porla_kzg_retrieve_aligned_batch_device(arr, len(reqs), n_rows, n_total, RETRIEVE_FORM[form], ctypes.c_void_p(stream)))


def extract_requests(reqs):
    """(a ctypes array of porla_extract_req, what must stay alive beside it) from per-file tuples (write_step, data_x, mac_x, d_top_rows or
    0, d_top_macs or 0, d_top_align or 0, d_prf, d_work or 0, d_blocks, d_steps, d_flags, d_row_status, d_counts or 0): device addresses as
    integers; data_x and mac_x are sequences of the levels' device addresses (entries of non-resident levels may be 0), or None"""
    from .loader import ExtractReq
    arr = (ExtractReq * max(len(reqs), 1))()
    keep = []
    for i, r in enumerate(reqs):
        if len(r) != 13:
            raise ValueError("extract_batch_device: request %d has %d fields, want 13" % (i, len(r)))
        fams = []
        for fam in r[1:3]:
            if fam is None:
                fams.append(None)
                continue
            host = (ctypes.c_void_p * max(len(fam), 1))(*[p or None for p in fam])
            keep.append(host)
            fams.append(ctypes.cast(host, ctypes.c_void_p))
        arr[i] = ExtractReq(r[0], fams[0], fams[1], *(x or None for x in r[3:]))
    return arr, keep


def kzg_extract_batch_device(reqs, n_total, top_form, stream=0):
    """The verified file extraction of len(reqs) files in ONE asynchronous call on `stream` (porla_kzg_extract_batch_device): every
    resident level checked row by row as kzg_retrieve_aligned_batch_device checks it, the X halves decoded, the decoded blocks merged
    per slot by "newest authentic copy wins" -- d_blocks, d_steps, d_flags (PORLA_EXTRACT_*), d_row_status, d_counts.  top_form: "exact"
    or "residue32", the form of the top level's X half.  `reqs`: tuples as extract_requests takes them."""
    arr, keep = extract_requests(reqs)
    _check(lib.porla_kzg_extract_batch_device(arr, len(reqs), n_total, RETRIEVE_FORM[top_form], ctypes.c_void_p(stream)))
    del keep


def _host_pointer_array(fam, keep):
    """a HOST array of device addresses as a c_void_p (None stays None); the array itself goes into `keep`"""
    if fam is None:
        return None
    host = (ctypes.c_void_p * max(len(fam), 1))(*[p or None for p in fam])
    keep.append(host)
    return ctypes.cast(host, ctypes.c_void_p)


def extract_xy_requests(reqs):
    """(a ctypes array of porla_extract_xy_req, what must stay alive beside it) from per-file tuples: the 13 fields extract_requests
    takes, then (data_y, mac_y, align_y, d_prf_y or 0, d_work_y or 0, d_row_status_y or 0, y_levels) -- the three families sequences of
    the levels' device addresses (entries of untried levels, and any entry of align_y, may be 0), or None"""
    from .loader import ExtractXyReq
    arr = (ExtractXyReq * max(len(reqs), 1))()
    keep = []
    for i, r in enumerate(reqs):
        if len(r) != 20:
            raise ValueError("extract_xy_batch_device: request %d has %d fields, want 20" % (i, len(r)))
        x = [_host_pointer_array(fam, keep) for fam in r[1:3]]
        y = [_host_pointer_array(fam, keep) for fam in r[13:16]]
        arr[i] = ExtractXyReq(r[0], x[0], x[1], *([v or None for v in r[3:13]] + y + [v or None for v in r[16:19]] + [r[19]]))
    return arr, keep


def kzg_extract_xy_batch_device(reqs, n_total, top_form, stream=0):
    """kzg_extract_batch_device with the lower levels' Y halves as a second source (porla_kzg_extract_xy_batch_device): a level of
    y_levels whose X half has a failed row is taken from its Y half -- chunks mod p_icc, flags FOUND | RESIDUE | FROM_Y -- when that
    half checks clean; a Y block whose index is ambiguous mod p_icc is set aside and counted in d_counts[5] (six words).  `reqs`:
    tuples as extract_xy_requests takes them."""
    arr, keep = extract_xy_requests(reqs)
    _check(lib.porla_kzg_extract_xy_batch_device(arr, len(reqs), n_total, RETRIEVE_FORM[top_form], ctypes.c_void_p(stream)))
    del keep


def extract_xyt_requests(reqs):
    """(a ctypes array of porla_extract_xyt_req, what must stay alive beside it) from per-file tuples: the 20 fields extract_xy_requests
    takes, then (d_top_rows_y, d_top_macs_y, d_top_align_y, d_prf_top_y, d_top_patch, d_row_status_top_y -- device addresses or 0 --
    top_step, top_y)"""
    from .loader import ExtractXytReq
    arr = (ExtractXytReq * max(len(reqs), 1))()
    keep = []
    for i, r in enumerate(reqs):
        if len(r) != 28:
            raise ValueError("extract_xyt_batch_device: request %d has %d fields, want 28" % (i, len(r)))
        x = [_host_pointer_array(fam, keep) for fam in r[1:3]]
        y = [_host_pointer_array(fam, keep) for fam in r[13:16]]
        arr[i] = ExtractXytReq(r[0], x[0], x[1], *([v or None for v in r[3:13]] + y + [v or None for v in r[16:19]] + [r[19]] +
                                                   [v or None for v in r[20:26]] + [r[26], r[27]]))
    return arr, keep


def kzg_extract_xyt_batch_device(reqs, n_total, top_form, stream=0):
    """kzg_extract_xy_batch_device with the top level's Y half as a second source, row by row (porla_kzg_extract_xyt_batch_device): a
    top-level X row that fails its check is replaced by wt^-1 times its Y row when that row checks OK, and the top level's one decode
    runs on the patched half; a slot the top level then wins carries FROM_Y; d_counts has eight words ([6] the tried top Y rows with
    status 0, [7] the rows taken from the Y half).  `reqs`: tuples as extract_xyt_requests takes them."""
    arr, keep = extract_xyt_requests(reqs)
    _check(lib.porla_kzg_extract_xyt_batch_device(arr, len(reqs), n_total, RETRIEVE_FORM[top_form], ctypes.c_void_p(stream)))
    del keep


def repair_top_requests(reqs):
    """a ctypes array of porla_repair_top_req from per-file tuples (d_rows_x, d_macs_x, d_align_x, d_prf_x, d_rows_y, d_macs_y, d_align_y,
    d_prf_y, d_status_x, d_status_y, d_action_x, d_action_y, d_counts -- device addresses or 0 -- top_step[, reserved])"""
    from .loader import RepairTopReq
    arr = (RepairTopReq * max(len(reqs), 1))()
    for i, r in enumerate(reqs):
        if len(r) not in (14, 15):
            raise ValueError("repair_top_batch_device: request %d has %d fields, want 14 or 15" % (i, len(r)))
        arr[i] = RepairTopReq(*([v or None for v in r[:13]] + [r[13], r[14] if len(r) == 15 else 0]))
    return arr


def kzg_repair_top_batch_device(reqs, n_total, top_form, stream=0):
    """the top-level repair (porla_kzg_repair_top_batch_device): every row of both halves of a file's top level is checked, and a row
    that fails while row j of the other half passes is written back IN PLACE -- wt^-1 Y_j over an X row, wt X_j over a Y row, then its
    MAC row.  d_status_*: the statuses before the repair; d_action_*: PORLA_REPAIR_DATA | _MAC | _LOST per row; d_counts: eight words.
    Asynchronous on `stream`.  `reqs`: tuples as repair_top_requests takes them."""
    arr = repair_top_requests(reqs)
    _check(lib.porla_kzg_repair_top_batch_device(arr, len(reqs), n_total, RETRIEVE_FORM[top_form], ctypes.c_void_p(stream)))


def repair_levels_requests(reqs):
    """(a ctypes array of porla_repair_levels_req, what must stay alive beside it) from per-file tuples (write_step, levels, data_x,
    mac_x, d_prf_x, d_prf_y, data_y, mac_y, align_y, d_work, d_status_x, d_status_y, d_action_y, d_level, d_counts[, reserved]): the five
    families sequences of the levels' device addresses (entries of unnamed levels may be 0) or None, the rest device addresses or 0"""
    from .loader import RepairLevelsReq
    arr = (RepairLevelsReq * max(len(reqs), 1))()
    keep = []
    for i, r in enumerate(reqs):
        if len(r) not in (15, 16):
            raise ValueError("repair_levels_batch_device: request %d has %d fields, want 15 or 16" % (i, len(r)))
        x = [_host_pointer_array(fam, keep) for fam in r[2:4]]
        y = [_host_pointer_array(fam, keep) for fam in r[6:9]]
        arr[i] = RepairLevelsReq(r[0], r[1], x[0], x[1], r[4] or None, r[5] or None, y[0], y[1], y[2],
                                 *([v or None for v in r[9:15]] + [r[15] if len(r) == 16 else 0]))
    return arr, keep


def repair_levels_work_bytes(n_total, n_cols, write_step, levels):
    """the byte size of porla_repair_levels_req.d_work (porla_repair_levels_work_bytes; no device is touched)"""
    return int(lib.porla_repair_levels_work_bytes(n_total, n_cols, write_step, levels))


def kzg_repair_levels_batch_device(reqs, n_total, stream=0):
    """the lower-level repair (porla_kzg_repair_levels_batch_device): every row of both halves of the named lower levels of a file is
    checked, and the failed Y rows of a level whose X half is clean are rebuilt from that half -- decode, per-block y_p and c_p, the data
    network, one commitment per row -- and written back IN PLACE: data, alignment and MAC row.  d_status_*: the statuses before the
    repair; d_action_y: PORLA_REPAIR_DATA | _MAC | _ALIGN per row; d_level: PORLA_REPAIR_LEVEL_* per level; d_counts: eight words.
    Asynchronous on `stream`.  `reqs`: tuples as repair_levels_requests takes them."""
    arr, keep = repair_levels_requests(reqs)
    _check(lib.porla_kzg_repair_levels_batch_device(arr, len(reqs), n_total, ctypes.c_void_p(stream)))
    del keep


def kzg_retrieve_aligned_host(rows, macs, prf, n_rows, n_total, form, align=None, write_steps=None, want_blocks=True):
    """one level from host memory (porla_kzg_retrieve_aligned_host; it waits) -> what kzg_retrieve_host returns"""
    n_cols = kzg_row_coefficients()
    f = RETRIEVE_FORM[form]
    return _retrieve_aligned_host(lambda r, m, p, a, ws, out, st, cn: lib.porla_kzg_retrieve_aligned_host(r, m, p, a, ws, n_rows, n_total, f,
                                                                                                        out, st, cn),
                                  rows, macs, prf, align, write_steps, n_rows, n_cols, form, want_blocks)


# ---- batched fixed-base commitments (include/porla_gpu.h) ------------------------------------------
CURVES = {"bn254": 0, "secp256k1": 1}


def _alpha_be(alpha):
    """an integer or 32 bytes -> the 32 big-endian bytes the aligned retrieval takes; None stays None (the library refuses it)"""
    if alpha is None:
        return None
    return alpha.to_bytes(32, "big") if isinstance(alpha, int) else bytes(alpha)


class FixedBase:
    """Resident window-multiples table of a fixed base; commit() = compute_digest_from_srs / compute_commitment
    hoisted over many rows (Server.hpp:550-560, Client.hpp:374-406)."""

    def __init__(self, curve, points, n_points, window_bits=0):
        self.h = ctypes.c_void_p()
        _check(lib.porla_fixed_base_create(CURVES[curve], bytes(points), n_points, window_bits, ctypes.byref(self.h)))

    def info(self):
        c, w, b = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_ulonglong(0)
        _check(lib.porla_fixed_base_info(self.h, ctypes.byref(c), ctypes.byref(w), ctypes.byref(b)))
        return {"window_bits": c.value, "windows": w.value, "table_bytes": b.value}

    def commit_host(self, rows, n_rows, n_coeffs, row_stride=None):
        out = ctypes.create_string_buffer(64 * max(n_rows, 1))
        _check(lib.porla_fixed_base_commit_host(self.h, bytes(rows), n_rows, n_coeffs, row_stride or 32 * n_coeffs, out))
        return out.raw[:64 * n_rows]

    def commit_device(self, d_rows, n_rows, n_coeffs, d_out, stream=0, row_stride=None):
        _check(lib.porla_fixed_base_commit_device(self.h, ctypes.c_void_p(d_rows), n_rows, n_coeffs,
                                                  row_stride or 32 * n_coeffs, ctypes.c_void_p(d_out),
                                                  ctypes.c_void_p(stream)))

    def ipa_audit_device(self, d_rows64, d_idx64, d_coef64, n64, d_rows32, d_idx32, d_coef32, n32, n_cols, d_mac_store, d_align_store,
                         d_mac_idx, d_mac_coef, n_macs, stream=0):
        """Server::audit (IPA build) up to the proof, self = the generators' fixed base ->
        dict(combined_mac, combined_align, align_value, commitment, b)"""
        vp = ctypes.c_void_p
        o = [ctypes.create_string_buffer(k) for k in (64, 64, 64, 64, 32 * n_cols)]
        _check(lib.porla_ipa_audit_device(self.h, vp(d_rows64 or None), vp(d_idx64 or None), vp(d_coef64 or None), n64,
                                          vp(d_rows32 or None), vp(d_idx32 or None), vp(d_coef32 or None), n32, n_cols, vp(d_mac_store),
                                          vp(d_align_store), vp(d_mac_idx), vp(d_mac_coef), n_macs, *o, vp(stream)))
        return dict(zip(("combined_mac", "combined_align", "align_value", "commitment", "b"), (x.raw for x in o)))

    def ipa_audit_batch_device(self, audits, d_out, d_b=None, stream=0):
        """Server::audit (IPA) of len(audits) independent audits, proofs included, in ONE asynchronous call on `stream`
        (porla_ipa_audit_batch_device); self = the fixed base over generators[0..127] || u.  Record k (655 bytes at d_out + 655 k) =
        commitment(33) | combined_MAC(33) | combined_align(33) | proof(556); d_b (optional): B mod p_icc of every audit, 128 x 32 bytes
        each.  `audits`: tuples as ipa_audit_requests takes."""
        arr = ipa_audit_requests(audits)
        _check(lib.porla_ipa_audit_batch_device(self.h, arr, len(audits), ctypes.c_void_p(d_out), ctypes.c_void_p(d_b or None),
                                                ctypes.c_void_p(stream)))

    def ipa_update_batch_device(self, reqs, n_total, stream=0):
        """Server::update's H path of len(reqs) independent files in ONE asynchronous call on `stream`, IPA build (128 columns);
        self = a secp256k1 fixed base whose first 128 points are the generators.  `reqs`: tuples as icc.update_requests takes them."""
        from .icc import update_requests
        arr = update_requests(reqs)
        _check(lib.porla_ipa_update_batch_device(self.h, arr, len(reqs), n_total, ctypes.c_void_p(stream)))

    def ipa_server_rebuild_aligned_batch_device(self, reqs, n_total, stream=0):
        """The server's rebuild write in the CRebuild_No_Cached form of len(reqs) independent files in ONE asynchronous call on `stream`,
        IPA build (porla_ipa_server_rebuild_aligned_batch_device: 128 columns, rows mod p_icc, an alignment commitment per row); self as
        for ipa_update_batch_device.  `reqs`: tuples as icc.server_rebuild_requests takes them."""
        from .icc import server_rebuild_requests
        arr = server_rebuild_requests(reqs)
        _check(lib.porla_ipa_server_rebuild_aligned_batch_device(self.h, arr, len(reqs), n_total, ctypes.c_void_p(stream)))

    def ipa_client_update_batch_device(self, h_fb, reqs, n_total, stream=0):
        """Client::update's preprocessing of len(reqs) independent writes in ONE asynchronous call on `stream`, IPA build
        (porla_ipa_client_update_batch_device); self = a secp256k1 fixed base whose first 128 points are the alpha generators, h_fb = a
        FixedBase over the one hiding point.  `reqs`: tuples as client_update_requests takes them."""
        arr = client_update_requests(reqs)
        _check(lib.porla_ipa_client_update_batch_device(self.h, h_fb.h if h_fb is not None else None, arr, len(reqs), n_total,
                                                        ctypes.c_void_p(stream)))

    def ipa_retrieve_batch_device(self, h_fb, reqs, n_rows, n_total, stream=0):
        """kzg_retrieve_batch_device for the IPA build (porla_ipa_retrieve_batch_device: 128 columns; the expected MAC of a row is
        sum_c (sym_c mod n) alpha_generators[c] + prf h); self and h_fb as for ipa_client_update_batch_device.  `reqs`: tuples as
        retrieve_requests takes them."""
        arr = retrieve_requests(reqs)
        _check(lib.porla_ipa_retrieve_batch_device(self.h, h_fb.h if h_fb is not None else None, arr, len(reqs), n_rows, n_total,
                                                   ctypes.c_void_p(stream)))

    def ipa_retrieve_host(self, h_fb, rows, macs, prf, n_rows, n_total, want_blocks=True):
        """one level from host memory (porla_ipa_retrieve_host; it waits) -> what kzg_retrieve_host returns"""
        hh = h_fb.h if h_fb is not None else None
        return _retrieve_host(lambda r, m, p, out, st, cn: lib.porla_ipa_retrieve_host(self.h, hh, r, m, p, n_rows, n_total, out, st, cn),
                              rows, macs, prf, n_rows, 128, want_blocks)

    def ipa_retrieve_aligned_batch_device(self, h_fb, alpha, reqs, n_rows, n_total, form, stream=0):
        """kzg_retrieve_aligned_batch_device for the IPA build (porla_ipa_retrieve_aligned_batch_device); self and h_fb as for
        ipa_retrieve_batch_device.  alpha: the scalar with alpha_generators[c] = alpha * generators[c], an integer or 32 big-endian
        bytes -- the call cannot check it: a wrong alpha fails every row whose alignment is finite."""
        arr = retrieve_aligned_requests(reqs)
        _check(lib.porla_ipa_retrieve_aligned_batch_device(self.h, h_fb.h if h_fb is not None else None, _alpha_be(alpha), arr, len(reqs),
                                                           n_rows, n_total, RETRIEVE_FORM[form], ctypes.c_void_p(stream)))

    def ipa_extract_batch_device(self, h_fb, alpha, reqs, n_total, top_form, stream=0):
        """kzg_extract_batch_device for the IPA build (porla_ipa_extract_batch_device: 128 columns); self, h_fb and alpha as for
        ipa_retrieve_aligned_batch_device."""
        arr, keep = extract_requests(reqs)
        _check(lib.porla_ipa_extract_batch_device(self.h, h_fb.h if h_fb is not None else None, _alpha_be(alpha), arr, len(reqs), n_total,
                                                  RETRIEVE_FORM[top_form], ctypes.c_void_p(stream)))
        del keep

    def ipa_extract_xy_batch_device(self, h_fb, alpha, reqs, n_total, top_form, stream=0):
        """kzg_extract_xy_batch_device for the IPA build (porla_ipa_extract_xy_batch_device: 128 columns); self, h_fb and alpha as for
        ipa_extract_batch_device."""
        arr, keep = extract_xy_requests(reqs)
        _check(lib.porla_ipa_extract_xy_batch_device(self.h, h_fb.h if h_fb is not None else None, _alpha_be(alpha), arr, len(reqs), n_total,
                                                     RETRIEVE_FORM[top_form], ctypes.c_void_p(stream)))
        del keep

    def ipa_extract_xyt_batch_device(self, h_fb, alpha, reqs, n_total, top_form, stream=0):
        """kzg_extract_xyt_batch_device for the IPA build (porla_ipa_extract_xyt_batch_device: 128 columns); self, h_fb and alpha as for
        ipa_extract_batch_device."""
        arr, keep = extract_xyt_requests(reqs)
        _check(lib.porla_ipa_extract_xyt_batch_device(self.h, h_fb.h if h_fb is not None else None, _alpha_be(alpha), arr, len(reqs), n_total,
                                                      RETRIEVE_FORM[top_form], ctypes.c_void_p(stream)))
        del keep

    def ipa_repair_top_batch_device(self, h_fb, alpha, reqs, n_total, top_form, stream=0):
        """kzg_repair_top_batch_device for the IPA build (porla_ipa_repair_top_batch_device: 128 columns); self, h_fb and alpha as for
        ipa_extract_batch_device."""
        arr = repair_top_requests(reqs)
        _check(lib.porla_ipa_repair_top_batch_device(self.h, h_fb.h if h_fb is not None else None, _alpha_be(alpha), arr, len(reqs), n_total,
                                                     RETRIEVE_FORM[top_form], ctypes.c_void_p(stream)))

    def ipa_repair_levels_batch_device(self, h_fb, alpha, reqs, n_total, stream=0):
        """kzg_repair_levels_batch_device for the IPA build (porla_ipa_repair_levels_batch_device: 128 columns); self, h_fb and alpha as
        for ipa_extract_batch_device.  self holds the ALPHA generators: the call commits the alignment scalars times alpha^-1."""
        arr, keep = repair_levels_requests(reqs)
        _check(lib.porla_ipa_repair_levels_batch_device(self.h, h_fb.h if h_fb is not None else None, _alpha_be(alpha), arr, len(reqs), n_total,
                                                        ctypes.c_void_p(stream)))
        del keep

    def ipa_retrieve_aligned_host(self, h_fb, alpha, rows, macs, prf, n_rows, n_total, form, align=None, write_steps=None,
                                  want_blocks=True):
        """one level from host memory (porla_ipa_retrieve_aligned_host; it waits) -> what kzg_retrieve_host returns"""
        hh = h_fb.h if h_fb is not None else None
        f, ab = RETRIEVE_FORM[form], _alpha_be(alpha)
        return _retrieve_aligned_host(lambda r, m, p, a, ws, out, st, cn: lib.porla_ipa_retrieve_aligned_host(self.h, hh, ab, r, m, p, a, ws,
                                                                                                            n_rows, n_total, f, out, st, cn),
                                      rows, macs, prf, align, write_steps, n_rows, 128, form, want_blocks)

    def ipa_client_rebuild_batch_device(self, h_fb, reqs, n_total, stream=0):
        """The client's rebuild write (Client::CRebuild's step) of len(reqs) independent writes in ONE asynchronous call on `stream`, IPA
        build (porla_ipa_client_rebuild_batch_device); self and h_fb as for ipa_client_update_batch_device.  `reqs`: tuples as
        client_rebuild_requests takes them."""
        arr = client_rebuild_requests(reqs)
        _check(lib.porla_ipa_client_rebuild_batch_device(self.h, h_fb.h if h_fb is not None else None, arr, len(reqs), n_total,
                                                         ctypes.c_void_p(stream)))

    def ipa_prove_batch_device(self, d_a, d_b, k, d_proofs, stream=0):
        """k proofs of Server::inner_product_prove(a, b) in ONE asynchronous call (porla_ipa_prove_batch_device): d_a, d_b = k x 128 x
        32 bytes big-endian, d_proofs = k x 556 bytes"""
        _check(lib.porla_ipa_prove_batch_device(self.h, ctypes.c_void_p(d_a), ctypes.c_void_p(d_b), k, ctypes.c_void_p(d_proofs),
                                                ctypes.c_void_p(stream)))

    def ipa_verify_batch_device(self, verifs, d_records, d_status=None, stream=0):
        """Client::audit's check (IPA) of len(verifs) replies in ONE asynchronous call on `stream` (porla_ipa_verify_batch_device);
        self = the fixed base over generators[0..127] || u.  Reply k is the 655-byte record at d_records + 655 k (as
        ipa_audit_batch_device writes it), verifs[k] the client's side as ipa_verify_requests takes it.  The status bytes go to
        d_status (a device address, len(verifs) bytes, complete when `stream` is).  d_status=None: a status buffer is allocated, the
        stream synchronised and the bytes returned as a list of ints; reply k passes the reference's checks iff status[k] &
        IPA_VERIFY_PASS == IPA_VERIFY_PASS, and is bound to its challenge as well iff status[k] == IPA_VERIFY_PASS_BOUND."""
        k = len(verifs)
        arr = ipa_verify_requests(verifs)
        if d_status is not None:
            _check(lib.porla_ipa_verify_batch_device(self.h, arr, k, ctypes.c_void_p(d_records or None), ctypes.c_void_p(d_status),
                                                     ctypes.c_void_p(stream)))
            return None
        if k == 0:
            _check(lib.porla_ipa_verify_batch_device(self.h, arr, 0, ctypes.c_void_p(d_records or None), None, ctypes.c_void_p(stream)))
            return []
        import torch
        s = torch.cuda.ExternalStream(stream) if stream else torch.cuda.default_stream()
        with torch.cuda.stream(s):
            st = torch.zeros(k, dtype=torch.uint8, device="cuda")
        _check(lib.porla_ipa_verify_batch_device(self.h, arr, k, ctypes.c_void_p(d_records or None), ctypes.c_void_p(st.data_ptr()),
                                                 ctypes.c_void_p(stream)))
        s.synchronize()
        return list(bytes(st.cpu().numpy()))

    def close(self):
        if self.h:
            lib.porla_fixed_base_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def kzg_commit_batch_host(rows, n_rows):
    out = ctypes.create_string_buffer(64 * max(n_rows, 1))
    _check(lib.porla_kzg_commit_batch_host(bytes(rows), n_rows, out))
    return out.raw[:64 * n_rows]


def kzg_commit_batch_host_multi(rows, n_rows, devices=0):
    """row range split over `devices` GPUs of this process (0 = every visible one)"""
    out = ctypes.create_string_buffer(64 * max(n_rows, 1))
    _check(lib.porla_kzg_commit_batch_host_multi(bytes(rows), n_rows, out, devices))
    return out.raw[:64 * n_rows]


def shard_range(n, rank, world):
    """[begin, end) of shard `rank` of `world` over n units -- the engine's own range rule (porla_shard_range)"""
    b, e = ctypes.c_size_t(0), ctypes.c_size_t(0)
    _check(lib.porla_shard_range(n, rank, world, ctypes.byref(b), ctypes.byref(e)))
    return b.value, e.value


def kzg_commit_batch_device(d_rows, n_rows, d_out, stream=0):
    _check(lib.porla_kzg_commit_batch_device(ctypes.c_void_p(d_rows), n_rows, ctypes.c_void_p(d_out), ctypes.c_void_p(stream)))


def kzg_commit_batch_device_to_host(d_rows, n_rows, stream=0):
    """commitments of rows resident on the device, results on the host (blocking; <= 64 rows: one launch)"""
    out = ctypes.create_string_buffer(64 * n_rows)
    _check(lib.porla_kzg_commit_batch_device_to_host(ctypes.c_void_p(d_rows), n_rows, out, ctypes.c_void_p(stream)))
    return out.raw


def kzg_audit_device(d_rows64, d_idx64, d_coef64, n64, d_rows32, d_idx32, d_coef32, n32, d_mac_store, d_align_store, d_mac_idx,
                     d_mac_coef, n_macs, z, n_cols=None, stream=0):
    """Server::audit (KZG) in one call -> dict(combined_mac, combined_align, align_value, commitment, proof_h, point, claim, b).
    The library writes 32 bytes per SRS coefficient into `b`: n_cols, if given, must be the SRS size"""
    vp = ctypes.c_void_p
    srs_n = kzg_row_coefficients()
    if n_cols is None:
        n_cols = srs_n
    elif n_cols != srs_n:
        raise ValueError("kzg_audit_device: n_cols=%d but the SRS holds %d coefficients" % (n_cols, srs_n))
    o = [ctypes.create_string_buffer(k) for k in (64, 64, 64, 64, 64, 32, 32, 32 * n_cols)]
    _check(lib.porla_kzg_audit_device(vp(d_rows64 or None), vp(d_idx64 or None), vp(d_coef64 or None), n64, vp(d_rows32 or None),
                                      vp(d_idx32 or None), vp(d_coef32 or None), n32, vp(d_mac_store), vp(d_align_store), vp(d_mac_idx),
                                      vp(d_mac_coef), n_macs, z, *o, vp(stream)))
    return dict(zip(("combined_mac", "combined_align", "align_value", "commitment", "proof_h", "point", "claim", "b"), (x.raw for x in o)))


_REQ_POINTERS = (0, 1, 2, 4, 5, 6, 8, 9, 10, 11)   # fields of porla_kzg_audit_req that are device pointers (0 -> NULL)
KZG_AUDIT_RECORD_BYTES = 320   # commitment | proof_h | point | claim | combined_mac | combined_align (include/porla_gpu.h)


def kzg_audit_requests(audits):
    """a ctypes array of porla_kzg_audit_req from per-audit tuples in kzg_audit_device's argument order (without n_cols and stream):
    (d_rows64, d_idx64, d_coef64, n64, d_rows32, d_idx32, d_coef32, n32, d_mac_store, d_align_store, d_mac_idx, d_mac_coef, n_macs, z)"""
    arr = (KzgAuditReq * max(len(audits), 1))()
    for i, a in enumerate(audits):
        if len(a) != 14:
            raise ValueError("kzg_audit_batch_device: audit %d has %d fields, want 14" % (i, len(a)))
        arr[i] = KzgAuditReq(*[(x or None) if j in _REQ_POINTERS else x for j, x in enumerate(a)])
    return arr


def kzg_audit_batch_device(audits, d_out, d_b=None, stream=0):
    """Server::audit (KZG) of len(audits) independent audits in ONE asynchronous call on `stream` (porla_kzg_audit_batch_device):
    record k (320 bytes at d_out + 320 k) = commitment | proof_h | point | claim | combined_mac | combined_align, the reply of
    Server::audit; d_b (optional): B mod p_icc of every audit, n x 32 bytes each.  `audits`: tuples as kzg_audit_requests takes."""
    arr = kzg_audit_requests(audits)
    _check(lib.porla_kzg_audit_batch_device(arr, len(audits), ctypes.c_void_p(d_out), ctypes.c_void_p(d_b or None),
                                            ctypes.c_void_p(stream)))


def split_audit_records(raw, k):
    """k records -> list of dicts with the fields of kzg_audit_device's reply (combined_align after align_MAC)"""
    out = []
    for i in range(k):
        r = raw[KZG_AUDIT_RECORD_BYTES * i:KZG_AUDIT_RECORD_BYTES * (i + 1)]
        out.append(dict(commitment=r[0:64], proof_h=r[64:128], point=r[128:160], claim=r[160:192], combined_mac=r[192:256],
                        combined_align=r[256:320]))
    return out


IPA_AUDIT_RECORD_BYTES = 655   # commitment(33) | combined_mac(33) | combined_align(33) | proof(556) (include/porla_gpu.h)
IPA_PROOF_BYTES = 556          # c(32) | 6 x (L(33) | R(33)) | a0 b0 a1 b1 (4 x 32)


def ipa_audit_requests(audits):
    """a ctypes array of porla_ipa_audit_req from per-audit tuples: the first 13 fields as kzg_audit_requests takes them, then a_value
    (audit_values[n_points]) as an integer or as big-endian bytes of at most 32 (left-padded)"""
    arr = (IpaAuditReq * max(len(audits), 1))()
    for i, a in enumerate(audits):
        if len(a) != 14:
            raise ValueError("ipa_audit_batch_device: audit %d has %d fields, want 14" % (i, len(a)))
        v = a[13].to_bytes(32, "big") if isinstance(a[13], int) else bytes(a[13]).rjust(32, b"\0")
        if len(v) != 32:
            raise ValueError("ipa_audit_batch_device: audit %d: a_value longer than 32 bytes" % i)
        arr[i] = IpaAuditReq(*[(x or None) if j in _REQ_POINTERS else x for j, x in enumerate(a[:13])], (ctypes.c_uint8 * 32)(*v))
    return arr


def split_ipa_records(raw, k):
    """k records of porla_ipa_audit_batch_device -> list of dicts: the three compressed points and the proof, and the proof's parts
    (c, a0, b0, a1, b1 as integers; rounds: six (L, R) pairs of 33 bytes)"""
    out = []
    le = lambda b: int.from_bytes(b, "little")
    for i in range(k):
        r = raw[IPA_AUDIT_RECORD_BYTES * i:IPA_AUDIT_RECORD_BYTES * (i + 1)]
        p = r[99:]
        tail = p[32 + 6 * 66:]
        out.append(dict(commitment=r[0:33], combined_mac=r[33:66], combined_align=r[66:99], proof=p, c=le(p[:32]),
                        rounds=[(p[32 + 66 * j:65 + 66 * j], p[65 + 66 * j:98 + 66 * j]) for j in range(6)],
                        a0=le(tail[0:32]), b0=le(tail[32:64]), a1=le(tail[64:96]), b1=le(tail[96:128])))
    return out


IPA_VERIFY_FULL = 1         # alpha C + sum coef comp == M + alpha A (Client.hpp:801-829)
IPA_VERIFY_PROOF = 2        # Client::inner_product_verify's equation holds
IPA_VERIFY_MALFORMED = 4    # a compressed point of the record does not parse
IPA_VERIFY_BVEC = 8         # the proof's b0, b1 are the fold of b = (v, v^2, v^4, ...), v = a_value
IPA_VERIFY_PASS = IPA_VERIFY_FULL | IPA_VERIFY_PROOF                 # the reference's verdict
IPA_VERIFY_PASS_BOUND = IPA_VERIFY_PASS | IPA_VERIFY_BVEC            # ... with the proof bound to the challenge


def _be32(v, what, i):
    b = v.to_bytes(32, "big") if isinstance(v, int) else bytes(v)
    if len(b) > 32:
        raise ValueError("ipa_verify_batch_device: %s of reply %d is longer than 32 bytes" % (what, i))
    return (ctypes.c_uint8 * 32)(*b.rjust(32, b"\0"))


def ipa_verify_requests(verifs):
    """a ctypes array of porla_ipa_verify_req from per-reply tuples (d_comp_store, d_idx, d_coef, n, alpha, a_value): device pointers
    (0 -> NULL), the challenge length, and the client's alpha and the audit's a_value as integers or big-endian bytes of at most 32
    (left-padded)"""
    arr = (IpaVerifyReq * max(len(verifs), 1))()
    for i, v in enumerate(verifs):
        if len(v) != 6:
            raise ValueError("ipa_verify_batch_device: reply %d has %d fields, want 6" % (i, len(v)))
        comp, idx, coef, n, alpha, a_value = v
        arr[i] = IpaVerifyReq(comp or None, idx or None, coef or None, n, _be32(alpha, "alpha", i), _be32(a_value, "a_value", i))
    return arr


KZG_VERIFY_FULL = 1        # alpha C + sum coef comp == M + alpha A (Client.hpp:849-869)
KZG_VERIFY_PROOF = 2       # the opening verifies (verify_proof)
KZG_VERIFY_MALFORMED = 4   # a point of the record has a coordinate >= p or is off the curve
KZG_VERIFY_PASS = KZG_VERIFY_FULL | KZG_VERIFY_PROOF
KZG_VERIFY_MAX_K = 10922   # replies per call (include/porla_gpu.h)


def kzg_verify_requests(verifs):
    """a ctypes array of porla_kzg_verify_req from per-reply tuples (d_comp_store, d_idx, d_coef, n, alpha): device pointers (0 ->
    NULL), the challenge length and the client's alpha as big-endian bytes of at most 32 (left-padded: a 16-byte SECRET_KEY lands in
    bytes 16..31, as Client::audit places it)"""
    arr = (KzgVerifyReq * max(len(verifs), 1))()
    for i, v in enumerate(verifs):
        if len(v) != 5:
            raise ValueError("kzg_verify_batch_device: reply %d has %d fields, want 5" % (i, len(v)))
        comp, idx, coef, n, alpha = v
        alpha = bytes(alpha)
        if len(alpha) > 32:
            raise ValueError("kzg_verify_batch_device: alpha of reply %d is longer than 32 bytes" % i)
        arr[i] = KzgVerifyReq(comp or None, idx or None, coef or None, n, (ctypes.c_uint8 * 32)(*alpha.rjust(32, b"\0")))
    return arr


def kzg_verify_batch_device(verifs, d_records, weights=None, stream=0):
    """Client::audit's check of len(verifs) replies in ONE blocking call (porla_kzg_verify_batch_device): reply k is the 320-byte record
    at d_records + 320 k (as kzg_audit_batch_device writes it), verifs[k] the client's side as kzg_verify_requests takes it.  Returns
    the status bytes; reply k passes iff status[k] == KZG_VERIFY_PASS.  weights: None (drawn per call, the normal use) or k secret
    random nonzero weights, as 16-byte big-endian bytes or ints < 2^128."""
    k = len(verifs)
    arr = kzg_verify_requests(verifs)
    w = None
    if weights is not None:
        if len(weights) != k:
            raise ValueError("kzg_verify_batch_device: %d weights for %d replies" % (len(weights), k))
        w = b"".join(x.to_bytes(16, "big") if isinstance(x, int) else bytes(x) for x in weights)
        if len(w) != 16 * k:
            raise ValueError("kzg_verify_batch_device: every weight is 16 bytes")
    status = ctypes.create_string_buffer(max(k, 1))
    _check(lib.porla_kzg_verify_batch_device(arr, k, ctypes.c_void_p(d_records or None), w, status, ctypes.c_void_p(stream)))
    return list(status.raw[:k])


def kzg_digest_batch_device(d_rows, n_rows, d_out, stream=0):
    """compute_digest (Client.hpp:408-419) over n_rows rows resident in HBM"""
    _check(lib.porla_kzg_digest_batch_device(ctypes.c_void_p(d_rows), n_rows, ctypes.c_void_p(d_out), ctypes.c_void_p(stream)))


def kzg_complement_batch_device(d_scalars, n, d_out, stream=0):
    """compute_digest_complement (Client.hpp:445-453) over n 32-byte big-endian scalars resident in HBM"""
    _check(lib.porla_kzg_complement_batch_device(ctypes.c_void_p(d_scalars), n, ctypes.c_void_p(d_out), ctypes.c_void_p(stream)))


def kzg_mac_batch_device(d_rows, d_scalars, n_rows, d_out, stream=0):
    """digest(row) + complement(scalar) per block, the MAC Client::initialize / update send (Client.hpp:229-236, 468-478)"""
    _check(lib.porla_kzg_mac_batch_device(ctypes.c_void_p(d_rows), ctypes.c_void_p(d_scalars), n_rows, ctypes.c_void_p(d_out),
                                          ctypes.c_void_p(stream)))


def kzg_digest_batch_host(rows, n_rows):
    """compute_digest over n_rows rows in host memory -> n_rows * 64 bytes"""
    out = ctypes.create_string_buffer(64 * n_rows)
    _check(lib.porla_kzg_digest_batch_host(rows, n_rows, out))
    return out.raw


def kzg_complement_batch_host(scalars, n):
    """compute_digest_complement over n 32-byte big-endian scalars in host memory -> n * 64 bytes"""
    out = ctypes.create_string_buffer(64 * n)
    _check(lib.porla_kzg_complement_batch_host(scalars, n, out))
    return out.raw


def kzg_mac_batch_host(rows, scalars, n_rows):
    """digest(row) + complement(scalar) per block, host buffers -> n_rows * 64 bytes"""
    out = ctypes.create_string_buffer(64 * n_rows)
    _check(lib.porla_kzg_mac_batch_host(rows, scalars, n_rows, out))
    return out.raw


def profile_enable(on=True):
    """False/0: off; True/1: HIP events around every kernel; 2: around the workload's dominant kernel only"""
    lib.porla_gpu_profile_enable(int(on))


def kzg_row_coefficients():
    """coefficients per commitment row = the SRS size of this process (0 before init_SRS / init_SRS_from_data)"""
    n = ctypes.c_size_t(0)
    _check(lib.porla_kzg_row_coefficients(ctypes.byref(n)))
    return n.value


def kzg_commit_shape():
    """(window bits, windows per coefficient) of the resident SRS table"""
    c, w = ctypes.c_int(0), ctypes.c_int(0)
    lib.porla_kzg_commit_shape(ctypes.byref(c), ctypes.byref(w))
    return c.value, w.value


def last_msm_shape():
    """(window bits, window count, GLV flag) of the most recently launched MSM"""
    c, w, g = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    lib.porla_gpu_last_msm_shape(ctypes.byref(c), ctypes.byref(w), ctypes.byref(g))
    return c.value, w.value, bool(g.value)


SMALL_FORMS = {"lone": 0, "pair": 1, "hint": 2, "any": 3}


def msm_small_shape(curve, n, used_bits, c_flags, form):
    """porla_msm_small_shape on arrays of equal length (no device needed): curve 0 = BN254 / 1 = secp256k1, n, used_bits, c_flags (forced
    window bits | 0x100 = never split), form (SMALL_FORMS).  Returns an int32 array of shape (count, 6): the shape fits and is launched (1) or not (0;
    a pair then runs as two lone single launches), blocks, split flag, c, W, S."""
    import numpy as np
    arrs = [np.ascontiguousarray(a, dtype=t) for a, t in
            zip((curve, n, used_bits, c_flags, form), (np.int32, np.uint32, np.int32, np.int32, np.int32))]
    count = len(arrs[0])
    if any(len(a) != count for a in arrs):
        raise ValueError("msm_small_shape: arrays of unequal length")
    out = np.zeros((count, 6), dtype=np.int32)
    ptr = lambda a, t: a.ctypes.data_as(ctypes.POINTER(t))
    rc = lib.porla_msm_small_shape(count, ptr(arrs[0], ctypes.c_int32), ptr(arrs[1], ctypes.c_uint32), ptr(arrs[2], ctypes.c_int32),
                                   ptr(arrs[3], ctypes.c_int32), ptr(arrs[4], ctypes.c_int32), ptr(out, ctypes.c_int32))
    if rc != 0:
        raise RuntimeError("porla_msm_small_shape failed (%d): %s" % (rc, lib.porla_gpu_last_error().decode()))
    return out


def profile_get():
    """[(kernel name, total ms, launches)]"""
    res = []
    i = 0
    while True:
        name = ctypes.create_string_buffer(64)
        ms = ctypes.c_double(0)
        cnt = ctypes.c_longlong(0)
        if lib.porla_gpu_profile_get(i, name, 64, ctypes.byref(ms), ctypes.byref(cnt)) != 0:
            break
        res.append((name.value.decode(), ms.value, cnt.value))
        i += 1
    return res
