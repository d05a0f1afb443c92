"""AES on the device (include/porla_gpu.h: porla_mac_prf_*, porla_client_prf_runs, porla_audit_challenge_*,
porla_audit_complement_scalar_*): the d_prf of the client write batches from their run lists, an audit's index / coefficient lists from
its 16-byte seed, and the client's complement scalar.  The calls here PRODUCE what the batches of multiexp.py / icc.py consume."""
import ctypes

from .loader import AuditChallengeInfo, AuditChallengeReq, AuditLevel, AuditScalarReq, PrfRun, lib

CURVE = {"bn254": 0, "secp256k1": 1}
PRF_KIND = {"update": 0, "rebuild": 1}
SECRET_KEY = bytes.fromhex("00112233445566778899aabbccddeeff")   # config.hpp:38
LIST_NAMES = ("idx64", "coef64", "idx32", "coef32", "mac_idx", "mac_coef")


def _check(rc):
    if rc != 0:
        raise RuntimeError("porla engine error %d: %s" % (rc, lib.porla_gpu_last_error().decode()))


def prf_runs(runs):
    """a ctypes array of porla_prf_run from tuples (level, index0, count, time0, time_stride)"""
    arr = (PrfRun * max(len(runs), 1))()
    for i, r in enumerate(runs):
        if len(r) != 5:
            raise ValueError("prf_runs: run %d has %d fields, want 5" % (i, len(r)))
        arr[i] = PrfRun(*r)
    return arr


def client_prf_runs(kind, block_id, write_step, n_total, level=0):
    """the run list of one client write ("update": level + 2 runs, "rebuild": 3) as tuples, and the number of values: the d_prf length
    porla_*_client_update_batch_device / porla_*_client_rebuild_batch_device document"""
    arr = (PrfRun * 32)()
    n_runs, n_values = ctypes.c_size_t(0), ctypes.c_size_t(0)
    _check(lib.porla_client_prf_runs(PRF_KIND[kind], block_id, write_step, level, n_total, arr, 32, ctypes.byref(n_runs),
                                     ctypes.byref(n_values)))
    return [(r.level, r.index0, r.count, r.time0, r.time_stride) for r in arr[:n_runs.value]], n_values.value


def mac_prf_host(key16, runs):
    """the 16-byte PRF outputs of all runs back to back, on the host"""
    n = sum(r[2] for r in runs)
    out = ctypes.create_string_buffer(max(16 * n, 1))
    _check(lib.porla_mac_prf_host(bytes(key16), prf_runs(runs), len(runs), ctypes.cast(out, ctypes.c_void_p)))
    return out.raw[:16 * n]


def mac_prf_batch_device(key16, runs, d_out, stream=0):
    """the same into device memory at d_out (16-byte aligned), asynchronously on `stream`"""
    _check(lib.porla_mac_prf_batch_device(bytes(key16), prf_runs(runs), len(runs), ctypes.c_void_p(d_out or None), ctypes.c_void_p(stream)))


def audit_levels(levels):
    """a ctypes array of porla_audit_level from tuples (data_x, data_y, mac_x, mac_y, form)"""
    arr = (AuditLevel * max(len(levels), 1))()
    for i, l in enumerate(levels):
        arr[i] = AuditLevel(l[0], l[1], l[2], l[3], l[4], l[5] if len(l) > 5 else 0)
    return arr


def challenge_requests(reqs):
    """a ctypes array of porla_audit_challenge_req from tuples (seed, write_step, num_blocks, levels, lists): levels as audit_levels
    takes them (log2 num_blocks + 1 of them), lists None (plan only) or six addresses in the order of LIST_NAMES (0 = NULL).  The
    array keeps the level arrays alive (arr._keep)."""
    arr = (AuditChallengeReq * max(len(reqs), 1))()
    keep = []
    for i, r in enumerate(reqs):
        seed, write_step, num_blocks, levels, lists = r
        lv = audit_levels(levels)
        keep.append(lv)
        lists = lists or (0,) * 6
        arr[i] = AuditChallengeReq((ctypes.c_uint8 * 16)(*bytes(seed)), write_step, num_blocks, lv, *[(x or None) for x in lists])
    arr._keep = keep
    return arr


def _infos(arr, k):
    return [dict(n64=i.n64, n32=i.n32, n_macs=i.n_macs, random_point=i.random_point, a_raw=i.a_raw, a_value=bytes(i.a_value))
            for i in arr[:k]]


def audit_challenge_plan(reqs):
    """the infos of the challenges alone (list lengths, KZG's random_point, IPA's a): no list is written, no device touched"""
    arr = challenge_requests([(r[0], r[1], r[2], r[3], None) for r in reqs])
    infos = (AuditChallengeInfo * max(len(reqs), 1))()
    _check(lib.porla_audit_challenge_host(arr, len(reqs), infos))
    return _infos(infos, len(reqs))


def audit_challenge_host(seed, write_step, num_blocks, levels):
    """one challenge on the host: (info, lists), lists a dict of LIST_NAMES -> list of ints"""
    info = audit_challenge_plan([(seed, write_step, num_blocks, levels)])[0]
    n = {"idx64": info["n64"], "coef64": info["n64"], "idx32": info["n32"], "coef32": info["n32"], "mac_idx": info["n_macs"],
         "mac_coef": info["n_macs"]}
    bufs = {name: ((ctypes.c_uint64 if "idx" in name else ctypes.c_uint32) * max(n[name], 1))() for name in LIST_NAMES}
    arr = challenge_requests([(seed, write_step, num_blocks, levels, [ctypes.addressof(bufs[name]) for name in LIST_NAMES])])
    infos = (AuditChallengeInfo * 1)()
    _check(lib.porla_audit_challenge_host(arr, 1, infos))
    return _infos(infos, 1)[0], {name: list(bufs[name][:n[name]]) for name in LIST_NAMES}


def audit_challenge_batch_device(reqs, stream=0):
    """the challenges of len(reqs) audits drawn on the device in ONE asynchronous call on `stream`; returns the infos (complete on
    return: a caller fills the audit batch's requests from them and enqueues it right behind, on the same stream)"""
    arr = challenge_requests(reqs)
    infos = (AuditChallengeInfo * max(len(reqs), 1))()
    _check(lib.porla_audit_challenge_batch_device(arr, len(reqs), infos, ctypes.c_void_p(stream)))
    return _infos(infos, len(reqs))


def scalar_requests(reqs):
    """a ctypes array of porla_audit_scalar_req from tuples (seed, write_step, num_blocks)"""
    arr = (AuditScalarReq * max(len(reqs), 1))()
    for i, (seed, write_step, num_blocks) in enumerate(reqs):
        arr[i] = AuditScalarReq((ctypes.c_uint8 * 16)(*bytes(seed)), write_step, num_blocks)
    return arr


def audit_complement_scalar_host(key16, reqs, curve):
    """sum_p coef_p * prf_p of every challenge as integers, on the host"""
    out = ctypes.create_string_buffer(max(32 * len(reqs), 1))
    _check(lib.porla_audit_complement_scalar_host(bytes(key16), scalar_requests(reqs), len(reqs), CURVE[curve], ctypes.cast(out, ctypes.c_void_p)))
    return [int.from_bytes(out.raw[32 * i:32 * i + 32], "big") for i in range(len(reqs))]


def audit_complement_scalar_batch_device(key16, reqs, curve, d_scalars, stream=0):
    """the same as 32-byte big-endian scalars at d_scalars (device memory), asynchronously on `stream`: what
    kzg_complement_batch_device, or a commit against the one-point base h_fb, turns into the ONE point of a reply's MAC check"""
    _check(lib.porla_audit_complement_scalar_batch_device(bytes(key16), scalar_requests(reqs), len(reqs), CURVE[curve],
                                                          ctypes.c_void_p(d_scalars or None), ctypes.c_void_p(stream)))


def diag_audit_walk(stream_ints, write_step, num_blocks, levels, on_device=False):
    """the walk over an int stream the caller wrote (porla_diag_audit_walk): (info, lists) as audit_challenge_host returns them"""
    n_ints = len(stream_ints)
    ints = (ctypes.c_int32 * max(n_ints, 1))(*stream_ints)
    cap = 256 * 25
    bufs = {name: ((ctypes.c_uint64 if "idx" in name else ctypes.c_uint32) * cap)() for name in LIST_NAMES}
    info = AuditChallengeInfo()
    _check(lib.porla_diag_audit_walk(ctypes.cast(ints, ctypes.c_void_p), n_ints, write_step, num_blocks, audit_levels(levels),
                                     1 if on_device else 0, *[ctypes.cast(bufs[name], ctypes.c_void_p) for name in LIST_NAMES],
                                     ctypes.byref(info)))
    info = _infos([info], 1)[0]
    n = {"idx64": info["n64"], "coef64": info["n64"], "idx32": info["n32"], "coef32": info["n32"], "mac_idx": info["n_macs"],
         "mac_coef": info["n_macs"]}
    return info, {name: list(bufs[name][:n[name]]) for name in LIST_NAMES}


def verify_reqs_from_scalars(d_points, k, alphas, a_values=None):
    """The seeded client check through the unchanged verifiers: reply j's whole complement side is the ONE point P_j = s_j * h at
    d_points + 64 j (kzg_complement_batch_device of the complement scalars, or h_fb's commit of them for IPA).  Returns (verifs, keep):
    verifs as kzg_verify_requests (a_values None) or ipa_verify_requests takes them, with d_comp_store = d_points, idx = [j],
    coef = [1], n = 1; keep holds the two small device arrays the requests point into: they are made on torch's current stream (run
    the verifier on that stream, or behind it) and must outlive the verifier's call."""
    import torch
    idx = torch.arange(k, dtype=torch.int64, device="cuda")
    coef = torch.ones(k, dtype=torch.int32, device="cuda")
    verifs = []
    for j in range(k):
        v = (d_points, idx.data_ptr() + 8 * j, coef.data_ptr() + 4 * j, 1, alphas[j])
        verifs.append(v if a_values is None else v + (a_values[j],))
    return verifs, (idx, coef)
