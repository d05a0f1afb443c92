"""ctypes loader for libmultiexp.so (fails loudly when the HIP extension is not built)."""
import ctypes
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
lib_path = os.path.join(_HERE, "libmultiexp.so")
_lib = None


class GoSlice(ctypes.Structure):
    """cgo slice header, porla/Utils/libmultiexp.h:61."""
    _fields_ = [("data", ctypes.c_void_p), ("len", ctypes.c_longlong), ("cap", ctypes.c_longlong)]


class KzgAuditReq(ctypes.Structure):
    """porla_kzg_audit_req, include/porla_gpu.h: one audit of porla_kzg_audit_batch_device (PORLA_KZG_AUDIT_REQ_BYTES = 112)."""
    _fields_ = [("d_rows64", ctypes.c_void_p), ("d_idx64", ctypes.c_void_p), ("d_coef64", ctypes.c_void_p), ("n64", ctypes.c_size_t),
                ("d_rows32", ctypes.c_void_p), ("d_idx32", ctypes.c_void_p), ("d_coef32", ctypes.c_void_p), ("n32", ctypes.c_size_t),
                ("d_mac_store", ctypes.c_void_p), ("d_align_store", ctypes.c_void_p), ("d_mac_idx", ctypes.c_void_p),
                ("d_mac_coef", ctypes.c_void_p), ("n_macs", ctypes.c_size_t), ("random_point", ctypes.c_ulonglong)]


class IpaAuditReq(ctypes.Structure):
    """porla_ipa_audit_req, include/porla_gpu.h: one audit of porla_ipa_audit_batch_device (PORLA_IPA_AUDIT_REQ_BYTES = 136)."""
    _fields_ = KzgAuditReq._fields_[:13] + [("a_value", ctypes.c_uint8 * 32)]


class KzgVerifyReq(ctypes.Structure):
    """porla_kzg_verify_req, include/porla_gpu.h: one reply of porla_kzg_verify_batch_device (PORLA_KZG_VERIFY_REQ_BYTES = 64)."""
    _fields_ = [("d_comp_store", ctypes.c_void_p), ("d_idx", ctypes.c_void_p), ("d_coef", ctypes.c_void_p), ("n", ctypes.c_size_t),
                ("alpha", ctypes.c_uint8 * 32)]


class IpaVerifyReq(ctypes.Structure):
    """porla_ipa_verify_req, include/porla_gpu.h: one reply of porla_ipa_verify_batch_device (PORLA_IPA_VERIFY_REQ_BYTES = 96)."""
    _fields_ = KzgVerifyReq._fields_ + [("a_value", ctypes.c_uint8 * 32)]


class UpdateReq(ctypes.Structure):
    """porla_update_req, include/porla_gpu.h: one write of porla_kzg_update_batch_device / porla_ipa_update_batch_device
    (PORLA_UPDATE_REQ_BYTES = 88); the six family fields are HOST arrays of level + 1 device pointers."""
    _fields_ = [("d_block", ctypes.c_void_p), ("d_mac", ctypes.c_void_p), ("d_complements", ctypes.c_void_p),
                ("write_step", ctypes.c_ulonglong), ("level", ctypes.c_int), ("pad", ctypes.c_int),
                ("data_x", ctypes.POINTER(ctypes.c_void_p)), ("data_y", ctypes.POINTER(ctypes.c_void_p)),
                ("mac_x", ctypes.POINTER(ctypes.c_void_p)), ("mac_y", ctypes.POINTER(ctypes.c_void_p)),
                ("align_x", ctypes.POINTER(ctypes.c_void_p)), ("align_y", ctypes.POINTER(ctypes.c_void_p))]


PORLA_UPDATE_REQ_BYTES = 88
assert ctypes.sizeof(UpdateReq) == PORLA_UPDATE_REQ_BYTES


class ClientUpdateReq(ctypes.Structure):
    """porla_client_update_req, include/porla_gpu.h: one write of porla_kzg_client_update_batch_device /
    porla_ipa_client_update_batch_device (PORLA_CLIENT_UPDATE_REQ_BYTES = 48)."""
    _fields_ = [("d_block", ctypes.c_void_p), ("d_prf", ctypes.c_void_p), ("d_mac_out", ctypes.c_void_p),
                ("d_complements_out", ctypes.c_void_p), ("write_step", ctypes.c_ulonglong), ("level", ctypes.c_int), ("pad", ctypes.c_int)]


PORLA_CLIENT_UPDATE_REQ_BYTES = 48
assert ctypes.sizeof(ClientUpdateReq) == PORLA_CLIENT_UPDATE_REQ_BYTES



class ClientRebuildReq(ctypes.Structure):
    """porla_client_rebuild_req, include/porla_gpu.h: one write of porla_kzg_client_rebuild_batch_device /
    porla_ipa_client_rebuild_batch_device (PORLA_CLIENT_REBUILD_REQ_BYTES = 40)."""
    _fields_ = [("d_block", ctypes.c_void_p), ("d_prf", ctypes.c_void_p), ("d_mac_out", ctypes.c_void_p),
                ("d_complements_out", ctypes.c_void_p), ("write_step", ctypes.c_ulonglong)]


PORLA_CLIENT_REBUILD_REQ_BYTES = 40
assert ctypes.sizeof(ClientRebuildReq) == PORLA_CLIENT_REBUILD_REQ_BYTES


class ServerRebuildReq(ctypes.Structure):
    """porla_server_rebuild_req, include/porla_gpu.h: one write of porla_server_rebuild_batch_device
    (PORLA_SERVER_REBUILD_REQ_BYTES = 104)."""
    _fields_ = [("d_block", ctypes.c_void_p), ("d_mac", ctypes.c_void_p), ("d_complements", ctypes.c_void_p),
                ("d_u_blocks", ctypes.c_void_p), ("d_u_macs", ctypes.c_void_p),
                ("d_data_x", ctypes.c_void_p), ("d_data_y", ctypes.c_void_p), ("d_mac_x", ctypes.c_void_p), ("d_mac_y", ctypes.c_void_p),
                ("d_align_x", ctypes.c_void_p), ("d_align_y", ctypes.c_void_p),
                ("write_step", ctypes.c_ulonglong), ("index", ctypes.c_ulonglong)]


PORLA_SERVER_REBUILD_REQ_BYTES = 104
assert ctypes.sizeof(ServerRebuildReq) == PORLA_SERVER_REBUILD_REQ_BYTES


class IccDecodeReq(ctypes.Structure):
    """porla_icc_decode_req, include/porla_gpu.h: one level of porla_icc_decode_batch_device (PORLA_ICC_DECODE_REQ_BYTES = 32)."""
    _fields_ = [("d_rows", ctypes.c_void_p), ("d_out", ctypes.c_void_p), ("d_write_steps", ctypes.c_void_p), ("d_bad", ctypes.c_void_p)]


PORLA_ICC_DECODE_REQ_BYTES = 32
assert ctypes.sizeof(IccDecodeReq) == PORLA_ICC_DECODE_REQ_BYTES


class IccDecodeRaggedReq(ctypes.Structure):
    """porla_icc_decode_ragged_req, include/porla_gpu.h: one level of porla_icc_decode_ragged_batch_device: porla_icc_decode_req, then
    the level's own n_rows (PORLA_ICC_DECODE_RAGGED_REQ_BYTES = 40)."""
    _fields_ = [("d_rows", ctypes.c_void_p), ("d_out", ctypes.c_void_p), ("d_write_steps", ctypes.c_void_p), ("d_bad", ctypes.c_void_p),
                ("n_rows", ctypes.c_ulonglong)]


PORLA_ICC_DECODE_RAGGED_REQ_BYTES = 40
assert ctypes.sizeof(IccDecodeRaggedReq) == PORLA_ICC_DECODE_RAGGED_REQ_BYTES


class IccMacDecodeReq(ctypes.Structure):
    """porla_icc_mac_decode_req, include/porla_gpu.h: one level of porla_icc_mac_decode_batch_device
    (PORLA_ICC_MAC_DECODE_REQ_BYTES = 32)."""
    _fields_ = [("d_macs", ctypes.c_void_p), ("d_out", ctypes.c_void_p), ("d_write_steps", ctypes.c_void_p), ("d_sub", ctypes.c_void_p)]


PORLA_ICC_MAC_DECODE_REQ_BYTES = 32
assert ctypes.sizeof(IccMacDecodeReq) == PORLA_ICC_MAC_DECODE_REQ_BYTES


class RetrieveReq(ctypes.Structure):
    """porla_retrieve_req, include/porla_gpu.h: one half of porla_kzg_retrieve_batch_device / porla_ipa_retrieve_batch_device
    (PORLA_RETRIEVE_REQ_BYTES = 48)."""
    _fields_ = [("d_rows", ctypes.c_void_p), ("d_macs", ctypes.c_void_p), ("d_prf", ctypes.c_void_p), ("d_out", ctypes.c_void_p),
                ("d_status", ctypes.c_void_p), ("d_counts", ctypes.c_void_p)]


PORLA_RETRIEVE_REQ_BYTES = 48
PORLA_RETRIEVE_ROW_OK = 1
assert ctypes.sizeof(RetrieveReq) == PORLA_RETRIEVE_REQ_BYTES


class RetrieveAlignedReq(ctypes.Structure):
    """porla_retrieve_aligned_req, include/porla_gpu.h: one half of porla_kzg_retrieve_aligned_batch_device /
    porla_ipa_retrieve_aligned_batch_device (PORLA_RETRIEVE_ALIGNED_REQ_BYTES = 64)."""
    _fields_ = [("d_rows", ctypes.c_void_p), ("d_macs", ctypes.c_void_p), ("d_prf", ctypes.c_void_p), ("d_align", ctypes.c_void_p),
                ("d_write_steps", ctypes.c_void_p), ("d_out", ctypes.c_void_p), ("d_status", ctypes.c_void_p), ("d_counts", ctypes.c_void_p)]


PORLA_RETRIEVE_ALIGNED_REQ_BYTES = 64
assert ctypes.sizeof(RetrieveAlignedReq) == PORLA_RETRIEVE_ALIGNED_REQ_BYTES


class ExtractReq(ctypes.Structure):
    """porla_extract_req, include/porla_gpu.h: one file of porla_kzg_extract_batch_device / porla_ipa_extract_batch_device
    (PORLA_EXTRACT_REQ_BYTES = 104).  data_x and mac_x are HOST arrays of device pointers."""
    _fields_ = [("write_step", ctypes.c_ulonglong), ("data_x", ctypes.c_void_p), ("mac_x", ctypes.c_void_p), ("d_top_rows", ctypes.c_void_p),
                ("d_top_macs", ctypes.c_void_p), ("d_top_align", ctypes.c_void_p), ("d_prf", ctypes.c_void_p), ("d_work", ctypes.c_void_p),
                ("d_blocks", ctypes.c_void_p), ("d_steps", ctypes.c_void_p), ("d_flags", ctypes.c_void_p), ("d_row_status", ctypes.c_void_p),
                ("d_counts", ctypes.c_void_p)]


PORLA_EXTRACT_REQ_BYTES = 104
PORLA_EXTRACT_FOUND, PORLA_EXTRACT_UNSURE, PORLA_EXTRACT_RESIDUE = 1, 2, 4
assert ctypes.sizeof(ExtractReq) == PORLA_EXTRACT_REQ_BYTES


class ExtractXyReq(ctypes.Structure):
    """porla_extract_xy_req, include/porla_gpu.h: one file of porla_kzg_extract_xy_batch_device / porla_ipa_extract_xy_batch_device
    (PORLA_EXTRACT_XY_REQ_BYTES = 160): ExtractReq field for field, then the Y stores.  data_y, mac_y and align_y are HOST arrays of
    device pointers."""
    _fields_ = ExtractReq._fields_ + [("data_y", ctypes.c_void_p), ("mac_y", ctypes.c_void_p), ("align_y", ctypes.c_void_p),
                                      ("d_prf_y", ctypes.c_void_p), ("d_work_y", ctypes.c_void_p), ("d_row_status_y", ctypes.c_void_p),
                                      ("y_levels", ctypes.c_ulonglong)]


PORLA_EXTRACT_XY_REQ_BYTES = 160
PORLA_EXTRACT_FROM_Y = 8
PORLA_EXTRACT_ROW_NOT_TRIED = 2
assert ctypes.sizeof(ExtractXyReq) == PORLA_EXTRACT_XY_REQ_BYTES


class ExtractXytReq(ctypes.Structure):
    """porla_extract_xyt_req, include/porla_gpu.h: one file of porla_kzg_extract_xyt_batch_device / porla_ipa_extract_xyt_batch_device
    (PORLA_EXTRACT_XYT_REQ_BYTES = 224): ExtractXyReq field for field, then the top level's Y half."""
    _fields_ = ExtractXyReq._fields_ + [("d_top_rows_y", ctypes.c_void_p), ("d_top_macs_y", ctypes.c_void_p), ("d_top_align_y", ctypes.c_void_p),
                                        ("d_prf_top_y", ctypes.c_void_p), ("d_top_patch", ctypes.c_void_p),
                                        ("d_row_status_top_y", ctypes.c_void_p), ("top_step", ctypes.c_ulonglong), ("top_y", ctypes.c_ulonglong)]


PORLA_EXTRACT_XYT_REQ_BYTES = 224
assert ctypes.sizeof(ExtractXytReq) == PORLA_EXTRACT_XYT_REQ_BYTES


class RepairTopReq(ctypes.Structure):
    """porla_repair_top_req, include/porla_gpu.h: one file's top level of porla_kzg_repair_top_batch_device /
    porla_ipa_repair_top_batch_device (PORLA_REPAIR_TOP_REQ_BYTES = 120).  The four stores are read AND written."""
    _fields_ = [("d_rows_x", ctypes.c_void_p), ("d_macs_x", ctypes.c_void_p), ("d_align_x", ctypes.c_void_p), ("d_prf_x", ctypes.c_void_p),
                ("d_rows_y", ctypes.c_void_p), ("d_macs_y", ctypes.c_void_p), ("d_align_y", ctypes.c_void_p), ("d_prf_y", ctypes.c_void_p),
                ("d_status_x", ctypes.c_void_p), ("d_status_y", ctypes.c_void_p), ("d_action_x", ctypes.c_void_p),
                ("d_action_y", ctypes.c_void_p), ("d_counts", ctypes.c_void_p), ("top_step", ctypes.c_ulonglong),
                ("reserved", ctypes.c_ulonglong)]


PORLA_REPAIR_TOP_REQ_BYTES = 120
PORLA_REPAIR_DATA, PORLA_REPAIR_MAC, PORLA_REPAIR_LOST = 1, 2, 4
assert ctypes.sizeof(RepairTopReq) == PORLA_REPAIR_TOP_REQ_BYTES


class RepairLevelsReq(ctypes.Structure):
    """porla_repair_levels_req, include/porla_gpu.h: one file's lower levels of porla_kzg_repair_levels_batch_device /
    porla_ipa_repair_levels_batch_device (PORLA_REPAIR_LEVELS_REQ_BYTES = 128).  The five families are HOST arrays of device pointers;
    the Y stores are read AND written."""
    _fields_ = [("write_step", ctypes.c_ulonglong), ("levels", ctypes.c_ulonglong), ("data_x", ctypes.c_void_p), ("mac_x", ctypes.c_void_p),
                ("d_prf_x", ctypes.c_void_p), ("d_prf_y", ctypes.c_void_p), ("data_y", ctypes.c_void_p), ("mac_y", ctypes.c_void_p),
                ("align_y", ctypes.c_void_p), ("d_work", ctypes.c_void_p), ("d_status_x", ctypes.c_void_p), ("d_status_y", ctypes.c_void_p),
                ("d_action_y", ctypes.c_void_p), ("d_level", ctypes.c_void_p), ("d_counts", ctypes.c_void_p), ("reserved", ctypes.c_ulonglong)]


PORLA_REPAIR_LEVELS_REQ_BYTES = 128
PORLA_REPAIR_ALIGN = 8
PORLA_REPAIR_LEVEL_CLEAN, PORLA_REPAIR_LEVEL_X_DAMAGED, PORLA_REPAIR_LEVEL_INCONSISTENT, PORLA_REPAIR_LEVEL_REPAIRED = 1, 2, 3, 4
assert ctypes.sizeof(RepairLevelsReq) == PORLA_REPAIR_LEVELS_REQ_BYTES


class PrfRun(ctypes.Structure):
    """porla_prf_run, include/porla_gpu.h: count triples (level, index0 + t, time0 + t * time_stride) of the MAC PRF
    (PORLA_PRF_RUN_BYTES = 32)."""
    _fields_ = [("level", ctypes.c_int), ("index0", ctypes.c_int), ("count", ctypes.c_ulonglong), ("time0", ctypes.c_longlong),
                ("time_stride", ctypes.c_longlong)]


PORLA_PRF_RUN_BYTES = 32
assert ctypes.sizeof(PrfRun) == PORLA_PRF_RUN_BYTES


class AuditLevel(ctypes.Structure):
    """porla_audit_level, include/porla_gpu.h: where a level's halves begin inside the caller's stores (PORLA_AUDIT_LEVEL_BYTES = 40)."""
    _fields_ = [("data_x", ctypes.c_ulonglong), ("data_y", ctypes.c_ulonglong), ("mac_x", ctypes.c_ulonglong), ("mac_y", ctypes.c_ulonglong),
                ("form", ctypes.c_int), ("pad", ctypes.c_int)]


PORLA_AUDIT_LEVEL_BYTES = 40
assert ctypes.sizeof(AuditLevel) == PORLA_AUDIT_LEVEL_BYTES


class AuditChallengeReq(ctypes.Structure):
    """porla_audit_challenge_req, include/porla_gpu.h: one audit of porla_audit_challenge_batch_device / _host
    (PORLA_AUDIT_CHALLENGE_REQ_BYTES = 88)."""
    _fields_ = [("seed", ctypes.c_uint8 * 16), ("write_step", ctypes.c_ulonglong), ("num_blocks", ctypes.c_ulonglong),
                ("levels", ctypes.POINTER(AuditLevel)), ("d_idx64", ctypes.c_void_p), ("d_coef64", ctypes.c_void_p),
                ("d_idx32", ctypes.c_void_p), ("d_coef32", ctypes.c_void_p), ("d_mac_idx", ctypes.c_void_p), ("d_mac_coef", ctypes.c_void_p)]


PORLA_AUDIT_CHALLENGE_REQ_BYTES = 88
assert ctypes.sizeof(AuditChallengeReq) == PORLA_AUDIT_CHALLENGE_REQ_BYTES


class AuditChallengeInfo(ctypes.Structure):
    """porla_audit_challenge_info, include/porla_gpu.h: what the host knows of a challenge when the call returns
    (PORLA_AUDIT_CHALLENGE_INFO_BYTES = 72)."""
    _fields_ = [("n64", ctypes.c_ulonglong), ("n32", ctypes.c_ulonglong), ("n_macs", ctypes.c_ulonglong), ("random_point", ctypes.c_ulonglong),
                ("a_raw", ctypes.c_int), ("pad", ctypes.c_int), ("a_value", ctypes.c_uint8 * 32)]


PORLA_AUDIT_CHALLENGE_INFO_BYTES = 72
assert ctypes.sizeof(AuditChallengeInfo) == PORLA_AUDIT_CHALLENGE_INFO_BYTES


class AuditScalarReq(ctypes.Structure):
    """porla_audit_scalar_req, include/porla_gpu.h: one audit of porla_audit_complement_scalar_batch_device / _host
    (PORLA_AUDIT_SCALAR_REQ_BYTES = 32)."""
    _fields_ = [("seed", ctypes.c_uint8 * 16), ("write_step", ctypes.c_ulonglong), ("num_blocks", ctypes.c_ulonglong)]


PORLA_AUDIT_SCALAR_REQ_BYTES = 32
assert ctypes.sizeof(AuditScalarReq) == PORLA_AUDIT_SCALAR_REQ_BYTES


def load():
    """Load the engine.  When torch is importable it is imported FIRST so that the HIP runtime the process
    ends up with is the one torch ships (both have soname libamdhip64.so.7; two runtimes in one process
    cannot share device pointers)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(lib_path):
        raise ImportError(
            "porla_amd: %s is missing -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C porla_amd/csrc` (hipcc, gfx950). There is no CPU fallback." % lib_path)
    if os.environ.get("PORLA_NO_TORCH", "0") != "1":
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    _lib = ctypes.CDLL(lib_path, mode=ctypes.RTLD_GLOBAL)
    _declare(_lib)
    return _lib


def _declare(L):
    P = ctypes.POINTER(GoSlice)
    vp, sz, u8p = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p
    L.init_key.argtypes = [P, P]; L.init_key.restype = None
    L.init_SRS.argtypes = [ctypes.c_longlong, P, ctypes.POINTER(ctypes.c_longlong)]; L.init_SRS.restype = None
    L.init_SRS_from_data.argtypes = [ctypes.c_longlong, P]; L.init_SRS_from_data.restype = None
    for name in ("compute_digest", "compute_digest_complement", "compute_digest_from_srs", "add_point", "mult_point"):
        getattr(L, name).argtypes = [P, P]; getattr(L, name).restype = None
    L.compute_multi_exp.argtypes = [P, P, ctypes.c_longlong, P]; L.compute_multi_exp.restype = None
    L.compare_commitment.argtypes = [P, P]; L.compare_commitment.restype = ctypes.c_ubyte
    L.create_proof.argtypes = [ctypes.c_ulonglong, P, P, P, P, P]; L.create_proof.restype = None
    L.verify_proof.argtypes = [P, P, P, P]; L.verify_proof.restype = ctypes.c_ubyte
    L.neg_point.argtypes = [P]; L.neg_point.restype = None
    L.set_inf_point.argtypes = [P]; L.set_inf_point.restype = None

    L.porla_gpu_device_count.argtypes = []; L.porla_gpu_device_count.restype = ctypes.c_int
    L.porla_gpu_set_device.argtypes = [ctypes.c_int]; L.porla_gpu_set_device.restype = ctypes.c_int
    L.porla_gpu_last_error.argtypes = []; L.porla_gpu_last_error.restype = ctypes.c_char_p
    L.porla_gpu_profile_enable.argtypes = [ctypes.c_int]; L.porla_gpu_profile_enable.restype = ctypes.c_int
    L.porla_gpu_profile_get.argtypes = [ctypes.c_int, ctypes.c_char_p, sz, ctypes.POINTER(ctypes.c_double),
                                        ctypes.POINTER(ctypes.c_longlong)]
    L.porla_gpu_profile_get.restype = ctypes.c_int
    L.porla_gpu_set_msm_window.argtypes = [ctypes.c_int]; L.porla_gpu_set_msm_window.restype = ctypes.c_int
    L.porla_gpu_set_msm_glv.argtypes = [ctypes.c_int]; L.porla_gpu_set_msm_glv.restype = ctypes.c_int
    L.porla_gpu_set_msm_small.argtypes = [ctypes.c_int, ctypes.c_int]; L.porla_gpu_set_msm_small.restype = ctypes.c_int
    L.porla_gpu_last_msm_shape.argtypes = [ctypes.POINTER(ctypes.c_int)] * 3; L.porla_gpu_last_msm_shape.restype = ctypes.c_int
    L.porla_glv_split.argtypes = [ctypes.c_int, u8p, u8p, ctypes.POINTER(ctypes.c_int), u8p, ctypes.POINTER(ctypes.c_int)]
    L.porla_glv_split.restype = ctypes.c_int
    i32p, u32p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint32)
    L.porla_msm_small_shape.argtypes = [sz, i32p, u32p, i32p, i32p, i32p, i32p]; L.porla_msm_small_shape.restype = ctypes.c_int
    L.porla_diag_fe_op.argtypes = [ctypes.c_int, ctypes.c_int, u8p, u8p, u8p]; L.porla_diag_fe_op.restype = ctypes.c_int
    for curve in ("bn254", "secp256k1"):
        f = getattr(L, "porla_%s_msm_device_begin" % curve); f.argtypes = [ctypes.c_int, vp, vp, sz, vp]; f.restype = ctypes.c_int
        f = getattr(L, "porla_%s_msm_device_end" % curve); f.argtypes = [ctypes.c_int, u8p, ctypes.c_int]; f.restype = ctypes.c_int
    for curve in ("bn254", "secp256k1"):
        f = getattr(L, "porla_%s_msm_device" % curve); f.argtypes = [vp, vp, sz, u8p, vp]; f.restype = ctypes.c_int
        f = getattr(L, "porla_%s_msm_device_partial" % curve); f.argtypes = [vp, vp, sz, u8p, vp]; f.restype = ctypes.c_int
        f = getattr(L, "porla_%s_msm_host" % curve); f.argtypes = [u8p, u8p, sz, u8p]; f.restype = ctypes.c_int
        f = getattr(L, "porla_%s_msm_pair_device" % curve); f.argtypes = [vp, vp, vp, sz, u8p, u8p, vp]; f.restype = ctypes.c_int
        f = getattr(L, "porla_%s_audit_msm_pair_device" % curve); f.argtypes = [vp, vp, vp, vp, sz, u8p, u8p, vp]; f.restype = ctypes.c_int
        f = getattr(L, "porla_%s_audit_msm_pair_begin" % curve); f.argtypes = [ctypes.c_int, vp, vp, vp, vp, sz, vp]; f.restype = ctypes.c_int
        f = getattr(L, "porla_%s_audit_msm_pair_end" % curve); f.argtypes = [ctypes.c_int, u8p, u8p]; f.restype = ctypes.c_int
        f = getattr(L, "porla_%s_msm_pair_host" % curve); f.argtypes = [u8p, u8p, u8p, sz, u8p, u8p]; f.restype = ctypes.c_int
        u64p = ctypes.POINTER(ctypes.c_uint64)
        f = getattr(L, "porla_%s_msm_batch_device" % curve); f.argtypes = [vp, vp, u64p, sz, vp, vp]; f.restype = ctypes.c_int
        f = getattr(L, "porla_%s_msm_batch_host" % curve); f.argtypes = [u8p, u8p, u64p, sz, u8p]; f.restype = ctypes.c_int
        f = getattr(L, "porla_%s_msm_host_multi" % curve); f.argtypes = [u8p, u8p, sz, ctypes.c_int, ctypes.c_int, u8p]; f.restype = ctypes.c_int
        f = getattr(L, "porla_%s_dist_fold" % curve); f.argtypes = [u8p, u8p]; f.restype = ctypes.c_int
        f = getattr(L, "porla_%s_msm_device_dist" % curve); f.argtypes = [vp, vp, sz, u8p, vp]; f.restype = ctypes.c_int
        f = getattr(L, "porla_%s_jac_sum" % curve); f.argtypes = [u8p, sz, u8p]; f.restype = ctypes.c_int
        f = getattr(L, "porla_%s_tree_fold" % curve); f.argtypes = [u8p, ctypes.c_int, ctypes.c_int, u8p]; f.restype = ctypes.c_int
    L.porla_icc_hadd_host.argtypes = [u8p, sz, sz, ctypes.c_ulonglong, ctypes.c_int, u8p, u8p, ctypes.c_int, u8p]; L.porla_icc_hadd_host.restype = ctypes.c_int
    L.porla_icc_mac_scale_host.argtypes = [u8p, sz, ctypes.c_ulonglong, ctypes.c_int, u8p]; L.porla_icc_mac_scale_host.restype = ctypes.c_int
    L.porla_kzg_hadd_host.argtypes = [u8p, u8p, sz, ctypes.c_ulonglong, u8p, u8p, u8p]; L.porla_kzg_hadd_host.restype = ctypes.c_int
    L.porla_icc_hrebuild_host.argtypes = [ctypes.POINTER(vp), ctypes.c_int, sz, sz, ctypes.c_int]; L.porla_icc_hrebuild_host.restype = ctypes.c_int
    L.porla_icc_mac_hrebuild_host.argtypes = [ctypes.POINTER(vp), ctypes.c_int, sz, ctypes.c_int]; L.porla_icc_mac_hrebuild_host.restype = ctypes.c_int
    L.porla_shard_range.argtypes = [sz, ctypes.c_int, ctypes.c_int, ctypes.POINTER(sz), ctypes.POINTER(sz)]; L.porla_shard_range.restype = ctypes.c_int
    L.porla_kzg_commit_batch_host_multi.argtypes = [u8p, sz, u8p, ctypes.c_int]; L.porla_kzg_commit_batch_host_multi.restype = ctypes.c_int
    L.porla_icc_encode_cols_host.argtypes = [u8p, sz, sz, sz, sz, ctypes.c_int, ctypes.c_ulonglong, ctypes.c_int, vp, vp, vp, ctypes.c_int]
    L.porla_icc_encode_cols_host.restype = ctypes.c_int
    L.porla_icc_encode_host_multi.argtypes = [u8p, sz, sz, ctypes.c_int, ctypes.c_ulonglong, ctypes.c_int, vp, vp, vp, ctypes.c_int, ctypes.c_int]
    L.porla_icc_encode_host_multi.restype = ctypes.c_int
    L.porla_gpu_last_msm_multi.argtypes = [ctypes.POINTER(ctypes.c_int)] * 2; L.porla_gpu_last_msm_multi.restype = ctypes.c_int
    L.porla_dist_unique_id.argtypes = [u8p]; L.porla_dist_unique_id.restype = ctypes.c_int
    L.porla_dist_init.argtypes = [u8p, ctypes.c_int, ctypes.c_int]; L.porla_dist_init.restype = ctypes.c_int
    L.porla_dist_info.argtypes = [ctypes.POINTER(ctypes.c_int)] * 2; L.porla_dist_info.restype = ctypes.c_int
    L.porla_dist_finalize.argtypes = []; L.porla_dist_finalize.restype = ctypes.c_int
    L.porla_dist_allgather_partials.argtypes = [u8p, u8p]; L.porla_dist_allgather_partials.restype = ctypes.c_int
    L.porla_fixed_base_create.argtypes = [ctypes.c_int, u8p, sz, ctypes.c_int, ctypes.POINTER(vp)]
    L.porla_fixed_base_create.restype = ctypes.c_int
    L.porla_fixed_base_info.argtypes = [vp, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                        ctypes.POINTER(ctypes.c_ulonglong)]
    L.porla_fixed_base_info.restype = ctypes.c_int
    L.porla_fixed_base_commit_device.argtypes = [vp, vp, sz, sz, sz, vp, vp]; L.porla_fixed_base_commit_device.restype = ctypes.c_int
    L.porla_fixed_base_commit_host.argtypes = [vp, u8p, sz, sz, sz, u8p]; L.porla_fixed_base_commit_host.restype = ctypes.c_int
    L.porla_fixed_base_destroy.argtypes = [vp]; L.porla_fixed_base_destroy.restype = None
    L.porla_kzg_commit_batch_device.argtypes = [vp, sz, vp, vp]; L.porla_kzg_commit_batch_device.restype = ctypes.c_int
    L.porla_kzg_commit_batch_host.argtypes = [u8p, sz, u8p]; L.porla_kzg_commit_batch_host.restype = ctypes.c_int
    L.porla_kzg_commit_batch_device_to_host.argtypes = [vp, sz, u8p, vp]; L.porla_kzg_commit_batch_device_to_host.restype = ctypes.c_int
    L.porla_ipa_audit_device.argtypes = [vp, vp, vp, vp, sz, vp, vp, vp, sz, sz, vp, vp, vp, vp, sz] + [u8p] * 5 + [vp]
    L.porla_ipa_audit_device.restype = ctypes.c_int
    L.porla_kzg_audit_device.argtypes = [vp, vp, vp, sz, vp, vp, vp, sz, vp, vp, vp, vp, sz, ctypes.c_ulonglong] + [u8p] * 8 + [vp]
    L.porla_kzg_audit_device.restype = ctypes.c_int
    L.porla_kzg_audit_batch_device.argtypes = [ctypes.POINTER(KzgAuditReq), sz, vp, vp, vp]
    L.porla_kzg_audit_batch_device.restype = ctypes.c_int
    L.porla_ipa_audit_batch_device.argtypes = [vp, ctypes.POINTER(IpaAuditReq), sz, vp, vp, vp]
    L.porla_ipa_audit_batch_device.restype = ctypes.c_int
    L.porla_kzg_update_batch_device.argtypes = [ctypes.POINTER(UpdateReq), sz, sz, vp]; L.porla_kzg_update_batch_device.restype = ctypes.c_int
    L.porla_ipa_update_batch_device.argtypes = [vp, ctypes.POINTER(UpdateReq), sz, sz, vp]; L.porla_ipa_update_batch_device.restype = ctypes.c_int
    L.porla_kzg_client_update_batch_device.argtypes = [ctypes.POINTER(ClientUpdateReq), sz, sz, vp]
    L.porla_kzg_client_update_batch_device.restype = ctypes.c_int
    L.porla_ipa_client_update_batch_device.argtypes = [vp, vp, ctypes.POINTER(ClientUpdateReq), sz, sz, vp]
    L.porla_ipa_client_update_batch_device.restype = ctypes.c_int
    L.porla_kzg_client_rebuild_batch_device.argtypes = [ctypes.POINTER(ClientRebuildReq), sz, sz, vp]
    L.porla_kzg_client_rebuild_batch_device.restype = ctypes.c_int
    L.porla_ipa_client_rebuild_batch_device.argtypes = [vp, vp, ctypes.POINTER(ClientRebuildReq), sz, sz, vp]
    L.porla_ipa_client_rebuild_batch_device.restype = ctypes.c_int
    L.porla_server_rebuild_batch_device.argtypes = [ctypes.POINTER(ServerRebuildReq), sz, sz, sz, ctypes.c_int, vp]
    L.porla_server_rebuild_batch_device.restype = ctypes.c_int
    L.porla_kzg_server_rebuild_aligned_batch_device.argtypes = [ctypes.POINTER(ServerRebuildReq), sz, sz, vp]
    L.porla_kzg_server_rebuild_aligned_batch_device.restype = ctypes.c_int
    L.porla_ipa_server_rebuild_aligned_batch_device.argtypes = [vp, ctypes.POINTER(ServerRebuildReq), sz, sz, vp]
    L.porla_ipa_server_rebuild_aligned_batch_device.restype = ctypes.c_int
    L.porla_icc_decode_batch_device.argtypes = [ctypes.POINTER(IccDecodeReq), sz, sz, sz, sz, ctypes.c_int, ctypes.c_int, vp]
    L.porla_icc_decode_batch_device.restype = ctypes.c_int
    L.porla_icc_decode_ragged_batch_device.argtypes = [ctypes.POINTER(IccDecodeRaggedReq), sz, sz, sz, ctypes.c_int, ctypes.c_int, vp]
    L.porla_icc_decode_ragged_batch_device.restype = ctypes.c_int
    L.porla_icc_decode_host.argtypes = [u8p, sz, sz, sz, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_ulonglong), vp,
                                        ctypes.POINTER(ctypes.c_uint)]
    L.porla_icc_decode_host.restype = ctypes.c_int
    L.porla_icc_mac_decode_batch_device.argtypes = [ctypes.POINTER(IccMacDecodeReq), sz, sz, sz, ctypes.c_int, vp]
    L.porla_icc_mac_decode_batch_device.restype = ctypes.c_int
    L.porla_icc_mac_decode_host.argtypes = [u8p, sz, sz, ctypes.c_int, ctypes.POINTER(ctypes.c_ulonglong), u8p, vp]
    L.porla_icc_mac_decode_host.restype = ctypes.c_int
    L.porla_kzg_retrieve_batch_device.argtypes = [ctypes.POINTER(RetrieveReq), sz, sz, sz, vp]
    L.porla_kzg_retrieve_batch_device.restype = ctypes.c_int
    L.porla_ipa_retrieve_batch_device.argtypes = [vp, vp, ctypes.POINTER(RetrieveReq), sz, sz, sz, vp]
    L.porla_ipa_retrieve_batch_device.restype = ctypes.c_int
    L.porla_kzg_retrieve_host.argtypes = [u8p, u8p, u8p, sz, sz, vp, vp, ctypes.POINTER(ctypes.c_uint)]
    L.porla_kzg_retrieve_host.restype = ctypes.c_int
    L.porla_ipa_retrieve_host.argtypes = [vp, vp, u8p, u8p, u8p, sz, sz, vp, vp, ctypes.POINTER(ctypes.c_uint)]
    L.porla_ipa_retrieve_host.restype = ctypes.c_int
    L.porla_kzg_retrieve_aligned_batch_device.argtypes = [ctypes.POINTER(RetrieveAlignedReq), sz, sz, sz, ctypes.c_int, vp]
    L.porla_kzg_retrieve_aligned_batch_device.restype = ctypes.c_int
    L.porla_ipa_retrieve_aligned_batch_device.argtypes = [vp, vp, u8p, ctypes.POINTER(RetrieveAlignedReq), sz, sz, sz, ctypes.c_int, vp]
    L.porla_ipa_retrieve_aligned_batch_device.restype = ctypes.c_int
    L.porla_kzg_extract_batch_device.argtypes = [ctypes.POINTER(ExtractReq), sz, sz, ctypes.c_int, vp]
    L.porla_kzg_extract_batch_device.restype = ctypes.c_int
    L.porla_ipa_extract_batch_device.argtypes = [vp, vp, u8p, ctypes.POINTER(ExtractReq), sz, sz, ctypes.c_int, vp]
    L.porla_ipa_extract_batch_device.restype = ctypes.c_int
    L.porla_kzg_extract_xy_batch_device.argtypes = [ctypes.POINTER(ExtractXyReq), sz, sz, ctypes.c_int, vp]
    L.porla_kzg_extract_xy_batch_device.restype = ctypes.c_int
    L.porla_ipa_extract_xy_batch_device.argtypes = [vp, vp, u8p, ctypes.POINTER(ExtractXyReq), sz, sz, ctypes.c_int, vp]
    L.porla_ipa_extract_xy_batch_device.restype = ctypes.c_int
    L.porla_kzg_extract_xyt_batch_device.argtypes = [ctypes.POINTER(ExtractXytReq), sz, sz, ctypes.c_int, vp]
    L.porla_kzg_extract_xyt_batch_device.restype = ctypes.c_int
    L.porla_ipa_extract_xyt_batch_device.argtypes = [vp, vp, u8p, ctypes.POINTER(ExtractXytReq), sz, sz, ctypes.c_int, vp]
    L.porla_ipa_extract_xyt_batch_device.restype = ctypes.c_int
    L.porla_kzg_repair_top_batch_device.argtypes = [ctypes.POINTER(RepairTopReq), sz, sz, ctypes.c_int, vp]
    L.porla_kzg_repair_top_batch_device.restype = ctypes.c_int
    L.porla_ipa_repair_top_batch_device.argtypes = [vp, vp, u8p, ctypes.POINTER(RepairTopReq), sz, sz, ctypes.c_int, vp]
    L.porla_ipa_repair_top_batch_device.restype = ctypes.c_int
    L.porla_repair_levels_work_bytes.argtypes = [sz, sz, ctypes.c_ulonglong, ctypes.c_ulonglong]
    L.porla_repair_levels_work_bytes.restype = sz
    L.porla_kzg_repair_levels_batch_device.argtypes = [ctypes.POINTER(RepairLevelsReq), sz, sz, vp]
    L.porla_kzg_repair_levels_batch_device.restype = ctypes.c_int
    L.porla_ipa_repair_levels_batch_device.argtypes = [vp, vp, u8p, ctypes.POINTER(RepairLevelsReq), sz, sz, vp]
    L.porla_ipa_repair_levels_batch_device.restype = ctypes.c_int
    L.porla_kzg_retrieve_aligned_host.argtypes = [u8p, u8p, u8p, u8p, vp, sz, sz, ctypes.c_int, vp, vp, ctypes.POINTER(ctypes.c_uint)]
    L.porla_kzg_retrieve_aligned_host.restype = ctypes.c_int
    L.porla_ipa_retrieve_aligned_host.argtypes = [vp, vp, u8p, u8p, u8p, u8p, u8p, vp, sz, sz, ctypes.c_int, vp, vp,
                                                  ctypes.POINTER(ctypes.c_uint)]
    L.porla_ipa_retrieve_aligned_host.restype = ctypes.c_int
    L.porla_mac_prf_batch_device.argtypes = [u8p, ctypes.POINTER(PrfRun), sz, vp, vp]; L.porla_mac_prf_batch_device.restype = ctypes.c_int
    L.porla_mac_prf_host.argtypes = [u8p, ctypes.POINTER(PrfRun), sz, vp]; L.porla_mac_prf_host.restype = ctypes.c_int
    L.porla_client_prf_runs.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_ulonglong, ctypes.c_int, sz, ctypes.POINTER(PrfRun), sz,
                                        ctypes.POINTER(sz), ctypes.POINTER(sz)]
    L.porla_client_prf_runs.restype = ctypes.c_int
    L.porla_audit_challenge_batch_device.argtypes = [ctypes.POINTER(AuditChallengeReq), sz, ctypes.POINTER(AuditChallengeInfo), vp]
    L.porla_audit_challenge_batch_device.restype = ctypes.c_int
    L.porla_audit_challenge_host.argtypes = [ctypes.POINTER(AuditChallengeReq), sz, ctypes.POINTER(AuditChallengeInfo)]
    L.porla_audit_challenge_host.restype = ctypes.c_int
    L.porla_audit_complement_scalar_batch_device.argtypes = [u8p, ctypes.POINTER(AuditScalarReq), sz, ctypes.c_int, vp, vp]
    L.porla_audit_complement_scalar_batch_device.restype = ctypes.c_int
    L.porla_audit_complement_scalar_host.argtypes = [u8p, ctypes.POINTER(AuditScalarReq), sz, ctypes.c_int, vp]
    L.porla_audit_complement_scalar_host.restype = ctypes.c_int
    L.porla_diag_audit_walk.argtypes = [vp, sz, ctypes.c_ulonglong, ctypes.c_ulonglong, ctypes.POINTER(AuditLevel), ctypes.c_int, vp, vp, vp, vp,
                                        vp, vp, ctypes.POINTER(AuditChallengeInfo)]
    L.porla_diag_audit_walk.restype = ctypes.c_int
    L.porla_ipa_prove_batch_device.argtypes = [vp, vp, vp, sz, vp, vp]; L.porla_ipa_prove_batch_device.restype = ctypes.c_int
    L.porla_ipa_verify_batch_device.argtypes = [vp, ctypes.POINTER(IpaVerifyReq), sz, vp, vp, vp]
    L.porla_ipa_verify_batch_device.restype = ctypes.c_int
    L.porla_kzg_verify_batch_device.argtypes = [ctypes.POINTER(KzgVerifyReq), sz, vp, u8p, u8p, vp]
    L.porla_kzg_verify_batch_device.restype = ctypes.c_int
    L.porla_kzg_digest_batch_device.argtypes = [vp, sz, vp, vp]; L.porla_kzg_digest_batch_device.restype = ctypes.c_int
    L.porla_kzg_complement_batch_device.argtypes = [vp, sz, vp, vp]; L.porla_kzg_complement_batch_device.restype = ctypes.c_int
    L.porla_kzg_mac_batch_device.argtypes = [vp, vp, sz, vp, vp]; L.porla_kzg_mac_batch_device.restype = ctypes.c_int
    L.porla_kzg_digest_batch_host.argtypes = [ctypes.c_char_p, sz, ctypes.c_char_p]; L.porla_kzg_digest_batch_host.restype = ctypes.c_int
    L.porla_kzg_complement_batch_host.argtypes = [ctypes.c_char_p, sz, ctypes.c_char_p]; L.porla_kzg_complement_batch_host.restype = ctypes.c_int
    L.porla_kzg_mac_batch_host.argtypes = [ctypes.c_char_p, ctypes.c_char_p, sz, ctypes.c_char_p]; L.porla_kzg_mac_batch_host.restype = ctypes.c_int
    L.porla_bn254_g2_mul_generator.argtypes = [u8p, u8p]; L.porla_bn254_g2_mul_generator.restype = ctypes.c_int
    L.porla_bn254_pairing_product_is_one.argtypes = [u8p, u8p, u8p, u8p, ctypes.c_int]; L.porla_bn254_pairing_product_is_one.restype = ctypes.c_int
    L.porla_kzg_set_commit_window.argtypes = [ctypes.c_int]; L.porla_kzg_set_commit_window.restype = ctypes.c_int
    L.porla_kzg_commit_shape.argtypes = [ctypes.POINTER(ctypes.c_int)] * 2; L.porla_kzg_commit_shape.restype = ctypes.c_int
    L.porla_kzg_row_coefficients.argtypes = [ctypes.POINTER(ctypes.c_size_t)]; L.porla_kzg_row_coefficients.restype = ctypes.c_int
    L.porla_kzg_release_device_memory.argtypes = []; L.porla_kzg_release_device_memory.restype = ctypes.c_int
    L.porla_gpu_release_msm_workspaces.argtypes = []; L.porla_gpu_release_msm_workspaces.restype = ctypes.c_int
    L.porla_icc_mac_encode_device.argtypes = [vp, sz, ctypes.c_int, ctypes.c_ulonglong, ctypes.c_int, vp, vp]
    L.porla_icc_mac_encode_device.restype = ctypes.c_int
    L.porla_icc_encode_xy_device.argtypes = [vp, sz, sz, ctypes.c_int, ctypes.c_ulonglong, vp, vp, vp, vp, vp, vp, ctypes.c_int, vp]
    L.porla_icc_encode_xy_device.restype = ctypes.c_int
    L.porla_icc_mac_encode_xy_device.argtypes = [vp, sz, ctypes.c_int, ctypes.c_ulonglong, vp, vp, vp]
    L.porla_icc_mac_encode_xy_device.restype = ctypes.c_int
    L.porla_icc_mac_encode_xy_host.argtypes = [u8p, sz, ctypes.c_int, ctypes.c_ulonglong, u8p, u8p]
    L.porla_icc_mac_encode_xy_host.restype = ctypes.c_int
    L.porla_icc_mac_encode_host.argtypes = [u8p, sz, ctypes.c_int, ctypes.c_ulonglong, ctypes.c_int, u8p]
    L.porla_icc_mac_encode_host.restype = ctypes.c_int
    L.porla_icc_mac_set_matrix_max.argtypes = [sz]; L.porla_icc_mac_set_matrix_max.restype = ctypes.c_int
    L.porla_icc_mix_device.argtypes = [vp, vp, sz, sz, sz, ctypes.c_int, vp, vp]; L.porla_icc_mix_device.restype = ctypes.c_int
    L.porla_icc_mix_host.argtypes = [u8p, u8p, sz, sz, sz, ctypes.c_int, u8p]; L.porla_icc_mix_host.restype = ctypes.c_int
    L.porla_server_mix_device.argtypes = [vp] * 6 + [sz, sz, sz, ctypes.c_int, vp, vp, vp, vp]; L.porla_server_mix_device.restype = ctypes.c_int
    L.porla_icc_mac_mix_pair_device.argtypes = [vp, vp, vp, vp, sz, sz, ctypes.c_int, vp, vp, vp]; L.porla_icc_mac_mix_pair_device.restype = ctypes.c_int
    L.porla_icc_mac_mix_device.argtypes = [vp, vp, sz, sz, ctypes.c_int, vp, vp]; L.porla_icc_mac_mix_device.restype = ctypes.c_int
    L.porla_icc_mac_mix_host.argtypes = [u8p, u8p, sz, sz, ctypes.c_int, u8p]; L.porla_icc_mac_mix_host.restype = ctypes.c_int
    L.porla_audit_combine_device.argtypes = [vp, vp, vp, sz, vp, vp, vp, sz, sz, ctypes.c_int, vp, vp, vp, vp, vp]
    L.porla_audit_combine_device.restype = ctypes.c_int
    L.porla_icc_encode_device.argtypes = [vp, sz, sz, ctypes.c_int, ctypes.c_ulonglong, ctypes.c_int, vp, vp, vp, ctypes.c_int, vp]
    L.porla_icc_encode_device.restype = ctypes.c_int
    L.porla_icc_encode_host.argtypes = [u8p, sz, sz, ctypes.c_int, ctypes.c_ulonglong, ctypes.c_int, vp, vp, vp, ctypes.c_int]
    L.porla_icc_encode_host.restype = ctypes.c_int


class _LazyLib:
    def __getattr__(self, name):
        return getattr(load(), name)


lib = _LazyLib()
