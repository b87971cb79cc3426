"""ctypes binding of libkeaki_hip.so (include/keaki_hip.h). Plumbing only -- no arithmetic here.

Arrays are numpy uint64 in the C-ABI layouts (Montgomery limbs, see the header). The *_dev methods
take raw device pointers (ints), e.g. torch_tensor.data_ptr(), so callers can keep data resident
in HBM; torch itself is never imported here.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

EXPORTS = [
    "keaki_hip_ctx_create", "keaki_hip_ctx_destroy", "keaki_hip_last_error", "keaki_hip_synchronize", "keaki_hip_version",
    "keaki_hip_srs_g1_upload", "keaki_hip_srs_g1_wrap_dev", "keaki_hip_srs_g1_slice", "keaki_hip_srs_g1_len", "keaki_hip_srs_g1_precompute", "keaki_hip_srs_g1_free",
    "keaki_hip_srs_g2_upload", "keaki_hip_srs_g2_wrap_dev", "keaki_hip_srs_g2_precompute", "keaki_hip_srs_g2_free",
    "keaki_hip_msm_g1", "keaki_hip_msm_g1_dev", "keaki_hip_msm_g2", "keaki_hip_msm_g2_dev",
    "keaki_hip_msm_g1_batch", "keaki_hip_msm_g1_batch_dev", "keaki_hip_kzg_open_batch", "keaki_hip_kzg_open_batch_dev",
    "keaki_hip_open_fk_poly_batch", "keaki_hip_open_fk_poly_batch_dev", "keaki_hip_vec_commit_batch", "keaki_hip_vec_commit_batch_dev",
    "keaki_hip_g1_sum_dev", "keaki_hip_g1_sum",
    "keaki_hip_g1_mul_batch", "keaki_hip_g2_mul_batch", "keaki_hip_g1_mul_batch_dev", "keaki_hip_g2_mul_batch_dev",
    "keaki_hip_pairing_batch", "keaki_hip_pairing_batch_dev",
    "keaki_hip_encap_batch", "keaki_hip_encap_batch_dev", "keaki_hip_decap_batch", "keaki_hip_decap_batch_dev",
    "keaki_hip_encrypt_batch", "keaki_hip_encrypt_batch_dev", "keaki_hip_decrypt_batch", "keaki_hip_decrypt_batch_dev",
    "keaki_hip_group_encrypt_batch", "keaki_hip_group_decrypt_batch",
    "keaki_hip_encap_multi", "keaki_hip_encap_multi_dev", "keaki_hip_encrypt_multi", "keaki_hip_encrypt_multi_dev",
    "keaki_hip_selftest_field", "keaki_hip_selftest_field_ops", "keaki_hip_selftest_tower_ops", "keaki_hip_selftest_point_ops", "keaki_hip_open_fk", "keaki_hip_open_fk_poly", "keaki_hip_srs_g1_precompute_fk", "keaki_hip_fk_shard_create", "keaki_hip_fk_shard_free", "keaki_hip_fk_shard_sizes", "keaki_hip_fk_shard_setup", "keaki_hip_fk_shard_open", "keaki_hip_fr_fft", "keaki_hip_srs_g1_check", "keaki_hip_g2_check", "keaki_hip_g1_compress", "keaki_hip_g2_compress", "keaki_hip_g1_compress_dev", "keaki_hip_g2_compress_dev", "keaki_hip_g1_decompress", "keaki_hip_g2_decompress", "keaki_hip_g1_decompress_dev", "keaki_hip_g2_decompress_dev", "keaki_hip_g2_subgroup_check", "keaki_hip_g2_subgroup_check_dev", "keaki_hip_kzg_open", "keaki_hip_kzg_verify", "keaki_hip_kzg_verify_batch", "keaki_hip_kzg_verify_batch_dev", "keaki_hip_kzg_verify_each", "keaki_hip_kzg_verify_each_dev", "keaki_hip_final_exp_batch", "keaki_hip_miller_loop_batch", "keaki_hip_g2_prepare", "keaki_hip_set_timing", "keaki_hip_last_msm_bucket_ms", "keaki_hip_last_msm_total_ms", "keaki_hip_last_msm_window_bits",
    "keaki_hip_last_fk_ms", "keaki_hip_ctx_stream", "keaki_hip_ctx_device", "keaki_hip_ctx_set_option", "keaki_hip_debug_set_alloc_limit", "keaki_hip_debug_poison_workspaces", "keaki_hip_ctx_memory", "keaki_hip_ctx_trim", "keaki_hip_kzg_quotient", "keaki_hip_vec_commit", "keaki_hip_encap_prepare",
    "keaki_hip_srs_g1_precompute_update", "keaki_hip_vec_update", "keaki_hip_vec_update_dev",
    "keaki_hip_kzg_set_polys", "keaki_hip_kzg_set_polys_dev", "keaki_hip_kzg_open_multi", "keaki_hip_kzg_open_multi_dev",
    "keaki_hip_kzg_aggregate", "keaki_hip_kzg_aggregate_dev", "keaki_hip_kzg_verify_multi",
    "keaki_hip_srs_g1_precompute_fk_cosets", "keaki_hip_open_fk_cosets", "keaki_hip_open_fk_cosets_poly", "keaki_hip_open_fk_cosets_poly_dev",
    "keaki_hip_kzg_verify_cosets", "keaki_hip_kzg_verify_cosets_dev",
    "keaki_hip_kzg_verify_sets", "keaki_hip_kzg_verify_sets_dev", "keaki_hip_pairing_product", "keaki_hip_pairing_product_dev",
    "keaki_hip_srs_g1_precompute_cosets", "keaki_hip_kzg_coset_pairs", "keaki_hip_kzg_coset_pairs_dev",
    "keaki_hip_kzg_verify_cosets_each", "keaki_hip_kzg_verify_cosets_each_dev",
    "keaki_hip_srs_g2_precompute_sets", "keaki_hip_kzg_set_pairs", "keaki_hip_kzg_set_pairs_dev",
    "keaki_hip_kzg_verify_sets_each", "keaki_hip_kzg_verify_sets_each_dev",
    "keaki_hip_group_create", "keaki_hip_group_destroy", "keaki_hip_group_size", "keaki_hip_group_ctx", "keaki_hip_group_last_error",
    "keaki_hip_group_peer_note", "keaki_hip_group_srs_g1_upload", "keaki_hip_group_srs_g1_len", "keaki_hip_group_srs_g1_has_tables", "keaki_hip_group_srs_g1_free", "keaki_hip_group_msm_g1",
    "keaki_hip_group_kzg_open", "keaki_hip_group_encap_batch", "keaki_hip_group_decap_batch",
    "keaki_hip_group_fk_create", "keaki_hip_group_fk_open", "keaki_hip_group_fk_free",
]

KEAKI_ERR_TOO_LARGE = -5
# the `stream` argument of keaki_hip_ctx_create (include/keaki_hip.h): the context's own non-blocking stream | the device's legacy default stream
KEAKI_HIP_STREAM_PRIVATE = None
KEAKI_HIP_STREAM_LEGACY = 1


def field_op_codes() -> dict:
    """{'U29_MUL': 0, ...}: the op codes of keaki_hip_selftest_field_ops with the record geometry ('SLOTS', 'SLOT_WORDS', 'MAX_RECORDS',
    'FIRST_PAIR'), read from include/keaki_hip.h so that no second list exists"""
    import re
    hdr = open(os.path.join(os.path.dirname(_HERE), "include", "keaki_hip.h")).read()
    codes = {m.group(1): int(m.group(2)) for m in re.finditer(r"\bKEAKI_FOP_([A-Z0-9_]+)\s*=\s*(\d+)", hdr)}
    for m in re.finditer(r"#define\s+KEAKI_FOP_([A-Z_]+)\s+(\w+)", hdr):
        v = m.group(2)
        codes[m.group(1)] = int(v) if v.isdigit() else codes[v[len("KEAKI_FOP_"):]]
    return codes


def tower_op_codes() -> dict:
    """{'FQ12_MUL': 0, ...}: the op codes of keaki_hip_selftest_tower_ops with the record geometry ('REC_WORDS', 'OUT_WORDS', 'MAX_RECORDS',
    'FIRST_WIDE'), read from include/keaki_hip.h so that no second list exists"""
    import re
    hdr = open(os.path.join(os.path.dirname(_HERE), "include", "keaki_hip.h")).read()
    codes = {m.group(1): int(m.group(2)) for m in re.finditer(r"\bKEAKI_TOP_([A-Z0-9_]+)\s*=\s*(\d+)", hdr)}
    for m in re.finditer(r"#define\s+KEAKI_TOP_([A-Z_]+)\s+(\w+)", hdr):
        v = m.group(2)
        codes[m.group(1)] = int(v) if v.isdigit() else codes[v[len("KEAKI_TOP_"):]]
    return codes


def point_op_codes() -> dict:
    """{'X29_ADD': 0, ...}: the op codes of keaki_hip_selftest_point_ops with the record geometry ('SLOTS', 'SLOT_WORDS', 'FLAG_SLOT', 'OUT_SLOTS',
    'OUT_FLAG_SLOT', 'MAX_RECORDS', 'FIRST_G2'), read from include/keaki_hip.h so that no second list exists"""
    import re
    hdr = open(os.path.join(os.path.dirname(_HERE), "include", "keaki_hip.h")).read()
    codes = {m.group(1): int(m.group(2)) for m in re.finditer(r"\bKEAKI_POP_([A-Z0-9_]+)\s*=\s*(\d+)", hdr)}
    for m in re.finditer(r"#define\s+KEAKI_POP_([A-Z0-9_]+)\s+(\w+)", hdr):
        v = m.group(2)
        codes[m.group(1)] = int(v) if v.isdigit() else codes[v[len("KEAKI_POP_"):]]
    return codes


class KeakiHipError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"keaki_hip error {status}: {message}")
        self.status = status
        self.message = message


def lib_path() -> str:
    return os.path.join(_HERE, "libkeaki_hip.so")


def share_torch_runtime(names=("libamdhip64.so",)):    # the HIP runtime only: loading PyTorch's librccl ahead of torch aborts at exit
    """A process must end up with ONE HIP runtime. PyTorch wheels bundle their own copy (torch/lib/libamdhip64.so, the same SONAME as the
    system's): when torch is imported FIRST, libkeaki_hip.so binds to that copy and everything shares it; the other way round the process
    would hold two runtimes and torch fails with "No HIP GPUs are available". So, when PyTorch is installed but not loaded yet, its copy
    of the named libraries is loaded here (by path, without importing torch) before ours. KEAKI_HIP_RUNTIME=system keeps the system's
    runtime (a process that never imports torch does not care)."""
    import sys
    if os.environ.get("KEAKI_HIP_RUNTIME", "") == "system" or "torch" in sys.modules:
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    libdir = os.path.join(os.path.dirname(spec.origin), "lib")
    for name in names:
        path = os.path.join(libdir, name)
        if os.path.exists(path):
            try:
                C.CDLL(path)        # local scope is enough: later NEEDED entries resolve to a loaded object by its SONAME
            except OSError:
                pass        # an unusable bundle: the system's runtime serves


def load_library():
    """Loads libkeaki_hip.so. Raises (never falls back) when the HIP extension is missing."""
    global _LIB
    if _LIB is None:
        path = lib_path()
        if not os.path.exists(path):
            raise KeakiHipError(-100, f"{path} not built; run `python -c 'import __graft_entry__ as g; g.build()'` "
                                      f"or `make -C keaki_amd/csrc`. There is no CPU fallback.")
        share_torch_runtime()
        lib = C.CDLL(path)
        vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int32
        lib.keaki_hip_version.restype = C.c_char_p
        lib.keaki_hip_last_error.restype = C.c_char_p
        lib.keaki_hip_last_error.argtypes = [vp]
        lib.keaki_hip_ctx_create.argtypes = [i32, vp, C.POINTER(vp)]
        lib.keaki_hip_ctx_destroy.argtypes = [vp]
        lib.keaki_hip_ctx_destroy.restype = None
        lib.keaki_hip_synchronize.argtypes = [vp]
        for g in ("g1", "g2"):
            getattr(lib, f"keaki_hip_srs_{g}_upload").argtypes = [vp, vp, sz, C.POINTER(vp)]
            getattr(lib, f"keaki_hip_srs_{g}_wrap_dev").argtypes = [vp, vp, sz, C.POINTER(vp)]
            getattr(lib, f"keaki_hip_srs_{g}_free").argtypes = [vp, vp]
            getattr(lib, f"keaki_hip_srs_{g}_free").restype = None
            getattr(lib, f"keaki_hip_msm_{g}").argtypes = [vp, vp, vp, sz, vp]
            getattr(lib, f"keaki_hip_msm_{g}_dev").argtypes = [vp, vp, vp, sz, vp]
            getattr(lib, f"keaki_hip_{g}_mul_batch").argtypes = [vp, vp, i32, vp, sz, vp]
            getattr(lib, f"keaki_hip_{g}_mul_batch_dev").argtypes = [vp, vp, i32, vp, sz, vp]
        lib.keaki_hip_srs_g1_precompute.argtypes = [vp, vp, C.POINTER(C.c_size_t)]
        lib.keaki_hip_srs_g2_precompute.argtypes = [vp, vp, C.POINTER(C.c_size_t)]
        lib.keaki_hip_srs_g1_slice.argtypes = [vp, vp, sz, sz, C.POINTER(vp)]
        lib.keaki_hip_srs_g1_len.argtypes = [vp]
        lib.keaki_hip_srs_g1_len.restype = sz
        lib.keaki_hip_g1_sum.argtypes = [vp, vp, sz, vp]
        lib.keaki_hip_g1_sum_dev.argtypes = [vp, vp, sz, vp]
        lib.keaki_hip_pairing_batch.argtypes = [vp, vp, vp, i32, sz, vp]
        lib.keaki_hip_pairing_batch_dev.argtypes = [vp, vp, vp, i32, sz, vp]
        lib.keaki_hip_encap_batch.argtypes = [vp, vp, vp, vp, vp, vp, sz, vp, vp, vp, sz]
        lib.keaki_hip_encap_batch_dev.argtypes = [vp, vp, vp, vp, vp, vp, sz, vp, vp, vp, sz]
        lib.keaki_hip_decap_batch.argtypes = [vp, vp, vp, sz, vp, vp, sz]
        lib.keaki_hip_decap_batch_dev.argtypes = [vp, vp, vp, sz, vp, vp, sz]
        lib.keaki_hip_selftest_field.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
        lib.keaki_hip_selftest_field_ops.argtypes = [vp, C.c_uint32, vp, sz, vp]
        lib.keaki_hip_selftest_tower_ops.argtypes = [vp, C.c_uint32, vp, sz, vp]
        lib.keaki_hip_selftest_point_ops.argtypes = [vp, C.c_uint32, vp, sz, vp]
        lib.keaki_hip_open_fk.argtypes = [vp, vp, C.c_uint32, vp, vp, vp, vp, vp]
        lib.keaki_hip_open_fk_poly.argtypes = [vp, vp, C.c_uint32, vp, vp, vp, vp, vp]
        lib.keaki_hip_fr_fft.argtypes = [vp, vp, C.c_uint32, vp, vp]
        lib.keaki_hip_srs_g1_precompute_fk.argtypes = [vp, vp, C.c_uint32, vp]
        lib.keaki_hip_fk_shard_create.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, C.POINTER(vp)]
        lib.keaki_hip_fk_shard_free.argtypes = [vp, vp]
        lib.keaki_hip_fk_shard_free.restype = None
        lib.keaki_hip_fk_shard_sizes.argtypes = [vp, C.POINTER(C.c_size_t)]
        lib.keaki_hip_fk_shard_setup.argtypes = [vp, vp, C.c_int32, vp, vp]
        lib.keaki_hip_fk_shard_open.argtypes = [vp, vp, C.c_int32, vp, vp, vp, vp]
        lib.keaki_hip_srs_g1_check.argtypes = [vp, vp, vp, vp]
        lib.keaki_hip_kzg_open.argtypes = [vp, vp, vp, C.c_size_t, vp, vp, vp]
        lib.keaki_hip_g2_check.argtypes = [vp, vp, C.c_size_t, vp, vp]
        for name in ("keaki_hip_g1_compress", "keaki_hip_g2_compress", "keaki_hip_g1_compress_dev", "keaki_hip_g2_compress_dev"):
            getattr(lib, name).argtypes = [vp, vp, sz, vp]
        lib.keaki_hip_g1_decompress.argtypes = lib.keaki_hip_g1_decompress_dev.argtypes = [vp, vp, sz, vp, vp, vp, vp]
        lib.keaki_hip_g2_decompress.argtypes = lib.keaki_hip_g2_decompress_dev.argtypes = [vp, vp, sz, i32, vp, vp, vp, vp]
        lib.keaki_hip_g2_subgroup_check.argtypes = lib.keaki_hip_g2_subgroup_check_dev.argtypes = [vp, vp, sz, vp, vp]
        lib.keaki_hip_kzg_verify.argtypes = [vp, vp, vp, vp, vp, vp, C.POINTER(C.c_int32)]
        lib.keaki_hip_kzg_verify_batch.argtypes = [vp, vp, i32, vp, vp, i32, vp, vp, vp, sz, C.POINTER(C.c_int32), vp]
        lib.keaki_hip_kzg_verify_batch_dev.argtypes = [vp, vp, i32, vp, vp, i32, vp, vp, vp, sz, C.POINTER(C.c_int32), vp]
        lib.keaki_hip_kzg_verify_each.argtypes = lib.keaki_hip_kzg_verify_each_dev.argtypes = [vp, vp, i32, vp, vp, i32, vp, vp, sz, vp, vp, vp, vp]
        lib.keaki_hip_final_exp_batch.argtypes = [vp, vp, sz, vp]
        lib.keaki_hip_miller_loop_batch.argtypes = [vp, vp, vp, sz, vp]
        lib.keaki_hip_set_timing.argtypes = [vp, i32]
        lib.keaki_hip_last_msm_bucket_ms.argtypes = [vp]
        lib.keaki_hip_last_msm_bucket_ms.restype = C.c_float
        lib.keaki_hip_last_msm_total_ms.argtypes = [vp]
        lib.keaki_hip_last_msm_total_ms.restype = C.c_float
        lib.keaki_hip_last_msm_window_bits.argtypes = [vp]
        lib.keaki_hip_last_fk_ms.argtypes = [vp, C.POINTER(C.c_float)]
        lib.keaki_hip_ctx_set_option.argtypes = [vp, C.c_char_p, C.c_int64]
        lib.keaki_hip_debug_set_alloc_limit.argtypes = [vp, sz]
        lib.keaki_hip_debug_poison_workspaces.argtypes = [vp, C.c_uint32, i32]
        lib.keaki_hip_ctx_memory.argtypes = [vp, C.POINTER(C.c_size_t)]
        lib.keaki_hip_ctx_trim.argtypes = [vp]
        lib.keaki_hip_ctx_stream.argtypes = [vp]
        lib.keaki_hip_ctx_stream.restype = vp
        lib.keaki_hip_ctx_device.argtypes = [vp]
        lib.keaki_hip_ctx_device.restype = C.c_int32
        lib.keaki_hip_kzg_quotient.argtypes = [vp, vp, sz, vp, vp, vp]
        lib.keaki_hip_msm_g1_batch.argtypes = [vp, vp, vp, sz, sz, sz, vp]
        lib.keaki_hip_msm_g1_batch_dev.argtypes = [vp, vp, vp, sz, sz, sz, vp]
        lib.keaki_hip_kzg_open_batch.argtypes = [vp, vp, vp, sz, sz, sz, vp, vp, vp]
        lib.keaki_hip_kzg_open_batch_dev.argtypes = [vp, vp, vp, sz, sz, sz, vp, vp, vp]
        lib.keaki_hip_open_fk_poly_batch.argtypes = [vp, vp, C.c_uint32, vp, sz, sz, vp, vp, vp, vp]
        lib.keaki_hip_open_fk_poly_batch_dev.argtypes = [vp, vp, C.c_uint32, vp, sz, sz, vp, vp, vp, vp]
        lib.keaki_hip_vec_commit_batch.argtypes = [vp, vp, vp, sz, sz, sz, C.c_uint32, vp, vp, vp, vp, vp, vp, vp]
        lib.keaki_hip_vec_commit_batch_dev.argtypes = [vp, vp, vp, sz, sz, sz, C.c_uint32, vp, vp, vp, vp, vp, vp, vp]
        lib.keaki_hip_encap_prepare.argtypes = [vp, vp, sz]
        lib.keaki_hip_vec_commit.argtypes = [vp, vp, vp, sz, vp, C.c_uint32, vp, vp, vp, vp, vp, vp, vp]
        lib.keaki_hip_srs_g1_precompute_update.argtypes = [vp, vp, C.c_uint32, vp, vp, vp]
        lib.keaki_hip_vec_update.argtypes = [vp, vp, C.c_uint32, vp, vp, vp, vp, vp, sz, vp, vp]
        lib.keaki_hip_vec_update_dev.argtypes = [vp, vp, C.c_uint32, vp, vp, vp, vp, vp, sz, vp, vp]
        lib.keaki_hip_kzg_set_polys.argtypes = [vp, vp, vp, sz, vp, vp, vp]
        lib.keaki_hip_kzg_set_polys_dev.argtypes = [vp, vp, vp, sz, vp, vp, vp]
        lib.keaki_hip_kzg_open_multi.argtypes = [vp, vp, vp, sz, vp, sz, vp, vp]
        lib.keaki_hip_kzg_open_multi_dev.argtypes = [vp, vp, vp, sz, vp, sz, vp, vp]
        lib.keaki_hip_kzg_aggregate.argtypes = [vp, vp, vp, sz, vp]
        lib.keaki_hip_kzg_aggregate_dev.argtypes = [vp, vp, vp, sz, vp]
        lib.keaki_hip_kzg_verify_cosets.argtypes = [vp, vp, vp, i32, vp, vp, i32, vp, sz, sz, C.c_uint32, vp, vp, vp, vp, sz, C.POINTER(C.c_int32), vp]
        lib.keaki_hip_kzg_verify_cosets_dev.argtypes = [vp, vp, vp, i32, vp, vp, i32, vp, sz, sz, C.c_uint32, vp, vp, vp, vp, sz, C.POINTER(C.c_int32), vp]
        lib.keaki_hip_kzg_verify_sets.argtypes = lib.keaki_hip_kzg_verify_sets_dev.argtypes = [
            vp, vp, vp, vp, i32, vp, i32, vp, vp, sz, sz, vp, vp, sz, C.POINTER(C.c_int32), vp]
        lib.keaki_hip_pairing_product.argtypes = [vp, vp, vp, sz, vp]
        lib.keaki_hip_pairing_product_dev.argtypes = [vp, vp, vp, sz, vp]
        lib.keaki_hip_srs_g1_precompute_cosets.argtypes = [vp, vp, C.c_uint32]
        lib.keaki_hip_kzg_coset_pairs.argtypes = lib.keaki_hip_kzg_coset_pairs_dev.argtypes = [vp, vp, vp, i32, vp, i32, vp, sz, sz, C.c_uint32, vp, vp, sz, vp, vp]
        lib.keaki_hip_kzg_verify_cosets_each.argtypes = lib.keaki_hip_kzg_verify_cosets_each_dev.argtypes = [
            vp, vp, vp, i32, vp, vp, i32, vp, sz, sz, C.c_uint32, vp, vp, vp, sz, vp, vp, vp, vp]
        lib.keaki_hip_srs_g2_precompute_sets.argtypes = [vp, vp, sz]
        lib.keaki_hip_kzg_set_pairs.argtypes = lib.keaki_hip_kzg_set_pairs_dev.argtypes = [vp, vp, vp, vp, i32, vp, i32, vp, vp, sz, sz, sz, vp, vp]
        lib.keaki_hip_kzg_verify_sets_each.argtypes = lib.keaki_hip_kzg_verify_sets_each_dev.argtypes = [
            vp, vp, vp, vp, i32, vp, i32, vp, vp, sz, sz, vp, sz, vp, vp, vp, vp, vp]
        lib.keaki_hip_kzg_verify_multi.argtypes = [vp, vp, vp, vp, vp, vp, sz, vp, C.POINTER(C.c_int32), vp]
        lib.keaki_hip_srs_g1_precompute_fk_cosets.argtypes = [vp, vp, C.c_uint32, C.c_uint32, vp]
        lib.keaki_hip_open_fk_cosets.argtypes = [vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp]
        lib.keaki_hip_open_fk_cosets_poly.argtypes = [vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp]
        lib.keaki_hip_open_fk_cosets_poly_dev.argtypes = [vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp]
        lib.keaki_hip_group_create.argtypes = [C.POINTER(i32), sz, C.POINTER(vp)]
        lib.keaki_hip_group_destroy.argtypes = [vp]
        lib.keaki_hip_group_destroy.restype = None
        lib.keaki_hip_group_size.argtypes = [vp]
        lib.keaki_hip_group_size.restype = sz
        lib.keaki_hip_group_ctx.argtypes = [vp, sz]
        lib.keaki_hip_group_ctx.restype = vp
        lib.keaki_hip_group_last_error.argtypes = [vp]
        lib.keaki_hip_group_last_error.restype = C.c_char_p
        lib.keaki_hip_group_srs_g1_upload.argtypes = [vp, vp, sz, i32, C.POINTER(vp)]
        lib.keaki_hip_group_srs_g1_len.argtypes = [vp]
        lib.keaki_hip_group_srs_g1_len.restype = sz
        lib.keaki_hip_group_peer_note.argtypes = [vp]
        lib.keaki_hip_group_peer_note.restype = C.c_char_p
        lib.keaki_hip_group_srs_g1_has_tables.argtypes = [vp]
        lib.keaki_hip_group_srs_g1_has_tables.restype = C.c_int32
        lib.keaki_hip_group_srs_g1_free.argtypes = [vp, vp]
        lib.keaki_hip_group_srs_g1_free.restype = None
        lib.keaki_hip_group_msm_g1.argtypes = [vp, vp, vp, sz, vp]
        lib.keaki_hip_group_kzg_open.argtypes = [vp, vp, vp, sz, vp, vp, vp]
        lib.keaki_hip_group_encap_batch.argtypes = [vp, vp, vp, vp, vp, vp, sz, vp, vp, vp, sz]
        lib.keaki_hip_group_decap_batch.argtypes = [vp, vp, vp, sz, vp, vp, sz]
        lib.keaki_hip_encrypt_batch.argtypes = [vp, vp, vp, vp, vp, vp, vp, sz, vp, vp, sz]
        lib.keaki_hip_encrypt_batch_dev.argtypes = [vp, vp, vp, vp, vp, vp, sz, vp, vp, sz]
        lib.keaki_hip_encap_multi.argtypes = [vp, vp, vp, sz, vp, vp, vp, vp, sz, vp, vp, vp, sz]
        lib.keaki_hip_encap_multi_dev.argtypes = [vp, vp, vp, sz, vp, vp, vp, vp, sz, vp, vp, vp, sz]
        lib.keaki_hip_encrypt_multi.argtypes = [vp, vp, vp, sz, vp, vp, vp, vp, vp, sz, vp, vp, sz]
        lib.keaki_hip_encrypt_multi_dev.argtypes = [vp, vp, vp, sz, vp, vp, vp, vp, sz, vp, vp, sz]
        lib.keaki_hip_decrypt_batch.argtypes = [vp, vp, vp, vp, sz, vp, sz]
        lib.keaki_hip_decrypt_batch_dev.argtypes = [vp, vp, vp, sz, vp, sz]
        lib.keaki_hip_group_encrypt_batch.argtypes = [vp, vp, vp, vp, vp, vp, vp, sz, vp, vp, sz]
        lib.keaki_hip_group_decrypt_batch.argtypes = [vp, vp, vp, vp, sz, vp, sz]
        lib.keaki_hip_group_fk_create.argtypes = [vp, vp, C.c_uint32, vp, vp, vp, C.POINTER(vp)]
        lib.keaki_hip_group_fk_open.argtypes = [vp, vp, vp, vp]
        lib.keaki_hip_group_fk_free.argtypes = [vp, vp]
        lib.keaki_hip_group_fk_free.restype = None
        _LIB = lib
    return _LIB


def _np(a, width=None):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if width is not None:
        a = a.reshape(-1, width)
    return a


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class SrsG1:
    def __init__(self, owner, handle, n):
        self.owner, self.handle, self.n = owner, handle, n

    def free(self):
        if self.handle:
            self.owner.lib.keaki_hip_srs_g1_free(self.owner.ctx, self.handle)
            self.handle = None


class SrsG2(SrsG1):
    def free(self):
        if self.handle:
            self.owner.lib.keaki_hip_srs_g2_free(self.owner.ctx, self.handle)
            self.handle = None


class FkShardHandle:
    """one rank's part of a sharded FK23 (keaki_hip_fk_shard). sizes = (buffer bytes, all-to-all bytes per peer of the 2d-point
    transforms, of the d-point transform, all-gather bytes per rank)"""

    def __init__(self, owner, handle, log2d, rank, world, sizes):
        self.owner, self.handle, self.log2d, self.rank, self.world, self.sizes = owner, handle, log2d, rank, world, sizes

    def free(self):
        if self.handle:
            self.owner.lib.keaki_hip_fk_shard_free(self.owner.ctx, self.handle)
            self.handle = None


class KeakiHip:
    """One context = one GPU (one process per GPU in multi-GPU runs)."""

    STREAM_LEGACY = KEAKI_HIP_STREAM_LEGACY          # the device's legacy default stream (torch's default stream has handle 0 = this one)

    def __init__(self, device: int = 0, stream: int | None = None):
        """stream: None -> private non-blocking stream (order *_dev calls with synchronize()); 0 or STREAM_LEGACY -> the legacy default
        stream (what `torch.cuda.current_stream().cuda_stream` == 0 means); else a hipStream_t handle, e.g. torch.cuda.Stream().cuda_stream."""
        self.lib = load_library()
        ctx = C.c_void_p()
        if stream is not None and stream == 0:
            stream = self.STREAM_LEGACY
        st = self.lib.keaki_hip_ctx_create(device, C.c_void_p(stream) if stream is not None else None, C.byref(ctx))
        if st != 0:
            raise KeakiHipError(st, self.lib.keaki_hip_last_error(None).decode())
        self.ctx = ctx

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.keaki_hip_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, st):
        if st != 0:
            raise KeakiHipError(st, self.lib.keaki_hip_last_error(self.ctx).decode())

    def synchronize(self):
        self._ck(self.lib.keaki_hip_synchronize(self.ctx))

    def set_option(self, name: str, value: int):
        """tuning / A-B switch of this context (keaki_hip_ctx_set_option); the environment is only read when a context is created"""
        self._ck(self.lib.keaki_hip_ctx_set_option(self.ctx, name.encode(), int(value)))

    def debug_set_alloc_limit(self, nbytes: int):
        """test hook: single allocations of this context above nbytes fail with KEAKI_ERR_OOM (0 = no limit)"""
        self._ck(self.lib.keaki_hip_debug_set_alloc_limit(self.ctx, int(nbytes)))

    def debug_poison_workspaces(self, byte: int, also_new: bool = True):
        """test hook: fill every scratch workspace of this context with `byte`; also_new: and every allocation it makes from now on"""
        self._ck(self.lib.keaki_hip_debug_poison_workspaces(self.ctx, int(byte) & 0xFF, 1 if also_new else 0))

    def memory(self) -> dict:
        out = (C.c_size_t * 4)()
        self._ck(self.lib.keaki_hip_ctx_memory(self.ctx, out))
        return {"tables": int(out[0]), "workspaces": int(out[1]), "gt_tables": int(out[2]), "total": int(out[3])}

    def trim(self):
        """release every workspace / encapsulate table of the context (rebuilt on demand)"""
        self._ck(self.lib.keaki_hip_ctx_trim(self.ctx))

    def version(self) -> str:
        return self.lib.keaki_hip_version().decode()

    def kzg_quotient(self, coeffs, point):
        """-> ((n - 1) x u64[4] quotient coefficients, p(point) u64[4])"""
        c = _np(coeffs, 4); n = c.shape[0]
        q = np.zeros((max(n - 1, 0), 4), np.uint64); val = np.zeros(4, np.uint64)
        self._ck(self.lib.keaki_hip_kzg_quotient(self.ctx, _ptr(c) if n else None, n, _ptr(_np(point)), _ptr(q) if n > 1 else None, _ptr(val)))
        return q, val

    def vec_commit(self, srs: "SrsG1", values, pad, log2d: int, omega_d_inv, inv_d, omega_2d, omega_2d_inv, inv_2d):
        """the body of vec::vec_commit behind the padding draw -> (commitment as normalised Jacobian u64[12], d affine proofs)"""
        v = _np(values, 4); d = 1 << log2d
        com = np.zeros(12, np.uint64); proofs = np.zeros((d, 8), np.uint64)
        self._ck(self.lib.keaki_hip_vec_commit(self.ctx, srs.handle, _ptr(v) if v.shape[0] else None, v.shape[0], _ptr(_np(pad)) if pad is not None else None, log2d,
                                               _ptr(_np(omega_d_inv)), _ptr(_np(inv_d)), _ptr(_np(omega_2d)), _ptr(_np(omega_2d_inv)), _ptr(_np(inv_2d)),
                                               _ptr(com), _ptr(proofs)))
        return com, proofs

    def srs_g1_precompute_update(self, srs: "SrsG1", log2d: int, omega_d, omega_d_inv, inv_d):
        """setup-time build of the handle's vec_update tables for d = 2^log2d (192 B x d; vec_update builds them on first use anyway)"""
        self._ck(self.lib.keaki_hip_srs_g1_precompute_update(self.ctx, srs.handle, log2d, _ptr(_np(omega_d)), _ptr(_np(omega_d_inv)), _ptr(_np(inv_d))))

    def vec_update(self, srs: "SrsG1", log2d: int, omega_d, omega_d_inv, inv_d, idx, deltas, com=None, proofs=None):
        """evaluation idx[t] += deltas[t] (t < k) of a committed vector: `com` (u64[12] normalised Jacobian) and `proofs` ((d, 8) affine), either
        may be None, are updated IN PLACE to the bytes vec_commit returns for the changed vector (keaki_hip_vec_update) -> (com, proofs).
        Measured crossover (profiles/vec_update_times.txt): the update wins up to k = 16 and loses at k = 64 at d = 2^12, 2^16 and 2^20 (break-even near
        k = 32, near 48 at 2^16): above it a fresh vec_commit is cheaper."""
        ix = np.ascontiguousarray(idx, dtype=np.uint32).reshape(-1)
        dl = _np(deltas, 4)
        if dl.shape[0] != ix.shape[0]:
            raise ValueError("vec_update: %d indices but %d deltas" % (ix.shape[0], dl.shape[0]))
        for name, a, shape in (("com", com, (12,)), ("proofs", proofs, (1 << log2d, 8))):
            if a is not None and not (isinstance(a, np.ndarray) and a.dtype == np.uint64 and a.flags.c_contiguous and a.flags.writeable and a.shape == shape):
                raise ValueError("vec_update: %s must be a writable contiguous uint64 array of shape %s (it is updated in place)" % (name, shape))
        self._ck(self.lib.keaki_hip_vec_update(self.ctx, srs.handle, log2d, _ptr(_np(omega_d)), _ptr(_np(omega_d_inv)), _ptr(_np(inv_d)),
                                               _ptr(ix) if ix.shape[0] else None, _ptr(dl) if ix.shape[0] else None, ix.shape[0], _ptr(com), _ptr(proofs)))
        return com, proofs

    def vec_update_dev(self, srs: "SrsG1", log2d: int, omega_d, omega_d_inv, inv_d, d_idx: int, d_deltas: int, k: int, d_com: int, d_proofs: int):
        """the same on device-resident arrays (u32 indices, Fr deltas, 96-byte commitment, d x 64-byte proofs; 0 = absent), asynchronous on the ctx stream"""
        vp = lambda p: C.c_void_p(p) if p else None
        self._ck(self.lib.keaki_hip_vec_update_dev(self.ctx, srs.handle, log2d, _ptr(_np(omega_d)), _ptr(_np(omega_d_inv)), _ptr(_np(inv_d)),
                                                   vp(d_idx), vp(d_deltas), k, vp(d_com), vp(d_proofs)))

    def set_timing(self, on: bool):
        self._ck(self.lib.keaki_hip_set_timing(self.ctx, 1 if on else 0))

    def last_msm_stats(self):
        return {"bucket_ms": float(self.lib.keaki_hip_last_msm_bucket_ms(self.ctx)),
                "total_ms": float(self.lib.keaki_hip_last_msm_total_ms(self.ctx)),
                "window_bits": int(self.lib.keaki_hip_last_msm_window_bits(self.ctx))}

    def last_fk_stats(self):
        out = (C.c_float * 3)()
        self._ck(self.lib.keaki_hip_last_fk_ms(self.ctx, out))
        return {"pointwise_ms": float(out[0]), "stages_ms": float(out[1]), "device_ms": float(out[2])}

    def selftest_field(self, blocks: int = 1024, iters: int = 64, seed: int = 1) -> int:
        """mismatch count of the hand-scheduled Fq streams vs the portable code (must be 0)"""
        bad = C.c_uint64(1)
        self._ck(self.lib.keaki_hip_selftest_field(self.ctx, blocks, iters, seed, C.byref(bad)))
        return int(bad.value)

    def field_ops(self, op: int, operands) -> np.ndarray:
        """one shipped field function on host-chosen operands (keaki_hip_selftest_field_ops): operands n x 12 x 9 uint32 -> raw results n x 9 uint32"""
        a = np.ascontiguousarray(operands, dtype=np.uint32).reshape(-1, 12, 9)
        out = np.zeros((a.shape[0], 9), np.uint32)
        self._ck(self.lib.keaki_hip_selftest_field_ops(self.ctx, op, _ptr(a), a.shape[0], _ptr(out)))
        return out

    def tower_ops(self, op: int, operands) -> np.ndarray:
        """one shipped function of the Fq12 tower on host-chosen operands (keaki_hip_selftest_tower_ops): operands n x 344 uint32 -> the twelve result
        words n x 12 x 8 uint32"""
        a = np.ascontiguousarray(operands, dtype=np.uint32).reshape(-1, 344)
        out = np.zeros((a.shape[0], 12, 8), np.uint32)
        self._ck(self.lib.keaki_hip_selftest_tower_ops(self.ctx, op, _ptr(a), a.shape[0], _ptr(out)))
        return out

    def point_ops(self, op: int, operands) -> np.ndarray:
        """one shipped function of the lazy-limb group law on host-chosen operands (keaki_hip_selftest_point_ops): operands n x SLOTS x SLOT_WORDS uint32 ->
        the raw result slots n x OUT_SLOTS x SLOT_WORDS uint32 (flags, return value and `special` in slot OUT_FLAG_SLOT; geometry: point_op_codes())"""
        g = point_op_codes()
        a = np.ascontiguousarray(operands, dtype=np.uint32).reshape(-1, g["SLOTS"], g["SLOT_WORDS"])
        out = np.zeros((a.shape[0], g["OUT_SLOTS"], g["SLOT_WORDS"]), np.uint32)
        self._ck(self.lib.keaki_hip_selftest_point_ops(self.ctx, op, _ptr(a), a.shape[0], _ptr(out)))
        return out

    # ---- SRS
    def srs_g1_upload(self, points) -> SrsG1:
        pts = _np(points, 8); h = C.c_void_p()
        self._ck(self.lib.keaki_hip_srs_g1_upload(self.ctx, _ptr(pts), pts.shape[0], C.byref(h)))
        return SrsG1(self, h, pts.shape[0])

    def srs_g1_wrap_dev(self, dptr: int, n: int) -> SrsG1:
        h = C.c_void_p()
        self._ck(self.lib.keaki_hip_srs_g1_wrap_dev(self.ctx, C.c_void_p(dptr), n, C.byref(h)))
        return SrsG1(self, h, n)

    def srs_g1_slice(self, srs: SrsG1, offset: int, n: int) -> SrsG1:
        """non-owning view of points [offset, offset + n): one rank's chunk of a sharded MSM"""
        h = C.c_void_p()
        self._ck(self.lib.keaki_hip_srs_g1_slice(self.ctx, srs.handle, offset, n, C.byref(h)))
        return SrsG1(self, h, n)

    def srs_g2_upload(self, points) -> SrsG2:
        pts = _np(points, 16); h = C.c_void_p()
        self._ck(self.lib.keaki_hip_srs_g2_upload(self.ctx, _ptr(pts), pts.shape[0], C.byref(h)))
        return SrsG2(self, h, pts.shape[0])

    def srs_g2_wrap_dev(self, dptr: int, n: int) -> SrsG2:
        h = C.c_void_p()
        self._ck(self.lib.keaki_hip_srs_g2_wrap_dev(self.ctx, C.c_void_p(dptr), n, C.byref(h)))
        return SrsG2(self, h, n)

    def srs_g1_precompute(self, srs: "SrsG1") -> int:
        """one-time window-table build for a fixed SRS; returns the table size in bytes"""
        nbytes = C.c_size_t(0)
        self._ck(self.lib.keaki_hip_srs_g1_precompute(self.ctx, srs.handle, C.byref(nbytes)))
        return int(nbytes.value)

    def srs_g2_precompute(self, srs: "SrsG2") -> int:
        nbytes = C.c_size_t(0)
        self._ck(self.lib.keaki_hip_srs_g2_precompute(self.ctx, srs.handle, C.byref(nbytes)))
        return int(nbytes.value)

    # ---- MSM
    def msm_g1(self, srs: SrsG1, scalars) -> np.ndarray:
        sc = _np(scalars, 4); out = np.zeros(12, np.uint64)
        self._ck(self.lib.keaki_hip_msm_g1(self.ctx, srs.handle, _ptr(sc), sc.shape[0], _ptr(out)))
        return out

    def msm_g1_dev(self, srs: SrsG1, d_scalars: int, n: int, d_out: int):
        self._ck(self.lib.keaki_hip_msm_g1_dev(self.ctx, srs.handle, C.c_void_p(d_scalars), n, C.c_void_p(d_out)))

    def msm_g1_batch(self, srs: SrsG1, rows, n: int = None) -> np.ndarray:
        """m MSMs over one SRS in one call (keaki_hip_msm_g1_batch). rows: (m, stride, 4) Montgomery Fr; the first n (default: stride) scalars
        of every row count, the rest of a row is never read -> (m, 12) normalised Jacobian"""
        r = np.ascontiguousarray(rows, dtype=np.uint64)
        r = r if r.ndim == 3 else r.reshape(r.shape[0], -1, 4)
        m, stride = r.shape[0], r.shape[1]
        n = stride if n is None else int(n)
        out = np.zeros((m, 12), np.uint64)
        self._ck(self.lib.keaki_hip_msm_g1_batch(self.ctx, srs.handle, _ptr(r) if r.size else None, n, m, stride, _ptr(out) if m else None))
        return out

    def msm_g1_batch_dev(self, srs: SrsG1, d_rows: int, n: int, m: int, stride: int, d_out: int):
        self._ck(self.lib.keaki_hip_msm_g1_batch_dev(self.ctx, srs.handle, C.c_void_p(d_rows), n, m, stride, C.c_void_p(d_out)))

    def kzg_open_batch(self, srs: SrsG1, rows, points, n: int = None):
        """m openings in one call (keaki_hip_kzg_open_batch): row j (the first n coefficients of it, low degree first, zero-padded) is opened at
        points[j] -> (proofs (m, 12) normalised Jacobian, values (m, 4))"""
        r = np.ascontiguousarray(rows, dtype=np.uint64)
        r = r if r.ndim == 3 else r.reshape(r.shape[0], -1, 4)
        m, stride = r.shape[0], r.shape[1]
        n = stride if n is None else int(n)
        z = _np(points, 4)
        if z.shape[0] != m:
            raise ValueError("kzg_open_batch: one point per row")
        out = np.zeros((m, 12), np.uint64); val = np.zeros((m, 4), np.uint64)
        self._ck(self.lib.keaki_hip_kzg_open_batch(self.ctx, srs.handle, _ptr(r) if r.size else None, n, m, stride, _ptr(z) if m else None,
                                                   _ptr(out) if m else None, _ptr(val) if m else None))
        return out, val

    def kzg_open_batch_dev(self, srs: SrsG1, d_rows: int, n: int, m: int, stride: int, d_points: int, d_proofs: int, d_values: int):
        self._ck(self.lib.keaki_hip_kzg_open_batch_dev(self.ctx, srs.handle, C.c_void_p(d_rows), n, m, stride, C.c_void_p(d_points), C.c_void_p(d_proofs),
                                                       C.c_void_p(d_values) if d_values else None))

    def open_fk_poly_batch(self, srs: SrsG1, log2d: int, rows, omega_2d, omega_2d_inv, inv_2d) -> np.ndarray:
        """all d = 2^log2d FK23 proofs of each of m polynomials in one call (keaki_hip_open_fk_poly_batch). rows: (m, stride, 4) Montgomery Fr,
        the first d coefficients of every row count, the rest of a row is never read -> (m, d, 8) affine proofs in natural order"""
        r = np.ascontiguousarray(rows, dtype=np.uint64)
        r = r if r.ndim == 3 else r.reshape(r.shape[0], -1, 4)
        m, stride, d = r.shape[0], r.shape[1], 1 << log2d
        out = np.zeros((m, d, 8), np.uint64)
        self._ck(self.lib.keaki_hip_open_fk_poly_batch(self.ctx, srs.handle, log2d, _ptr(r) if r.size else None, m, stride, _ptr(_np(omega_2d)),
                                                       _ptr(_np(omega_2d_inv)), _ptr(_np(inv_2d)), _ptr(out) if m else None))
        return out

    def open_fk_poly_batch_dev(self, srs: SrsG1, log2d: int, d_rows: int, m: int, stride: int, omega_2d, omega_2d_inv, inv_2d, d_proofs: int):
        self._ck(self.lib.keaki_hip_open_fk_poly_batch_dev(self.ctx, srs.handle, log2d, C.c_void_p(d_rows), m, stride, _ptr(_np(omega_2d)),
                                                           _ptr(_np(omega_2d_inv)), _ptr(_np(inv_2d)), C.c_void_p(d_proofs)))

    def vec_commit_batch(self, srs: SrsG1, rows, log2d: int, omega_d_inv, inv_d, omega_2d, omega_2d_inv, inv_2d, n: int = None):
        """the body of vec::vec_commit for m vectors over one domain (keaki_hip_vec_commit_batch). rows: (m, stride, 4) Montgomery Fr; the first n
        (default: stride) evaluations of every row count -- the vector, its padding scalar, zeros -- -> (commitments (m, 12) normalised Jacobian,
        proofs (m, d, 8) affine)"""
        r = np.ascontiguousarray(rows, dtype=np.uint64)
        r = r if r.ndim == 3 else r.reshape(r.shape[0], -1, 4)
        m, stride, d = r.shape[0], r.shape[1], 1 << log2d
        n = stride if n is None else int(n)
        com = np.zeros((m, 12), np.uint64); proofs = np.zeros((m, d, 8), np.uint64)
        self._ck(self.lib.keaki_hip_vec_commit_batch(self.ctx, srs.handle, _ptr(r) if r.size and n else None, n, m, stride, log2d, _ptr(_np(omega_d_inv)),
                                                     _ptr(_np(inv_d)), _ptr(_np(omega_2d)), _ptr(_np(omega_2d_inv)), _ptr(_np(inv_2d)),
                                                     _ptr(com) if m else None, _ptr(proofs) if m else None))
        return com, proofs

    def vec_commit_batch_dev(self, srs: SrsG1, d_rows: int, n: int, m: int, stride: int, log2d: int, omega_d_inv, inv_d, omega_2d, omega_2d_inv, inv_2d,
                             d_com: int, d_proofs: int):
        self._ck(self.lib.keaki_hip_vec_commit_batch_dev(self.ctx, srs.handle, C.c_void_p(d_rows) if d_rows else None, n, m, stride, log2d,
                                                         _ptr(_np(omega_d_inv)), _ptr(_np(inv_d)), _ptr(_np(omega_2d)), _ptr(_np(omega_2d_inv)),
                                                         _ptr(_np(inv_2d)), C.c_void_p(d_com), C.c_void_p(d_proofs)))

    def msm_g2(self, srs: SrsG2, scalars) -> np.ndarray:
        sc = _np(scalars, 4); out = np.zeros(24, np.uint64)
        self._ck(self.lib.keaki_hip_msm_g2(self.ctx, srs.handle, _ptr(sc), sc.shape[0], _ptr(out)))
        return out

    def msm_g2_dev(self, srs: SrsG2, d_scalars: int, n: int, d_out: int):
        self._ck(self.lib.keaki_hip_msm_g2_dev(self.ctx, srs.handle, C.c_void_p(d_scalars), n, C.c_void_p(d_out)))

    def g1_sum(self, points_jac) -> np.ndarray:
        p = _np(points_jac, 12); out = np.zeros(12, np.uint64)
        self._ck(self.lib.keaki_hip_g1_sum(self.ctx, _ptr(p), p.shape[0], _ptr(out)))
        return out

    def g1_sum_dev(self, d_points: int, k: int, d_out: int):
        self._ck(self.lib.keaki_hip_g1_sum_dev(self.ctx, C.c_void_p(d_points), k, C.c_void_p(d_out)))

    # ---- batched scalar multiplication
    def g1_mul_batch(self, points, scalars) -> np.ndarray:
        pts = _np(points); sc = _np(scalars, 4); n = sc.shape[0]
        stride = 0 if pts.size == 8 else 1
        out = np.zeros((n, 8), np.uint64)
        self._ck(self.lib.keaki_hip_g1_mul_batch(self.ctx, _ptr(pts), stride, _ptr(sc), n, _ptr(out)))
        return out

    def g2_mul_batch(self, points, scalars) -> np.ndarray:
        pts = _np(points); sc = _np(scalars, 4); n = sc.shape[0]
        stride = 0 if pts.size == 16 else 1
        out = np.zeros((n, 16), np.uint64)
        self._ck(self.lib.keaki_hip_g2_mul_batch(self.ctx, _ptr(pts), stride, _ptr(sc), n, _ptr(out)))
        return out

    def g1_mul_batch_dev(self, d_points: int, stride: int, d_scalars: int, n: int, d_out: int):
        self._ck(self.lib.keaki_hip_g1_mul_batch_dev(self.ctx, C.c_void_p(d_points), stride, C.c_void_p(d_scalars), n, C.c_void_p(d_out)))

    def g2_mul_batch_dev(self, d_points: int, stride: int, d_scalars: int, n: int, d_out: int):
        self._ck(self.lib.keaki_hip_g2_mul_batch_dev(self.ctx, C.c_void_p(d_points), stride, C.c_void_p(d_scalars), n, C.c_void_p(d_out)))

    # ---- pairing
    def pairing_batch(self, g1, g2) -> np.ndarray:
        p = _np(g1, 8); q = _np(g2); n = p.shape[0]
        stride = 0 if q.size == 16 else 1
        out = np.zeros((n, 384), np.uint8)
        self._ck(self.lib.keaki_hip_pairing_batch(self.ctx, _ptr(p), _ptr(q), stride, n, _ptr(out)))
        return out

    def pairing_batch_dev(self, d_g1: int, d_g2: int, stride: int, n: int, d_gt: int):
        self._ck(self.lib.keaki_hip_pairing_batch_dev(self.ctx, C.c_void_p(d_g1), C.c_void_p(d_g2), stride, n, C.c_void_p(d_gt)))

    def g2_prepare(self, g2) -> np.ndarray:
        """line table of a fixed Q: (96, 2 parities, 3 coefficients, 4 limbs) Montgomery"""
        q = _np(g2); out = np.zeros(96 * 2 * 3 * 4, np.uint64)
        self.lib.keaki_hip_g2_prepare.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        self._ck(self.lib.keaki_hip_g2_prepare(self.ctx, _ptr(q), _ptr(out), out.nbytes))
        return out.reshape(96, 2, 3, 4)

    def miller_loop_batch(self, g1, g2) -> np.ndarray:
        p = _np(g1, 8); q = _np(g2, 16); n = p.shape[0]
        out = np.zeros((n, 48), np.uint64)
        self._ck(self.lib.keaki_hip_miller_loop_batch(self.ctx, _ptr(p), _ptr(q), n, _ptr(out)))
        return out

    def final_exp_batch(self, f_mont) -> np.ndarray:
        f = _np(f_mont, 48); n = f.shape[0]
        out = np.zeros((n, 384), np.uint8)
        self._ck(self.lib.keaki_hip_final_exp_batch(self.ctx, _ptr(f), n, _ptr(out)))
        return out

    def kzg_open(self, srs: "SrsG1", coeffs, point):
        """-> (proof as normalised Jacobian u64[12], p(point) u64[4])"""
        c = _np(coeffs, 4)
        out = np.zeros(12, np.uint64); val = np.zeros(4, np.uint64)
        self._ck(self.lib.keaki_hip_kzg_open(self.ctx, srs.handle, _ptr(c) if c.shape[0] else None, c.shape[0], _ptr(_np(point)), _ptr(out), _ptr(val)))
        return out, val

    # ---- KZG set openings: one proof for k DISTINCT points (the library does not look for repeated points: the caller's contract) ----
    SET_MAX = 1024

    def kzg_set_polys(self, points, values=None):
        """-> (Z: k + 1 Fr, monic, low degree first; weights 1 / Z'(z_j): k Fr; I: k Fr, the interpolant of (points, values), or None without values)"""
        z = _np(points, 4); k = z.shape[0]
        y = _np(values, 4) if values is not None else None
        if y is not None and y.shape[0] != k:
            raise ValueError("kzg_set_polys: %d points but %d values" % (k, y.shape[0]))
        zc = np.zeros((k + 1, 4), np.uint64); w = np.zeros((k, 4), np.uint64)
        ic = np.zeros((k, 4), np.uint64) if y is not None else None
        self._ck(self.lib.keaki_hip_kzg_set_polys(self.ctx, _ptr(z) if k else None, _ptr(y), k, _ptr(zc), _ptr(w), _ptr(ic)))
        return zc, w, ic

    def kzg_set_polys_dev(self, d_points: int, d_values: int, k: int, d_z_coeffs: int, d_weights: int, d_i_coeffs: int):
        self._ck(self.lib.keaki_hip_kzg_set_polys_dev(self.ctx, C.c_void_p(d_points), C.c_void_p(d_values), k, C.c_void_p(d_z_coeffs), C.c_void_p(d_weights),
                                                      C.c_void_p(d_i_coeffs)))

    def kzg_open_multi(self, srs: "SrsG1", coeffs, points):
        """ONE proof for the k points (keaki_hip_kzg_open_multi) -> (proof as normalised Jacobian u64[12], the k values p(z_j))"""
        c = _np(coeffs, 4); z = _np(points, 4); k = z.shape[0]
        out = np.zeros(12, np.uint64); val = np.zeros((k, 4), np.uint64)
        self._ck(self.lib.keaki_hip_kzg_open_multi(self.ctx, srs.handle, _ptr(c) if c.shape[0] else None, c.shape[0], _ptr(z) if k else None, k, _ptr(out),
                                                   _ptr(val)))
        return out, val

    def kzg_open_multi_dev(self, srs: "SrsG1", d_coeffs: int, n: int, d_points: int, k: int, d_proof: int, d_values: int):
        self._ck(self.lib.keaki_hip_kzg_open_multi_dev(self.ctx, srs.handle, C.c_void_p(d_coeffs), n, C.c_void_p(d_points), k, C.c_void_p(d_proof),
                                                       C.c_void_p(d_values)))

    def kzg_aggregate(self, points, proofs_aff) -> np.ndarray:
        """the set proof from the k single proofs at the k points, without the polynomial -> normalised Jacobian u64[12]"""
        z = _np(points, 4); pr = _np(proofs_aff, 8); k = z.shape[0]
        if pr.shape[0] != k:
            raise ValueError("kzg_aggregate: %d points but %d proofs" % (k, pr.shape[0]))
        out = np.zeros(12, np.uint64)
        self._ck(self.lib.keaki_hip_kzg_aggregate(self.ctx, _ptr(z) if k else None, _ptr(pr) if k else None, k, _ptr(out)))
        return out

    def kzg_aggregate_dev(self, d_points: int, d_proofs_aff: int, k: int, d_proof: int):
        self._ck(self.lib.keaki_hip_kzg_aggregate_dev(self.ctx, C.c_void_p(d_points), C.c_void_p(d_proofs_aff), k, C.c_void_p(d_proof)))

    def kzg_verify_multi(self, srs_g1: "SrsG1", srs_g2: "SrsG2", com_aff, points, values, proof_aff, want_pair: bool = False):
        """e(C - [I(tau)]_1, g2) == e(proof, [Z(tau)]_2) (keaki_hip_kzg_verify_multi; srs_g2 holds [tau^i]_2) -> ok, or (ok, C - [I]_1 u64[8],
        [Z]_2 u64[16]) with want_pair"""
        z = _np(points, 4); y = _np(values, 4); k = z.shape[0]
        if y.shape[0] != k:
            raise ValueError("kzg_verify_multi: %d points but %d values" % (k, y.shape[0]))
        ok = C.c_int32(0); pair = np.zeros(24, np.uint64)
        self._ck(self.lib.keaki_hip_kzg_verify_multi(self.ctx, srs_g1.handle, srs_g2.handle, _ptr(_np(com_aff)), _ptr(z) if k else None, _ptr(y) if k else None,
                                                     k, _ptr(_np(proof_aff)), C.byref(ok), _ptr(pair) if want_pair else None))
        return (bool(ok.value), pair[:8].copy(), pair[8:].copy()) if want_pair else bool(ok.value)

    def kzg_verify(self, com_aff, tau_g2_aff, point, value, proof_aff) -> bool:
        """src/kzg.rs:127-146 on the device (affine Montgomery points, Montgomery Fr)"""
        ok = C.c_int32(0)
        self._ck(self.lib.keaki_hip_kzg_verify(self.ctx, _ptr(_np(com_aff)), _ptr(_np(tau_g2_aff)), _ptr(_np(point)), _ptr(_np(value)),
                                               _ptr(_np(proof_aff)), C.byref(ok)))
        return bool(ok.value)

    def kzg_verify_batch(self, com_aff, tau_g2_aff, points, values, proofs_aff, gammas, point_mode: int = 0):
        """n openings in one call (keaki_hip_kzg_verify_batch) -> (ok, L u64[8], R u64[8]). com_aff: one affine point (u64[8]: the commitment of
        every item) or n of them; points: n Fr, or with point_mode = 1 the ONE Fr omega (item i is opened at omega^i); gammas: n Fr the CALLER drew"""
        v = _np(values, 4); n = v.shape[0]
        pr, g, c, z = _np(proofs_aff, 8), _np(gammas, 4), _np(com_aff, 8), _np(points, 4)
        com_stride = 0 if c.shape[0] == 1 else 1
        if pr.shape[0] != n or g.shape[0] != n or (com_stride and c.shape[0] != n) or z.shape[0] != (1 if point_mode else n):
            raise ValueError("kzg_verify_batch: array lengths disagree")
        ok = C.c_int32(0); sums = np.zeros(16, np.uint64)
        self._ck(self.lib.keaki_hip_kzg_verify_batch(self.ctx, _ptr(c), com_stride, _ptr(_np(tau_g2_aff)), _ptr(z), int(point_mode), _ptr(v), _ptr(pr), _ptr(g),
                                                     n, C.byref(ok), _ptr(sums)))
        return bool(ok.value), sums[:8].copy(), sums[8:].copy()

    def kzg_verify_batch_dev(self, d_com, com_stride: int, d_tau_g2, d_points, point_mode: int, d_values, d_proofs, d_gammas, n: int):
        """the same with every array resident: device pointers (ints) or torch tensors -> (ok, L, R) on the host (the call synchronises)"""
        dp = lambda x: C.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else x)
        ok = C.c_int32(0); sums = np.zeros(16, np.uint64)
        self._ck(self.lib.keaki_hip_kzg_verify_batch_dev(self.ctx, dp(d_com), int(com_stride), dp(d_tau_g2), dp(d_points), int(point_mode), dp(d_values),
                                                         dp(d_proofs), dp(d_gammas), int(n), C.byref(ok), _ptr(sums)))
        return bool(ok.value), sums[:8].copy(), sums[8:].copy()

    def kzg_verify_cosets(self, srs_g1: "SrsG1", com_aff, tau_l_g2_aff, points, values, item_stride: int, t_stride: int, log2l: int, omega_l_inv, inv_l,
                          proofs_aff, gammas, point_mode: int = 0):
        """n set proofs over cosets of size l = 2^log2l in one call (keaki_hip_kzg_verify_cosets) -> (ok, L u64[8], R u64[8]). com_aff: one affine
        point or n of them; points: the n shifts h_k, or with point_mode = 1 the ONE Fr omega (h_k = omega^k); values: a flat Fr array in which value
        (k, t) is entry k * item_stride + t * t_stride -- rows: (l, 1); a vector in domain order: (1, n); tau_l_g2_aff: [tau^l]_2; gammas: n Fr
        the CALLER drew"""
        pr, g, c, z, v = _np(proofs_aff, 8), _np(gammas, 4), _np(com_aff, 8), _np(points, 4), _np(values, 4)
        n = g.shape[0]
        com_stride = 0 if c.shape[0] == 1 else 1
        if pr.shape[0] != n or (com_stride and c.shape[0] != n) or z.shape[0] != (1 if point_mode else n):
            raise ValueError("kzg_verify_cosets: array lengths disagree")
        if n and 0 <= log2l < 32 and v.shape[0] < (n - 1) * int(item_stride) + ((1 << log2l) - 1) * int(t_stride) + 1:
            raise ValueError("kzg_verify_cosets: the strides reach past the %d values given" % v.shape[0])
        ok = C.c_int32(0); sums = np.zeros(16, np.uint64)
        self._ck(self.lib.keaki_hip_kzg_verify_cosets(self.ctx, srs_g1.handle, _ptr(c), com_stride, _ptr(_np(tau_l_g2_aff)), _ptr(z), int(point_mode), _ptr(v),
                                                      int(item_stride), int(t_stride), int(log2l), _ptr(_np(omega_l_inv)), _ptr(_np(inv_l)), _ptr(pr), _ptr(g), n,
                                                      C.byref(ok), _ptr(sums)))
        return bool(ok.value), sums[:8].copy(), sums[8:].copy()

    def kzg_verify_cosets_dev(self, srs_g1: "SrsG1", d_com, com_stride: int, d_tau_l_g2, d_points, point_mode: int, d_values, item_stride: int, t_stride: int,
                              log2l: int, omega_l_inv, inv_l, d_proofs, d_gammas, n: int):
        """the same with every array resident: device pointers (ints) or torch tensors; omega_l_inv and inv_l stay host arrays -> (ok, L, R) on the
        host (the call synchronises). The caller answers for the extent of d_values under the strides"""
        dp = lambda x: C.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else x)
        ok = C.c_int32(0); sums = np.zeros(16, np.uint64)
        self._ck(self.lib.keaki_hip_kzg_verify_cosets_dev(self.ctx, srs_g1.handle, dp(d_com), int(com_stride), dp(d_tau_l_g2), dp(d_points), int(point_mode),
                                                          dp(d_values), int(item_stride), int(t_stride), int(log2l), _ptr(_np(omega_l_inv)), _ptr(_np(inv_l)),
                                                          dp(d_proofs), dp(d_gammas), int(n), C.byref(ok), _ptr(sums)))
        return bool(ok.value), sums[:8].copy(), sums[8:].copy()

    VERIFY_SETS_K_MAX = 64

    def kzg_verify_sets(self, srs_g1: "SrsG1", srs_g2: "SrsG2", com_aff, points, values, k: int, proofs_aff, gammas, item_stride: int = None, omega=None):
        """n set proofs over arbitrary sets of k points in one call (keaki_hip_kzg_verify_sets) -> (ok, sums u64[k + 1, 8]: L, then R_1 .. R_k).
        com_aff: one affine point or n of them; points: a flat Fr array in which point (i, j) is entry i * item_stride + j (item_stride defaults to
        k), or -- with omega, ONE Fr -- a flat uint32 array of domain indices at the same offsets (point_mode 1: z = omega^idx); values: a flat Fr
        array addressed the same way; srs_g2 holds [tau^t]_2; gammas: n Fr the CALLER drew"""
        pr, g, c, v = _np(proofs_aff, 8), _np(gammas, 4), _np(com_aff, 8), _np(values, 4)
        n, k = g.shape[0], int(k)
        stride = k if item_stride is None else int(item_stride)
        point_mode = 0 if omega is None else 1
        z = np.ascontiguousarray(points, np.uint32).reshape(-1) if point_mode else _np(points, 4)
        com_stride = 0 if c.shape[0] == 1 else 1
        if pr.shape[0] != n or (com_stride and c.shape[0] != n):
            raise ValueError("kzg_verify_sets: array lengths disagree")
        if n and stride >= k >= 1 and min(z.shape[0], v.shape[0]) < (n - 1) * stride + k:
            raise ValueError("kzg_verify_sets: the stride reaches past the %d points / %d values given" % (z.shape[0], v.shape[0]))
        ok = C.c_int32(0); sums = np.zeros((max(k, 0) + 1, 8), np.uint64)
        self._ck(self.lib.keaki_hip_kzg_verify_sets(self.ctx, srs_g1.handle, srs_g2.handle, _ptr(c), com_stride, _ptr(z), point_mode,
                                                    _ptr(_np(omega)) if point_mode else None, _ptr(v), stride, k, _ptr(pr), _ptr(g), n, C.byref(ok), _ptr(sums)))
        return bool(ok.value), sums

    def kzg_verify_sets_dev(self, srs_g1: "SrsG1", srs_g2: "SrsG2", d_com, com_stride: int, d_points, point_mode: int, omega, d_values, item_stride: int,
                            k: int, d_proofs, d_gammas, n: int):
        """the same with every array resident: device pointers (ints) or torch tensors; omega stays a host array (None in point_mode 0) -> (ok, sums)
        on the host (the call synchronises). The caller answers for the extent of d_points and d_values under the stride"""
        dp = lambda x: C.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else x)
        ok = C.c_int32(0); sums = np.zeros((max(int(k), 0) + 1, 8), np.uint64)
        self._ck(self.lib.keaki_hip_kzg_verify_sets_dev(self.ctx, srs_g1.handle, srs_g2.handle, dp(d_com), int(com_stride), dp(d_points), int(point_mode),
                                                        _ptr(_np(omega)) if omega is not None else None, dp(d_values), int(item_stride), int(k), dp(d_proofs),
                                                        dp(d_gammas), int(n), C.byref(ok), _ptr(sums)))
        return bool(ok.value), sums

    def pairing_product(self, g1, g2) -> np.ndarray:
        """serialize_uncompressed(prod_i e(g1[i], g2[i])): n Miller loops, a GT product tree, ONE final exponentiation -> uint8[384]"""
        p = _np(g1, 8); q = _np(g2, 16); n = p.shape[0]
        if q.shape[0] != n:
            raise ValueError("pairing_product: %d G1 points but %d G2 points" % (n, q.shape[0]))
        out = np.zeros(384, np.uint8)
        self._ck(self.lib.keaki_hip_pairing_product(self.ctx, _ptr(p) if n else None, _ptr(q) if n else None, n, _ptr(out)))
        return out

    def pairing_product_dev(self, d_g1, d_g2, n: int, d_gt):
        dp = lambda x: C.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else x)
        self._ck(self.lib.keaki_hip_pairing_product_dev(self.ctx, dp(d_g1), dp(d_g2), int(n), dp(d_gt)))

    def srs_g1_precompute_cosets(self, srs: "SrsG1", log2l: int):
        """builds the handle's window table over its first l = 2^log2l points ahead of the first kzg_coset_pairs / kzg_verify_cosets_each call
        (keaki_hip_srs_g1_precompute_cosets); results never depend on it"""
        self._ck(self.lib.keaki_hip_srs_g1_precompute_cosets(self.ctx, srs.handle, int(log2l)))

    def kzg_coset_pairs(self, srs_g1: "SrsG1", com_aff, points, values, item_stride: int, t_stride: int, log2l: int, omega_l_inv, inv_l, n: int,
                        point_mode: int = 0):
        """the per-item points of the coset check (keaki_hip_kzg_coset_pairs) -> (A u64[n, 8], c u64[n, 4]): A_k = C_k - [I_k(tau)]_1 and c_k = h_k^l.
        Arguments as kzg_verify_cosets; n is explicit because with point_mode = 1 and one commitment no array carries it"""
        c, z, v = _np(com_aff, 8), _np(points, 4), _np(values, 4)
        n = int(n)
        com_stride = 0 if c.shape[0] == 1 else 1
        if (com_stride and c.shape[0] != n) or z.shape[0] != (1 if point_mode else n):
            raise ValueError("kzg_coset_pairs: array lengths disagree")
        if n and 0 <= log2l < 32 and v.shape[0] < (n - 1) * int(item_stride) + ((1 << log2l) - 1) * int(t_stride) + 1:
            raise ValueError("kzg_coset_pairs: the strides reach past the %d values given" % v.shape[0])
        lhs = np.zeros((n, 8), np.uint64); cs = np.zeros((n, 4), np.uint64)
        self._ck(self.lib.keaki_hip_kzg_coset_pairs(self.ctx, srs_g1.handle, _ptr(c), com_stride, _ptr(z), int(point_mode), _ptr(v), int(item_stride),
                                                    int(t_stride), int(log2l), _ptr(_np(omega_l_inv)), _ptr(_np(inv_l)), n, _ptr(lhs), _ptr(cs)))
        return lhs, cs

    def kzg_coset_pairs_dev(self, srs_g1: "SrsG1", d_com, com_stride: int, d_points, point_mode: int, d_values, item_stride: int, t_stride: int, log2l: int,
                            omega_l_inv, inv_l, n: int, d_lhs_out, d_c_out):
        """the same with every array resident: device pointers (ints) or torch tensors; omega_l_inv and inv_l stay host arrays. Asynchronous on the
        context's stream. The caller answers for the extent of d_values under the strides"""
        dp = lambda x: C.c_void_p(None if x is None else (x.data_ptr() if hasattr(x, "data_ptr") else x))
        self._ck(self.lib.keaki_hip_kzg_coset_pairs_dev(self.ctx, srs_g1.handle, dp(d_com), int(com_stride), dp(d_points), int(point_mode), dp(d_values),
                                                        int(item_stride), int(t_stride), int(log2l), _ptr(_np(omega_l_inv)), _ptr(_np(inv_l)), int(n),
                                                        dp(d_lhs_out), dp(d_c_out)))

    def kzg_verify_cosets_each(self, srs_g1: "SrsG1", com_aff, tau_l_g2_aff, points, values, item_stride: int, t_stride: int, log2l: int, omega_l_inv, inv_l,
                               proofs_aff, point_mode: int = 0, want_lhs: bool = False):
        """one verdict per coset (keaki_hip_kzg_verify_cosets_each) -> (status uint8[n]: 0 valid / 1 invalid, n_bad, first_bad or None), and with
        want_lhs a fourth element: the L_k = A_k + c_k proof_k (u64[n, 8]). Arguments as kzg_verify_cosets, without gammas"""
        pr, c, z, v = _np(proofs_aff, 8), _np(com_aff, 8), _np(points, 4), _np(values, 4)
        n = pr.shape[0]
        com_stride = 0 if c.shape[0] == 1 else 1
        if (com_stride and c.shape[0] != n) or z.shape[0] != (1 if point_mode else n):
            raise ValueError("kzg_verify_cosets_each: array lengths disagree")
        if n and 0 <= log2l < 32 and v.shape[0] < (n - 1) * int(item_stride) + ((1 << log2l) - 1) * int(t_stride) + 1:
            raise ValueError("kzg_verify_cosets_each: the strides reach past the %d values given" % v.shape[0])
        status = np.zeros(n, np.uint8); lhs = np.zeros((n, 8), np.uint64) if want_lhs else None
        bad, first = C.c_uint64(0), C.c_uint64(0)
        self._ck(self.lib.keaki_hip_kzg_verify_cosets_each(self.ctx, srs_g1.handle, _ptr(c), com_stride, _ptr(_np(tau_l_g2_aff)), _ptr(z), int(point_mode), _ptr(v),
                                                           int(item_stride), int(t_stride), int(log2l), _ptr(_np(omega_l_inv)), _ptr(_np(inv_l)), _ptr(pr), n,
                                                           _ptr(status), C.byref(bad), C.byref(first), _ptr(lhs) if want_lhs else None))
        res = (status, bad.value, (None if bad.value == 0 else first.value))
        return res + (lhs,) if want_lhs else res

    def kzg_verify_cosets_each_dev(self, srs_g1: "SrsG1", d_com, com_stride: int, d_tau_l_g2, d_points, point_mode: int, d_values, item_stride: int,
                                   t_stride: int, log2l: int, omega_l_inv, inv_l, d_proofs, n: int, d_status, d_lhs=None):
        """the same with every array resident; the status bytes (and the L_k) stay on the device -> (n_bad, first_bad or None) on the host (the
        call synchronises)"""
        dp = lambda x: C.c_void_p(None if x is None else (x.data_ptr() if hasattr(x, "data_ptr") else x))
        bad, first = C.c_uint64(0), C.c_uint64(0)
        self._ck(self.lib.keaki_hip_kzg_verify_cosets_each_dev(self.ctx, srs_g1.handle, dp(d_com), int(com_stride), dp(d_tau_l_g2), dp(d_points), int(point_mode),
                                                               dp(d_values), int(item_stride), int(t_stride), int(log2l), _ptr(_np(omega_l_inv)),
                                                               _ptr(_np(inv_l)), dp(d_proofs), int(n), dp(d_status), C.byref(bad), C.byref(first), dp(d_lhs)))
        return bad.value, (None if bad.value == 0 else first.value)

    def srs_g2_precompute_sets(self, srs: "SrsG2", k_max: int):
        """builds the G2 handle's window table over its first k_max points ahead of the first kzg_set_pairs / kzg_verify_sets_each call
        (keaki_hip_srs_g2_precompute_sets); results never depend on it"""
        self._ck(self.lib.keaki_hip_srs_g2_precompute_sets(self.ctx, srs.handle, int(k_max)))

    def _set_items(self, what, com_aff, points, values, k, n, item_stride, omega):
        c, v = _np(com_aff, 8), _np(values, 4)
        n, k = int(n), int(k)
        stride = k if item_stride is None else int(item_stride)
        point_mode = 0 if omega is None else 1
        z = np.ascontiguousarray(points, np.uint32).reshape(-1) if point_mode else _np(points, 4)
        com_stride = 0 if c.shape[0] == 1 else 1
        if com_stride and c.shape[0] != n:
            raise ValueError("%s: array lengths disagree" % what)
        if n and stride >= k >= 1 and min(z.shape[0], v.shape[0]) < (n - 1) * stride + k:
            raise ValueError("%s: the stride reaches past the %d points / %d values given" % (what, z.shape[0], v.shape[0]))
        return c, com_stride, z, point_mode, (_ptr(_np(omega)) if point_mode else None), v, stride, k, n

    def kzg_set_pairs(self, srs_g1: "SrsG1", srs_g2: "SrsG2", com_aff, points, values, k: int, n: int, item_stride: int = None, omega=None):
        """the per-item points of the set check over arbitrary point sets (keaki_hip_kzg_set_pairs) -> (A u64[n, 8], Z2 u64[n, 16]): A_i = C_i - [I_i(tau)]_1
        and Z2_i = [Z_i(tau)]_2. Arguments as kzg_verify_sets, without proofs and gammas; n is explicit because with one commitment no array carries it"""
        c, com_stride, z, point_mode, om, v, stride, k, n = self._set_items("kzg_set_pairs", com_aff, points, values, k, n, item_stride, omega)
        lhs = np.zeros((n, 8), np.uint64); z2 = np.zeros((n, 16), np.uint64)
        self._ck(self.lib.keaki_hip_kzg_set_pairs(self.ctx, srs_g1.handle, srs_g2.handle, _ptr(c), com_stride, _ptr(z), point_mode, om, _ptr(v), stride, k, n,
                                                  _ptr(lhs), _ptr(z2)))
        return lhs, z2

    def kzg_set_pairs_dev(self, srs_g1: "SrsG1", srs_g2: "SrsG2", d_com, com_stride: int, d_points, point_mode: int, omega, d_values, item_stride: int, k: int,
                          n: int, d_lhs_out, d_z2_out):
        """the same with every array resident: device pointers (ints) or torch tensors; omega stays a host array (None in point_mode 0). Asynchronous on
        the context's stream. The caller answers for the extent of d_points and d_values under the stride"""
        dp = lambda x: C.c_void_p(None if x is None else (x.data_ptr() if hasattr(x, "data_ptr") else x))
        self._ck(self.lib.keaki_hip_kzg_set_pairs_dev(self.ctx, srs_g1.handle, srs_g2.handle, dp(d_com), int(com_stride), dp(d_points), int(point_mode),
                                                      _ptr(_np(omega)) if omega is not None else None, dp(d_values), int(item_stride), int(k), int(n),
                                                      dp(d_lhs_out), dp(d_z2_out)))

    def kzg_verify_sets_each(self, srs_g1: "SrsG1", srs_g2: "SrsG2", com_aff, points, values, k: int, proofs_aff, item_stride: int = None, omega=None,
                             want_pairs: bool = False):
        """one verdict per set proof over arbitrary point sets (keaki_hip_kzg_verify_sets_each) -> (status uint8[n]: 0 valid / 1 invalid, n_bad, first_bad
        or None), and with want_pairs two more elements: A (u64[n, 8]) and Z2 (u64[n, 16]). Arguments as kzg_verify_sets, without gammas"""
        pr = _np(proofs_aff, 8)
        c, com_stride, z, point_mode, om, v, stride, k, n = self._set_items("kzg_verify_sets_each", com_aff, points, values, k, pr.shape[0], item_stride, omega)
        status = np.zeros(n, np.uint8)
        lhs = np.zeros((n, 8), np.uint64) if want_pairs else None
        z2 = np.zeros((n, 16), np.uint64) if want_pairs else None
        bad, first = C.c_uint64(0), C.c_uint64(0)
        self._ck(self.lib.keaki_hip_kzg_verify_sets_each(self.ctx, srs_g1.handle, srs_g2.handle, _ptr(c), com_stride, _ptr(z), point_mode, om, _ptr(v), stride, k,
                                                         _ptr(pr), n, _ptr(status), C.byref(bad), C.byref(first), _ptr(lhs) if want_pairs else None,
                                                         _ptr(z2) if want_pairs else None))
        res = (status, bad.value, (None if bad.value == 0 else first.value))
        return res + (lhs, z2) if want_pairs else res

    def kzg_verify_sets_each_dev(self, srs_g1: "SrsG1", srs_g2: "SrsG2", d_com, com_stride: int, d_points, point_mode: int, omega, d_values, item_stride: int,
                                 k: int, d_proofs, n: int, d_status, d_lhs=None, d_z2=None):
        """the same with every array resident; the status bytes (and the pairs) stay on the device -> (n_bad, first_bad or None) on the host (the call
        synchronises)"""
        dp = lambda x: C.c_void_p(None if x is None else (x.data_ptr() if hasattr(x, "data_ptr") else x))
        bad, first = C.c_uint64(0), C.c_uint64(0)
        self._ck(self.lib.keaki_hip_kzg_verify_sets_each_dev(self.ctx, srs_g1.handle, srs_g2.handle, dp(d_com), int(com_stride), dp(d_points), int(point_mode),
                                                             _ptr(_np(omega)) if omega is not None else None, dp(d_values), int(item_stride), int(k),
                                                             dp(d_proofs), int(n), dp(d_status), C.byref(bad), C.byref(first), dp(d_lhs), dp(d_z2)))
        return bad.value, (None if bad.value == 0 else first.value)

    def kzg_verify_each(self, com_aff, tau_g2_aff, points, values, proofs_aff, point_mode: int = 0, want_lhs: bool = False):
        """one verdict per opening (keaki_hip_kzg_verify_each) -> (status uint8[n]: 0 valid / 1 invalid, n_bad, first_bad or None), and with
        want_lhs a fourth element: the L_i = C_i - y_i g1 + z_i proof_i (u64[n, 8]). Arguments as kzg_verify_batch, without gammas"""
        v = _np(values, 4); n = v.shape[0]
        pr, c, z = _np(proofs_aff, 8), _np(com_aff, 8), _np(points, 4)
        com_stride = 0 if c.shape[0] == 1 else 1
        if pr.shape[0] != n or (com_stride and c.shape[0] != n) or z.shape[0] != (1 if point_mode else n):
            raise ValueError("kzg_verify_each: array lengths disagree")
        status = np.zeros(n, np.uint8); lhs = np.zeros((n, 8), np.uint64) if want_lhs else None
        bad, first = C.c_uint64(0), C.c_uint64(0)
        self._ck(self.lib.keaki_hip_kzg_verify_each(self.ctx, _ptr(c), com_stride, _ptr(_np(tau_g2_aff)), _ptr(z), int(point_mode), _ptr(v), _ptr(pr), n,
                                                    _ptr(status), C.byref(bad), C.byref(first), _ptr(lhs) if want_lhs else None))
        res = (status, bad.value, (None if bad.value == 0 else first.value))
        return res + (lhs,) if want_lhs else res

    def kzg_verify_each_dev(self, d_com, com_stride: int, d_tau_g2, d_points, point_mode: int, d_values, d_proofs, n: int, d_status, d_lhs=None):
        """the same with every array resident: device pointers (ints) or torch tensors; the status bytes (and the L_i) stay on the device ->
        (n_bad, first_bad or None) on the host (the call synchronises)"""
        dp = lambda x: C.c_void_p(None if x is None else (x.data_ptr() if hasattr(x, "data_ptr") else x))
        bad, first = C.c_uint64(0), C.c_uint64(0)
        self._ck(self.lib.keaki_hip_kzg_verify_each_dev(self.ctx, dp(d_com), int(com_stride), dp(d_tau_g2), dp(d_points), int(point_mode), dp(d_values),
                                                        dp(d_proofs), int(n), dp(d_status), C.byref(bad), C.byref(first), dp(d_lhs)))
        return bad.value, (None if bad.value == 0 else first.value)

    def srs_g1_check(self, srs: "SrsG1"):
        """-> (number of off-curve points, index of the first or None)"""
        bad, first = C.c_uint64(0), C.c_uint64(0)
        self._ck(self.lib.keaki_hip_srs_g1_check(self.ctx, srs.handle, C.byref(bad), C.byref(first)))
        return bad.value, (None if bad.value == 0 else first.value)

    def g2_check(self, points):
        pts = _np(points, 16)
        bad, first = C.c_uint64(0), C.c_uint64(0)
        self._ck(self.lib.keaki_hip_g2_check(self.ctx, _ptr(pts), pts.shape[0], C.byref(bad), C.byref(first)))
        return bad.value, (None if bad.value == 0 else first.value)

    # ---- compressed point wire format (ark-serialize `serialize_compressed`: 32 B per G1 point, 64 B per G2 point) ----
    def _compress(self, points, g2: bool) -> np.ndarray:
        pts = _np(points, 16 if g2 else 8); n = pts.shape[0]
        out = np.zeros((n, 64 if g2 else 32), np.uint8)
        self._ck((self.lib.keaki_hip_g2_compress if g2 else self.lib.keaki_hip_g1_compress)(self.ctx, _ptr(pts), n, _ptr(out)))
        return out

    def g1_compress(self, points_aff) -> np.ndarray:
        """n affine G1 points (u64[n, 8], Montgomery limbs, zeros = identity) -> uint8[n, 32]"""
        return self._compress(points_aff, False)

    def g2_compress(self, points_aff) -> np.ndarray:
        """n affine G2 points (u64[n, 16]) -> uint8[n, 64]"""
        return self._compress(points_aff, True)

    def _decompress(self, data, g2: bool, check_subgroup):
        wire = 64 if g2 else 32
        b = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1, wire); n = b.shape[0]
        out = np.zeros((n, 16 if g2 else 8), np.uint64); status = np.zeros(n, np.uint8)
        bad, first = C.c_uint64(0), C.c_uint64(0)
        if g2:
            self._ck(self.lib.keaki_hip_g2_decompress(self.ctx, _ptr(b), n, int(check_subgroup), _ptr(out), _ptr(status), C.byref(bad), C.byref(first)))
        else:
            self._ck(self.lib.keaki_hip_g1_decompress(self.ctx, _ptr(b), n, _ptr(out), _ptr(status), C.byref(bad), C.byref(first)))
        return out, status, bad.value, (None if bad.value == 0 else first.value)

    def g1_decompress(self, data):
        """uint8[n, 32] -> (points u64[n, 8], status uint8[n], n_bad, first_bad or None). status: 0 ok, 1 malformed, 2 not on the curve; a
        rejected item's point is all zero"""
        return self._decompress(data, False, 0)

    def g2_decompress(self, data, check_subgroup: int = 1):
        """uint8[n, 64] -> (points u64[n, 16], status, n_bad, first_bad or None); status 3: on the twist but outside the order-r subgroup
        (tested when check_subgroup = 1)"""
        return self._decompress(data, True, check_subgroup)

    def g2_subgroup_check(self, points_aff):
        """-> (number of points outside the order-r subgroup, index of the first or None); the points are assumed to be on the twist"""
        pts = _np(points_aff, 16)
        bad, first = C.c_uint64(0), C.c_uint64(0)
        self._ck(self.lib.keaki_hip_g2_subgroup_check(self.ctx, _ptr(pts), pts.shape[0], C.byref(bad), C.byref(first)))
        return bad.value, (None if bad.value == 0 else first.value)

    def point_codec_dev(self, what: str, d_in, n: int, d_out=None, d_status=None, check_subgroup: int = 1):
        """the resident forms: `what` in g1_compress, g2_compress, g1_decompress, g2_decompress, g2_subgroup_check; device pointers (ints) or
        torch tensors. compress -> None; the others -> (n_bad, first_bad or None) on the host (the call synchronises)"""
        dp = lambda x: C.c_void_p(None if x is None else (x.data_ptr() if hasattr(x, "data_ptr") else x))
        fn = getattr(self.lib, "keaki_hip_%s_dev" % what)
        if what.endswith("_compress"):
            self._ck(fn(self.ctx, dp(d_in), int(n), dp(d_out)))
            return None
        bad, first = C.c_uint64(0), C.c_uint64(0)
        if what == "g2_subgroup_check":
            self._ck(fn(self.ctx, dp(d_in), int(n), C.byref(bad), C.byref(first)))
        elif what == "g2_decompress":
            self._ck(fn(self.ctx, dp(d_in), int(n), int(check_subgroup), dp(d_out), dp(d_status), C.byref(bad), C.byref(first)))
        else:
            self._ck(fn(self.ctx, dp(d_in), int(n), dp(d_out), dp(d_status), C.byref(bad), C.byref(first)))
        return bad.value, (None if bad.value == 0 else first.value)

    def fr_fft(self, data, log2n: int, omega, scale=None) -> np.ndarray:
        a = _np(data, 4).copy()
        assert a.shape[0] == 1 << log2n
        self._ck(self.lib.keaki_hip_fr_fft(self.ctx, _ptr(a), log2n, _ptr(_np(omega)), _ptr(_np(scale)) if scale is not None else None))
        return a

    def open_fk(self, srs: "SrsG1", log2d: int, hat_a, tw_2d, tw_2d_inv, tw_d) -> np.ndarray:
        d = 1 << log2d
        ha = _np(hat_a, 4); t1 = _np(tw_2d, 4); t2 = _np(tw_2d_inv, 4); t3 = _np(tw_d, 4) if d >= 2 else np.zeros((1, 4), np.uint64)
        out = np.zeros((d, 8), np.uint64)
        self._ck(self.lib.keaki_hip_open_fk(self.ctx, srs.handle, log2d, _ptr(ha), _ptr(t1), _ptr(t2), _ptr(t3), _ptr(out)))
        return out

    def open_fk_poly(self, srs: "SrsG1", log2d: int, coeffs, omega_2d, omega_2d_inv, inv_2d) -> np.ndarray:
        d = 1 << log2d
        p = _np(coeffs, 4)
        assert p.shape[0] == d
        out = np.zeros((d, 8), np.uint64)
        self._ck(self.lib.keaki_hip_open_fk_poly(self.ctx, srs.handle, log2d, _ptr(p), _ptr(_np(omega_2d)), _ptr(_np(omega_2d_inv)), _ptr(_np(inv_2d)), _ptr(out)))
        return out

    def srs_g1_precompute_fk(self, srs: "SrsG1", log2d: int, omega_2d):
        """setup-time build of the handle's cached FK23 transform for d = 2^log2d (later open_fk / open_fk_poly / vec_commit calls at this d reuse it)"""
        self._ck(self.lib.keaki_hip_srs_g1_precompute_fk(self.ctx, srs.handle, log2d, _ptr(_np(omega_2d))))

    # FK23 coset openings: all r = d / l set proofs of the l-point cosets {i + t r} in one call (keaki_hip_open_fk_cosets*). omega_2r: the generator
    # of the size-2r domain (= omega_2d^l); proof i belongs to c_i = omega_r^i and equals the affine form of kzg_open_multi on coset i
    def open_fk_cosets_poly(self, srs: "SrsG1", log2d: int, log2l: int, coeffs, omega_2r, omega_2r_inv, inv_2r) -> np.ndarray:
        p = _np(coeffs, 4)
        assert p.shape[0] == 1 << log2d and log2l <= log2d
        out = np.zeros((1 << (log2d - log2l), 8), np.uint64)
        self._ck(self.lib.keaki_hip_open_fk_cosets_poly(self.ctx, srs.handle, log2d, log2l, _ptr(p), _ptr(_np(omega_2r)), _ptr(_np(omega_2r_inv)),
                                                        _ptr(_np(inv_2r)), _ptr(out)))
        return out

    def open_fk_cosets_poly_dev(self, srs: "SrsG1", log2d: int, log2l: int, d_coeffs: int, omega_2r, omega_2r_inv, inv_2r, d_proofs: int):
        self._ck(self.lib.keaki_hip_open_fk_cosets_poly_dev(self.ctx, srs.handle, log2d, log2l, C.c_void_p(d_coeffs), _ptr(_np(omega_2r)),
                                                            _ptr(_np(omega_2r_inv)), _ptr(_np(inv_2r)), C.c_void_p(d_proofs)))

    def open_fk_cosets(self, srs: "SrsG1", log2d: int, log2l: int, hat_a, omega_2r, omega_2r_inv) -> np.ndarray:
        """the raw form: hat_a = l rows of 2r Fr (natural order, divided by 2r), row j = DFT_2r(r zeros, then the coefficients u l + j)"""
        ha = _np(hat_a, 4)
        assert ha.shape[0] == 2 << log2d and log2l <= log2d
        out = np.zeros((1 << (log2d - log2l), 8), np.uint64)
        self._ck(self.lib.keaki_hip_open_fk_cosets(self.ctx, srs.handle, log2d, log2l, _ptr(ha), _ptr(_np(omega_2r)), _ptr(_np(omega_2r_inv)), _ptr(out)))
        return out

    def srs_g1_precompute_fk_cosets(self, srs: "SrsG1", log2d: int, log2l: int, omega_2r):
        """setup-time build of the handle's cached coset transforms for (d, l) = (2^log2d, 2^log2l)"""
        self._ck(self.lib.keaki_hip_srs_g1_precompute_fk_cosets(self.ctx, srs.handle, log2d, log2l, _ptr(_np(omega_2r))))

    # ---- KEM composites
    # FK23 sharded over `world` ranks: the steps between the caller's exchanges (keaki_amd/dist.py::ShardedFk drives them)
    def fk_shard_create(self, srs: "SrsG1", log2d: int, rank: int, world: int, omega_2d, omega_2d_inv, inv_2d) -> "FkShardHandle":
        h = C.c_void_p()
        self._ck(self.lib.keaki_hip_fk_shard_create(self.ctx, srs.handle, log2d, rank, world, _ptr(_np(omega_2d)), _ptr(_np(omega_2d_inv)),
                                                    _ptr(_np(inv_2d)), C.byref(h)))
        sizes = (C.c_size_t * 4)()
        self._ck(self.lib.keaki_hip_fk_shard_sizes(h, sizes))
        return FkShardHandle(self, h, log2d, rank, world, tuple(int(x) for x in sizes))

    def fk_shard_setup(self, fk: "FkShardHandle", step: int, d_send: int, d_recv: int):
        self._ck(self.lib.keaki_hip_fk_shard_setup(self.ctx, fk.handle, step, C.c_void_p(d_send), C.c_void_p(d_recv)))

    def fk_shard_open(self, fk: "FkShardHandle", step: int, d_send: int, d_recv: int, coeffs=None, out=None):
        """steps 0-2 return None; step 3 returns the d affine proofs (u64[d, 8]) in natural order (written into `out` if given)"""
        if step == 3 and out is None:
            out = np.empty(((1 << fk.log2d), 8), dtype=np.uint64)
        p = _np(coeffs, 4) if coeffs is not None else None
        self._ck(self.lib.keaki_hip_fk_shard_open(self.ctx, fk.handle, step, _ptr(p), C.c_void_p(d_send), C.c_void_p(d_recv), _ptr(out)))
        return out

    def encap_batch(self, com, tau_g2, points, values, rs, msg_len: int = 32, want_gt: bool = True):
        """-> (ct, gt, key), or (ct, key) with want_gt=False (the GT bytes stay on the device: only the keys come back)"""
        com = _np(com); tau = _np(tau_g2); pts = _np(points, 4); vals = _np(values, 4); rs = _np(rs, 4)
        n = pts.shape[0]
        ct = np.zeros((n, 16), np.uint64); key = np.zeros((n, max(msg_len, 1)), np.uint8)
        gt = np.zeros((n, 384), np.uint8) if want_gt else None
        self._ck(self.lib.keaki_hip_encap_batch(self.ctx, _ptr(com), _ptr(tau), _ptr(pts), _ptr(vals), _ptr(rs), n,
                                                _ptr(ct), _ptr(gt) if want_gt else None, _ptr(key) if msg_len else None, msg_len))
        return (ct, gt, key[:, :msg_len]) if want_gt else (ct, key[:, :msg_len])

    def encap_prepare(self, tau_g2, batch_hint: int):
        """setup-time: the tables of encap_batch that depend on the setup only (keaki_hip_encap_prepare)"""
        self._ck(self.lib.keaki_hip_encap_prepare(self.ctx, _ptr(_np(tau_g2)), int(batch_hint)))

    def encap_batch_dev(self, d_com, d_tau, d_points, d_values, d_r, n, d_ct, d_gt, d_key, msg_len):
        v = lambda x: C.c_void_p(x) if x else None
        self._ck(self.lib.keaki_hip_encap_batch_dev(self.ctx, v(d_com), v(d_tau), v(d_points), v(d_values), v(d_r), n, v(d_ct), v(d_gt), v(d_key), msg_len))

    def encrypt_batch_dev(self, d_com, d_tau, d_points, d_values, d_r, n, d_ct, d_body_inout, msg_len):
        """d_body_inout: n x msg_len bytes of device memory, the messages on entry and the ciphertext bodies on exit"""
        v = lambda x: C.c_void_p(x) if x else None
        self._ck(self.lib.keaki_hip_encrypt_batch_dev(self.ctx, v(d_com), v(d_tau), v(d_points), v(d_values), v(d_r), n, v(d_ct), v(d_body_inout), msg_len))

    def decrypt_batch_dev(self, d_proofs, d_cts, n, d_body_inout, msg_len):
        """d_body_inout: the ciphertext bodies on entry and the messages on exit"""
        v = lambda x: C.c_void_p(x) if x else None
        self._ck(self.lib.keaki_hip_decrypt_batch_dev(self.ctx, v(d_proofs), v(d_cts), n, v(d_body_inout), msg_len))

    def decap_batch(self, proofs, cts, msg_len: int = 32):
        p = _np(proofs, 8); c = _np(cts, 16); n = p.shape[0]
        gt = np.zeros((n, 384), np.uint8); key = np.zeros((n, max(msg_len, 1)), np.uint8)
        self._ck(self.lib.keaki_hip_decap_batch(self.ctx, _ptr(p), _ptr(c), n, _ptr(gt), _ptr(key) if msg_len else None, msg_len))
        return gt, key[:, :msg_len]

    def encrypt_batch(self, com, tau_g2, points, values, rs, msgs, in_place: bool = False):
        """enc::encrypt over a batch (src/enc.rs:19-40 in the loop of src/vec.rs:63-66): msgs is an (n, msg_len) uint8 array.
        Returns (ct points (n, 16) u64, ciphertext bodies (n, msg_len) u8); the XOR runs on the device behind the KDF."""
        p, v, r = _np(points, 4), _np(values, 4), _np(rs, 4)
        m = np.ascontiguousarray(msgs, dtype=np.uint8)
        n, msg_len = m.shape
        ct = np.zeros((n, 16), np.uint64)
        body = m if in_place else np.zeros((n, msg_len), np.uint8)      # in_place: the message array doubles as the output (the ABI allows it)
        self._ck(self.lib.keaki_hip_encrypt_batch(self.ctx, _ptr(_np(com)), _ptr(_np(tau_g2)), _ptr(p), _ptr(v), _ptr(r), _ptr(m), n, _ptr(ct), _ptr(body), msg_len))
        return ct, body

    def decrypt_batch(self, proofs, cts, bodies):
        """enc::decrypt over a batch (src/enc.rs:44-55 in the loop of src/vec.rs:75-78): returns the (n, msg_len) messages."""
        pr, c = _np(proofs, 8), _np(cts, 16)
        b = np.ascontiguousarray(bodies, dtype=np.uint8)
        n, msg_len = b.shape
        out = np.zeros((n, msg_len), np.uint8)
        self._ck(self.lib.keaki_hip_decrypt_batch(self.ctx, _ptr(pr), _ptr(c), _ptr(b), n, _ptr(out), msg_len))
        return out

    def decap_batch_dev(self, d_proofs, d_cts, n, d_gt, d_key, msg_len):
        v = lambda x: C.c_void_p(x) if x else None
        self._ck(self.lib.keaki_hip_decap_batch_dev(self.ctx, v(d_proofs), v(d_cts), n, v(d_gt), v(d_key), msg_len))

    # ---- a commitment per GROUP of items (keaki_hip_encap_multi / keaki_hip_encrypt_multi): group j = items [offsets[j], offsets[j + 1])
    @staticmethod
    def _offsets(offsets):
        o = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
        if o.size == 0:
            raise ValueError("offsets holds m + 1 words: at least one")
        return o

    def encap_multi(self, coms, offsets, tau_g2, points, values, rs, msg_len: int = 32, want_gt: bool = True):
        """-> (ct, gt, key), or (ct, key) with want_gt=False; coms: (m, 8) u64, offsets: m + 1 item bounds"""
        c = _np(coms, 8); o = self._offsets(offsets); pts = _np(points, 4); vals = _np(values, 4); rs = _np(rs, 4)
        n = pts.shape[0]
        ct = np.zeros((n, 16), np.uint64); key = np.zeros((n, max(msg_len, 1)), np.uint8)
        gt = np.zeros((n, 384), np.uint8) if want_gt else None
        self._ck(self.lib.keaki_hip_encap_multi(self.ctx, _ptr(c) if c.size else None, _ptr(o), o.size - 1, _ptr(_np(tau_g2)), _ptr(pts), _ptr(vals), _ptr(rs), n,
                                                _ptr(ct), _ptr(gt) if want_gt else None, _ptr(key) if msg_len else None, msg_len))
        return (ct, gt, key[:, :msg_len]) if want_gt else (ct, key[:, :msg_len])

    def encrypt_multi(self, coms, offsets, tau_g2, points, values, rs, msgs, in_place: bool = False):
        """-> (ct points (n, 16) u64, bodies (n, msg_len) u8) of msgs, an (n, msg_len) uint8 array"""
        c = _np(coms, 8); o = self._offsets(offsets); p, v, r = _np(points, 4), _np(values, 4), _np(rs, 4)
        m = np.ascontiguousarray(msgs, dtype=np.uint8)
        n, msg_len = m.shape
        ct = np.zeros((n, 16), np.uint64)
        body = m if in_place else np.zeros((n, msg_len), np.uint8)
        self._ck(self.lib.keaki_hip_encrypt_multi(self.ctx, _ptr(c) if c.size else None, _ptr(o), o.size - 1, _ptr(_np(tau_g2)), _ptr(p), _ptr(v), _ptr(r), _ptr(m), n,
                                                  _ptr(ct), _ptr(body), msg_len))
        return ct, body

    def encap_multi_dev(self, d_coms, offsets, d_tau, d_points, d_values, d_r, n, d_ct, d_gt, d_key, msg_len):
        """offsets: a HOST array of m + 1 item bounds (read before the call returns); everything else device addresses"""
        v = lambda x: C.c_void_p(x) if x else None
        o = self._offsets(offsets)
        self._ck(self.lib.keaki_hip_encap_multi_dev(self.ctx, v(d_coms), _ptr(o), o.size - 1, v(d_tau), v(d_points), v(d_values), v(d_r), n, v(d_ct), v(d_gt), v(d_key), msg_len))

    def encrypt_multi_dev(self, d_coms, offsets, d_tau, d_points, d_values, d_r, n, d_ct, d_body_inout, msg_len):
        v = lambda x: C.c_void_p(x) if x else None
        o = self._offsets(offsets)
        self._ck(self.lib.keaki_hip_encrypt_multi_dev(self.ctx, v(d_coms), _ptr(o), o.size - 1, v(d_tau), v(d_points), v(d_values), v(d_r), n, v(d_ct), v(d_body_inout), msg_len))


class GroupSrsG1:
    def __init__(self, owner, handle, n):
        self.owner, self.handle, self.n = owner, handle, n

    def free(self):
        if self.handle:
            self.owner.lib.keaki_hip_group_srs_g1_free(self.owner.g, self.handle)
            self.handle = None


class KeakiHipGroup:
    """keaki_hip_group_*: one context + one host thread per entry of `devices` inside the library (in-process multi-GPU; an ordinal may
    repeat). The SRS is split into contiguous chunks, one per member, each with its own window tables."""

    def __init__(self, devices):
        self.lib = load_library()
        devs = (C.c_int32 * len(devices))(*devices)
        g = C.c_void_p()
        st = self.lib.keaki_hip_group_create(devs, len(devices), C.byref(g))
        if st != 0:
            raise KeakiHipError(st, self.lib.keaki_hip_group_last_error(None).decode())
        self.g = g
        self.size = len(devices)

    def close(self):
        if getattr(self, "g", None):
            self.lib.keaki_hip_group_destroy(self.g)
            self.g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, st):
        if st != 0:
            raise KeakiHipError(st, self.lib.keaki_hip_group_last_error(self.g).decode())

    def peer_note(self) -> str:
        """Empty when every pair of distinct devices of the group has direct (peer) access; otherwise the pairs whose copies the runtime stages."""
        return self.lib.keaki_hip_group_peer_note(self.g).decode()

    def member_memory(self, i: int) -> dict:
        out = (C.c_size_t * 4)()
        st = self.lib.keaki_hip_ctx_memory(self.lib.keaki_hip_group_ctx(self.g, i), out)
        if st != 0:
            raise KeakiHipError(st, "ctx_memory")
        return {"tables": int(out[0]), "workspaces": int(out[1]), "gt_tables": int(out[2]), "total": int(out[3])}

    def srs_g1_upload(self, points, precompute: bool = True) -> GroupSrsG1:
        pts = _np(points, 8); h = C.c_void_p()
        self._ck(self.lib.keaki_hip_group_srs_g1_upload(self.g, _ptr(pts), pts.shape[0], 1 if precompute else 0, C.byref(h)))
        return GroupSrsG1(self, h, pts.shape[0])

    def msm_g1(self, srs: GroupSrsG1, scalars) -> np.ndarray:
        sc = _np(scalars, 4); out = np.zeros(12, np.uint64)
        self._ck(self.lib.keaki_hip_group_msm_g1(self.g, srs.handle, _ptr(sc) if sc.shape[0] else None, sc.shape[0], _ptr(out)))
        return out

    def kzg_open(self, srs: GroupSrsG1, coeffs, point):
        c = _np(coeffs, 4)
        out = np.zeros(12, np.uint64); val = np.zeros(4, np.uint64)
        self._ck(self.lib.keaki_hip_group_kzg_open(self.g, srs.handle, _ptr(c) if c.shape[0] else None, c.shape[0], _ptr(_np(point)), _ptr(out), _ptr(val)))
        return out, val

    def fk_create(self, points, log2d: int, omega_2d, omega_2d_inv, inv_2d):
        """FK23 over the members (keaki_hip_group_fk_*): handle for domain size 2^log2d over the first 2^log2d points"""
        pts = _np(points, 8)
        assert pts.shape[0] >= 1 << log2d
        h = C.c_void_p()
        self._ck(self.lib.keaki_hip_group_fk_create(self.g, _ptr(pts), log2d, _ptr(_np(omega_2d)), _ptr(_np(omega_2d_inv)), _ptr(_np(inv_2d)), C.byref(h)))
        return h

    def fk_open(self, fk, log2d: int, coeffs) -> np.ndarray:
        p = _np(coeffs, 4)
        assert p.shape[0] == 1 << log2d
        out = np.zeros((1 << log2d, 8), np.uint64)
        self._ck(self.lib.keaki_hip_group_fk_open(self.g, fk, _ptr(p), _ptr(out)))
        return out

    def fk_free(self, fk):
        self.lib.keaki_hip_group_fk_free(self.g, fk)

    def encap_batch(self, com, tau_g2, points, values, rs, msg_len: int = 32):
        com = _np(com); tau = _np(tau_g2); pts = _np(points, 4); vals = _np(values, 4); rs = _np(rs, 4)
        n = pts.shape[0]
        ct = np.zeros((n, 16), np.uint64); gt = np.zeros((n, 384), np.uint8); key = np.zeros((n, max(msg_len, 1)), np.uint8)
        self._ck(self.lib.keaki_hip_group_encap_batch(self.g, _ptr(com), _ptr(tau), _ptr(pts), _ptr(vals), _ptr(rs), n,
                                                      _ptr(ct), _ptr(gt), _ptr(key) if msg_len else None, msg_len))
        return ct, gt, key[:, :msg_len]

    def encrypt_batch(self, com, tau_g2, points, values, rs, msgs):
        p, v, r = _np(points, 4), _np(values, 4), _np(rs, 4)
        m = np.ascontiguousarray(msgs, dtype=np.uint8)
        n, msg_len = m.shape
        ct = np.zeros((n, 16), np.uint64); body = np.zeros((n, msg_len), np.uint8)
        self._ck(self.lib.keaki_hip_group_encrypt_batch(self.g, _ptr(_np(com)), _ptr(_np(tau_g2)), _ptr(p), _ptr(v), _ptr(r), _ptr(m), n, _ptr(ct), _ptr(body), msg_len))
        return ct, body

    def decrypt_batch(self, proofs, cts, bodies):
        pr, c = _np(proofs, 8), _np(cts, 16)
        b = np.ascontiguousarray(bodies, dtype=np.uint8)
        n, msg_len = b.shape
        out = np.zeros((n, msg_len), np.uint8)
        self._ck(self.lib.keaki_hip_group_decrypt_batch(self.g, _ptr(pr), _ptr(c), _ptr(b), n, _ptr(out), msg_len))
        return out

    def decap_batch(self, proofs, cts, msg_len: int = 32):
        p = _np(proofs, 8); c = _np(cts, 16); n = p.shape[0]
        gt = np.zeros((n, 384), np.uint8); key = np.zeros((n, max(msg_len, 1)), np.uint8)
        self._ck(self.lib.keaki_hip_group_decap_batch(self.g, _ptr(p), _ptr(c), n, _ptr(gt), _ptr(key) if msg_len else None, msg_len))
        return gt, key[:, :msg_len]


def jac_to_affine_words(jac) -> np.ndarray:
    """normalised Jacobian u64[12] (x, y, 1 | 1, 1, 0) -> affine u64[8] (identity = zeros). Pure relabelling."""
    j = _np(jac).reshape(-1)
    w = j.size // 3
    out = np.zeros(2 * w, np.uint64)
    if np.any(j[2 * w:]):
        out[:] = j[:2 * w]
    return out
