"""ctypes binding of libcdml_hip.so (the C ABI declared in include/cdml.h).

There is deliberately NO fallback: if the HIP library is missing or a call
fails, the product raises.  PyTorch is used only for device memory and streams.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libcdml_hip.so"


class CdmlError(RuntimeError):
    """A C-ABI call returned a negative cdml_status."""

    def __init__(self, code, message):
        super().__init__(f"cdml status {code}: {message}")
        self.code = code


def lib_path():
    """Path of the built library; CDML_LIB_PATH overrides it (kernel A/B builds)."""
    return os.environ.get("CDML_LIB_PATH") or os.path.join(_HERE, "lib", _LIB_NAME)


def source_id(csrc=None, header=None):
    """sha256[:16] over the sources the library is built from -- csrc/*.hip, csrc/*.h (sorted by name),
    include/cdml.h and the feature headers beside it (include/cdml_*.h, sorted by name).  __graft_entry__.build() compiles it into the library (``cdml_build_id()``); ``load_library``
    compares the two, so a prebuilt .so that travelled with a tree it was not built from is refused instead of
    silently passing for it (file times say nothing after a copy).  None when the tree has no sources."""
    import glob
    import hashlib
    csrc = csrc or os.path.join(_HERE, "csrc")
    header = header or os.path.join(os.path.dirname(_HERE), "include", "cdml.h")
    files = sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h")))
    if not files or not os.path.exists(header):
        return None
    h = hashlib.sha256()
    for f in files + [header] + sorted(glob.glob(os.path.join(os.path.dirname(header), "cdml_*.h"))):
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def embedded_id(path):
    """The build id compiled into the library file at ``path`` (read from the file, nothing is loaded), or None."""
    import re
    try:
        m = re.search(rb"CDML_BUILD_ID=([0-9a-f]{16})", open(path, "rb").read())
    except OSError:
        return None
    return m.group(1).decode() if m else None


_p = C.c_void_p
_i = C.c_int
_i64 = C.c_int64
_u64 = C.c_uint64
_f = C.c_float
_sz = C.c_size_t

# name -> (restype, argtypes); must list every symbol include/cdml.h declares
SIGNATURES = {
    "cdml_version": (_i, []),
    "cdml_build_id": (C.c_char_p, []),
    "cdml_last_error": (C.c_char_p, []),
    "cdml_fill_uniform_table": (_i, [_p, _i64, _i64, _i, _i64, _u64, _p]),
    "cdml_sample_uniform": (_i, [_p, _i64, _i64, _u64, _u64, _p, _i, _i64, _i64, _p, _p]),
    "cdml_sample_inbatch": (_i, [_p, _i64, _u64, _u64, _p, _i, _i64, _i64, _p, _p, _p]),
    "cdml_step_advance": (_i, [_p, _p]),
    "cdml_gather_rows": (_i, [_p, _i64, _i64, _i64, _p, _i, _i, _i, _p, _i64, _p, _p, _p]),
    "cdml_sample_gather": (_i, [_i, _p, _i64, _u64, _u64, _p, _i, _i64, _i64, _p, _i64, _i64, _i,
                                _p, _p, _p, _i64, _i, _i64, _i64, _p, _p]),
    "cdml_route_rows": (_i, [_p, _i, _i64, _i, _i, _p, _p, _p, _p]),
    "cdml_scatter_rows": (_i, [_p, _i64, _p, _i, _i, _p, _i64, _p]),
    "cdml_sample_gather_f16": (_i, [_i, _p, _i64, _u64, _u64, _p, _i, _i64, _i64, _p, _i64, _i64, _i,
                                    _p, _p, _p, _i64, _i, _i64, _i64, _p, _p]),
    "cdml_l2norm_fwd": (_i, [_p, _i64, _i, _i, _p, _i64, _p, _p]),
    "cdml_l2norm_bwd": (_i, [_p, _i64, _p, _i64, _i, _i, _f, _p, _i64, _p]),
    "cdml_fc_lrelu_fwd": (_i, [_p, _i64, _p, _i64, _p, _f, _i, _i, _i, _p, _i64, _p]),
    "cdml_fc_bwd_data": (_i, [_p, _i64, _p, _i64, _p, _i64, _f, _i, _i, _i, _p, _i64, _p]),
    "cdml_fc_bwd_weight_workspace": (_sz, [_i, _i, _i]),
    "cdml_fc_bwd_weight": (_i, [_p, _i64, _p, _i64, _i, _i, _i, _p, _i64, _p, _p, _sz, _p]),
    "cdml_fc_bwd_weight2_workspace": (_sz, [_i, _i, _i, _i, _i]),
    "cdml_fc_bwd_weight2": (_i, [_p, _i64, _p, _i64, _i, _i, _p, _i64, _p, _p, _i64, _p, _i64, _i, _i, _p, _i64, _p,
                                 _i, _p, _sz, _p]),
    "cdml_triplet_hinge": (_i, [_p, _i64, _i, _i, _f, _p, _p, _p, _p, _p, _i64, _p]),
    "cdml_triplet_hinge_inbatch": (_i, [_p, _i64, _p, _p, _i, _i, _f, _p, _p, _p, _p, _p, _p,
                                        _i64, _p]),
    "cdml_vnet_tail_workspace": (_sz, [_i, _i]),
    "cdml_vnet_tail": (_i, [_i, _p, _i64, _p, _p, _i, _i, _f, _f, _p, _i64, _p, _p, _p, _p, _p, _i64, _p, _i64,
                            _p, _p, _p]),
    "cdml_vnet_tail_planes": (_i, [_i, _p, _i64, _p, _p, _i, _i, _f, _f, _p, _i64, _p, _p, _p, _p, _p, _i64, _p, _i64, _i64,
                                   _p, _p, _p]),
    "cdml_vnet_tail_h2": (_i, [_i, _p, _i64, _p, _p, _i, _i, _f, _f, _p, _i64, _p, _p, _p, _p, _p, _i64, _p, _i64, _i64, _f,
                               _p, _p, _p]),
    "cdml_semihard_select": (_i, [_p, _i64, _p, _i64, _p, _i, _i, _p, _p, _p]),
    "cdml_semihard_mine_x3_workspace": (_sz, [_i]),
    "cdml_semihard_mine_x3": (_i, [_p, _i64, _p, _i, _i, _p, _i64, _i64, _p, _p, _p, _sz, _p, _p]),
    "cdml_semihard_mine_x3_z": (_i, [_p, _i64, _p, _i64, _p, _i, _i, _p, _i64, _i64, _p, _p, _p, _sz, _p, _p]),
    "cdml_semihard_mine_h2": (_i, [_p, _i64, _p, _i64, _p, _i, _i, _p, _i64, _i64, _f, _p, _p, _p, _sz, _p, _p]),
    "cdml_triplet_hinge_indexed": (_i, [_p, _i64, _p, _i, _i, _f, _p, _p, _p, _p, _p, _p, _i64, _p]),
    "cdml_x3_slab_steps": (_i, [_i]),
    "cdml_triplet_hinge_indexed_tail": (_i, [_p, _i64, _p, _i, _i, _f, _p, _p, _p, _p, _p, _p, _i64, _p, _i64, _f, _p, _i64,
                                             _p, _i64, _i64, _p]),
    "cdml_npair_workspace": (_sz, [_i]),
    "cdml_npair_stats": (_i, [_p, _i64, _p, _i, _f, _i, _p, _p, _p, _sz, _p]),
    "cdml_npair_grad_x3": (_i, [_p, _i64, _p, _i, _f, _i, _p, _p, _i64, _i64, _p]),
    "cdml_npair_grad_f32": (_i, [_p, _i64, _p, _i, _f, _i, _p, _p, _i64, _p]),
    "cdml_npair_memory_workspace": (_sz, [_i, _i]),
    "cdml_npair_memory_stats": (_i, [_p, _i64, _p, _i, _i64, _p, _i, _f, _i, _p, _p, _p, _sz, _p]),
    "cdml_npair_memory_grad_x3": (_i, [_p, _i64, _p, _i, _i64, _p, _i, _f, _i, _p, _p, _i64, _i64, _p]),
    "cdml_npair_memory_grad_f32": (_i, [_p, _i64, _p, _i, _i64, _p, _i, _f, _i, _p, _p, _i64, _p]),
    "cdml_npair_memory_push": (_i, [_p, _i64, _p, _i, _i, _u64, _p, _i64, _i, _p, _i64, _p, _p, _i64, _i64, _p, _i64,
                                    _i64, _p]),
    "cdml_npair_logq_stats": (_i, [_p, _i64, _p, _i, _p, _f, _i, _p, _p, _p, _sz, _p]),
    "cdml_npair_logq_grad_x3": (_i, [_p, _i64, _p, _i, _p, _f, _i, _p, _p, _i64, _i64, _p]),
    "cdml_npair_logq_grad_f32": (_i, [_p, _i64, _p, _i, _p, _f, _i, _p, _p, _i64, _p]),
    "cdml_npair_memory_logq_stats": (_i, [_p, _i64, _p, _i, _p, _i64, _p, _p, _i, _f, _i, _p, _p, _p, _sz, _p]),
    "cdml_npair_memory_logq_grad_x3": (_i, [_p, _i64, _p, _i, _i64, _p, _p, _i, _f, _i, _p, _p, _i64, _i64, _p]),
    "cdml_npair_memory_logq_grad_f32": (_i, [_p, _i64, _p, _i, _i64, _p, _p, _i, _f, _i, _p, _p, _i64, _p]),
    "cdml_logq_table_gather": (_i, [_p, _i64, _p, _i, _p, _i, _p, _p, _p]),
    "cdml_logq_stream_gather": (_i, [_p, _p, _i64, _p, _i, _p, _i, _p, _p, _p, _p, _p]),
    "cdml_logq_stream_update": (_i, [_p, _p, _i64, _p, _i, _p, _p, _f, _u64, _p, _p]),
    "cdml_logq_stream_reset": (_i, [_p, _p, _i64, _f, _p]),
    "cdml_pair_dist": (_i, [_p, _i64, _i, _p, _i, _i, _p, _p, _p, _p]),
    "cdml_cowatch_workspace": (_sz, [_i64]),
    "cdml_cowatch_graph": (_i, [_p, _i64, _p, _p, _p, _p, _p, _sz, _p]),
    "cdml_cowatch_select": (_i, [_p, _i64, _i, _i, _p, _p, _p, _p, _sz, _p]),
    "cdml_knn_list_capacity": (_i, []),
    "cdml_row_sqnorm": (_i, [_p, _i64, _i, _i, _p, _p]),
    "cdml_knn_merge": (_i, [_p, _i64, _i, _i, _i, _i, _p, _p, _i, _p, _p, _i, _p]),
    "cdml_knn_filter_x3": (_i, [_p, _i64, _i64, _p, _i64, _i64, _i, _i, _i, _p, _p, _p, _i, _i, _p, _p, _i, _p]),
    "cdml_knn_filter_h2": (_i, [_p, _i64, _i64, _p, _i64, _i64, _i, _i, _i, _f, _p, _p, _p, _i, _i, _p, _p, _i, _p]),
    "cdml_knn_merge_list": (_i, [_p, _p, _i, _i, _i, _p, _p, _p, _p]),
    "cdml_knn_desim_prep": (_i, [_p, _i, _i64, _p, _i64, _i, _i, _f, _p, _i, _p]),
    "cdml_knn_desim": (_i, [_p, _i64, _i, _i, _p, _i, _p, _i, _i, _p, _i64, _p]),
    "cdml_rank_tau_x3": (_i, [_p, _i64, _i64, _p, _i64, _i64, _i, _i, _p, _p, _p, _p]),
    "cdml_rank_tau_h2": (_i, [_p, _i64, _i64, _p, _i64, _i64, _i, _i, _f, _p, _p, _p, _p]),
    "cdml_rank_count_x3": (_i, [_p, _i64, _i64, _p, _i64, _i64, _i, _i, _i, _p, _p, _p, _p, _p, _i, _i, _p, _p]),
    "cdml_rank_count_h2": (_i, [_p, _i64, _i64, _p, _i64, _i64, _i, _i, _i, _f, _p, _p, _p, _p, _p, _i, _i, _p, _p]),
    "cdml_gemm_bf16_workspace": (_sz, [_i, _i, _i]),
    "cdml_gemm_bf16_epilogue_supported": (_i, [_i, _i, _i, _i, _i64, _i64, _i64, _i64]),
    "cdml_gemm_bf16_nt": (_i, [_i, _p, _i64, _p, _i64, _i, _i, _i, _p, _i64, _p, _p, _i64, _f, _p, _sz, _p]),
    "cdml_gemm_bf16_tn_supported": (_i, [_i, _i, _i, _i64, _i64]),
    "cdml_gemm_bf16_tn_workspace": (_sz, [_i, _i, _i]),
    "cdml_gemm_bf16_tn2_workspace": (_sz, [_i, _i, _i, _i, _i]),
    "cdml_gemm_bf16_tn2": (_i, [_p, _i64, _p, _i64, _i, _i, _p, _i64, _p, _p, _i64, _p, _i64, _i, _i, _p, _i64, _p, _i,
                                _p, _sz, _p]),
    "cdml_gemm_bf16_tn": (_i, [_p, _i64, _p, _i64, _i, _i, _i, _p, _i64, _p, _p, _sz, _p]),
    "cdml_sample_gather_x3": (_i, [_i, _p, _i64, _u64, _u64, _p, _i, _i64, _i64, _p, _i64, _i64, _i,
                                   _p, _p, _p, _i64, _i, _i64, _i64, _p, _p]),
    "cdml_sample_gather_h2": (_i, [_i, _p, _i64, _u64, _u64, _p, _i, _i64, _i64, _p, _i64, _i64, _i,
                                   _p, _p, _p, _i64, _i, _i64, _i64, _p, _p]),
    "cdml_gather_rows_x3": (_i, [_p, _i64, _i64, _p, _i, _i, _i, _p, _i64, _p, _p]),
    "cdml_sample_gather_x3k": (_i, [_i, _p, _i64, _u64, _u64, _p, _i, _i64, _i64, _p, _i64, _i64, _i,
                                    _p, _p, _p, _i64, _i, _i64, _i64, _p, _p, _i64, _p]),
    "cdml_split_f32_bf16x3": (_i, [_p, _i64, _i, _i, _p, _i64, _i64, _i, _p]),
    "cdml_gemm_bf16x3_workspace": (_sz, [_i, _i, _i, _i, _i]),
    "cdml_gemm_bf16x3_nt": (_i, [_i, _p, _i64, _i64, _p, _i64, _i64, _i, _i, _i, _i, _p, _i64, _i64, _p, _p, _i64, _f,
                                 _p, _p, _sz, _p]),
    "cdml_gemm_bf16x3_tn": (_i, [_p, _i64, _i64, _p, _i64, _i64, _i, _i, _i, _i, _p, _i64, _p, _f, _p, _p, _sz, _p]),
    "cdml_split_f32_f16x2": (_i, [_p, _i64, _i, _i, _p, _i64, _i64, _i, _f, _p]),
    "cdml_gemm_f16x2_workspace": (_sz, [_i, _i, _i, _i]),
    "cdml_gemm_f16x2_nt": (_i, [_i, _p, _i64, _i64, _p, _i64, _i64, _i, _i, _i, _p, _i64, _i64, _p, _p, _i64, _f, _f, _f,
                                _p, _sz, _p]),
    "cdml_gemm_f16x2_tn": (_i, [_p, _i64, _i64, _p, _i64, _i64, _i, _i, _i, _p, _i64, _f, _p, _f, _p, _sz, _p]),
    "cdml_interleave8_bf16x3": (_i, [_p, _i64, _i64, _i, _i, _p, _p]),
    "cdml_gemm_bf16x3_tnk": (_i, [_p, _i, _i, _p, _i, _i, _i, _i, _i, _p, _i64, _p, _p, _sz, _p]),
    "cdml_transpose_to_bf16": (_i, [_i, _p, _i64, _i, _i, _p, _i64, _p]),
    "cdml_cast_f32_bf16": (_i, [_p, _i64, _i, _i, _p, _i64, _p]),
    "cdml_colsum_workspace_floats": (_sz, [_i, _i]),
    "cdml_colsum": (_i, [_i, _p, _i64, _i, _i, _p, _p, _p]),
    "cdml_fill_uniform_table_f16": (_i, [_p, _i64, _i64, _i, _i64, _u64, _p]),
    "cdml_gather_rows_f16": (_i, [_p, _i64, _i64, _i64, _p, _i, _i, _p, _i64, _p, _p]),
    "cdml_ew_combine": (_i, [_i, _p, _i64, _p, _i64, _i, _i, _p, _i64, _p]),
    "cdml_ew_fusion_bwd": (_i, [_i, _p, _i64, _p, _i64, _p, _i64, _i, _i, _f, _p, _i64, _p, _i64, _p]),
    "cdml_lrelu_bwd": (_i, [_p, _i64, _p, _i64, _i, _i, _f, _p, _i64, _p]),
    "cdml_adam_step": (_i, [_p, _p, _p, _p, _i64, _f, _p, _f, _f, _f, _i64, _p, _i, _p, _p]),
    "cdml_adam_matrix_bf16": (_i, [_p, _p, _p, _p, _i, _i, _f, _p, _f, _f, _f, _i64, _p, _p, _i64, _p, _i64,
                                   _p, _p, _p, _p, _i, _i, _p, _p]),
    "cdml_adam_matrix_planes": (_i, [_p, _p, _p, _p, _i, _i, _f, _p, _f, _f, _f, _i64, _p, _p, _i64, _i64, _p, _i64, _i64,
                                     _p, _p, _p, _p, _i, _i, _p, _p]),
    "cdml_adam_matrix_h2": (_i, [_p, _p, _p, _p, _i, _i, _f, _p, _f, _f, _f, _i64, _p, _p, _i64, _i64, _p, _i64, _i64, _f,
                                 _p, _p, _p, _p, _i, _i, _p, _p]),
    "cdml_table_adam_rows": (_i, [_p, _i64, _i64, _i64, _i, _p, _i, _p, _i64, _p, _p, _p, _p, _f, _f, _p, _f, _f, _f,
                                  _i64, _p, _p]),
    "cdml_grad_prepare": (_i, [_p, _p, _i64, _f, _f, _p, _p, _p]),
    "cdml_momentum_step": (_i, [_p, _p, _p, _i64, _f, _p, _f, _i, _p]),
    "cdml_lars_scratch_floats": (_sz, []),
    "cdml_lars_step": (_i, [_p, _p, _p, _i64, _f, _p, _f, _f, _f, _f, _p, _p]),
    "cdml_lars_multi_scratch_floats": (_sz, []),
    "cdml_lars_multi": (_i, [_p, _p, _p, _p, _p, _i, _f, _p, _f, _f, _f, _f, _p, _p, _p, _p, _p]),
    "cdml_lars_multi_norms": (_i, [_p, _p, _p, _p, _i, _p, _p]),
    "cdml_lars_matrix": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _f, _p, _f, _f, _f, _f, _p, _p, _p, _i64, _i64, _p,
                              _i64, _i64, _i, _p, _p, _p]),
    "cdml_momentum_matrix": (_i, [_p, _p, _p, _i, _i, _f, _p, _f, _i, _p, _i64, _i64, _p, _i64, _i64, _i, _p, _p, _p, _i,
                                  _p, _p, _p]),
    "cdml_lars_matrix_h2": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _f, _p, _f, _f, _f, _f, _p, _p, _p, _i64, _i64, _p,
                                 _i64, _i64, _f, _p, _p, _p]),
    "cdml_momentum_matrix_h2": (_i, [_p, _p, _p, _i, _i, _f, _p, _f, _i, _p, _i64, _i64, _p, _i64, _i64, _f, _p, _p, _p, _i,
                                     _p, _p, _p]),
}

# name -> (restype, argtypes); must list every symbol include/cdml_npair_mixed.h declares (the N-pair loss with mixed
# negative sampling: a header and a table of its own)
SIGNATURES_MIXED = {
    "cdml_npair_mixed_workspace": (_sz, [_i, _i]),
    "cdml_npair_mixed_stats": (_i, [_p, _i64, _p, _i, _i64, _i64, _p, _i, _p, _f, _p, _f, _i, _p, _p, _p, _sz, _p]),
    "cdml_npair_mixed_grad_x3": (_i, [_p, _i64, _p, _i, _i64, _i64, _p, _i, _p, _f, _p, _f, _i, _p, _p, _i64, _i64, _p]),
    "cdml_npair_mixed_grad_f32": (_i, [_p, _i64, _p, _i, _i64, _i64, _p, _i, _p, _f, _p, _f, _i, _p, _p, _i64, _p]),
    "cdml_npair_mixed_split_x3": (_i, [_p, _i64, _i, _i, _p, _i64, _i64, _p, _i64, _i64, _p, _i64, _i64, _i64, _p]),
}

# name -> (restype, argtypes); must list every symbol include/cdml_npair_dp.h declares (the data-parallel N-pair loss)
SIGNATURES_DP = {
    "cdml_npair_dp_workspace": (_sz, [_i, _i]),
    "cdml_npair_dp_local_stats": (_i, [_p, _i64, _p, _i, _i, _i, _f, _i, _p, _p, _p, _sz, _p]),
    "cdml_npair_dp_col_fold": (_i, [_p, _i, _i, _p, _p]),
    "cdml_npair_dp_stats": (_i, [_p, _i64, _i, _i, _i, _f, _i, _p, _p, _p, _sz, _p]),
    "cdml_npair_dp_grad_x3": (_i, [_p, _i64, _p, _i, _i, _i, _f, _i, _p, _p, _p, _i64, _i64, _p]),
    "cdml_npair_dp_grad_f32": (_i, [_p, _i64, _p, _i, _i, _i, _f, _i, _p, _p, _p, _i64, _p]),
    "cdml_npair_dp_pos_fold": (_i, [_p, _i64, _i, _i, _i, _p, _i64, _p]),
}

# name -> (restype, argtypes); must list every symbol include/cdml_npair_bf16.h declares (the N-pair loss on the config-4
# precision: one-plane bf16 operands and gradient weights)
SIGNATURES_BF16 = {
    "cdml_npair_operands_bf16": (_i, [_p, _i64, _i, _i, _p, _i64, _p, _i64, _p, _i64, _p]),
    "cdml_npair_grad_bf16": (_i, [_p, _i64, _p, _i, _f, _i, _p, _p, _i64, _p]),
    "cdml_npair_logq_grad_bf16": (_i, [_p, _i64, _p, _i, _p, _f, _i, _p, _p, _i64, _p]),
    "cdml_npair_memory_grad_bf16": (_i, [_p, _i64, _p, _i, _i64, _p, _i, _f, _i, _p, _p, _i64, _p]),
    "cdml_npair_memory_logq_grad_bf16": (_i, [_p, _i64, _p, _i, _i64, _p, _p, _i, _f, _i, _p, _p, _i64, _p]),
    "cdml_npair_memory_push_bf16": (_i, [_p, _i64, _p, _i, _i, _u64, _p, _i64, _i, _p, _i64, _p, _p, _i64, _p, _i64, _p]),
}

# name -> (restype, argtypes); must list every symbol include/cdml_hardneg.h declares (listed "hard" negatives: sampler mode 2)
SIGNATURES_HARDNEG = {
    "cdml_sample_listed": (_i, [_p, _i64, _i64, _u64, _u64, _p, _i, _i64, _i64, _p, _i64, _i, _u64, _p, _p, _p]),
    "cdml_sample_gather_listed": (_i, [_p, _i64, _u64, _u64, _p, _i, _i64, _i64, _p, _i64, _i64, _i, _p, _i64, _i, _u64,
                                       _p, _p, _p, _i64, _i, _i64, _i64, _i64, _p, _p]),
    "cdml_sample_gather_listed_x3": (_i, [_p, _i64, _u64, _u64, _p, _i, _i64, _i64, _p, _i64, _i64, _i, _p, _i64, _i, _u64,
                                          _p, _p, _p, _i64, _i, _i64, _i64, _i64, _p, _p, _i64, _p]),
    "cdml_sample_gather_listed_f16": (_i, [_p, _i64, _u64, _u64, _p, _i, _i64, _i64, _p, _i64, _i64, _i, _p, _i64, _i, _u64,
                                           _p, _p, _p, _i64, _i, _i64, _i64, _i64, _p, _p]),
}

# name -> (restype, argtypes); must list every symbol include/cdml_negweights.h declares (weighted negatives: sampler mode 3,
# and the per-negative bias of the mixed N-pair chain)
SIGNATURES_NEGW = {
    "cdml_sample_weighted": (_i, [_p, _i64, _i64, _u64, _u64, _p, _i, _i64, _i64, _p, _i64, _p, _i, _p, _p, _p]),
    "cdml_sample_gather_weighted": (_i, [_p, _i64, _u64, _u64, _p, _i, _i64, _i64, _p, _i64, _i64, _i, _p, _i64, _p, _i,
                                         _p, _p, _p, _i64, _i, _i64, _i64, _i64, _p, _p]),
    "cdml_sample_gather_weighted_x3": (_i, [_p, _i64, _u64, _u64, _p, _i, _i64, _i64, _p, _i64, _i64, _i, _p, _i64, _p, _i,
                                            _p, _p, _p, _i64, _i, _i64, _i64, _i64, _p, _p, _i64, _p]),
    "cdml_sample_gather_weighted_f16": (_i, [_p, _i64, _u64, _u64, _p, _i, _i64, _i64, _p, _i64, _i64, _i, _p, _i64, _p, _i,
                                             _p, _p, _p, _i64, _i, _i64, _i64, _i64, _p, _p]),
    "cdml_npair_mixed_stats_nb": (_i, [_p, _i64, _p, _i, _i64, _i64, _p, _i, _p, _p, _p, _f, _i, _p, _p, _p, _sz, _p]),
    "cdml_npair_mixed_grad_x3_nb": (_i, [_p, _i64, _p, _i, _i64, _i64, _p, _i, _p, _p, _p, _f, _i, _p, _p, _i64, _i64, _p]),
    "cdml_npair_mixed_grad_f32_nb": (_i, [_p, _i64, _p, _i, _i64, _i64, _p, _i, _p, _p, _p, _f, _i, _p, _p, _i64, _p]),
    "cdml_negw_bias": (_i, [_p, _i64, _p, _i, _f, _p, _p]),
}

# name -> (restype, argtypes); must list every symbol include/cdml_x3_wide.h declares (dW1 with dz1 k8-interleaved)
SIGNATURES_WIDE = {
    "cdml_gemm_bf16x3_tn_kb": (_i, [_p, _i64, _i64, _p, _i, _i, _i, _i, _i, _p, _i64, _p, _p, _sz, _p]),
}

# name -> (restype, argtypes); must list every symbol include/cdml_f8.h declares (the fp8 catalogue of precision "bf16": its
# gathers, the _f16 entry points' twins, and its quantiser)
SIGNATURES_F8 = {
    "cdml_sample_gather_f8": (_i, [_i, _p, _i64, _u64, _u64, _p, _i, _i64, _i64, _p, _i64, _i64, _i,
                                   _p, _p, _p, _i64, _i, _i64, _i64, _p, _p]),
    "cdml_sample_gather_listed_f8": (_i, [_p, _i64, _u64, _u64, _p, _i, _i64, _i64, _p, _i64, _i64, _i, _p, _i64, _i, _u64,
                                          _p, _p, _p, _i64, _i, _i64, _i64, _i64, _p, _p]),
    "cdml_sample_gather_weighted_f8": (_i, [_p, _i64, _u64, _u64, _p, _i, _i64, _i64, _p, _i64, _i64, _i, _p, _i64, _p, _i,
                                            _p, _p, _p, _i64, _i, _i64, _i64, _i64, _p, _p]),
    "cdml_gather_rows_f8": (_i, [_p, _i64, _i64, _i64, _p, _i, _i, _p, _i64, _p, _p]),
    "cdml_quantize_rows_f8_f32": (_i, [_p, _i64, _i64, _i, _p, _i64, _i64, _p, _p]),
    "cdml_quantize_rows_f8_f16": (_i, [_p, _i64, _i64, _i, _p, _i64, _i64, _p, _p]),
}

# name -> (restype, argtypes); must list every symbol include/cdml_ivf.h declares (the IVF index of the kNN: Lloyd's centroid
# update, the grouped score product over probed lists, the merge over ragged score segments)
SIGNATURES_IVF = {
    "cdml_ivf_centroid_sums": (_i, [_p, _i64, _p, _p, _i, _i, _p, _i64, _p]),
    "cdml_ivf_scan_f32": (_i, [_p, _i64, _i, _p, _p, _p, _p, _i64, _p, _i, _p, _i, _p, _p]),
    "cdml_ivf_merge": (_i, [_p, _p, _p, _p, _i, _i, _p, _p, _p, _p, _i, _p, _p, _p]),
}

# name -> (restype, argtypes); must list every symbol include/cdml_ivf_f16.h declares (the fp16 lists of the IVF index: the
# grouped score product on the fp16 MFMA and the exact fp32 re-rank of the merge's candidates)
SIGNATURES_IVF_F16 = {
    "cdml_ivf_scan_f16": (_i, [_p, _i64, _i, _p, _p, _p, _p, _i64, _p, _i, _p, _i, _p, _p]),
    "cdml_ivf_refine": (_i, [_p, _i64, _i, _p, _i64, _i64, _i, _p, _i, _i, _p, _p, _p]),
}

# name -> (restype, argtypes); must list every symbol include/cdml_ivf_filter.h declares (the threshold-filter scan of the IVF
# index: the grouped score product whose epilogue appends what is within tau to the query's candidate list, no score buffer)
_IVF_FILTER_ARGS = [_p, _i64, _i, _p, _p, _p, _p, _p, _p, _i64, _p, _p, _p, _i, _p, _i, _p, _i, _p]
SIGNATURES_IVF_FILTER = {
    "cdml_ivf_filter_f32": (_i, _IVF_FILTER_ARGS),
    "cdml_ivf_filter_f16": (_i, list(_IVF_FILTER_ARGS)),
}

# name -> (restype, argtypes); must list every symbol include/cdml_knn_writer.h declares (the export's text lists formatted on
# the device: the host entry point of the shortest-repr routine and the two launches)
SIGNATURES_KNN_WRITER = {
    "cdml_f32_shortest": (_i, [_f, C.c_char_p]),
    "cdml_knn_line_sizes": (_i, [_p, _i64, _p, _i64, _i64, _i, _i, _p, _i64, _i64, _p, _p, _p]),
    "cdml_knn_line_write": (_i, [_p, _i64, _p, _i64, _i64, _i, _i, _p, _p, _i64, _i64, _p, _p, _i64, _p]),
}

# name -> (restype, argtypes); must list every symbol include/cdml_ivf_pq.h declares (the product-quantised lists of the IVF
# index: the encoder, the per-query lookup tables, the scan's tile and the table-lookup scan)
SIGNATURES_IVF_PQ = {
    "cdml_pq_encode": (_i, [_p, _i64, _i64, _p, _i, _i, _p, _i64, _p, _i64, _p]),
    "cdml_pq_lut": (_i, [_p, _i64, _i, _p, _i, _i, _p, _p]),
    "cdml_ivf_pq_tile": (_i, [_i, _p, _p]),
    "cdml_ivf_scan_pq": (_i, [_p, _i, _p, _p, _p, _p, _i64, _p, _i, _p, _i, _p, _p]),
}

# name -> (restype, argtypes); must list every symbol include/cdml_ivf_pqr.h declares (residual product quantisation: the fused
# residual encoder, the slot scalars <query, centroid> and the table-lookup scan that starts from them)
SIGNATURES_IVF_PQR = {
    "cdml_pqr_encode": (_i, [_p, _i64, _i64, _p, _i64, _i, _p, _p, _i, _i, _p, _i64, _p, _i64, _p]),
    "cdml_ivf_slot_dots": (_i, [_p, _i64, _i, _p, _i64, _i, _p, _p, _i, _p, _p]),
    "cdml_ivf_scan_pqr": (_i, [_p, _i, _p, _p, _p, _p, _p, _i64, _p, _i, _p, _i, _p, _p]),
}

# name -> (restype, argtypes); must list every symbol include/cdml_ivf_pq4.h declares (4-bit product quantisation: two codes a
# byte, 16-entry lookup tables; the argument lists are those of the 8-bit entry points)
SIGNATURES_IVF_PQ4 = {
    "cdml_pq4_encode": (_i, [_p, _i64, _i64, _p, _i, _i, _p, _i64, _p, _i64, _p]),
    "cdml_pq4_lut": (_i, [_p, _i64, _i, _p, _i, _i, _p, _p]),
    "cdml_ivf_pq4_tile": (_i, [_i, _p, _p]),
    "cdml_ivf_scan_pq4": (_i, [_p, _i, _p, _p, _p, _p, _i64, _p, _i, _p, _i, _p, _p]),
}

# name -> (restype, argtypes); must list every symbol include/cdml_ivf_update.h declares (the index's add / remove: the one
# launch that writes the new lists, and the id -> position search)
SIGNATURES_IVF_UPDATE = {
    "cdml_ivf_lists_move": (_i, [_p, _i64, _p, _p, _i64, _p, _i64, _p, _i64, _p, _i64, _p, _i64, _i, _p, _p, _p, _i, _i64, _p, _i64,
                                 _p, _p, _i64, _p]),
    "cdml_ivf_locate": (_i, [_p, _i64, _p, _i64, _p, _i64, _p, _i, _p, _p]),
}

# name -> (restype, argtypes); must list every symbol include/cdml_ivf_range.h declares (the filter scan over 8-bit
# product-quantised lists: the scans' arguments with the filter's candidate set in place of the score buffer)
SIGNATURES_IVF_RANGE = {
    "cdml_ivf_filter_pq": (_i, [_p, _i, _p, _p, _p, _p, _p, _p, _i64, _p, _p, _p, _i, _p, _i, _p, _i, _p]),
    "cdml_ivf_filter_pqr": (_i, [_p, _i, _p, _p, _p, _p, _p, _p, _p, _i64, _p, _p, _p, _i, _p, _i, _p, _i, _p]),
}

_lib = None


def load_library():
    """Load libcdml_hip.so (built by __graft_entry__.build()); raise if absent."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise CdmlError(-2, f"{path} not found: build it with "
                            f"`python -c 'import __graft_entry__ as g; g.build()'` "
                            f"(there is no CPU fallback)")
    # torch first: the process must end up with ONE HIP runtime, the one torch ships and allocates
    # device memory with.  Loaded before torch, this library pulls in the system libamdhip64 and
    # its launches then fail with "no ROCm-capable device is detected".
    import torch  # noqa: F401
    lib = C.CDLL(path)
    for name, (res, args) in (list(SIGNATURES.items()) + list(SIGNATURES_MIXED.items()) + list(SIGNATURES_DP.items())
                               + list(SIGNATURES_BF16.items()) + list(SIGNATURES_HARDNEG.items()) + list(SIGNATURES_WIDE.items())
                               + list(SIGNATURES_NEGW.items()) + list(SIGNATURES_F8.items()) + list(SIGNATURES_IVF.items())
                               + list(SIGNATURES_IVF_F16.items()) + list(SIGNATURES_IVF_FILTER.items())
                               + list(SIGNATURES_KNN_WRITER.items()) + list(SIGNATURES_IVF_PQ.items())
                               + list(SIGNATURES_IVF_PQR.items()) + list(SIGNATURES_IVF_PQ4.items())
                               + list(SIGNATURES_IVF_UPDATE.items()) + list(SIGNATURES_IVF_RANGE.items())):
        fn = getattr(lib, name)          # AttributeError if the ABI lost a symbol
        fn.restype = res
        fn.argtypes = args
    # the library must be the one THIS tree builds (a variant library named by CDML_LIB_PATH is built from a scratch
    # copy of the sources on purpose and is exempt; CDML_ALLOW_STALE_LIB=1 for a deliberate mismatch)
    want = source_id()
    if want is not None and not os.environ.get("CDML_LIB_PATH") and os.environ.get("CDML_ALLOW_STALE_LIB") != "1":
        have = lib.cdml_build_id().decode()
        if have != "CDML_BUILD_ID=" + want:
            raise CdmlError(-2, f"{path} was built from other sources ({have}; this tree is {want}): rebuild it with "
                                f"`python -c 'import __graft_entry__ as g; g.build()'`")
    _lib = lib
    return lib


def call(name, *args):
    """Invoke a status-returning entry point; raise CdmlError on failure."""
    lib = load_library()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise CdmlError(rc, lib.cdml_last_error().decode("utf-8", "replace"))
    return rc
