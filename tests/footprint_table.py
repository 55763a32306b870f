"""The write-footprint table: one entry per launch of the C ABI (include/cdml.h) that tests/test_gpu_footprint.py runs
into poisoned, guarded buffers.  This module is DATA -- it imports nothing of the package and never touches a GPU; the
launch code lives in tests/test_gpu_footprint.py under the same entry ids, and tests/test_footprint_host.py holds the
accounting: every ``cdml_*`` name of the header is in exactly one of ENTRIES, NO_LAUNCH and NOT_YET.

Operand roles: in (const, poisoned around the declared extent, must come back bit-identical), out (fully poisoned, every
payload element must be stored by the launch), inout (guards and reference only: the payload cannot be poisoned), ws
(exactly the queried bytes with the guard right behind; contents are scratch).  ``tol``: the tolerance of the existing
test of the same entry point, named after the colon.  ``operands`` describes the extents in words; OPERANDS below is the
structured list -- (buffer name, role) per entry -- that the GPU test compares with the buffers its launches allocate: a
launch may not use a buffer the table does not declare, and every declared buffer is used by some variant of the entry."""


def E(id, abi, operands, ref, tol, edge=""):
    return {"id": id, "abi": tuple(abi.split()), "operands": operands, "ref": ref, "tol": tol, "edge": edge}


_GATHER_OPS = "in pairs[n_pairs][2] table[n_rows][F] (row_stride > F); out idx shift x_planes[steps][rows][planes Fp]"
_NT_OPS = "in A[M][3 x K] (plane_a > K, lda > 2 plane_a + K) B[N][3 x K] bias/aux; out C[M][N] (ldc > N; planes plane_c > N)"
_NPAIR_OPS = "in S[B][B] (lds > B) ids[2B] lse[2B]; out W rows < B, columns < B of each plane / of the fp32 matrix inside [Bp][>= Bp]"

ENTRIES = [
    # ---- gather ---------------------------------------------------------------------------------------------------------
    E("sample_gather_x3", "cdml_sample_gather_x3", _GATHER_OPS, "oracle.sampler ids; fp64 l2-normalised rows",
      "atol 1e-6: test_gpu_parity gather tests; planes == split of their sum", "modes 0/1, n_steps 1/2"),
    E("sample_gather_x3k", "cdml_sample_gather_x3k", _GATHER_OPS + " x_ki[steps][3][rows/8][Fp][8]",
      "as sample_gather_x3; x_ki == torch interleave of the row-major planes", "bit-equal: test_sample_gather_writes_the_interleaved_copy",
      "modes 0/1, n_steps 1/2"),
    E("sample_gather_h2", "cdml_sample_gather_h2", _GATHER_OPS, "oracle.sampler ids; fp64 l2-normalised rows x 2^14",
      "atol 1e-6: test_gpu_parity gather tests", "modes 0/1"),
    E("gather_rows_x3", "cdml_gather_rows_x3", "in src[n][F] (row_stride > F) idx[R]; out planes[R][3 Fp] (rows of idx -1: untouched / NaN)",
      "torch split of src[idx]", "bit-equal: test_gather_rows_x3_is_the_split_of_the_gathered_rows", "with and without nan_missing"),
    # ---- splits ---------------------------------------------------------------------------------------------------------
    E("split_f32_bf16x3", "cdml_split_f32_bf16x3", "in src[rows][cols] (ld > cols); out dst 3 planes (plane > cols, ld > 2 plane + cols)",
      "torch split hi/mid/lo", "bit-equal: test_split_planes_are_exact", "plain and transposed, ragged rows/cols"),
    E("interleave8_bf16x3", "cdml_interleave8_bf16x3", "in src planes[rows][3 x cols] (plane gaps); out dst[3][rows/8][cols][8]",
      "torch permute", "bit-equal: test_gemm_x3_tnk_equals_tn"),
    E("split_f32_f16x2", "cdml_split_f32_f16x2", "in src[rows][cols] (ld > cols); out dst 2 planes (plane > cols)",
      "torch split hi/lo of src * scale", "bit-equal: tests/test_gpu_f16x2.py split test", "plain and transposed"),
    # ---- k-contiguous plane GEMM, one entry per epilogue -------------------------------------------------------------------
    E("x3_nt_bias_lrelu_f32", "cdml_gemm_bf16x3_nt", _NT_OPS, "fp64 lrelu(A B^T + bias)", "5e-6 rel max: test_gemm_x3_nt_matches_fp64_like_fp32",
      "M = 300 / 1000 as full tiles (last row tile ends in its first / second half), M = 1000 as half tiles, K = 192 (odd K-tiles)"),
    E("x3_nt_slab_n256", "cdml_gemm_bf16x3_nt", _NT_OPS + "; ws slabs", "fp64 lrelu(A B^T + bias)",
      "5e-6 rel max: test_gemm_x3_nt_matches_fp64_like_fp32", "N = 256 with workspace, K = 1344 (21 K-tiles), M = 300, the slab product's full-tile and half-tile launch"),
    E("x3_nt_f32_colsum", "cdml_gemm_bf16x3_nt", _NT_OPS + " colsum[N]; ws", "fp64 A B^T, B.sum(1)",
      "3e-6 / 5e-6 rel max: test_gemm_x3_nt_row_bias_planes_and_colsum", "M = 512 (colsum needs M % 256 == 0), K = 192"),
    E("x3_nt_bias_lrelu_x3", "cdml_gemm_bf16x3_nt", _NT_OPS, "fp64 lrelu(A B^T + bias)", "2e-6 rel max: test_gemm_x3_nt_plane_outputs_and_mask",
      "M = 300 / 1000 as full tiles, M = 1000 as half tiles"),
    E("x3_nt_rowbias_lrelu_x3", "cdml_gemm_bf16x3_nt", _NT_OPS, "fp64 lrelu(A B^T + bias[row])",
      "3e-6 rel max: test_gemm_x3_nt_row_bias_planes_and_colsum", "M = 300 / 1000 as full tiles, M = 1000 as half tiles"),
    E("x3_nt_bias_lrelu_x3_bits", "cdml_gemm_bf16x3_nt", _NT_OPS + "; out bits[M][N/8] (ldaux > N/8)", "fp64 lrelu(A B^T + bias); bits == (C > 0)",
      "2e-6 rel max; bits exact: test_sign_bitmask_epilogues_equal_the_value_mask", "M = 300 / 1000 as full tiles, M = 1000 as half tiles"),
    E("x3_nt_mask_x3", "cdml_gemm_bf16x3_nt", _NT_OPS, "fp64 (A B^T) * (aux > 0 ? 1 : alpha)", "2e-6 rel max: test_gemm_x3_nt_plane_outputs_and_mask",
      "M = 300 / 1000 as full tiles, M = 1000 as half tiles"),
    E("x3_nt_maskbits_x3", "cdml_gemm_bf16x3_nt", _NT_OPS, "fp64 (A B^T) * (bit ? 1 : alpha)", "2e-6 rel max: test_gemm_x3_nt_plane_outputs_and_mask",
      "M = 300 / 1000 as full tiles, M = 1000 as half tiles"),
    E("x3_nt_maskbits_x3_ki", "cdml_gemm_bf16x3_nt", _NT_OPS + "; out C[3][M/8][ldc > N][8]", "fp64 (A B^T) * (bit ? 1 : alpha), interleaved",
      "2e-6 rel max: test_gemm_x3_nt_plane_outputs_and_mask", "M = 328 / 1000 (multiples of 8, not of 64) as full tiles, M = 1000 as half tiles"),
    # ---- k-strided plane GEMMs ------------------------------------------------------------------------------------------------
    E("x3_tn", "cdml_gemm_bf16x3_tn", "in A[K][3 x M] B[K][3 x N] (plane gaps, ld gaps); out C[M][N] (ldc > N) colsum[N]; ws",
      "fp64 A^T B, B.sum(0)", "5e-6 rel max: test_gemm_x3_tn_weight_gradient", "K = 384 (three 128-row steps), with and without bias"),
    E("x3_tn_split_k", "cdml_gemm_bf16x3_tn", "as x3_tn", "fp64 A^T B, B.sum(0)", "5e-6 rel max, colsum 1e-4 abs: test_split_k_geometry_has_no_empty_split",
      "M = N = 256, K = 3072"),
    E("x3_tnk", "cdml_gemm_bf16x3_tnk", "in A[3][K/8][ma][8] B[3][K/8][nb][8] (columns outside the window are data); out C colsum; ws",
      "fp64 A[:, a0:a0+M]^T B[:, b0:b0+N]", "5e-6 rel max: test_gemm_x3_tnk_equals_tn", "a_col0 = 256, b_col0 = 256"),
    # ---- two-fp16-plane GEMMs -------------------------------------------------------------------------------------------------
    E("h2_nt", "cdml_gemm_f16x2_nt", "as the bf16x3 entries with two fp16 planes; epilogues 1, 3, 6, 7, 9, 10 and the N = 256 slab form",
      "fp64 as the bf16x3 entries", "2e-6 rel max: test_ragged_rows_and_small_shapes of tests/test_gpu_f16x2.py; plane scales by its _scale() rule",
      "M = 300 / 1000 (last row tile ends in its first / second half; the fp16 form has no half-tile launch)"),
    E("h2_tn", "cdml_gemm_f16x2_tn", "as x3_tn with two fp16 planes", "fp64 A^T B, B.sum(0)", "2e-6 rel max, product and colsum: test_resident_plane_walk_equals_the_general_loop of tests/test_gpu_f16x2.py",
      "K = 384; K = 3072"),
    # ---- tail and loss ---------------------------------------------------------------------------------------------------------
    E("vnet_tail_planes", "cdml_vnet_tail_planes", "in z[rows][D] (ldz > D) rows shift; out e pos neg hinge valid dz2 planes (plane_bf > D) stats[0..3]",
      "fp64 l2norm -> hinge -> gradients in torch", "1e-6 abs: test_gpu_parity tail tests; planes == split of dz2; bit for bit on exact operands, corner / clamp / masks included: tests/test_gpu_exact_tail.py", "modes 0 and 1"),
    E("triplet_hinge_indexed", "cdml_triplet_hinge_indexed", "in e[2B][D] (lde > D) neg_row[B]; out pos neg hinge stats de[2B][D]; ws scale_scratch[B]",
      "fp64 hinge over (2i, 2i+1, neg_row[i]) in torch", "1e-6: test_gpu_parity indexed hinge tests; bit for bit on exact operands, corner / clamp / masks included: tests/test_gpu_exact_tail.py", "masked triplets (-1), rows mined twice"),
    E("triplet_hinge_indexed_tail", "cdml_triplet_hinge_indexed_tail", "as triplet_hinge_indexed + in z; out dz2 dz2 planes (plane_bf > D)",
      "fp64 hinge + l2norm backward + lrelu' in torch", "1e-6: test_gpu_parity indexed hinge tests; planes == split of dz2; bit for bit on exact operands, corner / clamp / masks included: tests/test_gpu_exact_tail.py"),
    E("semihard_mine_x3", "cdml_semihard_mine_x3", "in e[2B][D] rows[2B]; out e_planes sqn dp neg_row; ws",
      "fp64 distances, the semi-hard rule", "2e-6 on the distances: test_gpu_parity / test_gpu_f32x3 semi-hard checks; bit for bit, ties included: tests/test_gpu_exact_select.py"),
    E("l2norm_fwd", "cdml_l2norm_fwd", "in x[M][N] (ldx > N); out y[M][N] (ldy > N) inv[M]", "fp64 x rsqrt(max(sum x^2, 1e-12))", "1e-6: test_gpu_parity l2norm; bit for bit on exact operands, corner / clamp / masks included: tests/test_gpu_exact_tail.py"),
    E("l2norm_bwd", "cdml_l2norm_bwd", "in z g; out dz (ld > N)", "fp64 l2norm backward (+ lrelu')", "1e-6: test_gpu_parity l2norm; bit for bit on exact operands, corner / clamp / masks included: tests/test_gpu_exact_tail.py"),
    # ---- N-pair family ---------------------------------------------------------------------------------------------------------
    E("npair_stats", "cdml_npair_stats", "in S ids; out lse[2B] stats[4]; ws", "tests/npair_ref.py", "1e-5: tests/test_gpu_npair.py", "B = 200 in Bp = 256"),
    E("npair_grad_x3", "cdml_npair_grad_x3", _NPAIR_OPS, "tests/npair_ref.py W", "1e-4 rel: tests/test_gpu_npair.py", "B = 200 in Bp = 256: the pad of W keeps its poison"),
    E("npair_grad_f32", "cdml_npair_grad_f32", _NPAIR_OPS, "tests/npair_ref.py W", "1e-4 rel: tests/test_gpu_npair.py", "B = 200 in Bp = 256"),
    E("npair_memory_stats", "cdml_npair_memory_stats", "in S[B][mem_col + M] ids mem_id; out lse stats; ws", "tests/npair_memory_ref.py",
      "1e-5: tests/test_gpu_npair_memory.py", "B = 200, mem_col = 256, M = 64 with empty slots"),
    E("npair_memory_grad_x3", "cdml_npair_memory_grad_x3", "out the memory block of W's planes only", "tests/npair_memory_ref.py W_mem", "1e-4 rel: tests/test_gpu_npair_memory.py"),
    E("npair_memory_grad_f32", "cdml_npair_memory_grad_f32", "out the memory block of W only", "tests/npair_memory_ref.py W_mem", "1e-4 rel: tests/test_gpu_npair_memory.py"),
    E("npair_memory_push", "cdml_npair_memory_push", "in P ids; inout mem mem_id R3 T3 (the ring: only the step's B slots change)", "tests/npair_memory_ref.py ring_after",
      "bit-equal: tests/test_gpu_npair_memory.py push test", "three pushes into a two-batch ring: a wrap"),
    E("npair_logq_stats", "cdml_npair_logq_stats", "as npair_stats + in bias[2B]", "tests/npair_logq_ref.py", "1e-5: tests/test_gpu_npair_logq.py"),
    E("npair_logq_grad_x3", "cdml_npair_logq_grad_x3", _NPAIR_OPS + " bias", "tests/npair_logq_ref.py W", "1e-4 rel: tests/test_gpu_npair_logq.py"),
    E("npair_logq_grad_f32", "cdml_npair_logq_grad_f32", _NPAIR_OPS + " bias", "tests/npair_logq_ref.py W", "1e-4 rel: tests/test_gpu_npair_logq.py"),
    E("npair_memory_logq_stats", "cdml_npair_memory_logq_stats", "as npair_memory_stats + in bias mem_bias", "tests/npair_logq_ref.py", "1e-5: tests/test_gpu_npair_logq.py"),
    E("npair_memory_logq_grad_x3", "cdml_npair_memory_logq_grad_x3", "out the memory block of W's planes only", "tests/npair_logq_ref.py W_mem", "1e-4 rel: tests/test_gpu_npair_logq.py"),
    E("npair_memory_logq_grad_f32", "cdml_npair_memory_logq_grad_f32", "out the memory block of W only", "tests/npair_logq_ref.py W_mem", "1e-4 rel: tests/test_gpu_npair_logq.py"),
    E("logq_table_gather", "cdml_logq_table_gather", "in table[n_videos] ids[2B] mem_id[M]; out bias[2B] mem_bias[M]", "table[id], 0 for -1 / out of range", "bit-equal: tests/test_gpu_npair_logq.py"),
    E("logq_stream_gather", "cdml_logq_stream_gather", "in last gap ids mem_id; out bias mem_bias snap_last[B] snap_gap[B]", "-log(gap[id]) in fp64", "1e-6: tests/test_gpu_npair_logq.py"),
    E("logq_stream_update", "cdml_logq_stream_update", "in ids snap_last snap_gap; inout last gap (the state past n_videos is a guard band)", "tests/npair_logq_ref.py estimator_after",
      "bit-equal: tests/test_gpu_npair_logq.py"),
    E("logq_stream_reset", "cdml_logq_stream_reset", "out last[n] gap[n]", "-1 / g0", "bit-equal"),
    # ---- optimizers -------------------------------------------------------------------------------------------------------------
    E("adam_step", "cdml_adam_step", "in g; inout w m v t_dev tickets", "fp64 Adam (TensorFlow form)", "1e-6: test_gpu_parity optimizer tests", "n = 1003 (not a multiple of 4)"),
    E("adam_matrix_planes", "cdml_adam_matrix_planes", "in g; inout W m v bias; out wt[N][3 x K] wc[K][3 x N] (plane gaps, ld gaps)", "fp64 Adam; planes sum to the new W exactly",
      "1e-6; bit-equal planes: smoke / test_gpu_f32x3 train-step tests"),
    E("lars_matrix", "cdml_lars_multi_norms cdml_lars_matrix", "in g; inout flat w acc; out wt wc planes norms; ws scratch", "fp64 LARS per segment", "1e-6: test_gpu_parity optimizer tests; planes sum to W"),
    E("momentum_matrix", "cdml_momentum_matrix", "in g; inout W acc bias; out wt wc planes", "fp64 ApplyMomentum (Nesterov)", "1e-6: test_gpu_parity optimizer tests; planes sum to W"),
    E("grad_prepare", "cdml_grad_prepare", "in w; inout g; out norms[2]; ws scratch", "fp64 g + l2 w, clip by norm", "2e-6 rel: test_gpu_parity grad_prepare test"),
    # ---- export and eval ----------------------------------------------------------------------------------------------------------
    E("row_sqnorm", "cdml_row_sqnorm", "in x[n][D] (ldx > D); out out[n]", "fp64 sum of squares", "1e-6 rel"),
    E("knn_merge", "cdml_knn_merge", "in scores[nq][nb] (lds > nb) q_sq b_sq; out best_d best_i [nq][128] (first = 1 starts the lists: all 128 columns are written)",
      "fp64 top-k by (distance, id)", "1e-5: tests/test_gpu_knn.py; bit for bit, ties included: tests/test_gpu_exact_select.py", "two blocks, n_valid inside the second"),
    E("knn_filter_x3", "cdml_knn_filter_x3", "in Q B planes q_sq b_sq tau; inout cnt[nq]; out cand[nq][cap][2] up to min(cnt, cap) slots, the guard right after cap entries",
      "fp64 distances <= tau as a set", "1e-5: tests/test_gpu_knn.py; bit for bit, ties included: tests/test_gpu_exact_select.py", "a capacity no list reaches and one every list overflows"),
    E("knn_merge_list", "cdml_knn_merge_list", "in cand; inout cnt (back to 0) best_d best_i; out overflow", "fp64 merge by (distance, id)", "1e-5: tests/test_gpu_knn.py; bit for bit, ties included: tests/test_gpu_exact_select.py", "with and without overflow"),
    E("rank_tau_x3", "cdml_rank_tau_x3", "in Q[nq] P[nq up to 256] planes q_sq p_sq; out tau[nq]", "fp64 max(|q|^2 + |p|^2 - 2 q.p, 0)", "1e-5: tests/test_gpu_retrieval.py; bit for bit, ties included: tests/test_gpu_exact_select.py", "nq = 300"),
    E("rank_count_x3", "cdml_rank_count_x3", "in Q B planes q_sq b_sq tau pos_id self_id; inout count[nq]", "fp64 rank by (distance, id)", "ranks equal off near-ties (1e-5): tests/test_gpu_retrieval.py; bit for bit, ties included: tests/test_gpu_exact_select.py",
      "n_valid = 700 inside the last 256-row tile, two launches accumulate"),
    E("knn_desim_prep", "cdml_knn_desim_prep", "in fI[n_f][kf] (ldf > kf) fD; out out[n_f][kp]", "oracle rule in numpy", "exact: tests/test_gpu_knn_desim.py", "int32 and int64 ids"),
    E("knn_desim", "cdml_knn_desim", "in eI[nq][ke] (lde > ke) f_filtered; out out[nq][ke] (ldo > ke)", "greedy rule in numpy", "exact: tests/test_gpu_knn_desim.py"),
]

# ---- queries and setters that enqueue nothing -------------------------------------------------------------------------------------
NO_LAUNCH = {
    "cdml_version": "returns the ABI version",
    "cdml_last_error": "returns the calling thread's last message",
    "cdml_build_id": "returns the embedded source hash",
    "cdml_fc_bwd_weight_workspace": "size query",
    "cdml_fc_bwd_weight2_workspace": "size query",
    "cdml_vnet_tail_workspace": "size query",
    "cdml_cowatch_workspace": "size query",
    "cdml_knn_list_capacity": "returns CDML_KNN_LIST",
    "cdml_gemm_bf16_workspace": "size query",
    "cdml_gemm_bf16_epilogue_supported": "shape query",
    "cdml_gemm_bf16_tn_supported": "shape query",
    "cdml_gemm_bf16_tn_workspace": "size query",
    "cdml_gemm_bf16_tn2_workspace": "size query",
    "cdml_x3_slab_steps": "sets a thread-local pin on the host",
    "cdml_colsum_workspace_floats": "size query",
    "cdml_lars_scratch_floats": "size query",
    "cdml_lars_multi_scratch_floats": "size query",
    "cdml_gemm_bf16x3_workspace": "size query (the x3 GEMM entries allocate exactly what it returns)",
    "cdml_gemm_f16x2_workspace": "size query (the h2 GEMM entries allocate exactly what it returns)",
    "cdml_npair_workspace": "size query (npair_stats allocates exactly what it returns)",
    "cdml_npair_memory_workspace": "size query (npair_memory_stats allocates exactly what it returns)",
    "cdml_semihard_mine_x3_workspace": "size query (semihard_mine_x3 allocates exactly what it returns)",
}

# ---- launches without a footprint entry yet, one by one -----------------------------------------------------------------------------
NOT_YET = [
    "cdml_fill_uniform_table", "cdml_sample_uniform", "cdml_sample_inbatch", "cdml_step_advance", "cdml_gather_rows",
    "cdml_route_rows", "cdml_scatter_rows", "cdml_sample_gather", "cdml_fc_lrelu_fwd", "cdml_fc_bwd_data", "cdml_fc_bwd_weight",
    "cdml_fc_bwd_weight2", "cdml_triplet_hinge", "cdml_triplet_hinge_inbatch", "cdml_vnet_tail", "cdml_semihard_select",
    "cdml_semihard_mine_x3_z", "cdml_pair_dist", "cdml_cowatch_graph", "cdml_cowatch_select", "cdml_rank_tau_h2", "cdml_rank_count_h2",
    "cdml_adam_matrix_bf16", "cdml_gemm_bf16_nt", "cdml_gemm_bf16_tn", "cdml_gemm_bf16_tn2", "cdml_vnet_tail_h2", "cdml_semihard_mine_h2",
    "cdml_knn_filter_h2", "cdml_lars_matrix_h2", "cdml_momentum_matrix_h2", "cdml_adam_matrix_h2", "cdml_transpose_to_bf16",
    "cdml_cast_f32_bf16", "cdml_colsum", "cdml_fill_uniform_table_f16", "cdml_gather_rows_f16", "cdml_sample_gather_f16",
    "cdml_ew_combine", "cdml_ew_fusion_bwd", "cdml_lrelu_bwd", "cdml_momentum_step", "cdml_table_adam_rows", "cdml_lars_step",
    "cdml_lars_multi",
]

# ---- the launches this table must hold (the headline step, BASELINE config 2, the N-pair chain, export / eval) ------------------------
REQUIRED = [
    "cdml_sample_gather_x3", "cdml_sample_gather_x3k", "cdml_gather_rows_x3", "cdml_sample_gather_h2",
    "cdml_split_f32_bf16x3", "cdml_interleave8_bf16x3", "cdml_split_f32_f16x2",
    "cdml_gemm_bf16x3_nt", "cdml_gemm_bf16x3_tn", "cdml_gemm_bf16x3_tnk", "cdml_gemm_f16x2_nt", "cdml_gemm_f16x2_tn",
    "cdml_vnet_tail_planes", "cdml_triplet_hinge_indexed", "cdml_triplet_hinge_indexed_tail", "cdml_semihard_mine_x3",
    "cdml_l2norm_fwd", "cdml_l2norm_bwd",
    "cdml_npair_stats", "cdml_npair_grad_x3", "cdml_npair_grad_f32", "cdml_npair_memory_stats", "cdml_npair_memory_grad_x3",
    "cdml_npair_memory_grad_f32", "cdml_npair_memory_push", "cdml_npair_logq_stats", "cdml_npair_logq_grad_x3",
    "cdml_npair_logq_grad_f32", "cdml_npair_memory_logq_stats", "cdml_npair_memory_logq_grad_x3", "cdml_npair_memory_logq_grad_f32",
    "cdml_logq_table_gather", "cdml_logq_stream_gather", "cdml_logq_stream_update", "cdml_logq_stream_reset",
    "cdml_adam_step", "cdml_adam_matrix_planes", "cdml_lars_matrix", "cdml_momentum_matrix", "cdml_grad_prepare",
    "cdml_row_sqnorm", "cdml_knn_filter_x3", "cdml_knn_merge_list", "cdml_knn_merge", "cdml_rank_tau_x3", "cdml_rank_count_x3",
    "cdml_knn_desim_prep", "cdml_knn_desim",
]
# the epilogues of cdml_gemm_bf16x3_nt that must each have an entry of their own
REQUIRED_ENTRY_IDS = [
    "x3_nt_bias_lrelu_f32", "x3_nt_f32_colsum", "x3_nt_bias_lrelu_x3", "x3_nt_rowbias_lrelu_x3", "x3_nt_bias_lrelu_x3_bits",
    "x3_nt_mask_x3", "x3_nt_maskbits_x3", "x3_nt_maskbits_x3_ki", "x3_nt_slab_n256", "x3_tn_split_k",
]


# ---- (buffer name, role) of every entry's launches: what tests/test_gpu_footprint.py allocates, checked there against Case.roles ------
OPERANDS = {
    "sample_gather_x3": (("pairs", "in"), ("table", "in"), ("idx", "out"), ("shift", "out"), ("x_planes", "out"),),
    "sample_gather_x3k": (("pairs", "in"), ("table", "in"), ("idx", "out"), ("shift", "out"), ("x_ki", "out"), ("x_planes", "out"),),
    "sample_gather_h2": (("pairs", "in"), ("table", "in"), ("idx", "out"), ("shift", "out"), ("x_planes", "out"),),
    "gather_rows_x3": (("idx", "in"), ("src", "in"), ("planes", "out"),),
    "split_f32_bf16x3": (("src", "in"), ("dst", "out"),),
    "interleave8_bf16x3": (("src", "in"), ("dst", "out"),),
    "split_f32_f16x2": (("src", "in"), ("dst", "out"),),
    "x3_nt_bias_lrelu_f32": (("A", "in"), ("B", "in"), ("bias", "in"), ("C", "out"),),
    "x3_nt_slab_n256": (("A", "in"), ("B", "in"), ("bias", "in"), ("C", "out"), ("workspace", "ws"),),
    "x3_nt_f32_colsum": (("A", "in"), ("B", "in"), ("C", "out"), ("colsum", "out"), ("workspace", "ws"),),
    "x3_nt_bias_lrelu_x3": (("A", "in"), ("B", "in"), ("bias", "in"), ("C_planes", "out"),),
    "x3_nt_rowbias_lrelu_x3": (("A", "in"), ("B", "in"), ("bias", "in"), ("C_planes", "out"),),
    "x3_nt_bias_lrelu_x3_bits": (("A", "in"), ("B", "in"), ("bias", "in"), ("C_planes", "out"), ("bits", "out"),),
    "x3_nt_mask_x3": (("A", "in"), ("B", "in"), ("aux", "in"), ("C_planes", "out"),),
    "x3_nt_maskbits_x3": (("A", "in"), ("B", "in"), ("bits", "in"), ("C_planes", "out"),),
    "x3_nt_maskbits_x3_ki": (("A", "in"), ("B", "in"), ("bits", "in"), ("C_ki", "out"),),
    "x3_tn": (("A", "in"), ("B", "in"), ("bias", "in"), ("C", "out"), ("colsum", "out"), ("workspace", "ws"),),
    "x3_tn_split_k": (("A", "in"), ("B", "in"), ("C", "out"), ("colsum", "out"), ("workspace", "ws"),),
    "x3_tnk": (("A", "in"), ("B", "in"), ("C", "out"), ("colsum", "out"), ("workspace", "ws"),),
    "h2_nt": (("A", "in"), ("B", "in"), ("aux", "in"), ("bias", "in"), ("bits", "in"), ("C", "out"), ("C_planes", "out"), ("bits", "out"), ("workspace", "ws"),),
    "h2_tn": (("A", "in"), ("B", "in"), ("C", "out"), ("colsum", "out"), ("workspace", "ws"),),
    "vnet_tail_planes": (("rows", "in"), ("shift", "in"), ("z", "in"), ("dz", "out"), ("dz2_planes", "out"), ("e", "out"), ("hinge", "out"), ("neg", "out"), ("pos", "out"), ("stats", "out"), ("valid", "out"),),
    "triplet_hinge_indexed": (("e", "in"), ("neg_row", "in"), ("de", "out"), ("hinge", "out"), ("neg", "out"), ("pos", "out"), ("stats", "out"), ("scale_scratch", "ws"),),
    "triplet_hinge_indexed_tail": (("e", "in"), ("neg_row", "in"), ("z", "in"), ("de", "out"), ("dz", "out"), ("dz2_planes", "out"), ("hinge", "out"), ("neg", "out"), ("pos", "out"), ("stats", "out"), ("scale_scratch", "ws"),),
    "semihard_mine_x3": (("e", "in"), ("rows", "in"), ("dp", "out"), ("e_planes", "out"), ("neg_row", "out"), ("sqn", "out"), ("workspace", "ws"),),
    "l2norm_fwd": (("x", "in"), ("inv", "out"), ("y", "out"),),
    "l2norm_bwd": (("g", "in"), ("z", "in"), ("dz", "out"),),
    "npair_stats": (("S", "in"), ("ids", "in"), ("lse", "out"), ("stats", "out"), ("workspace", "ws"),),
    "npair_grad_x3": (("S", "in"), ("ids", "in"), ("lse", "in"), ("W", "out"),),
    "npair_grad_f32": (("S", "in"), ("ids", "in"), ("lse", "in"), ("W", "out"),),
    "npair_memory_stats": (("S", "in"), ("ids", "in"), ("mem_id", "in"), ("lse", "out"), ("stats", "out"), ("workspace", "ws"),),
    "npair_memory_grad_x3": (("S", "in"), ("ids", "in"), ("lse", "in"), ("mem_id", "in"), ("W", "out"),),
    "npair_memory_grad_f32": (("S", "in"), ("ids", "in"), ("lse", "in"), ("mem_id", "in"), ("W", "out"),),
    "npair_memory_push": (("P", "in"), ("ids", "in"), ("step_dev", "in"), ("R3_image", "inout"), ("T3_image", "inout"), ("mem", "inout"), ("mem_id", "inout"),),
    "npair_logq_stats": (("S", "in"), ("bias", "in"), ("ids", "in"), ("lse", "out"), ("stats", "out"), ("workspace", "ws"),),
    "npair_logq_grad_x3": (("S", "in"), ("bias", "in"), ("ids", "in"), ("lse", "in"), ("W", "out"),),
    "npair_logq_grad_f32": (("S", "in"), ("bias", "in"), ("ids", "in"), ("lse", "in"), ("W", "out"),),
    "npair_memory_logq_stats": (("S", "in"), ("bias", "in"), ("ids", "in"), ("mem_bias", "in"), ("mem_id", "in"), ("lse", "out"), ("stats", "out"), ("workspace", "ws"),),
    "npair_memory_logq_grad_x3": (("S", "in"), ("ids", "in"), ("lse", "in"), ("mem_bias", "in"), ("mem_id", "in"), ("W", "out"),),
    "npair_memory_logq_grad_f32": (("S", "in"), ("ids", "in"), ("lse", "in"), ("mem_bias", "in"), ("mem_id", "in"), ("W", "out"),),
    "logq_table_gather": (("ids", "in"), ("mem_id", "in"), ("table", "in"), ("bias", "out"), ("mem_bias", "out"),),
    "logq_stream_gather": (("gap", "in"), ("ids", "in"), ("last", "in"), ("mem_id", "in"), ("bias", "out"), ("mem_bias", "out"), ("snap_gap", "out"), ("snap_last", "out"),),
    "logq_stream_update": (("ids", "in"), ("step_dev", "in"), ("gap", "inout"), ("last", "inout"), ("bias", "ws"), ("snap_gap", "ws"), ("snap_last", "ws"),),
    "logq_stream_reset": (("gap", "out"), ("last", "out"),),
    "adam_step": (("g", "in"), ("m", "inout"), ("t_dev", "inout"), ("tickets", "inout"), ("v", "inout"), ("w", "inout"),),
    "adam_matrix_planes": (("g", "in"), ("gb", "in"), ("W", "inout"), ("b", "inout"), ("m", "inout"), ("mb", "inout"), ("v", "inout"), ("vb", "inout"), ("wc", "out"), ("wt", "out"),),
    "lars_matrix": (("g", "in"), ("acc", "inout"), ("w", "inout"), ("norms", "out"), ("wc", "out"), ("wt", "out"), ("scratch", "ws"),),
    "momentum_matrix": (("g", "in"), ("gb", "in"), ("W", "inout"), ("ab", "inout"), ("acc", "inout"), ("b", "inout"), ("wc", "out"), ("wt", "out"),),
    "grad_prepare": (("w", "in"), ("g", "inout"), ("norms", "out"), ("scratch", "ws"),),
    "row_sqnorm": (("x", "in"), ("out", "out"),),
    "knn_merge": (("b_sq", "in"), ("q_sq", "in"), ("scores", "in"), ("best_d", "out"), ("best_i", "out"),),
    "knn_filter_x3": (("B", "in"), ("Q", "in"), ("b_sq", "in"), ("q_sq", "in"), ("tau", "in"), ("cand", "inout"), ("cnt", "inout"),),
    "knn_merge_list": (("B", "in"), ("Q", "in"), ("b_sq", "in"), ("q_sq", "in"), ("tau", "in"), ("best_d", "inout"), ("best_i", "inout"), ("cand", "inout"), ("cnt", "inout"), ("overflow", "inout"),),
    "rank_tau_x3": (("P", "in"), ("Q", "in"), ("p_sq", "in"), ("q_sq", "in"), ("tau", "out"),),
    "rank_count_x3": (("B", "in"), ("Q", "in"), ("b_sq", "in"), ("pos_id", "in"), ("q_sq", "in"), ("self_id", "in"), ("tau", "in"), ("count", "inout"),),
    "knn_desim_prep": (("fD", "in"), ("fI", "in"), ("out", "out"),),
    "knn_desim": (("eI", "in"), ("f_filtered", "in"), ("out", "out"),),
}


def abi_names_in_table():
    return sorted({n for e in ENTRIES for n in e["abi"]})
