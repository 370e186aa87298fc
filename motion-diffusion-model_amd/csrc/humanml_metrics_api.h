// humanml_metrics_api.h -- part of the ONE translation unit csrc/mdm_api.hip: mdm_retrieval_ranks, mdm_dist_matrix and mdm_confusion
// (include/mdm_hip.h) over the kernels of humanml_metrics.h.  Their workspace sizes are mdm_metrics_workspace_bytes' (metrics_api.h).
#pragma once
// (included by mdm_api.hip behind metrics_api.h; relies on its met_matrix / met_ptr / met_ws / met_vec / met_tiles)

extern "C" {

int mdm_retrieval_ranks(const float* q, const float* c, int32_t N, int32_t D, const int32_t* group_offsets, int32_t n_groups,
                        int32_t max_group_rows, int32_t top_k, int32_t* rank, float* diag, int64_t* topk_count, double* diag_sum,
                        void* ws, size_t ws_bytes, void* stream) {
  const std::string f = "mdm_retrieval_ranks: ";
  if (int rc = met_matrix(f, "q_dev", q, N, D)) return rc;
  if (int rc = met_matrix(f, "c_dev", c, N, D)) return rc;
  if (int rc = met_ptr(f, "group_offsets_dev", group_offsets, 4)) return rc;
  if (int rc = met_ptr(f, "rank_dev", rank, 4)) return rc;
  if (int rc = met_ptr(f, "diag_dev", diag, 4)) return rc;
  if (int rc = met_ptr(f, "topk_count_dev", topk_count, 8)) return rc;
  if (int rc = met_ptr(f, "diag_sum_dev", diag_sum, 8)) return rc;
  if (n_groups < 1) return fail(MDM_EINVAL, f + "n_groups must be at least 1");
  if (max_group_rows < 1) return fail(MDM_EINVAL, f + "max_group_rows must be at least 1");
  if (top_k < 1 || top_k > RET_TOPK_MAX) return fail(MDM_EINVAL, f + "top_k must be between 1 and 16");
  const int row_tiles = met_tiles(min(max_group_rows, N));
  if ((int64_t)n_groups * row_tiles >= (1ll << 31)) return fail(MDM_EUNSUPPORTED, f + "n_groups * ceil(max_group_rows / 64) must stay below 2^31");
  if (int rc = met_ws(f, ws, ws_bytes, mdm_metrics_workspace_bytes(MDM_METRICS_RETRIEVAL_RANKS, N, 1))) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  ChainGuard chain_guard(stream);
  RetrievalArgs p{q, c, group_offsets, rank, diag, N, D, n_groups, min(max_group_rows, N), row_tiles, met_vec(D, {q, c})};
  MDM_LAUNCH(retrieval_ranks_kernel, dim3((unsigned)(n_groups * row_tiles)), dim3(256), 0, s, p);
  if (int rc = rt_launch_status()) return rc;
  MDM_LAUNCH(retrieval_finish_kernel, dim3(1), dim3(256), 0, s, (const int*)rank, (const float*)diag, (int)N, (int)top_k,
             reinterpret_cast<long long*>(topk_count), diag_sum);
  return rt_launch_status();
}

int mdm_dist_matrix(const float* a, int32_t NA, const float* b, int32_t NB, int32_t D, float* out, void* ws, size_t ws_bytes,
                    void* stream) {
  const std::string f = "mdm_dist_matrix: ";
  if (int rc = met_matrix(f, "a_dev", a, NA, D)) return rc;
  if (int rc = met_matrix(f, "b_dev", b, NB, D)) return rc;
  if (int rc = met_ptr(f, "out_dev", out, 4)) return rc;
  if ((int64_t)NA * NB >= (1ll << 31)) return fail(MDM_EUNSUPPORTED, f + "NA * NB must stay below 2^31");
  if (met_tiles(NA) > 65535) return fail(MDM_EUNSUPPORTED, f + "NA must stay below 65536 * 64: chunk the rows of a_dev");
  if (int rc = met_ws(f, ws, ws_bytes, mdm_metrics_workspace_bytes(MDM_METRICS_DIST_MATRIX, NA, 1))) return rc;
  ChainGuard chain_guard(stream);
  DistMatrixArgs p{a, b, out, NA, NB, D, met_vec(D, {a, b})};
  MDM_LAUNCH(dist_matrix_kernel, dim3((unsigned)met_tiles(NB), (unsigned)met_tiles(NA)), dim3(256), 0, static_cast<hipStream_t>(stream), p);
  return rt_launch_status();
}

int mdm_confusion(const float* yhat, const int32_t* labels, int32_t N, int32_t C, int32_t* pred, int64_t* confusion, int32_t* bad,
                  void* ws, size_t ws_bytes, void* stream) {
  const std::string f = "mdm_confusion: ";
  if (yhat != nullptr && C < 1) return fail(MDM_EINVAL, f + "C must be at least 1");
  if (int rc = met_matrix(f, "yhat_dev", yhat, N, C)) return rc;        // (its D is the number of classes C)
  if (int rc = met_ptr(f, "labels_dev", labels, 4)) return rc;
  if (int rc = met_ptr(f, "pred_dev", pred, 4)) return rc;
  if (int rc = met_ptr(f, "confusion_dev", confusion, 8)) return rc;
  if (int rc = met_ptr(f, "bad_dev", bad, 4)) return rc;
  if ((int64_t)C * C >= (1ll << 31)) return fail(MDM_EUNSUPPORTED, f + "C * C must stay below 2^31");
  if (int rc = met_ws(f, ws, ws_bytes, mdm_metrics_workspace_bytes(MDM_METRICS_CONFUSION, N, 1))) return rc;
  ChainGuard chain_guard(stream);
  ConfusionArgs p{yhat, labels, pred, reinterpret_cast<long long*>(confusion), bad, N, C};
  MDM_LAUNCH(confusion_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), p);
  return rt_launch_status();
}

}  // extern "C"
