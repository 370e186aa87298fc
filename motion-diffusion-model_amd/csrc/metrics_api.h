// metrics_api.h -- part of the ONE translation unit csrc/mdm_api.hip: mdm_metrics_workspace_bytes, mdm_knn_radius,
// mdm_manifold_members, mdm_gather_dist, mdm_poly_mmd and mdm_feature_stats (include/mdm_hip.h) over the kernels of metrics.h.
// (humanml_metrics_api.h, included behind this file, shares the checks below and the workspace sizes.)
#pragma once
// (included by mdm_api.hip behind its other entry points; relies on its includes, api_runtime.h and `using namespace mdm`)

namespace {

// What every metrics call checks about a feature matrix [n][D] and about its workspace; 0 or a negative code with the message set
int met_matrix(const std::string& f, const char* name, const void* p, int n, int D) {
  if (p == nullptr) return fail(MDM_EINVAL, f + "null " + name);
  if ((reinterpret_cast<uintptr_t>(p) & 3) != 0) return fail(MDM_EINVAL, f + name + " must be 4-byte aligned");
  if (D < 1) return fail(MDM_EINVAL, f + "D must be at least 1");
  if (n < 1) return fail(MDM_EINVAL, f + name + " must hold at least one row");
  if ((int64_t)n * D >= (1ll << 31)) return fail(MDM_EUNSUPPORTED, f + name + ": rows * D must stay below 2^31");
  return 0;
}

int met_ptr(const std::string& f, const char* name, const void* p, unsigned align) {
  if (p == nullptr) return fail(MDM_EINVAL, f + "null " + name);
  if ((reinterpret_cast<uintptr_t>(p) & (align - 1)) != 0)
    return fail(MDM_EINVAL, f + name + " must be " + std::to_string(align) + "-byte aligned");
  return 0;
}

int met_ws(const std::string& f, const void* ws, size_t have, size_t need) {
  if (ws == nullptr) return fail(MDM_EINVAL, f + "null workspace_dev");
  if (need == 0) return MDM_EINVAL;      // (mdm_metrics_workspace_bytes has set the message)
  if (have < need) return fail(MDM_ENOSPC, f + "workspace_bytes too small (mdm_metrics_workspace_bytes)");
  return 0;
}

// 16-byte loads of whole rows: D a multiple of 4 and every matrix on a 16-byte boundary
int met_vec(int D, std::initializer_list<const void*> ptrs) {
  if ((D & 3) != 0) return 0;
  for (const void* p : ptrs)
    if ((reinterpret_cast<uintptr_t>(p) & 15) != 0) return 0;
  return 1;
}

inline int met_tiles(int n) { return (n + MET_TILE - 1) / MET_TILE; }

}  // namespace

extern "C" {

size_t mdm_metrics_workspace_bytes(int32_t kind, int32_t rows, int32_t subsets) {
  const char* f = "mdm_metrics_workspace_bytes: ";
  if (kind < MDM_METRICS_KNN_RADIUS || kind > MDM_METRICS_CONFUSION) { fail(MDM_EINVAL, std::string(f) + "unknown kind"); return 0; }
  if (rows < 1) { fail(MDM_EINVAL, std::string(f) + "rows must be at least 1"); return 0; }
  if (kind != MDM_METRICS_POLY_MMD) return ws_bytes_of(0);
  if (subsets < 1) { fail(MDM_EINVAL, std::string(f) + "subsets must be at least 1"); return 0; }
  if ((int64_t)subsets * rows >= (1ll << 31) || subsets > 65535) {
    fail(MDM_EUNSUPPORTED, std::string(f) + "subsets * subset_size must stay below 2^31 and subsets below 65536: chunk the subsets");
    return 0;
  }
  return ws_bytes_of((size_t)subsets * 2 * met_tiles(rows) * MMD_PARTIALS * (sizeof(double) / sizeof(float)));
}

int mdm_knn_radius(const float* a, int32_t N, int32_t D, int32_t k, float* radius2, void* ws, size_t ws_bytes, void* stream) {
  const std::string f = "mdm_knn_radius: ";
  if (int rc = met_matrix(f, "a_dev", a, N, D)) return rc;
  if (int rc = met_ptr(f, "radius2_dev", radius2, 4)) return rc;
  if (k < 1 || k > MET_KNN_MAX - 1) return fail(MDM_EINVAL, f + "k must be between 1 and 7");
  if (N < k + 1) return fail(MDM_EINVAL, f + "N must be at least k + 1 (the row itself is one of its neighbours)");
  if (int rc = met_ws(f, ws, ws_bytes, mdm_metrics_workspace_bytes(MDM_METRICS_KNN_RADIUS, N, 1))) return rc;
  ChainGuard chain_guard(stream);
  KnnArgs p{a, radius2, N, D, k, met_vec(D, {a})};
  MDM_LAUNCH(knn_radius_kernel, dim3((unsigned)met_tiles(N)), dim3(256), 0, static_cast<hipStream_t>(stream), p);
  return rt_launch_status();
}

int mdm_manifold_members(const float* a, const float* radius2, int32_t NA, const float* b, int32_t NB, int32_t D, uint8_t* member,
                         int32_t* count, void* ws, size_t ws_bytes, void* stream) {
  const std::string f = "mdm_manifold_members: ";
  if (int rc = met_matrix(f, "a_dev", a, NA, D)) return rc;
  if (int rc = met_matrix(f, "b_dev", b, NB, D)) return rc;
  if (int rc = met_ptr(f, "radius2_dev", radius2, 4)) return rc;
  if (int rc = met_ptr(f, "member_dev", member, 1)) return rc;
  if (int rc = met_ptr(f, "count_dev", count, 4)) return rc;
  if (int rc = met_ws(f, ws, ws_bytes, mdm_metrics_workspace_bytes(MDM_METRICS_MANIFOLD_MEMBERS, NB, 1))) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  ChainGuard chain_guard(stream);
  MemberArgs p{a, radius2, b, member, NA, NB, D, met_vec(D, {a, b})};
  MDM_LAUNCH(manifold_members_kernel, dim3((unsigned)met_tiles(NB)), dim3(256), 0, s, p);
  if (int rc = rt_launch_status()) return rc;
  MDM_LAUNCH(count_members_kernel, dim3(1), dim3(256), 0, s, (const uint8_t*)member, (int)NB, (int*)count);
  return rt_launch_status();
}

int mdm_gather_dist(const float* x, int32_t N, int32_t D, const int32_t* first, const int32_t* second, int32_t P, float* dist,
                    double* mean, void* ws, size_t ws_bytes, void* stream) {
  const std::string f = "mdm_gather_dist: ";
  if (int rc = met_matrix(f, "x_dev", x, N, D)) return rc;
  if (int rc = met_ptr(f, "first_dev", first, 4)) return rc;
  if (int rc = met_ptr(f, "second_dev", second, 4)) return rc;
  if (int rc = met_ptr(f, "dist_dev", dist, 4)) return rc;
  if (int rc = met_ptr(f, "mean_dev", mean, 8)) return rc;
  if (P < 1) return fail(MDM_EINVAL, f + "P must be at least 1");
  if (int rc = met_ws(f, ws, ws_bytes, mdm_metrics_workspace_bytes(MDM_METRICS_GATHER_DIST, N, 1))) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  ChainGuard chain_guard(stream);
  GatherDistArgs p{x, first, second, dist, P, D, met_vec(D, {x})};
  MDM_LAUNCH(gather_dist_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, p);
  if (int rc = rt_launch_status()) return rc;
  MDM_LAUNCH(mean_f64_kernel, dim3(1), dim3(256), 0, s, (const float*)dist, (int)P, mean);
  return rt_launch_status();
}

int mdm_poly_mmd(const float* g, int32_t Ng, const float* r, int32_t Nr, int32_t D, const int32_t* idx_g, const int32_t* idx_r, int32_t S,
                 int32_t m, double gamma, double coef0, int32_t degree, int32_t var_at_m, double* mmd2, double* var, void* ws,
                 size_t ws_bytes, void* stream) {
  const std::string f = "mdm_poly_mmd: ";
  if (int rc = met_matrix(f, "g_dev", g, Ng, D)) return rc;
  if (int rc = met_matrix(f, "r_dev", r, Nr, D)) return rc;
  if (int rc = met_ptr(f, "idx_g_dev", idx_g, 4)) return rc;
  if (int rc = met_ptr(f, "idx_r_dev", idx_r, 4)) return rc;
  if (int rc = met_ptr(f, "mmd2_dev", mmd2, 8)) return rc;
  if (int rc = met_ptr(f, "var_dev", var, 8)) return rc;
  if (S < 1) return fail(MDM_EINVAL, f + "S must be at least 1");
  if (m < 3) return fail(MDM_EINVAL, f + "m must be at least 3 (the variance estimate divides by m - 2)");
  if (degree < 1) return fail(MDM_EINVAL, f + "degree must be at least 1");
  if (var_at_m < 2) return fail(MDM_EINVAL, f + "var_at_m must be at least 2");
  if (int rc = met_ws(f, ws, ws_bytes, mdm_metrics_workspace_bytes(MDM_METRICS_POLY_MMD, m, S))) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  ChainGuard chain_guard(stream);
  double* partial = reinterpret_cast<double*>(ws_floats(ws));
  const int tiles = met_tiles(m);
  PolyMmdArgs p{g, r, idx_g, idx_r, partial, gamma, coef0, m, D, degree, tiles, met_vec(D, {g, r})};
  MDM_LAUNCH(poly_mmd_kernel, dim3((unsigned)tiles, 2u, (unsigned)S), dim3(256), 0, s, p);
  if (int rc = rt_launch_status()) return rc;
  PolyMmdFinishArgs q{partial, mmd2, var, S, m, tiles, var_at_m};
  MDM_LAUNCH(poly_mmd_finish_kernel, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, s, q);
  return rt_launch_status();
}

int mdm_feature_stats(const float* x, int32_t N, int32_t D, double* mu, double* sigma, void* ws, size_t ws_bytes, void* stream) {
  const std::string f = "mdm_feature_stats: ";
  if (int rc = met_matrix(f, "x_dev", x, N, D)) return rc;
  if (int rc = met_ptr(f, "mu_dev", mu, 8)) return rc;
  if (int rc = met_ptr(f, "sigma_dev", sigma, 8)) return rc;
  if (N < 2) return fail(MDM_EINVAL, f + "N must be at least 2 (the covariance divides by N - 1)");
  if ((int64_t)D * D >= (1ll << 31)) return fail(MDM_EUNSUPPORTED, f + "D * D must stay below 2^31");
  if (int rc = met_ws(f, ws, ws_bytes, mdm_metrics_workspace_bytes(MDM_METRICS_FEATURE_STATS, N, 1))) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  ChainGuard chain_guard(stream);
  MDM_LAUNCH(feature_mean_kernel, dim3((unsigned)((D + 255) / 256)), dim3(256), 0, s, x, (int)N, (int)D, mu);
  if (int rc = rt_launch_status()) return rc;
  const unsigned ct = (unsigned)((D + COV_TILE - 1) / COV_TILE);
  MDM_LAUNCH(feature_cov_kernel, dim3(ct, ct), dim3(256), 0, s, x, (const double*)mu, (int)N, (int)D, sigma);
  return rt_launch_status();
}

}  // extern "C"
