// frechet_api.h -- part of the ONE translation unit csrc/mdm_api.hip: mdm_frechet_workspace_bytes and mdm_frechet_distance
// (include/mdm_hip.h) over the kernels of frechet.h.
#pragma once
// (included by mdm_api.hip behind metrics_api.h; relies on its includes, api_runtime.h, metrics_api.h's met_ptr and `using namespace mdm`)

namespace {

inline int fr_even(int D) { return (D + 1) & ~1; }

// The workspace behind its first 16-byte boundary: the header, both spectra, then seven matrices [n][n]
struct FrWorkspace {
  FrHeader* h;
  double *w1, *w2;
  double *a[2], *v[2];      // the solver's ping-pong buffers
  double *s2, *s, *t;       // sigma2's symmetric part (later M before it is symmetrised), S, T
};

inline size_t fr_ws_doubles(int n) { return sizeof(FrHeader) / 8 + 2 * (size_t)FR_MAX_D + 7 * (size_t)n * n; }

inline FrWorkspace fr_carve(void* ws, int n) {
  FrWorkspace o;
  double* p = reinterpret_cast<double*>(ws_floats(ws));
  o.h = reinterpret_cast<FrHeader*>(p);
  p += sizeof(FrHeader) / 8;
  o.w1 = p;
  o.w2 = p + FR_MAX_D;
  p += 2 * FR_MAX_D;
  const size_t nn = (size_t)n * n;
  double** m[7] = {&o.a[0], &o.a[1], &o.v[0], &o.v[1], &o.s2, &o.s, &o.t};
  for (double** q : m) {
    *q = p;
    p += nn;
  }
  return o;
}

// One symmetric eigen-solve of a[0] (symmetric, pad zero): the eigenvalues to `w`, the vectors (when wanted) to v[h->vbuf]
int fr_solve(const std::string& f, const FrWorkspace& k, int n, int D, int solve, bool vectors, double* w, hipStream_t s) {
  MDM_LAUNCH(fr_norm_kernel, dim3(1), dim3(256), 0, s, (const double*)k.a[0], n, D, k.h, solve);
  if (int rc = rt_launch_status()) return rc;
  if (n <= FR_SMALL_MAX) {
    FrSmallArgs p{k.a[0], w, vectors ? k.v[0] : nullptr, k.h, n, D, solve};
    if (int rc = launch_fr_eig_small(p, s)) return lds_fail(rc, f.c_str());
    return rt_launch_status();
  }
  const dim3 grid((unsigned)((n + 63) / 64), (unsigned)((n + FR_ROUND_ROWS - 1) / FR_ROUND_ROWS), vectors ? 2u : 1u);
  int at = 0;
  for (int sweep = 0; sweep < FR_MAX_SWEEPS; ++sweep)
    for (int round = 0; round < n - 1; ++round, at ^= 1) {
      FrRoundArgs p{k.a[at], k.a[at ^ 1], vectors ? k.v[at] : nullptr, vectors ? k.v[at ^ 1] : nullptr, k.h, n, solve, sweep, round};
      MDM_LAUNCH(fr_round_kernel, grid, dim3(256), 0, s, p);
      if (int rc = rt_launch_status()) return rc;
    }
  MDM_LAUNCH(fr_extract_kernel, dim3(1), dim3(256), 0, s, (const double*)k.a[0], (const double*)k.a[1], n, D, k.h, solve, vectors ? 1 : 0, w);
  return rt_launch_status();
}

}  // namespace

extern "C" {

size_t mdm_frechet_workspace_bytes(int32_t D) {
  if (D < 1 || D > FR_MAX_D) {
    fail(MDM_EINVAL, "mdm_frechet_workspace_bytes: D must be between 1 and 1024");
    return 0;
  }
  return fr_ws_doubles(fr_even(D)) * sizeof(double) + 64;
}

int mdm_frechet_distance(const double* mu1, const double* sigma1, const double* mu2, const double* sigma2, int32_t D, double* result4,
                         int32_t* sweeps2, void* ws, size_t ws_bytes, void* stream) {
  const std::string f = "mdm_frechet_distance: ";
  if (int rc = met_ptr(f, "mu1_dev", mu1, 8)) return rc;
  if (int rc = met_ptr(f, "sigma1_dev", sigma1, 8)) return rc;
  if (int rc = met_ptr(f, "mu2_dev", mu2, 8)) return rc;
  if (int rc = met_ptr(f, "sigma2_dev", sigma2, 8)) return rc;
  if (int rc = met_ptr(f, "result4_dev", result4, 8)) return rc;
  if (int rc = met_ptr(f, "sweeps2_dev", sweeps2, 4)) return rc;
  if (D < 1 || D > FR_MAX_D) return fail(MDM_EINVAL, f + "D must be between 1 and 1024");
  if (ws == nullptr) return fail(MDM_EINVAL, f + "null workspace_dev");
  if (ws_bytes < mdm_frechet_workspace_bytes(D)) return fail(MDM_ENOSPC, f + "workspace_bytes too small (mdm_frechet_workspace_bytes)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  ChainGuard chain_guard(stream);
  const int n = fr_even(D);
  const FrWorkspace k = fr_carve(ws, n);
  const unsigned eb = (unsigned)(((size_t)n * n + 255) / 256), gt = (unsigned)((n + 63) / 64);
  // both inputs' symmetric parts, the vectors' identity; the first solve, with vectors
  MDM_LAUNCH(fr_sym_kernel, dim3(eb), dim3(256), 0, s, sigma1, (int)D, (int)D, k.a[0], n, k.v[0]);
  if (int rc = rt_launch_status()) return rc;
  MDM_LAUNCH(fr_sym_kernel, dim3(eb), dim3(256), 0, s, sigma2, (int)D, (int)D, k.s2, n, (double*)nullptr);
  if (int rc = rt_launch_status()) return rc;
  if (int rc = fr_solve(f, k, n, D, 0, true, k.w1, s)) return rc;
  // S = V sqrt(max(w, 0)), T = sigma2 S, M = S^T T (into sigma2's buffer, which T has consumed), symmetrised into the solver's buffer
  MDM_LAUNCH(fr_scale_kernel, dim3(eb), dim3(256), 0, s, (const double*)k.v[0], (const double*)k.v[1], (const FrHeader*)k.h,
             (const double*)k.w1, k.s, n);
  if (int rc = rt_launch_status()) return rc;
  MDM_LAUNCH(fr_gemm_kernel, dim3(gt, gt), dim3(256), 0, s, (const double*)k.s2, (const double*)k.s, k.t, n);
  if (int rc = rt_launch_status()) return rc;
  MDM_LAUNCH(fr_gemm_kernel, dim3(gt, gt), dim3(256), 0, s, (const double*)k.s, (const double*)k.t, k.s2, n);
  if (int rc = rt_launch_status()) return rc;
  MDM_LAUNCH(fr_sym_kernel, dim3(eb), dim3(256), 0, s, (const double*)k.s2, n, n, k.a[0], n, (double*)nullptr);
  if (int rc = rt_launch_status()) return rc;
  if (int rc = fr_solve(f, k, n, D, 1, false, k.w2, s)) return rc;
  FrFinishArgs q{mu1, sigma1, mu2, sigma2, k.w1, k.w2, k.h, result4, sweeps2, (int)D};
  MDM_LAUNCH(fr_finish_kernel, dim3(1), dim3(64), 0, s, q);
  return rt_launch_status();
}

}  // extern "C"
