// smplify_api.h -- part of the ONE translation unit csrc/mdm_api.hip: mdm_smplify_workspace_bytes, mdm_smplify_value_grad,
// mdm_smplify_fit and mdm_smplify_strong_wolfe (include/mdm_hip.h) over the kernels of smplify.h.  The control flow of
// torch.optim.LBFGS.step with line_search_fn='strong_wolfe' (torch 2.10 torch/optim/lbfgs.py) runs here, on the host.
#pragma once
// (included by mdm_api.hip behind its other entry points; relies on its includes, api_runtime.h and `using namespace mdm`)

namespace {

// A scalar of torch's LBFGS code: a Python float (double) or a 0-dim float32 tensor.  An operation with a tensor operand gives a
// tensor and is computed in float on the operands rounded to float, as torch does for a wrapped Python number; comparisons likewise.
struct SmfNum {
  double v = 0.0;
  bool t32 = false;
};
inline SmfNum smf_py(double v) { return SmfNum{v, false}; }
inline SmfNum smf_t32(float v) { return SmfNum{(double)v, true}; }
inline SmfNum operator+(SmfNum a, SmfNum b) { return (a.t32 || b.t32) ? smf_t32((float)a.v + (float)b.v) : smf_py(a.v + b.v); }
inline SmfNum operator-(SmfNum a, SmfNum b) { return (a.t32 || b.t32) ? smf_t32((float)a.v - (float)b.v) : smf_py(a.v - b.v); }
inline SmfNum operator*(SmfNum a, SmfNum b) { return (a.t32 || b.t32) ? smf_t32((float)a.v * (float)b.v) : smf_py(a.v * b.v); }
inline SmfNum operator/(SmfNum a, SmfNum b) { return (a.t32 || b.t32) ? smf_t32((float)a.v / (float)b.v) : smf_py(a.v / b.v); }
inline SmfNum operator-(SmfNum a) { return SmfNum{-a.v, a.t32}; }
inline bool operator<(SmfNum a, SmfNum b) { return (a.t32 || b.t32) ? (float)a.v < (float)b.v : a.v < b.v; }
inline bool operator>(SmfNum a, SmfNum b) { return b < a; }
inline bool operator<=(SmfNum a, SmfNum b) { return (a.t32 || b.t32) ? (float)a.v <= (float)b.v : a.v <= b.v; }
inline bool operator>=(SmfNum a, SmfNum b) { return b <= a; }
inline SmfNum smf_abs(SmfNum a) { return SmfNum{std::fabs(a.v), a.t32}; }
inline SmfNum smf_sqrt(SmfNum a) { return a.t32 ? smf_t32(std::sqrt((float)a.v)) : smf_py(std::sqrt(a.v)); }
inline SmfNum smf_max(SmfNum a, SmfNum b) { return b > a ? b : a; }     // Python's max(a, b) and min(a, b): the first unless the
inline SmfNum smf_min(SmfNum a, SmfNum b) { return b < a ? b : a; }     // second is strictly beyond it; the object keeps its type

// torch/optim/lbfgs.py _cubic_interpolate
SmfNum smf_cubic(SmfNum x1, SmfNum f1, SmfNum g1, SmfNum x2, SmfNum f2, SmfNum g2, const SmfNum* bounds) {
  SmfNum lo, hi;
  if (bounds != nullptr) { lo = bounds[0]; hi = bounds[1]; }
  else if (x1 <= x2) { lo = x1; hi = x2; }
  else { lo = x2; hi = x1; }
  const SmfNum d1 = g1 + g2 - smf_py(3.0) * (f1 - f2) / (x1 - x2);
  const SmfNum d2sq = d1 * d1 - g1 * g2;
  if (d2sq >= smf_py(0.0)) {
    const SmfNum d2 = smf_sqrt(d2sq);
    SmfNum pos;
    if (x1 <= x2) pos = x2 - (x2 - x1) * ((g2 + d2 - d1) / (g2 - g1 + smf_py(2.0) * d2));
    else pos = x1 - (x1 - x2) * ((g1 + d2 - d1) / (g1 - g2 + smf_py(2.0) * d2));
    return smf_min(smf_max(pos, lo), hi);
  }
  return (lo + hi) / smf_py(2.0);
}

// `eval(t, keep, nkeep, f, gtd, g)` is one evaluation of the line search's objective at step t: the loss, g . d and a handle of the
// gradient (the fit's buffer index); `keep` are the handles still referenced.  Non-zero: an error code, the search stops.

struct SmfLineResult { SmfNum f, t; int g = -1, evals = 0; };

// torch/optim/lbfgs.py _strong_wolfe (c1 = 1e-4, c2 = 0.9), statement for statement; the gradients are handles
template <class Eval>
int smf_strong_wolfe(const Eval& eval, SmfNum t, SmfNum f, int g, SmfNum gtd, SmfNum d_norm, double tolerance_change, int max_ls,
                     SmfLineResult& out) {
  const SmfNum c1 = smf_py(1e-4), c2 = smf_py(0.9);
  SmfNum f_new, gtd_new;
  int g_new = -1;
  { const int keep[1] = {g}; if (int rc = eval(t, keep, 1, f_new, gtd_new, g_new)) return rc; }
  int ls_func_evals = 1;
  SmfNum t_prev = smf_py(0.0), f_prev = f, gtd_prev = gtd;
  int g_prev = g;
  SmfNum bracket[2], bracket_f[2], bracket_gtd[2];
  int bracket_g[2] = {-1, -1}, nbracket = 0;
  bool done = false;
  int ls_iter = 0;
  while (ls_iter < max_ls) {
    if (f_new > (f + c1 * t * gtd) || (ls_iter > 1 && f_new >= f_prev)) {
      bracket[0] = t_prev; bracket[1] = t; bracket_f[0] = f_prev; bracket_f[1] = f_new;
      bracket_g[0] = g_prev; bracket_g[1] = g_new; bracket_gtd[0] = gtd_prev; bracket_gtd[1] = gtd_new; nbracket = 2;
      break;
    }
    if (smf_abs(gtd_new) <= -c2 * gtd) {
      bracket[0] = t; bracket_f[0] = f_new; bracket_g[0] = g_new; nbracket = 1;
      done = true;
      break;
    }
    if (gtd_new >= smf_py(0.0)) {
      bracket[0] = t_prev; bracket[1] = t; bracket_f[0] = f_prev; bracket_f[1] = f_new;
      bracket_g[0] = g_prev; bracket_g[1] = g_new; bracket_gtd[0] = gtd_prev; bracket_gtd[1] = gtd_new; nbracket = 2;
      break;
    }
    const SmfNum bounds[2] = {t + smf_py(0.01) * (t - t_prev), t * smf_py(10.0)};
    const SmfNum tmp = t;
    t = smf_cubic(t_prev, f_prev, gtd_prev, t, f_new, gtd_new, bounds);
    t_prev = tmp; f_prev = f_new; g_prev = g_new; gtd_prev = gtd_new;
    { const int keep[2] = {g, g_prev}; if (int rc = eval(t, keep, 2, f_new, gtd_new, g_new)) return rc; }
    ++ls_func_evals;
    ++ls_iter;
  }
  if (ls_iter == max_ls) {
    bracket[0] = smf_py(0.0); bracket[1] = t; bracket_f[0] = f; bracket_f[1] = f_new; bracket_g[0] = g; bracket_g[1] = g_new; nbracket = 2;
  }
  bool insuf_progress = false;
  int low_pos = 0, high_pos = 1;
  if (!(bracket_f[0] <= bracket_f[nbracket - 1])) { low_pos = 1; high_pos = 0; }
  while (!done && ls_iter < max_ls) {
    if (smf_abs(bracket[1] - bracket[0]) * d_norm < smf_py(tolerance_change)) break;
    t = smf_cubic(bracket[0], bracket_f[0], bracket_gtd[0], bracket[1], bracket_f[1], bracket_gtd[1], nullptr);
    const SmfNum bmax = smf_max(bracket[0], bracket[1]), bmin = smf_min(bracket[0], bracket[1]);
    const SmfNum eps = smf_py(0.1) * (bmax - bmin);
    if (smf_min(bmax - t, t - bmin) < eps) {
      if (insuf_progress || t >= bmax || t <= bmin) {
        if (smf_abs(t - bmax) < smf_abs(t - bmin)) t = bmax - eps;
        else t = bmin + eps;
        insuf_progress = false;
      } else {
        insuf_progress = true;
      }
    } else {
      insuf_progress = false;
    }
    { const int keep[3] = {g, bracket_g[0], bracket_g[1]}; if (int rc = eval(t, keep, 3, f_new, gtd_new, g_new)) return rc; }
    ++ls_func_evals;
    ++ls_iter;
    if (f_new > (f + c1 * t * gtd) || f_new >= bracket_f[low_pos]) {
      bracket[high_pos] = t; bracket_f[high_pos] = f_new; bracket_g[high_pos] = g_new; bracket_gtd[high_pos] = gtd_new;
      if (bracket_f[0] <= bracket_f[1]) { low_pos = 0; high_pos = 1; } else { low_pos = 1; high_pos = 0; }
    } else {
      if (smf_abs(gtd_new) <= -c2 * gtd) {
        done = true;
      } else if (gtd_new * (bracket[high_pos] - bracket[low_pos]) >= smf_py(0.0)) {
        bracket[high_pos] = bracket[low_pos]; bracket_f[high_pos] = bracket_f[low_pos];
        bracket_g[high_pos] = bracket_g[low_pos]; bracket_gtd[high_pos] = bracket_gtd[low_pos];
      }
      bracket[low_pos] = t; bracket_f[low_pos] = f_new; bracket_g[low_pos] = g_new; bracket_gtd[low_pos] = gtd_new;
    }
  }
  out.t = bracket[low_pos];
  out.f = bracket_f[low_pos];
  out.g = bracket_g[low_pos];
  out.evals = ls_func_evals;
  return 0;
}

constexpr int kSmfPool = 5;          // gradient buffers of a line search: the start's, the previous point's, the bracket's two, the new one

struct SmfPlan {
  int T, nwg, H;
  size_t n2;                         // 85 T: the stage-2 vector (stage 1 uses the first 6 T of each buffer)
  size_t body, betas, cam_est, x1, x, d, prev_g, pool, hist_y, hist_s, ro, scal, rec, partial, total;   // offsets, floats
};

int smf_plan(const std::string& f, const mdm_smplify_model_t* m, const mdm_smplify_call_t* c, int T, SmfPlan& p) {
  if (m == nullptr || c == nullptr) return fail(MDM_EINVAL, f + "null model or call");
  if (T < 1) return fail(MDM_EINVAL, f + "T must be at least 1");
  if (T > 4096) return fail(MDM_EUNSUPPORTED, f + "at most 4096 frames");
  if (c->history < 1 || c->history > SMF_HIST_MAX) return fail(MDM_EINVAL, f + "history must lie in [1, 128]");
  if (c->num_iters < 1 || c->stage1_calls < 0 || c->stage2_calls < 0) return fail(MDM_EINVAL, f + "num_iters must be at least 1 and the call counts non-negative");
  p.T = T;
  p.nwg = (T + SMF_FRAMES - 1) / SMF_FRAMES;
  p.H = c->history;
  p.n2 = (size_t)85 * T;
  size_t at = 0;
  auto take = [&](size_t n) { const size_t o = at; at += (n + 3) & ~(size_t)3; return o; };
  p.body = take((size_t)SMF_BODY * T);
  p.betas = take((size_t)SMF_BETAS * T);
  p.cam_est = take((size_t)3 * T);
  p.x1 = take((size_t)6 * T);
  p.x = take(p.n2);
  p.d = take(p.n2);
  p.prev_g = take(p.n2);
  p.pool = take(kSmfPool * p.n2);
  p.hist_y = take((size_t)p.H * p.n2);
  p.hist_s = take((size_t)p.H * p.n2);
  p.ro = take(SMF_HIST_MAX);
  p.scal = take(8);                  // H_diag, then the ring's two integers
  p.partial = take((size_t)p.nwg * SMF_REC);
  p.rec = take(SMF_DIR_REC);
  p.total = at;
  return 0;
}

int smf_model_check(const std::string& f, const mdm_smplify_model_t* m) {
  const void* ptrs[] = {m->j0, m->jdirs, m->means, m->precisions, m->neg_log_nll_weights};
  const char* names[] = {"j0", "jdirs", "means", "precisions", "neg_log_nll_weights"};
  if (int rc = check_weight_ptrs(f, ptrs, names, 5)) return rc;
  if (m->parents == nullptr) return fail(MDM_EINVAL, f + "null parents");
  if (m->parents[0] != -1) return fail(MDM_EINVAL, f + "parents[0] must be -1 (the root)");
  for (int i = 1; i < SMF_J; ++i)
    if (m->parents[i] < 0 || m->parents[i] >= i)
      return fail(MDM_EINVAL, f + "parents[" + std::to_string(i) + "] must lie in [0, " + std::to_string(i) + ")");
  return 0;
}

void smf_fill_model(SmplifyEvalArgs& a, const mdm_smplify_model_t* m, const mdm_smplify_call_t* c) {
  a = SmplifyEvalArgs{};
  a.j0 = m->j0; a.jdirs = m->jdirs; a.means = m->means; a.prec = m->precisions; a.nlw = m->neg_log_nll_weights;
  int depth[SMF_J];
  for (int i = 0; i < SMF_J; ++i) {
    a.parent[i] = i == 0 ? 0 : m->parents[i];
    depth[i] = i == 0 ? 0 : depth[m->parents[i]] + 1;
    a.anc[i] = (i == 0 ? 0u : a.anc[m->parents[i]]) | (1u << i);
  }
  int at = 0, lv = 0;
  for (; at < SMF_J; ++lv) {
    a.lvl_start[lv] = (uint8_t)at;
    for (int i = 0; i < SMF_J; ++i)
      if (depth[i] == lv) a.lvl_joint[at++] = (uint8_t)i;
  }
  a.lvl_start[lv] = (uint8_t)at;
  a.nlvl = lv;
  // Python squares the weights in double; the product with a float32 tensor rounds them to float
  a.w_joint = (float)(c->joint_weight * c->joint_weight);
  a.sigma2 = (float)(c->sigma * c->sigma);
  a.w_prior = (float)(c->pose_prior_weight * c->pose_prior_weight);
  a.w_angle = (float)(c->angle_prior_weight * c->angle_prior_weight);
  a.w_shape = (float)(c->shape_prior_weight * c->shape_prior_weight);
  a.w_preserve = (float)(c->pose_preserve_weight * c->pose_preserve_weight);
  a.w_depth = (float)(c->depth_weight * c->depth_weight);
}

template <int STAGE> void smf_launch_eval(const SmplifyEvalArgs& a, hipStream_t s) {
  auto k = &smplify_eval_kernel<STAGE>;
  MDM_LAUNCH(k, dim3((unsigned)((a.T + SMF_FRAMES - 1) / SMF_FRAMES)), dim3(SMF_THREADS), 0, s, a);
}

void smf_launch_direction(const SmplifyDirArgs& a, hipStream_t s) {
  if (a.n <= 1024) { auto k = &smplify_direction_kernel<64>; MDM_LAUNCH(k, dim3(1), dim3(64), 0, s, a); }
  else if (a.n <= 16384) { auto k = &smplify_direction_kernel<256>; MDM_LAUNCH(k, dim3(1), dim3(256), 0, s, a); }
  else { auto k = &smplify_direction_kernel<1024>; MDM_LAUNCH(k, dim3(1), dim3(1024), 0, s, a); }
}

int smf_refuse_capture(const std::string& f, hipStream_t s) {
  if (rt_is_capturing(s))
    return fail(MDM_EUNSUPPORTED, f + "the stream is being captured into a hipGraph -- the optimiser reads its scalars back on the host "
                "after every evaluation, so this call cannot be captured");
  return 0;
}

// the workgroups' records, added in order: loss, max|g|, g . d, non-finite
struct SmfScalars { float loss, gmax, gd, bad; };
int smf_read_scalars(const float* partial_dev, int nwg, hipStream_t s, SmfScalars& o) {
  float host[128 * SMF_REC];
  if (int rc = rt_read_back(host, partial_dev, (size_t)nwg * SMF_REC * sizeof(float), s)) return rc;
  o = SmfScalars{0.f, 0.f, 0.f, 0.f};
  for (int w = 0; w < nwg; ++w) {
    o.loss += host[w * SMF_REC];
    o.gmax = std::max(o.gmax, host[w * SMF_REC + 1]);
    o.gd += host[w * SMF_REC + 2];
    o.bad = std::max(o.bad, host[w * SMF_REC + 3]);
  }
  return 0;
}

// One stage of SMPLify3D.__call__: `calls` step() calls of one torch.optim.LBFGS over the flat vector x of n floats
struct SmfStage {
  const mdm_smplify_call_t* c;
  SmplifyEvalArgs ev;      // everything but x, d, t, grad
  int stage, nwg;
  int n;
  float *x, *d, *prev_g, *pool, *hist_y, *hist_s, *ro, *scal, *rec, *partial;
  size_t pool_stride;
  hipStream_t s;
  // results
  int64_t evals = 0, iters = 0;
  double loss = 0.0;

  int eval(const float* dir, float t, int gbuf, SmfScalars& o) {
    SmplifyEvalArgs a = ev;
    a.x = x; a.d = dir; a.t = t;
    a.grad = pool + (size_t)gbuf * pool_stride;
    a.partial = partial;
    if (stage == 1) smf_launch_eval<1>(a, s); else smf_launch_eval<2>(a, s);
    if (int rc = rt_launch_status()) return rc;
    ++evals;
    if (int rc = smf_read_scalars(partial, nwg, s, o)) return rc;
    if (o.bad != 0.f) return fail(MDM_EINVAL, "mdm_smplify_fit: the loss or its gradient left the finite range during the fit");
    return 0;
  }

  int run(int calls) {
    const int max_iter = c->num_iters, max_eval = max_iter * 5 / 4;
    const SmfNum tol_grad = smf_py(c->tolerance_grad), tol_change = smf_py(c->tolerance_change), lr = smf_py(c->step_size);
    int64_t state_n_iter = 0;
    SmfNum t = lr;
    float gmax_of[kSmfPool] = {};
    for (int call = 0; call < calls; ++call) {
      int cur = 0;                            // flat_grad's buffer
      SmfScalars sc;
      if (int rc = eval(nullptr, 0.f, cur, sc)) return rc;
      gmax_of[cur] = sc.gmax;
      loss = (double)sc.loss;
      int current_evals = 1;
      // every later call of this optimiser would evaluate the same point and return here too
      if (smf_t32(sc.gmax) <= tol_grad) break;
      int n_iter = 0;
      while (n_iter < max_iter) {
        ++n_iter;
        ++state_n_iter;
        ++iters;
        const bool first = state_n_iter == 1;
        SmplifyDirArgs da;
        da.g = pool + (size_t)cur * pool_stride; da.prev_g = prev_g; da.d = d; da.hist_y = hist_y; da.hist_s = hist_s; da.ro = ro;
        da.hdiag = scal; da.ring = reinterpret_cast<int32_t*>(scal + 4); da.rec = rec; da.t = (float)t.v; da.n = n;
        da.history = c->history; da.first = first ? 1 : 0;
        smf_launch_direction(da, s);
        if (int rc = rt_launch_status()) return rc;
        float rec_h[SMF_DIR_REC];
        if (int rc = rt_read_back(rec_h, rec, sizeof(rec_h), s)) return rc;
        const SmfNum gtd = smf_t32(rec_h[0]), d_norm = smf_t32(rec_h[1]);
        const double prev_loss = loss;
        if (first) t = smf_min(smf_py(1.0), smf_py(1.0) / smf_t32(rec_h[2])) * lr;
        else t = lr;
        if (gtd > -tol_change) break;
        auto le = [&](SmfNum tt, const int* keep, int nkeep, SmfNum& f, SmfNum& g_d, int& g) -> int {
          int buf = 0;
          for (;; ++buf) {
            bool used = false;
            for (int i = 0; i < nkeep; ++i) used = used || keep[i] == buf;
            if (!used) break;
          }
          SmfScalars o;
          if (int rc = eval(d, (float)tt.v, buf, o)) return rc;
          gmax_of[buf] = o.gmax;
          f = smf_py((double)o.loss);
          g_d = smf_t32(o.gd);
          g = buf;
          return 0;
        };
        SmfLineResult lr_out;
        if (int rc = smf_strong_wolfe(le, t, smf_py(loss), cur, gtd, d_norm, c->tolerance_change, max_eval - current_evals, lr_out)) return rc;
        loss = lr_out.f.v;
        cur = lr_out.g;
        t = lr_out.t;
        MDM_LAUNCH(smplify_step_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, (const float*)d, (float)t.v, n);
        if (int rc = rt_launch_status()) return rc;
        const bool opt_cond = smf_t32(gmax_of[cur]) <= tol_grad;
        current_evals += lr_out.evals;
        if (n_iter == max_iter) break;
        if (current_evals >= max_eval) break;
        if (opt_cond) break;
        // max|d t| = |t| max|d| in float: rounding is monotone, so the largest product is the product of the largest
        if (smf_abs(d_norm * SmfNum{(double)(float)t.v, true}) <= tol_change) break;
        if (std::fabs(loss - prev_loss) < c->tolerance_change) break;
      }
    }
    return 0;
  }
};

int smf_data_check(const std::string& f, std::initializer_list<std::pair<const char*, const void*>> ptrs) {
  for (const auto& p : ptrs) {
    if (p.second == nullptr) return fail(MDM_EINVAL, f + "null " + p.first);
    if ((reinterpret_cast<uintptr_t>(p.second) & 3) != 0) return fail(MDM_EINVAL, f + p.first + " must be 4-byte aligned");
  }
  return 0;
}

}  // namespace

extern "C" {

size_t mdm_smplify_workspace_bytes(const mdm_smplify_model_t* model, const mdm_smplify_call_t* call, int32_t T) {
  SmfPlan p;
  if (smf_plan("mdm_smplify_workspace_bytes: ", model, call, T, p) != 0) return 0;
  return ws_bytes_of(p.total);
}

int mdm_smplify_value_grad(const mdm_smplify_model_t* m, const mdm_smplify_call_t* c, int32_t stage, const float* x, const float* dir,
                           const float* fixed_pose, const float* fixed_betas, const float* cam_est, const float* j3d, const float* conf,
                           int32_t T, float* grad, float* terms, float* joints, float* scalars_host, void* ws, size_t ws_bytes,
                           void* stream) {
  const std::string f = "mdm_smplify_value_grad: ";
  SmfPlan p;
  if (int rc = smf_plan(f, m, c, T, p)) return rc;
  if (int rc = smf_model_check(f, m)) return rc;
  if (stage != 1 && stage != 2) return fail(MDM_EINVAL, f + "stage must be 1 or 2");
  if (int rc = smf_data_check(f, {{"x_dev", x}, {"fixed_pose_dev", fixed_pose}, {"j3d_dev", j3d}, {"conf_dev", conf}, {"grad_dev", grad},
                                  {"terms_dev", terms}})) return rc;
  if (stage == 1)
    if (int rc = smf_data_check(f, {{"fixed_betas_dev", fixed_betas}, {"cam_est_dev", cam_est}})) return rc;
  if (scalars_host == nullptr) return fail(MDM_EINVAL, f + "null scalars_host");
  if (ws == nullptr) return fail(MDM_EINVAL, f + "null workspace_dev");
  if (ws_bytes < ws_bytes_of(p.total)) return fail(MDM_ENOSPC, f + "workspace_bytes too small (mdm_smplify_workspace_bytes)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = smf_refuse_capture(f, s)) return rc;
  ChainGuard chain_guard(stream);
  float* w = ws_floats(ws);
  SmplifyEvalArgs a;
  smf_fill_model(a, m, c);
  a.x = x; a.d = nullptr; a.t = 0.f; a.T = T;
  if (stage == 1) { a.off_go = 0; a.off_cam = 3 * T; a.off_body = -1; a.off_betas = -1; a.fix_body = fixed_pose; a.fix_betas = fixed_betas; a.cam_est = cam_est; }
  else { a.off_body = 0; a.off_betas = SMF_BODY * T; a.off_go = 79 * T; a.off_cam = 82 * T; a.preserve = fixed_pose; }
  a.j3d = j3d; a.conf = conf;
  a.partial = w + p.partial;
  a.cam_out = w + p.cam_est;             // the check's kinematic pass writes its camera guess into the workspace
  smf_launch_eval<0>(a, s);
  if (int rc = rt_launch_status()) return rc;
  SmfScalars sc;
  if (int rc = smf_read_scalars(a.partial, p.nwg, s, sc)) return rc;
  if (sc.bad != 0.f) return fail(MDM_EINVAL, f + "non-finite value in the pose, betas, j3d or conf");
  a.d = dir; a.t = 0.f;                  // g . d at the point x itself
  a.grad = grad; a.terms = terms; a.joints = joints;
  if (stage == 1) smf_launch_eval<1>(a, s); else smf_launch_eval<2>(a, s);
  if (int rc = rt_launch_status()) return rc;
  if (int rc = smf_read_scalars(a.partial, p.nwg, s, sc)) return rc;
  if (sc.bad != 0.f)       // (the camera block of x, cam_est, preserve and dir are not part of the first pass: the outputs are written)
    return fail(MDM_EINVAL, f + "the loss, its gradient or g . dir is not finite (a non-finite x, cam_est, preserve or dir)");
  scalars_host[0] = sc.loss; scalars_host[1] = sc.gmax; scalars_host[2] = sc.gd;
  return MDM_OK;
}

int mdm_smplify_fit(const mdm_smplify_model_t* m, const mdm_smplify_call_t* c, const float* init_pose, const float* init_betas,
                    const float* j3d, const float* conf, int32_t T, float* pose_out, float* betas_out, float* cam_out, float* joints_out,
                    float* thetas_out, double* stats_host, void* ws, size_t ws_bytes, void* stream) {
  const std::string f = "mdm_smplify_fit: ";
  SmfPlan p;
  if (int rc = smf_plan(f, m, c, T, p)) return rc;
  if (int rc = smf_model_check(f, m)) return rc;
  if (int rc = smf_data_check(f, {{"init_pose_dev", init_pose}, {"init_betas_dev", init_betas}, {"j3d_dev", j3d}, {"conf_dev", conf},
                                  {"pose_out_dev", pose_out}, {"betas_out_dev", betas_out}, {"cam_out_dev", cam_out},
                                  {"joints_out_dev", joints_out}, {"thetas_out_dev", thetas_out}})) return rc;
  if (stats_host == nullptr) return fail(MDM_EINVAL, f + "null stats_host");
  if (ws == nullptr) return fail(MDM_EINVAL, f + "null workspace_dev");
  if (ws_bytes < ws_bytes_of(p.total)) return fail(MDM_ENOSPC, f + "workspace_bytes too small (mdm_smplify_workspace_bytes)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = smf_refuse_capture(f, s)) return rc;
  ChainGuard chain_guard(stream);
  float* w = ws_floats(ws);

  // the initial pose's parts, its kinematic chain and guess_init_3d; the inputs' finiteness
  SmplifyPackArgs pk{init_pose, init_betas, nullptr, nullptr, w + p.body, w + p.betas, w + p.x1, T, 1};
  MDM_LAUNCH(smplify_pack_kernel, dim3((unsigned)T), dim3(256), 0, s, pk);
  if (int rc = rt_launch_status()) return rc;
  SmplifyEvalArgs base;
  smf_fill_model(base, m, c);
  base.T = T; base.j3d = j3d; base.conf = conf; base.partial = w + p.partial;
  base.fix_body = w + p.body; base.fix_betas = w + p.betas; base.cam_est = w + p.cam_est; base.preserve = w + p.body;
  {
    SmplifyEvalArgs a = base;
    a.x = w + p.x1; a.off_go = 0; a.off_cam = 3 * T; a.off_body = -1; a.off_betas = -1;
    a.cam_out = w + p.cam_est; a.cam_out2 = w + p.x1 + 3 * (size_t)T;
    smf_launch_eval<0>(a, s);
    if (int rc = rt_launch_status()) return rc;
    SmfScalars sc;
    if (int rc = smf_read_scalars(a.partial, p.nwg, s, sc)) return rc;
    if (sc.bad != 0.f) return fail(MDM_EINVAL, f + "non-finite value in init_pose, init_betas, j3d or conf");
  }
  SmfStage st;
  st.c = c; st.nwg = p.nwg; st.s = s;
  st.d = w + p.d; st.prev_g = w + p.prev_g; st.pool = w + p.pool; st.hist_y = w + p.hist_y; st.hist_s = w + p.hist_s; st.ro = w + p.ro;
  st.scal = w + p.scal; st.rec = w + p.rec; st.partial = w + p.partial; st.pool_stride = p.n2;

  // step 1: the camera translation and the body orientation (camera_fitting_loss_3d)
  st.stage = 1; st.n = 6 * T; st.x = w + p.x1;
  st.ev = base; st.ev.off_go = 0; st.ev.off_cam = 3 * T; st.ev.off_body = -1; st.ev.off_betas = -1;
  if (int rc = st.run(c->stage1_calls)) return rc;
  stats_host[0] = (double)st.evals; stats_host[1] = (double)st.iters; stats_host[2] = st.loss;

  // step 2: everything (body_fitting_loss_3d); betas per frame
  SmplifyPackArgs pk2{nullptr, nullptr, nullptr, w + p.x1, w + p.body, w + p.betas, w + p.x, T, 2};
  MDM_LAUNCH(smplify_pack_kernel, dim3((unsigned)T), dim3(256), 0, s, pk2);
  if (int rc = rt_launch_status()) return rc;
  st.stage = 2; st.n = 85 * T; st.x = w + p.x; st.evals = 0; st.iters = 0; st.loss = 0.0;
  st.ev = base; st.ev.off_body = 0; st.ev.off_betas = SMF_BODY * T; st.ev.off_go = 79 * T; st.ev.off_cam = 82 * T;
  if (int rc = st.run(c->stage2_calls)) return rc;
  stats_host[3] = (double)st.evals; stats_host[4] = (double)st.iters;

  // the final loss as SMPLify3D reports it (pose_preserve_weight at its default of 0) and the model joints of the result
  {
    SmplifyEvalArgs a = st.ev;
    a.x = st.x; a.d = nullptr; a.t = 0.f; a.grad = nullptr; a.joints = joints_out; a.w_preserve = 0.f;
    smf_launch_eval<2>(a, s);
    if (int rc = rt_launch_status()) return rc;
    SmfScalars sc;
    if (int rc = smf_read_scalars(a.partial, p.nwg, s, sc)) return rc;
    stats_host[5] = (double)sc.loss;
  }
  SmplifyTailArgs ta{st.x, j3d, pose_out, betas_out, cam_out, thetas_out, T};
  MDM_LAUNCH(smplify_tail_kernel, dim3((unsigned)T), dim3(256), 0, s, ta);
  return rt_launch_status();
}

int mdm_smplify_strong_wolfe(const double* f_seq, const double* gtd_seq, int32_t n_seq, double t0, double f0, double gtd0, double d_norm,
                             double tolerance_change, int32_t max_ls, int32_t float32_tensors, double* t_seq, int32_t* n_evals,
                             double* t_final, double* f_final) {
  const std::string f = "mdm_smplify_strong_wolfe: ";
  if (f_seq == nullptr || gtd_seq == nullptr || t_seq == nullptr || n_evals == nullptr || t_final == nullptr || f_final == nullptr)
    return fail(MDM_EINVAL, f + "null pointer");
  if (n_seq < 1 || max_ls < 1) return fail(MDM_EINVAL, f + "n_seq and max_ls must be at least 1");
  int at = 0;
  // what is a 0-dim tensor in torch's code (g . d, max|d|): float32 as in the fit, or double
  auto tensor = [&](double v) { return float32_tensors ? smf_t32((float)v) : smf_py(v); };
  auto le = [&](SmfNum t, const int*, int, SmfNum& fv, SmfNum& gd, int& g) -> int {
    if (at >= n_seq) return fail(MDM_EINVAL, f + "the search asks for more evaluations than the sequence holds");
    t_seq[at] = t.v;
    fv = smf_py(f_seq[at]);
    gd = tensor(gtd_seq[at]);
    g = at + 1;
    ++at;
    return 0;
  };
  SmfLineResult out;
  if (int rc = smf_strong_wolfe(le, smf_py(t0), smf_py(f0), 0, tensor(gtd0), tensor(d_norm), tolerance_change, max_ls, out)) return rc;
  *n_evals = out.evals;
  *t_final = out.t.v;
  *f_final = out.f.v;
  return MDM_OK;
}

}  // extern "C"
