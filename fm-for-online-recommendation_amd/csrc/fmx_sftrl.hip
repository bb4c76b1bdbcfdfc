// fmx_sftrl.hip -- hot path B on the device and its C ABI: the sketched-FTRL
// family (fmx_sftrl_run, fmx_sftrl_grid; kernel: fmx_sftrl.inc), FM_FTRL (fmx_ftrl_dense_run, fmx_ftrl_dense_grid) and RRF_Online
// (fmx_rrf_run, fmx_rrf_grid; kernels: fmx_pathb.inc).
#include "fmx_common.h"

namespace {
#include "fmx_sftrl.inc"
#include "fmx_pathb.inc"

// the dynamic LDS of the three kernels, in bytes (their header comments give the layout)
size_t sftrl_lds(int D, int d, int m) {
  return ((size_t)2 * d * 2 * m + 2 * (size_t)d * d + d + 48 + D) * sizeof(double) + (size_t)d * sizeof(int) + 16;
}
size_t ftrl_dense_lds(int D, int m2) { return ((size_t)2 * PB_MAX_D + (size_t)m2 * ((D - 1) | 1)) * sizeof(double); }
size_t rrf_lds(int D, int Ds) { return ((size_t)2 * PB_MAX_D + PB_MAX_DS + (size_t)D * (Ds | 1)) * sizeof(double); }

// what a _run and its _grid check of a stream and of the (largest) setting before they launch; PB_MAX_D is the feature limit of
// all three kernels
int sftrl_check(const char *who, int32_t N, int32_t D, int32_t d, int32_t m, int32_t task) {
  if (N < 0 || D < 1 || d < 1 || d > D || m < 1) return fail(FMX_ERR_ARG, "%s: bad sizes", who);
  if (task != 0 && task != 1) return fail(FMX_ERR_ARG, "%s: task must be 0 (cls) or 1 (reg)", who);
  if (d > SF_MAX_D || 2 * m > SF_MAX_C || D > PB_MAX_D)
    return fail(FMX_ERR_UNSUPPORTED, "%s: needs sketch dim <= %d, 2 m <= %d, features <= %d (got %d, %d, %d)", who, SF_MAX_D, SF_MAX_C,
                PB_MAX_D, d, 2 * m, D);
  return FMX_OK;
}
int ftrl_dense_check(const char *who, int32_t N, int32_t D, int32_t m2, int32_t task) {
  if (N < 0 || D < 2 || m2 < 2 || (m2 & 1)) return fail(FMX_ERR_ARG, "%s: bad sizes (N >= 0, D >= 2, 2 m even and >= 2)", who);
  if (task != 0 && task != 1) return fail(FMX_ERR_ARG, "%s: task must be 0 (cls) or 1 (reg)", who);
  if (D > PB_MAX_D || m2 > PB_MAX_M2)
    return fail(FMX_ERR_UNSUPPORTED, "%s: needs features <= %d, 2 m <= %d (got %d, %d)", who, PB_MAX_D, PB_MAX_M2, D, m2);
  return FMX_OK;
}
int rrf_check(const char *who, int32_t N, int32_t D, int32_t Ds, int32_t loss) {
  if (N < 0 || D < 1 || Ds < 1) return fail(FMX_ERR_ARG, "%s: bad sizes", who);
  if (loss != 0 && loss != 1) return fail(FMX_ERR_ARG, "%s: loss must be 0 (logit) or 1 (l2); hinge and l1 are not implemented", who);
  if (D > PB_MAX_D || Ds > PB_MAX_DS)
    return fail(FMX_ERR_UNSUPPORTED, "%s: needs features <= %d, spectral samples <= %d (got %d, %d)", who, PB_MAX_D, PB_MAX_DS, D, Ds);
  return FMX_OK;
}

// One launcher per kernel, shared by its _run and its _grid.  A run: no settings arrays (the kernels branch on that), strides 0,
// one workgroup.  A grid: the settings arrays, every slab sized for the largest setting, n_settings workgroups.
int sftrl_launch(const double *X, const double *y, int32_t N, int32_t D, int32_t d, int32_t n_settings, const int32_t *ms,
                 const double *etas, int32_t m, double eta, double thres, int32_t task, double *BP, double *BN, int32_t *counts, double *w,
                 double *g_w, double *pred_out, int32_t *status, fmx_stream_t stream) {
  const bool grid = ms != nullptr;
  SftrlArgs a;
  a.X = X;
  a.y = y;
  a.BP = BP;
  a.BN = BN;
  a.counts = counts;
  a.w = w;
  a.g_w = g_w;
  a.pred = pred_out;
  a.status = status;
  a.eta = eta;
  a.thres = thres;
  a.N = N;
  a.D = D;
  a.d = d;
  a.m = m;
  a.cls = task == 0;
  a.ms = ms;
  a.etas = etas;
  a.B_stride = grid ? (long long)d * 2 * m : 0;
  a.w_stride = grid ? D : 0;
  a.pred_stride = grid ? N : 0;
  static bool raised = false;  // once per process, before the first launch: the sketches may need more than the default 64 KiB
  if (!raised) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_sftrl_online), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
    raised = true;
  }
  hipLaunchKernelGGL(k_sftrl_online, dim3(n_settings), dim3(64), sftrl_lds(D, d, m), static_cast<hipStream_t>(stream), a);
  return check_launch(grid ? "k_sftrl_online (grid)" : "k_sftrl_online");
}

int ftrl_dense_launch(const double *X, const double *y, int32_t N, int32_t D, int32_t n_settings, const int32_t *m2s, const double *etas,
                      int32_t m2, double eta, int32_t task, double *w1, double *W2, double *g_w1, double *g_W2, double *pred_out,
                      int32_t *status, fmx_stream_t stream) {
  const bool grid = m2s != nullptr;
  FtrlDenseArgs a;
  a.X = X;
  a.y = y;
  a.w1 = w1;
  a.g_w1 = g_w1;
  a.W2 = W2;
  a.g_W2 = g_W2;
  a.pred = pred_out;
  a.status = status;
  a.eta = eta;
  a.N = N;
  a.D = D;
  a.m2 = m2;
  a.cls = task == 0;
  a.m2s = m2s;
  a.etas = etas;
  a.W_stride = grid ? (long long)m2 * (D - 1) : 0;
  a.pred_stride = grid ? N : 0;
  hipLaunchKernelGGL(k_ftrl_dense, dim3(n_settings), dim3(64), ftrl_dense_lds(D, m2), static_cast<hipStream_t>(stream), a);
  return check_launch(grid ? "k_ftrl_dense (grid)" : "k_ftrl_dense");
}

int rrf_launch(const double *X, const double *y, int32_t N, int32_t D, int32_t n_settings, const int32_t *Dss, const double *lr_ws,
               const double *lr_gammas, int32_t Ds, double lr_w, double lr_gamma, int32_t loss, const double *eps, double *gamma, double *w,
               double *pred_out, int32_t *status, fmx_stream_t stream) {
  const bool grid = Dss != nullptr;
  RrfArgs a;
  a.X = X;
  a.y = y;
  a.eps = eps;
  a.gamma = gamma;
  a.w = w;
  a.pred = pred_out;
  a.status = status;
  a.lr_w = lr_w;
  a.lr_g = lr_gamma;
  a.N = N;
  a.D = D;
  a.Ds = Ds;
  a.l2 = loss == 1;
  a.Dss = Dss;
  a.lr_ws = lr_ws;
  a.lr_gs = lr_gammas;
  a.eps_stride = grid ? (long long)D * Ds : 0;
  a.w_stride = grid ? 2ll * Ds : 0;
  a.pred_stride = grid ? N : 0;
  hipLaunchKernelGGL(k_rrf_online, dim3(n_settings), dim3(64), rrf_lds(D, Ds), static_cast<hipStream_t>(stream), a);
  return check_launch(grid ? "k_rrf_online (grid)" : "k_rrf_online");
}
}  // namespace

extern "C" {

int fmx_sftrl_run(const double *X, const double *y, int32_t N, int32_t D, int32_t d, int32_t m, double eta, double thres,
                  int32_t task, double *BP, double *BN, int32_t *counts, double *w, double *g_w, double *pred_out,
                  int32_t *status, fmx_stream_t stream) {
  if (!X || !y || !BP || !BN || !counts || !pred_out || !status) return fail(FMX_ERR_ARG, "fmx_sftrl_run: null argument");
  if ((w == nullptr) != (g_w == nullptr)) return fail(FMX_ERR_ARG, "fmx_sftrl_run: w and g_w go together");
  if (const int rc = sftrl_check("fmx_sftrl_run", N, D, d, m, task)) return rc;
  if (N == 0) return FMX_OK;
  return sftrl_launch(X, y, N, D, d, 1, nullptr, nullptr, m, eta, thres, task, BP, BN, counts, w, g_w, pred_out, status, stream);
}

int fmx_sftrl_grid(const double *X, const double *y, int32_t N, int32_t D, int32_t d, int32_t n_settings, const int32_t *ms,
                   const double *etas, int32_t m_max, double thres, int32_t task, double *BP, double *BN, int32_t *counts, double *w,
                   double *g_w, double *pred_out, int32_t *status, fmx_stream_t stream) {
  if (!X || !y || !ms || !etas || !BP || !BN || !counts || !pred_out || !status) return fail(FMX_ERR_ARG, "fmx_sftrl_grid: null argument");
  if ((w == nullptr) != (g_w == nullptr)) return fail(FMX_ERR_ARG, "fmx_sftrl_grid: w and g_w go together");
  if (n_settings < 0) return fail(FMX_ERR_ARG, "fmx_sftrl_grid: bad sizes");
  if (const int rc = sftrl_check("fmx_sftrl_grid", N, D, d, m_max, task)) return rc;
  if (N == 0 || n_settings == 0) return FMX_OK;
  return sftrl_launch(X, y, N, D, d, n_settings, ms, etas, m_max, 0.0, thres, task, BP, BN, counts, w, g_w, pred_out, status, stream);
}

int fmx_ftrl_dense_run(const double *X, const double *y, int32_t N, int32_t D, int32_t m2, double eta, int32_t task, double *w1,
                       double *W2, double *g_w1, double *g_W2, double *pred_out, int32_t *status, fmx_stream_t stream) {
  if (!X || !y || !w1 || !W2 || !g_w1 || !g_W2 || !pred_out || !status) return fail(FMX_ERR_ARG, "fmx_ftrl_dense_run: null argument");
  if (const int rc = ftrl_dense_check("fmx_ftrl_dense_run", N, D, m2, task)) return rc;
  if (N == 0) return FMX_OK;
  return ftrl_dense_launch(X, y, N, D, 1, nullptr, nullptr, m2, eta, task, w1, W2, g_w1, g_W2, pred_out, status, stream);
}

int fmx_ftrl_dense_grid(const double *X, const double *y, int32_t N, int32_t D, int32_t n_settings, const int32_t *m2s, const double *etas,
                        int32_t m2_max, int32_t task, double *w1, double *W2, double *g_w1, double *g_W2, double *pred_out,
                        int32_t *status, fmx_stream_t stream) {
  if (!X || !y || !m2s || !etas || !w1 || !W2 || !g_w1 || !g_W2 || !pred_out || !status)
    return fail(FMX_ERR_ARG, "fmx_ftrl_dense_grid: null argument");
  if (n_settings < 0) return fail(FMX_ERR_ARG, "fmx_ftrl_dense_grid: bad sizes");
  if (const int rc = ftrl_dense_check("fmx_ftrl_dense_grid", N, D, m2_max, task)) return rc;
  if (N == 0 || n_settings == 0) return FMX_OK;
  return ftrl_dense_launch(X, y, N, D, n_settings, m2s, etas, m2_max, 0.0, task, w1, W2, g_w1, g_W2, pred_out, status, stream);
}

int fmx_rrf_run(const double *X, const double *y, int32_t N, int32_t D, int32_t Ds, double lr_w, double lr_gamma, int32_t loss,
                const double *eps, double *gamma, double *w, double *pred_out, int32_t *status, fmx_stream_t stream) {
  if (!X || !y || !eps || !gamma || !w || !pred_out || !status) return fail(FMX_ERR_ARG, "fmx_rrf_run: null argument");
  if (const int rc = rrf_check("fmx_rrf_run", N, D, Ds, loss)) return rc;
  if (N == 0) return FMX_OK;
  return rrf_launch(X, y, N, D, 1, nullptr, nullptr, nullptr, Ds, lr_w, lr_gamma, loss, eps, gamma, w, pred_out, status, stream);
}

int fmx_rrf_grid(const double *X, const double *y, int32_t N, int32_t D, int32_t n_settings, const int32_t *Dss, const double *lr_ws,
                 const double *lr_gammas, int32_t Ds_max, int32_t loss, const double *eps, double *gamma, double *w, double *pred_out,
                 int32_t *status, fmx_stream_t stream) {
  if (!X || !y || !Dss || !lr_ws || !lr_gammas || !eps || !gamma || !w || !pred_out || !status)
    return fail(FMX_ERR_ARG, "fmx_rrf_grid: null argument");
  if (n_settings < 0) return fail(FMX_ERR_ARG, "fmx_rrf_grid: bad sizes");
  if (const int rc = rrf_check("fmx_rrf_grid", N, D, Ds_max, loss)) return rc;
  if (N == 0 || n_settings == 0) return FMX_OK;
  return rrf_launch(X, y, N, D, n_settings, Dss, lr_ws, lr_gammas, Ds_max, 0.0, 0.0, loss, eps, gamma, w, pred_out, status, stream);
}

}  // extern "C"
