// fmx_pathb.inc -- the other two online learners of hot path B, FM_FTRL and RRF_Online, each as one wavefront walking a
// device-resident stream (DESIGN.md section 8 item 4).  Included by fmx_sftrl.hip after fmx_sftrl.inc (wave_sum_d), inside its
// anonymous namespace.  fp64 like the reference, strictly sequential: one workgroup of 64 lanes per stream (or per setting of a
// grid), the state in LDS / registers for the length of the stream, the next sample's row of X in flight while this one is computed.
// No atomics; fmx_common.h switches contraction off, so every expression rounds as written and fma() stands where one is meant.
constexpr int PB_MAX_D = 64, PB_MAX_M2 = 128, PB_MAX_DS = 64;  // features, rows of W2 (2 m), spectral samples

// ---------------------------------------------------------------------------------------------------------------------------
// FM_FTRL (reference models/models_online/FM_FTRL.py:61-80).  x' = x without its last feature, W2 [m2, D - 1]:
//     t = W2 x';  y_hat = w1 . x + t . t;  s = dloss / dy_hat;  g_w1 += s x;  g_W2 += 2 t x'^T  (no factor s: the reference's quirk);
//     w1 = -eta g_w1;  W2 = -eta g_W2.
// After the first sample W2 IS -eta g_W2, so the kernel holds g_W2 alone and derives W2 element by element with the host's
// rounding (one multiplication); the first sample reads the caller's W2.  The update of g_W2 does not depend on y_hat, so the pass
// that applies sample i - 1's update is the pass that computes sample i's t: one read and one write of g_W2 per sample.
//   lane r owns rows r and r + 64 of g_W2 (its t_r stays in a register, nothing crosses lanes but x and the sum for y_hat);
//   lane j owns w1[j], g_w1[j].
// LDS: g_W2 as [m2][ld] doubles, ld = (D - 1) | 1 -- an odd row pitch puts the 32 lanes of a ds_read_b64 group on 32 different
// bank pairs -- plus two rows of x (this sample's and the previous one's): at the limits 128 * 63 * 8 + 2 * 64 * 8 = 65,536 B of
// the CU's 160 KiB, two settings of a grid per CU.
struct FtrlDenseArgs {
  const double *X;     // [N, D]
  const double *y;     // [N]
  double *w1, *g_w1;   // [D], in / out
  double *W2, *g_W2;   // [m2, D - 1] row-major, in / out
  double *pred;        // [N] raw y_hat
  int32_t *status;     // [2]: (1, sample): y_hat of that sample was NaN, the walk stopped in front of its update;
                       //      (2, m2) (grid only): the setting's m2 is odd or outside [2, m2_max], nothing was run
  double eta;
  int32_t N, D, m2, cls;
  // a GRID of settings over the same stream (fmx_ftrl_dense_grid): workgroup s runs m2s[s], etas[s] on its own slabs; null: one run
  const int32_t *m2s;
  const double *etas;
  long long W_stride, pred_stride;  // elements between two settings' W2 / g_W2 slabs (m2_max (D - 1)) and pred rows (N)
};

// one row of the fused pass: g += u x_prev (the previous sample's update, u = 2 t_prev), t = sum_j (-eta g_j) x_j, j ascending
__device__ __forceinline__ double fd_row_pass(double *g_row, const double *x_prev, const double *x_cur, int n, double u, double neg_eta) {
  double t = 0.0;
#pragma unroll 4
  for (int j = 0; j < n; ++j) {
    const double g = g_row[j] + u * x_prev[j];
    g_row[j] = g;
    t = fma(neg_eta * g, x_cur[j], t);
  }
  return t;
}
__device__ __forceinline__ double fd_row_first(const double *w_row, const double *x_cur, int n) {  // the caller's W2
  double t = 0.0;
  for (int j = 0; j < n; ++j) t = fma(w_row[j], x_cur[j], t);
  return t;
}

__global__ __launch_bounds__(64) void k_ftrl_dense(FtrlDenseArgs a) {
  extern __shared__ __attribute__((aligned(16))) double pb_smem[];
  const int lane = threadIdx.x;
  if (a.m2s) {  // setting blockIdx.x of a grid
    const long long s = blockIdx.x;
    a.m2 = a.m2s[s];
    a.eta = a.etas[s];
    a.w1 += s * a.D;
    a.g_w1 += s * a.D;
    a.W2 += s * a.W_stride;
    a.g_W2 += s * a.W_stride;
    a.pred += s * a.pred_stride;
    a.status += 2 * s;
    // the launch's LDS and the slabs are sized for m2_max: a setting beyond it would overrun its neighbours (a direct caller of
    // the C ABI could pass one) -- refused here, like k_sftrl_online's
    if (a.m2 < 2 || (a.m2 & 1) || (long long)a.m2 * (a.D - 1) > a.W_stride) {
      if (lane == 0) {
        a.status[0] = 2;
        a.status[1] = a.m2;
      }
      return;
    }
  }
  const int D = a.D, n = D - 1, ld = n | 1, m2 = a.m2;
  double *xs = pb_smem, *G = pb_smem + 2 * PB_MAX_D;  // xs [2][64]; G [m2][ld]
  for (int e = lane; e < m2 * n; e += 64) {
    const int r = e / n, j = e - r * n;
    G[r * ld + j] = a.g_W2[e];
  }
  const int r0 = lane, r1 = lane + 64;
  const bool has0 = r0 < m2, has1 = r1 < m2;
  const double neg_eta = -a.eta;
  double w_l = lane < D ? a.w1[lane] : 0.0, g_l = lane < D ? a.g_w1[lane] : 0.0;
  double x_next = lane < D ? a.X[lane] : 0.0, y_next = a.y[0];  // N >= 1: the host launches nothing for an empty stream
  double t0 = 0.0, t1 = 0.0;
  int done = 0;  // samples whose update has been taken into g_w1 (and, one pass later, into g_W2)
  bool stopped = false;
  for (int i = 0; i < a.N; ++i) {
    const double yi = y_next, x_l = x_next;
    double *x_cur = xs + (i & 1) * PB_MAX_D, *x_prev = xs + ((i & 1) ^ 1) * PB_MAX_D;
    if (lane < D) x_cur[lane] = x_l;
    if (i + 1 < a.N) {
      if (lane < D) x_next = a.X[(size_t)(i + 1) * D + lane];
      y_next = a.y[i + 1];
    }
    __syncthreads();
    if (i == 0) {
      t0 = has0 ? fd_row_first(a.W2 + (size_t)r0 * n, x_cur, n) : 0.0;
      t1 = has1 ? fd_row_first(a.W2 + (size_t)r1 * n, x_cur, n) : 0.0;
    } else {
      const double u0 = 2.0 * t0, u1 = 2.0 * t1;
      t0 = has0 ? fd_row_pass(G + r0 * ld, x_prev, x_cur, n, u0, neg_eta) : 0.0;
      t1 = has1 ? fd_row_pass(G + r1 * ld, x_prev, x_cur, n, u1, neg_eta) : 0.0;
    }
    // y_hat: lane l adds w1[l] x[l] + t_l^2 + t_{l+64}^2, then the xor butterfly over the 64 lanes (1, 2, 4, ..., 32)
    const double scalar = wave_sum_d(fma(t1, t1, fma(t0, t0, w_l * x_l)));
    if (scalar != scalar) {  // NaN: wave-uniform
      if (lane == 0) {
        a.status[0] = 1;
        a.status[1] = i;
      }
      stopped = true;
      break;
    }
    if (lane == 0) a.pred[i] = scalar;
    const double sign = a.cls ? (-1.0 / (1.0 + exp(scalar * yi))) * yi : 2.0 * (scalar - yi);
    g_l = g_l + sign * x_l;
    w_l = neg_eta * g_l;
    done = i + 1;
    __syncthreads();  // x_prev is the next sample's x_cur
  }
  if (!stopped) {  // the last sample's update of g_W2, which no later pass carries
    double *x_last = xs + ((a.N - 1) & 1) * PB_MAX_D;
    const double u0 = 2.0 * t0, u1 = 2.0 * t1;
    if (has0)
      for (int j = 0; j < n; ++j) G[r0 * ld + j] = G[r0 * ld + j] + u0 * x_last[j];
    if (has1)
      for (int j = 0; j < n; ++j) G[r1 * ld + j] = G[r1 * ld + j] + u1 * x_last[j];
  }
  __syncthreads();
  for (int e = lane; e < m2 * n; e += 64) {
    const int r = e / n, j = e - r * n;
    const double g = G[r * ld + j];
    a.g_W2[e] = g;
    if (done > 0) a.W2[e] = neg_eta * g;  // a walk stopped at its first sample leaves the caller's W2
  }
  if (lane < D) {
    a.w1[lane] = w_l;
    a.g_w1[lane] = g_l;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// RRF_Online (reference models/models_online/RRF_Online.py:70-123).  eps [D, Ds] fixed, gamma [D], w [2 Ds]:
//     z = x (e^gamma * eps);  phi = [cos z, sin z];  y_hat = phi . w;  coef = -y (logit) or y_hat - y (l2);
//     d_w = lr_w exp(w) + coef phi;  d_phi = coef w;  q_d = -sin z_d d_phi_d + cos z_d d_phi_{Ds+d};
//     d_gamma_n = (sum_d x_n eps_nd q_d) e^gamma_n;  w -= lr_w d_w;  gamma -= lr_gamma d_gamma.
// A NaN y_hat leaves w and gamma as they are, writes NaN to that sample's pred and the walk goes on (the reference's loop skips
// such a sample); status[0] counts them.
//   lane d owns spectral sample d: z_d, cos, sin, w_d, w_{Ds+d}, q_d;   lane n owns feature n: x_n, gamma_n, e^gamma_n.
// LDS: eps as [D][lde] doubles, lde = Ds | 1 (lane d reads down a column, lane n along a row: both conflict-free), x, e^gamma and q:
// at the limits 64 * 65 * 8 + 3 * 64 * 8 = 34,816 B.
struct RrfArgs {
  const double *X, *y;  // [N, D], [N]
  const double *eps;    // [D, Ds] row-major, read only
  double *gamma, *w;    // [D], [2 Ds], in / out
  double *pred;         // [N] raw y_hat (NaN for a skipped sample)
  int32_t *status;      // [2]: (NaN samples, the first of them or -1);  (-2, Ds) (grid only): Ds outside [1, Ds_max], nothing was run
                        //      (the other grids' refusal code 2, negated: status[0] >= 0 is a count here)
  double lr_w, lr_g;
  int32_t N, D, Ds, l2;
  // a GRID of settings (fmx_rrf_grid): workgroup s runs Dss[s], lr_ws[s], lr_gs[s] on its own slabs; null: one run
  const int32_t *Dss;
  const double *lr_ws, *lr_gs;
  long long eps_stride, w_stride, pred_stride;  // D Ds_max, 2 Ds_max, N
};

__global__ __launch_bounds__(64) void k_rrf_online(RrfArgs a) {
  extern __shared__ __attribute__((aligned(16))) double pb_smem[];
  const int lane = threadIdx.x;
  if (a.Dss) {
    const long long s = blockIdx.x;
    a.Ds = a.Dss[s];
    a.lr_w = a.lr_ws[s];
    a.lr_g = a.lr_gs[s];
    a.eps += s * a.eps_stride;
    a.gamma += s * a.D;
    a.w += s * a.w_stride;
    a.pred += s * a.pred_stride;
    a.status += 2 * s;
    if (a.Ds < 1 || 2ll * a.Ds > a.w_stride) {
      if (lane == 0) {
        a.status[0] = -2;
        a.status[1] = a.Ds;
      }
      return;
    }
  }
  const int D = a.D, Ds = a.Ds, lde = Ds | 1;
  double *xs = pb_smem, *egs = xs + PB_MAX_D, *qs = egs + PB_MAX_D, *E = qs + PB_MAX_DS;  // E [D][lde]
  for (int e = lane; e < D * Ds; e += 64) {
    const int r = e / Ds, c = e - r * Ds;
    E[r * lde + c] = a.eps[e];
  }
  double gamma_l = lane < D ? a.gamma[lane] : 0.0;
  double wc = lane < Ds ? a.w[lane] : 0.0, ws = lane < Ds ? a.w[Ds + lane] : 0.0;
  double x_next = lane < D ? a.X[lane] : 0.0, y_next = a.y[0];
  int n_nan = 0, first_nan = -1;
  for (int i = 0; i < a.N; ++i) {
    const double yi = y_next, x_l = x_next;
    if (i + 1 < a.N) {
      if (lane < D) x_next = a.X[(size_t)(i + 1) * D + lane];
      y_next = a.y[i + 1];
    }
    const double eg = exp(gamma_l);
    if (lane < D) {
      xs[lane] = x_l;
      egs[lane] = eg;
    }
    __syncthreads();
    // z_d = sum_n x_n (e^gamma_n eps_nd), n ascending; y_hat: lane d adds cos z_d w_d + sin z_d w_{Ds+d}, then the xor butterfly
    double cz = 0.0, sz = 0.0, part = 0.0;
    if (lane < Ds) {
      double z = 0.0;
      for (int n = 0; n < D; ++n) z = fma(xs[n], egs[n] * E[n * lde + lane], z);
      sz = sin(z);
      cz = cos(z);
      part = fma(sz, ws, cz * wc);
    }
    const double scalar = wave_sum_d(part);
    if (lane == 0) a.pred[i] = scalar;
    const bool ok = scalar == scalar;  // wave-uniform
    if (ok) {
      const double coef = a.l2 ? scalar - yi : -yi;  // logit: -y times a softmax over a batch of one
      if (lane < Ds) {
        qs[lane] = (-sz) * (coef * wc) + cz * (coef * ws);
        wc = wc - a.lr_w * (a.lr_w * exp(wc) + coef * cz);
        ws = ws - a.lr_w * (a.lr_w * exp(ws) + coef * sz);
      }
    } else {
      ++n_nan;
      if (first_nan < 0) first_nan = i;
    }
    __syncthreads();
    if (ok && lane < D) {  // d_gamma_n = (sum_d (x_n eps_nd) q_d) e^gamma_n, d ascending
      double acc = 0.0;
      for (int d = 0; d < Ds; ++d) acc = fma(x_l * E[lane * lde + d], qs[d], acc);
      gamma_l = gamma_l - a.lr_g * (acc * eg);
    }
  }
  if (lane < D) a.gamma[lane] = gamma_l;
  if (lane < Ds) {
    a.w[lane] = wc;
    a.w[Ds + lane] = ws;
  }
  if (lane == 0) {
    a.status[0] = n_nan;
    a.status[1] = first_nan;
  }
}
