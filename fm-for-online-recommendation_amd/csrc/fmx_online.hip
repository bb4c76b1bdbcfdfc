// fmx_online.hip -- the stream walkers, one wavefront or one workgroup walking a device-resident stream sample by sample (predict,
// then fit on that sample), and their C ABI: k_fm_online (fmx_fm_online_run), k_fm_pair_online (fmx_fm_pair_online_run), k_mlp_small
// (fmx_mlp_forward / _fit / _fit_opt / _hedge_fit), k_mlp_small_pair (fmx_mlp_pair_fit), k_online_mlp (fmx_online_run_mlp / _opt) and
// k_online_mlp_pair (fmx_online_run_mlp_pair).  On the device they use fmx_common.h alone; the per-sample fallbacks of
// fmx_online_run_mlp and fmx_online_run_mlp_pair issue the batched launches of the other units through fmx_host.h.

#include "fmx_host.h"

namespace {

// ------------------------------------------------------------------------------------------------------------
// k_fm_online: the reference's online protocol on a device-resident stream (pure FM)
// ------------------------------------------------------------------------------------------------------------
// run_experiment (reference fm_adam.py:90-119): for every sample, predict (sigmoid(forward) > 0.5), then fit on that
// one sample.  Steps of one sample are inherently sequential (step i+1 reads the rows step i wrote), so ONE wavefront
// walks the stream: per sample it gathers the F rows (sc1 loads: a row may have been written by the previous sample),
// evaluates the logit, stores the prediction, and applies the rule to the same rows from registers -- the arithmetic of
// k_fm_forward + k_fm_update at B = 1 (each row of a sample is a run of one occurrence), so the tables end
// bit-identical to N calls of fmx_fm_step with B = 1.  The next sample's indices are fetched while the current one is
// processed; the bias lives in registers.  Per sample: one dependent gather + the store acknowledgement (~3 us).
struct OnlineArgs {
  float *rows;
  const int64_t *foff;
  float *bias;
  const int32_t *idx;  // [N, F]
  const float *xv;     // [N, F] or null
  const float *y;      // [N]
  uint8_t *pred;       // [N] sigmoid(logit) > 0.5 BEFORE the sample's update
  float *loss;         // [N] or null
  int32_t *error;
  fmx_hyper_t h;
  int32_t N, F, stride, zoff, loss_kind;
};

// (The field walk below and k_online_mlp's stay two copies: one shared walk left k_fm_online's forward waiting on the prefetch
// of the next sample with vmcnt(0) instead of the row loads only: 3.2 -> 3.6 us per sample.)
template <int LPR, int LAYOUT, int RULE, int NP>
__global__ __launch_bounds__(64) void k_fm_online(OnlineArgs a) {
  constexpr int SLOTS = WAVE / LPR;
  const int lane = threadIdx.x & 63;
  const int slot = lane / LPR, q = lane % LPR;
  const int kp = LPR * 4;
  constexpr bool MOM = LAYOUT == FMX_LAYOUT_MOMENTS;
  // the bias (or its (z, n), or (b, m_b, v_b)) stays in registers
  float b0 = a.bias[0], b1 = LAYOUT != FMX_LAYOUT_WEIGHTS ? a.bias[1] : 0.f, b2 = MOM ? a.bias[2] : 0.f;
  int64_t lo[NP];
  uint32_t vocab[NP];
  bool live[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int f = p * SLOTS + slot;
    live[p] = f < a.F;
    lo[p] = live[p] ? a.foff[f] : 0;
    vocab[p] = live[p] ? (uint32_t)(a.foff[f + 1] - lo[p]) : 0u;
  }
  uint32_t li_n[NP];
  float x_n[NP], y_n = 0.f;
  // branch-free (see forward_sample): beyond the stream or the last field the loads read element 0 and are dropped
  const float *xsrc = a.xv ? a.xv : reinterpret_cast<const float *>(a.idx);
  const bool has_x = a.xv != nullptr;
  auto fetch_inputs = [&](int i) {
    const bool in = i < a.N;
    uint32_t l_[NP];
    float x_[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const size_t o = (live[p] && in) ? (size_t)i * a.F + p * SLOTS + slot : (size_t)0;
      l_[p] = (uint32_t)a.idx[o];
      x_[p] = xsrc[o];
    }
    const float yy = a.y[in ? i : 0];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      li_n[p] = (live[p] && in) ? l_[p] : 0u;
      x_n[p] = (has_x && live[p] && in) ? x_[p] : 1.f;
    }
    y_n = in ? yy : 0.f;
  };
  fetch_inputs(0);
  bool bad = false;
  for (int i = 0; i < a.N; ++i) {
    uint32_t li[NP];
    float x[NP];
    const float y = y_n;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      li[p] = li_n[p];
      x[p] = x_n[p];
    }
    RowRegs row[NP];
    bool ok[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      ok[p] = live[p] && li[p] < vocab[p];
      // branch-free: a dead lane group or a bad index requests the table's first row and drops it (with a branch per
      // pass the rows of a sample went out in NP dependent round trips)
      row[p] = load_row_sc1<LAYOUT, RULE>(a.rows + (size_t)(ok[p] ? lo[p] + li[p] : 0) * a.stride, q, kp, a.zoff);
      bad = bad || (live[p] && !ok[p]);
    }
    fetch_inputs(i + 1);  // independent of the weights: in flight while this sample is processed
    // ---- forward: the arithmetic of k_fm_forward ----
    float4 s = splat(0.f), ss = splat(0.f);
    float fo = 0.f;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      if (ok[p]) {
        const float4 e = x[p] * row[p].v;
        s = s + e;
        ss = ss + e * e;
        fo += row[p].fo.x * x[p];
      }
    }
    fm_field_sums<LPR>(s, ss, fo, lane);
    float sbi;
    fm_bi<LPR>(s, ss, sbi);
    fo = __shfl(fo, 0);
    const float bias_w = bias_weight<LAYOUT>(b0, b1, a.h);
    const float z = fo + sbi + bias_w;
    // ADAM: sample i is step a.h.step + i + 1 -- its constants as the host derives them for a launch (same function, same bits)
    fmx_hyper_t h = a.h;
    if (RULE == FMX_RULE_ADAM) adam_consts(a.h.lr, a.h.beta1, a.h.beta2, a.h.step + i + 1, h.lr, h.beta1, h.beta2);
    float loss, dz;
    bce_loss_dz(a.loss_kind, z, y, 1.0f, loss, dz);
    if (lane == 0) {
      a.pred[i] = sigmoidf_(z) > 0.5f ? 1 : 0;
      if (a.loss) a.loss[i] = loss;
    }
    // ---- fit: every row of the sample is a run of one occurrence (k_fm_update's sums with B = 1, inv_b = 1) ----
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      if (ok[p]) {
        const float xG = x[p] * dz;
        update_row<LAYOUT, RULE>(a.rows + (size_t)(lo[p] + li[p]) * a.stride, q, kp, a.zoff, row[p], xG * s, splat(x[p] * xG),
                                 xG, h);
      }
    }
    bias_step<LAYOUT, RULE>(b0, b1, b2, dz, h);  // (h is a.h but under ADAM, which pairs with MOMENTS alone)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the row stores are acknowledged before the next sample's loads
  }
  const bool any_bad = __ballot(bad) != 0ull;  // an out-of-range index seen by any lane group
  if (lane == 0) {
    a.bias[0] = b0;
    if (LAYOUT == FMX_LAYOUT_FTRL || (MOM && RULE == FMX_RULE_ADAM)) a.bias[1] = b1;
    if (MOM) a.bias[2] = b2;
    if (any_bad && a.error) *a.error = 1;
  }
}

// ------------------------------------------------------------------------------------------------------------
// k_fm_pair_online: k_fm_online for pairs (the pairwise-ranking loss of fmx_pair.inc): one wavefront walks N pairs, predict
// (z_pos > z_neg) then fit on that pair
// ------------------------------------------------------------------------------------------------------------
struct PairOnlineArgs {
  float *rows;
  const int64_t *foff;
  float *bias;
  const int32_t *idx;  // [2N, F]: rows 2i (positive) and 2i + 1 (negative) of pair i
  const float *xv;     // [2N, F] or null
  uint8_t *pred;       // [N] z_pos > z_neg BEFORE the pair's update
  float *logit;        // [2N] or null
  float *loss;         // [N] or null
  int32_t *error;
  fmx_hyper_t h;
  int32_t N, F, stride, zoff;
  float margin;
};

// The fit of pair i is k_fm_update on a batch of two samples (fmx_fm_pair_step with B = 1, inv_b = 1): per field the sorted list
// holds the two occurrences by (row, sample).  Two different rows are two runs of one occurrence, each summed from zero; the same
// row is ONE run whose sums add the positive's terms, then the negative's -- (0 + c_pos) + c_neg -- and the row takes one
// update_row.  The bias gradient is block_sum's dz[0] + dz[1] = +0, which still goes through bias_step (ADAM's moments decay on a
// zero gradient); the mean loss is (loss_i + 0) * inv_b.
template <int LPR, int LAYOUT, int RULE, int NP>
__global__ __launch_bounds__(64) void k_fm_pair_online(PairOnlineArgs a) {
  constexpr int SLOTS = WAVE / LPR;
  const int lane = threadIdx.x & 63;
  const int slot = lane / LPR, q = lane % LPR;
  const int kp = LPR * 4;
  constexpr bool MOM = LAYOUT == FMX_LAYOUT_MOMENTS;
  float b0 = a.bias[0], b1 = LAYOUT != FMX_LAYOUT_WEIGHTS ? a.bias[1] : 0.f, b2 = MOM ? a.bias[2] : 0.f;
  int64_t lo[NP];
  uint32_t vocab[NP];
  bool live[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int f = p * SLOTS + slot;
    live[p] = f < a.F;
    lo[p] = live[p] ? a.foff[f] : 0;
    vocab[p] = live[p] ? (uint32_t)(a.foff[f + 1] - lo[p]) : 0u;
  }
  // the next pair's indices and values: sample t = 0 (positive), 1 (negative).  Branch-free, as in k_fm_online
  uint32_t li_n[2][NP];
  float x_n[2][NP];
  const float *xsrc = a.xv ? a.xv : reinterpret_cast<const float *>(a.idx);
  const bool has_x = a.xv != nullptr;
  auto fetch_inputs = [&](int i) {
    const bool in = i < a.N;
    uint32_t l_[2][NP];
    float x_[2][NP];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        const size_t o = (live[p] && in) ? ((size_t)2 * i + t) * a.F + p * SLOTS + slot : (size_t)0;
        l_[t][p] = (uint32_t)a.idx[o];
        x_[t][p] = xsrc[o];
      }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        li_n[t][p] = (live[p] && in) ? l_[t][p] : 0u;
        x_n[t][p] = (has_x && live[p] && in) ? x_[t][p] : 1.f;
      }
    }
  };
  fetch_inputs(0);
  bool bad = false;
  for (int i = 0; i < a.N; ++i) {
    uint32_t li[2][NP];
    float x[2][NP];
    RowRegs row[2][NP];
    bool ok[2][NP];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        li[t][p] = li_n[t][p];
        x[t][p] = x_n[t][p];
        ok[t][p] = live[p] && li[t][p] < vocab[p];
        row[t][p] = load_row_sc1<LAYOUT, RULE>(a.rows + (size_t)(ok[t][p] ? lo[p] + li[t][p] : 0) * a.stride, q, kp, a.zoff);
        bad = bad || (live[p] && !ok[t][p]);
      }
    }
    fetch_inputs(i + 1);  // independent of the weights: in flight while this pair is processed
    // ---- forward of both samples: the arithmetic of k_fm_forward ----
    const float bias_w = bias_weight<LAYOUT>(b0, b1, a.h);
    float4 S[2];
    float z[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      float4 s = splat(0.f), ss = splat(0.f);
      float fo = 0.f;
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        if (ok[t][p]) {
          const float4 e = x[t][p] * row[t][p].v;
          s = s + e;
          ss = ss + e * e;
          fo += row[t][p].fo.x * x[t][p];
        }
      }
      fm_field_sums<LPR>(s, ss, fo, lane);
      float sbi;
      fm_bi<LPR>(s, ss, sbi);
      fo = __shfl(fo, 0);
      S[t] = s;
      z[t] = fo + sbi + bias_w;
    }
    fmx_hyper_t h = a.h;  // ADAM: pair i is step a.h.step + i + 1 (adam_consts, as the host derives them for a launch)
    if (RULE == FMX_RULE_ADAM) adam_consts(a.h.lr, a.h.beta1, a.h.beta2, a.h.step + i + 1, h.lr, h.beta1, h.beta2);
    float loss, dzp;
    pair_loss_dz(z[0] - z[1], a.margin, 1.0f, loss, dzp);
    const float dz[2] = {dzp, -dzp};
    if (lane == 0) {
      a.pred[i] = z[0] > z[1] ? 1 : 0;
      if (a.logit) {
        a.logit[2 * (size_t)i] = z[0];
        a.logit[2 * (size_t)i + 1] = z[1];
      }
      if (a.loss) a.loss[i] = (0.f + loss) * 1.0f;
    }
    // ---- fit ----
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      float4 cV[2];
      float cA[2], cw[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {  // the occurrence's terms as update_body forms them (dz_bi == dz_first)
        const float xG = x[t][p] * dz[t];
        cV[t] = xG * S[t];
        cA[t] = x[t][p] * xG;
        cw[t] = x[t][p] * dz[t];
      }
      float *rp0 = a.rows + (size_t)(lo[p] + li[0][p]) * a.stride, *rp1 = a.rows + (size_t)(lo[p] + li[1][p]) * a.stride;
      if (ok[0][p] && ok[1][p] && li[0][p] == li[1][p]) {  // one run of two occurrences, in sample order
        const float4 rV = (splat(0.f) + cV[0]) + cV[1];
        const float rA = (0.f + cA[0]) + cA[1], rw = (0.f + cw[0]) + cw[1];
        update_row<LAYOUT, RULE>(rp0, q, kp, a.zoff, row[0][p], rV, splat(rA), rw, h);
      } else {
        if (ok[0][p]) update_row<LAYOUT, RULE>(rp0, q, kp, a.zoff, row[0][p], splat(0.f) + cV[0], splat(0.f + cA[0]), 0.f + cw[0], h);
        if (ok[1][p]) update_row<LAYOUT, RULE>(rp1, q, kp, a.zoff, row[1][p], splat(0.f) + cV[1], splat(0.f + cA[1]), 0.f + cw[1], h);
      }
    }
    bias_step<LAYOUT, RULE>(b0, b1, b2, dz[0] + dz[1], h);            // exactly +0
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the row stores are acknowledged before the next pair's loads
  }
  const bool any_bad = __ballot(bad) != 0ull;
  if (lane == 0) {
    a.bias[0] = b0;
    if (LAYOUT == FMX_LAYOUT_FTRL || (MOM && RULE == FMX_RULE_ADAM)) a.bias[1] = b1;
    if (MOM) a.bias[2] = b2;
    if (any_bad && a.error) *a.error = 1;
  }
}

template <int LPR, int LAYOUT, int RULE>
void launch_pair_online_np(const PairOnlineArgs &a, int np, hipStream_t st) {
  auto launch = [&](auto NP) { hipLaunchKernelGGL((k_fm_pair_online<LPR, LAYOUT, RULE, NP>), dim3(1), dim3(64), 0, st, a); };
  if (!with_one_of<1, 2, 3>(np, launch)) launch(std::integral_constant<int, 4>{});
}

// ------------------------------------------------------------------------------------------------------------
// k_mlp_small: the relu MLP on top of the bi-interaction vector for the online (small batch) steps of DeepFM / NFM
// (reference deepfm_adam.py:82-88,106-119) and the ONN classes' Hedge backprop (deepfm_onn.py:88-154).
// One workgroup does forward, loss, backward and the parameter update of every layer: at B = 1 the reference's autograd
// graph is ~40 ATen launches and a fresh Adam over the hidden layers; here it is one launch.  Limits (host-checked):
// B <= 16, k <= 64, hidden <= 64, layers <= 8; larger shapes stay on the caller's PyTorch path.
// ------------------------------------------------------------------------------------------------------------
constexpr int MLP_MAX_B = 16, MLP_MAX_W = 64, MLP_MAX_L = 8;

enum { MLP_MODE_FORWARD = 0, MLP_MODE_FIT = 1, MLP_MODE_HEDGE = 2 };

struct MlpArgs {
  float *params;  // packed: per layer W [out, in] row-major, then b [out]
  const float *bi;     // [B, kp]
  const float *base;   // [B] logit without the MLP term
  const float *y;      // [B]
  float *alpha;        // HEDGE: [L] in/out
  float *dz_out;       // FIT: [B]
  float *gbi_out;      // FIT: [B, kp]
  float *out;          // FORWARD: [B] logit (adam classes) ; FIT: [1] mean loss or null
  float *layers_out;   // FORWARD: [L, B] sigmoid(base + sum x_l) or null ; HEDGE: [L] losses or null
  float *pred_out;     // FIT: [B] the logit, HEDGE: [B] sigmoid(last layer's logit) -- what forward() returns, before the update; or null
  const float *base_bias;  // null, or the table's bias words: base[b] + bias weight is the logit without the MLP term (NFM)
  int32_t base_bias_ftrl;  // base_bias holds (z, n) of an FTRL table instead of the weight
  fmx_hyper_t h;       // lr / eps (FIT: rule) ; HEDGE: lr = n
  fmx_hyper_t h_table; // base_bias_ftrl: the table's FTRL hyper-parameters (alpha already inverted)
  float hedge_b, hedge_s;
  int32_t B, k, kp, hidden, n_layers, mode, rule, loss_kind;
  float inv_b;
  // FIT under a persistent rule of the network's own (fmx_mlp_opt_t; fmx_mlp_fit_opt / fmx_online_run_mlp_opt): opt_rule is
  // FMX_RULE_ADAGRAD or FMX_RULE_ADAM on the flat moments m, v (the layout of params; global or LDS), 0 otherwise (`rule` applies).
  // oh is what moments_upd reads: lr = the step's step size, eps (ADAM: eps sqrt(1 - beta2^t)), beta1 / beta2 = 1 - beta1 / 1 - beta2
  int32_t opt_rule;
  float *m, *v;
  fmx_hyper_t oh;
  // the pair mode of the FIT step (mlp_small_body<true>; appended: the offsets the other modes read do not depend on them)
  float margin;        // the pair loss's margin
  uint8_t *pair_pred;  // [B / 2] z[2i] > z[2i + 1], before the update; or null
};

// the network's rule for its step t (1-based) as k_mlp_small takes it: ADAM's constants in double, once per step (adam_consts)
inline void mlp_small_set_opt(MlpArgs &a, const fmx_mlp_opt_t &o, int32_t t) {
  a.m = o.m;
  a.v = o.v;
  if (o.rule == FMX_RULE_SGD) {  // the SGD line of the update as it stands, by the network's own learning rate
    a.opt_rule = 0;
    a.rule = FMX_RULE_SGD;
    a.h.lr = o.lr;
    return;
  }
  a.opt_rule = o.rule;
  a.oh.lr = o.lr;
  a.oh.eps = o.eps;
  if (o.rule == FMX_RULE_ADAM) adam_consts(o.lr, o.beta1, o.beta2, t, a.oh.lr, a.oh.beta1, a.oh.beta2, o.eps, &a.oh.eps);
}

__device__ __forceinline__ int mlp_in(const MlpArgs &a, int l) { return l == 0 ? a.k : a.hidden; }
__device__ __forceinline__ float *mlp_w(const MlpArgs &a, int l) {
  size_t off = 0;
  for (int i = 0; i < l; ++i) off += (size_t)a.hidden * mlp_in(a, i) + a.hidden;
  return a.params + off;
}

// the body of k_mlp_small; also called once per sample by k_online_mlp (every pointer may then point into LDS).
// PAIR (k_mlp_small_pair, k_online_mlp_pair; FIT mode only): the B rows are B / 2 pairs, row 2i the positive and row 2i + 1 the
// negative; the loss is pair_loss_dz of d_i = z[2i] - z[2i + 1] and no label is read.  The two rows of a pair belong to adjacent
// lanes of one wavefront (l * B is even), which exchange their logits and evaluate pair_loss_dz on identical operands: the
// negative's dz is the positive's float negated, its loss +0.  Everything else is the pointwise code, and the instantiation
// without PAIR is the body as it was.
template <bool PAIR>
__device__ void mlp_small_body(const MlpArgs &a) {
  __shared__ float acts[(MLP_MAX_L + 1) * MLP_MAX_B * MLP_MAX_W];  // x_0 .. x_L, [l][b][j]
  __shared__ float dA[MLP_MAX_B * MLP_MAX_W], dB[MLP_MAX_B * MLP_MAX_W];  // d x_l (ping-pong); dA is reused as d pre
  __shared__ float dout[MLP_MAX_L * MLP_MAX_B];  // d loss / d (out_l[b]) per layer (HEDGE) or for the last layer (FIT)
  __shared__ float lsum[MLP_MAX_L];
  const int tid = threadIdx.x, nt = blockDim.x;
  const int B = a.B, H = a.hidden, L = a.n_layers;
  auto X = [&](int l, int b, int j) -> float & { return acts[((size_t)l * MLP_MAX_B + b) * MLP_MAX_W + j]; };

  for (int i = tid; i < B * a.k; i += nt) X(0, i / a.k, i % a.k) = a.bi[(size_t)(i / a.k) * a.kp + (i % a.k)];
  __syncthreads();
  // ---- forward ----
  for (int l = 0; l < L; ++l) {
    const int in = mlp_in(a, l);
    const float *W = mlp_w(a, l), *bias = W + (size_t)H * in;
    for (int i = tid; i < B * H; i += nt) {
      const int b = i / H, j = i % H;
      float s = bias[j];
      for (int c = 0; c < in; ++c) s += W[(size_t)j * in + c] * X(l, b, c);
      X(l + 1, b, j) = fmaxf(s, 0.f);
    }
    __syncthreads();
  }
  // ---- per-layer outputs, losses and d loss / d out ----
  if (tid < L) lsum[tid] = 0.f;
  __syncthreads();
  if (tid < L * B) {
    const int l = tid / B, b = tid % B;  // layer l+1's output for sample b
    const bool need = a.mode == MLP_MODE_HEDGE || l == L - 1 || (a.mode == MLP_MODE_FORWARD && a.layers_out);
    float g = 0.f;
    if (need) {
      float s = 0.f;
      for (int j = 0; j < H; ++j) s += X(l + 1, b, j);
      float base_b = a.base[b];
      if (a.base_bias) base_b += a.base_bias_ftrl ? ftrl_w(a.base_bias[0], a.base_bias[1], a.h_table) : a.base_bias[0];
      const float z = base_b + s;
      if (a.pred_out && l == L - 1 && a.mode != MLP_MODE_FORWARD) a.pred_out[b] = a.mode == MLP_MODE_HEDGE ? sigmoidf_(z) : z;
      if (a.mode == MLP_MODE_FORWARD) {
        if (a.layers_out) a.layers_out[(size_t)l * B + b] = sigmoidf_(z);
        if (l == L - 1 && a.out) a.out[b] = z;
      } else if (a.mode == MLP_MODE_FIT) {
        float loss;
        if constexpr (PAIR) {
          const float zo = __shfl_xor(z, 1);  // the partner row's logit: b ^ 1 is lane ^ 1, and both lanes are here (same l)
          const bool pos = (b & 1) == 0;
          pair_loss_dz(pos ? z - zo : zo - z, a.margin, a.inv_b, loss, g);  // both lanes: the same operands, the same bits
          if (!pos) {
            g = -g;
            loss = 0.f;
          } else if (a.pair_pred) {
            a.pair_pred[b >> 1] = z > zo ? 1 : 0;
          }
        } else {
          bce_loss_dz(a.loss_kind, z, a.y[b], a.inv_b, loss, g);
        }
        a.dz_out[b] = g;
        X(0, b, MLP_MAX_W - 1) = loss;  // parked for the ordered sum below (k <= 63 is host-checked in FIT mode)
      } else {  // HEDGE: BCELoss(sigmoid(z), y), mean over the batch; d/dz = (p - y) / B
        const float yy = a.y[b];
        const float p = sigmoidf_(z);
        const float lp = fmaxf(logf(p), -100.f), l1p = fmaxf(log1pf(-p), -100.f);
        X(0, b, MLP_MAX_W - 1 - l) = -(yy * lp + (1.f - yy) * l1p);  // parked per layer
        // autograd through nn.BCELoss then sigmoid: (p - y) / max(p (1 - p), 1e-12) * p (1 - p) -- NOT (p - y) once p
        // saturates (p == 1.0f gives exactly 0, as in the reference)
        const float pq = p * (1.f - p);
        g = a.alpha[l] * ((p - yy) / fmaxf(pq, 1e-12f)) * pq * a.inv_b;
      }
    }
    dout[l * MLP_MAX_B + b] = g;
  }
  __syncthreads();
  if (a.mode == MLP_MODE_FORWARD) return;
  if (a.mode == MLP_MODE_FIT) {
    if (tid == 0 && a.out) {
      float s = 0.f;
      for (int b = 0; b < B; ++b) s += X(0, b, MLP_MAX_W - 1);
      a.out[0] = s * a.inv_b;
    }
  } else if (tid < L) {
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += X(0, b, MLP_MAX_W - 1 - tid);
    lsum[tid] = s * a.inv_b;
  }
  // ---- backward + update, top layer first ----
  float *dcur = dA, *dnext = dB;
  for (int i = tid; i < B * H; i += nt) dcur[(i / H) * MLP_MAX_W + (i % H)] = dout[(L - 1) * MLP_MAX_B + i / H];
  __syncthreads();
  for (int l = L - 1; l >= 0; --l) {
    const int in = mlp_in(a, l);
    float *W = mlp_w(a, l), *bias = W + (size_t)H * in;
    // d pre = d x_{l+1} * (x_{l+1} > 0), in place
    for (int i = tid; i < B * H; i += nt) {
      const int b = i / H, j = i % H;
      if (!(X(l + 1, b, j) > 0.f)) dcur[b * MLP_MAX_W + j] = 0.f;
    }
    __syncthreads();
    // d x_l = W^T d pre (+ this layer's own output gradient in HEDGE mode), with the OLD weights
    for (int i = tid; i < B * in; i += nt) {
      const int b = i / in, c = i % in;
      float s = 0.f;
      for (int j = 0; j < H; ++j) s += W[(size_t)j * in + c] * dcur[b * MLP_MAX_W + j];
      if (a.mode == MLP_MODE_HEDGE && l >= 1) s += dout[(l - 1) * MLP_MAX_B + b];
      dnext[b * MLP_MAX_W + c] = s;
    }
    __syncthreads();
    // parameter gradients (batch summed in sample order) and the update
    for (int i = tid; i < H * in + H; i += nt) {
      float g = 0.f;
      float *p;
      if (i < H * in) {
        const int j = i / in, c = i % in;
        for (int b = 0; b < B; ++b) g += dcur[b * MLP_MAX_W + j] * X(l, b, c);
        p = W + i;
      } else {
        const int j = i - H * in;
        for (int b = 0; b < B; ++b) g += dcur[b * MLP_MAX_W + j];
        p = bias + j;
      }
      if (a.opt_rule != 0) {  // the network's persistent rule: a workgroup-uniform run-time branch, as in mlp_reduce_block
        const size_t o = (size_t)(p - a.params);
        if (a.opt_rule == FMX_RULE_ADAM) {
          moments_upd<FMX_RULE_ADAM>(*p, a.m[o], a.v[o], g, a.oh);
        } else {  // ADAGRAD: m is neither loaded nor stored
          float unused = 0.f;
          moments_upd<FMX_RULE_ADAGRAD>(*p, unused, a.v[o], g, a.oh);
        }
      } else if (a.mode == MLP_MODE_HEDGE || a.rule == FMX_RULE_SGD) *p = *p - a.h.lr * g;
      else *p = *p - a.h.lr * g * rcp_(fabsf(g) + a.h.eps);
    }
    __syncthreads();
    float *t = dcur;
    dcur = dnext;
    dnext = t;
  }
  if (a.mode == MLP_MODE_FIT) {
    for (int i = tid; i < B * a.kp; i += nt) {
      const int b = i / a.kp, c = i % a.kp;
      a.gbi_out[i] = c < a.k ? dcur[b * MLP_MAX_W + c] : 0.f;
    }
  } else if (tid == 0) {  // Hedge: alpha_i *= b^loss_i, floor s / L, normalise (deepfm_onn.py:147-154)
    float al[MLP_MAX_L], z = 0.f;
    for (int i = 0; i < L; ++i) {
      al[i] = fmaxf(a.alpha[i] * powf(a.hedge_b, lsum[i]), a.hedge_s / (float)L);
      z += al[i];
    }
    for (int i = 0; i < L; ++i) {
      a.alpha[i] = al[i] / z;
      if (a.layers_out) a.layers_out[i] = lsum[i];
    }
  }
}

__global__ __launch_bounds__(256) void k_mlp_small(MlpArgs a) { mlp_small_body<false>(a); }
__global__ __launch_bounds__(256) void k_mlp_small_pair(MlpArgs a) { mlp_small_body<true>(a); }

// ------------------------------------------------------------------------------------------------------------
// k_online_mlp: the online predict-then-fit loop of the classes with an MLP, one workgroup walking the stream
// ------------------------------------------------------------------------------------------------------------
// Per sample: wave 0 gathers the sample's rows (sc1 loads: the previous sample may have written them) and evaluates the
// FM part exactly as k_fm_forward does; the whole workgroup runs the MLP step of k_mlp_small (fit or Hedge) on parameters
// that live in LDS for the length of the stream; wave 0 then applies the table update of k_fm_update at B = 1 from the
// rows it still holds (not with Hedge, which leaves the tables alone).  Same arithmetic as the per-sample launches
// (forward, k_mlp_small, sort, update), so the parameters end bit-identical; no launch gaps, no host in the loop.
// fmx_online_run_mlp_opt (has_opt): the network under its own persistent rule -- its moments live in LDS beside the parameters
// (v under ADAGRAD, v and m under ADAM) and are written back at the end -- and the tables under any rule but FTRL, the MOMENTS
// rules included.  Sample i is step hyper->step + i + 1 of the tables and opt.step + i + 1 of the network: ADAM's constants of
// both are derived once per sample by one lane of wave 1 (adam_consts, the function the host uses for a launch: same bits) while
// wave 0 waits for the sample's rows, and reach the other threads through LDS words.
struct OnlineMlpArgs {
  float *rows;
  const int64_t *foff;
  float *bias;
  const int32_t *idx;
  const float *xv;
  const float *y;
  float *pred;      // [N] what forward() returns for the sample, before its update
  int32_t *error;
  float *params;    // global: copied into LDS, written back at the end
  float *alpha;     // Hedge: global [L], same treatment
  fmx_hyper_t h;    // alpha already inverted (table rule); lr / eps also drive the MLP rule
  float hedge_b, hedge_s;
  int32_t N, F, stride, zoff, n_params;
  int32_t k, hidden, n_layers, hedge, fm_term, rule, loss_kind;
  int32_t has_opt;    // fmx_online_run_mlp_opt: the network under opt (m, v global: copied into LDS, written back at the end)
  fmx_mlp_opt_t opt;
};

__device__ __forceinline__ float uniform_f(float x) { return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(x))); }

// OPT: the instantiations of fmx_online_run_mlp_opt (has_opt); fmx_online_run_mlp's own carry none of it
template <int LPR, int LAYOUT, int RULE, bool OPT>
__global__ __launch_bounds__(256) void k_online_mlp(OnlineMlpArgs a) {
  constexpr int SLOTS = WAVE / LPR, NP = 4;
  constexpr bool MOM = LAYOUT == FMX_LAYOUT_MOMENTS;
  extern __shared__ float p_lds[];  // [n_params] the MLP's parameters; has_opt: then v [n_params] (ADAGRAD, ADAM), then m [n_params] (ADAM)
  __shared__ float kc[8];  // ADAM's constants of the sample: tables (step size, 1 - beta1, 1 - beta2), network (the same and eps sqrt(1 - beta2^t))
  __shared__ float bi_lds[MLP_MAX_W], gbi_lds[MLP_MAX_W], alpha_lds[MLP_MAX_L];
  __shared__ float base_lds, dz_lds;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int slot = lane / LPR, q = lane % LPR;
  const int kp = LPR * 4;
  for (int i = tid; i < a.n_params; i += blockDim.x) p_lds[i] = a.params[i];
  const int net_rule = OPT ? a.opt.rule : -1;  // workgroup-uniform
  const bool net_adaptive = net_rule == FMX_RULE_ADAGRAD || net_rule == FMX_RULE_ADAM, net_adam = net_rule == FMX_RULE_ADAM;
  float *v_lds = p_lds + a.n_params, *m_lds = v_lds + a.n_params;
  if (net_adaptive)
    for (int i = tid; i < a.n_params; i += blockDim.x) v_lds[i] = a.opt.v[i];
  if (net_adam)
    for (int i = tid; i < a.n_params; i += blockDim.x) m_lds[i] = a.opt.m[i];
  if (a.hedge && tid < a.n_layers) alpha_lds[tid] = a.alpha[tid];
  // the bias (or its (z, n), or (b, m_b, v_b)) stays in wave 0's registers
  float b0 = a.bias[0], b1 = LAYOUT != FMX_LAYOUT_WEIGHTS ? a.bias[1] : 0.f, b2 = MOM ? a.bias[2] : 0.f;
  int64_t lo[NP];
  uint32_t vocab[NP];
  bool live[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int f = p * SLOTS + slot;
    live[p] = f < a.F;
    lo[p] = live[p] ? a.foff[f] : 0;
    vocab[p] = live[p] ? (uint32_t)(a.foff[f + 1] - lo[p]) : 0u;
  }
  bool bad = false;
  // wave 0: the NEXT sample's indices (and values) are requested while this one is processed -- they do not depend on the
  // weights (as in k_fm_online); branch-free loads (see forward_sample)
  const float *xsrc = a.xv ? a.xv : reinterpret_cast<const float *>(a.idx);
  const bool has_x = a.xv != nullptr;
  uint32_t l_n[NP];
  float x_n[NP], y_n = 0.f;
  __shared__ float y_lds;  // the sample's label, for the MLP step (its own load of y would be one more exposed round trip)
  auto fetch_inputs = [&](int i) {
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const size_t o = (live[p] && i < a.N) ? (size_t)i * a.F + p * SLOTS + slot : (size_t)0;
      l_n[p] = (uint32_t)a.idx[o];
      x_n[p] = xsrc[o];
    }
    y_n = a.y[i < a.N ? i : 0];
  };
  if (wave == 0) fetch_inputs(0);
  __syncthreads();
  for (int i = 0; i < a.N; ++i) {
    uint32_t li[NP];
    float x[NP];
    RowRegs row[NP];
    bool ok[NP];
    float4 S = splat(0.f);
    if (OPT && tid == WAVE && (RULE == FMX_RULE_ADAM || net_adam)) {  // one lane of wave 1, idle until the MLP step
      if (RULE == FMX_RULE_ADAM) adam_consts(a.h.lr, a.h.beta1, a.h.beta2, a.h.step + i + 1, kc[0], kc[1], kc[2]);
      if (net_adam) adam_consts(a.opt.lr, a.opt.beta1, a.opt.beta2, a.opt.step + i + 1, kc[3], kc[4], kc[5], a.opt.eps, &kc[6]);
    }
    if (wave == 0) {
      // ---- the FM part: the arithmetic of k_fm_forward ----
      // branch-free, all row loads together (see forward_sample / k_fm_online): with the loads of a pass under
      // `if (live[p])` a sample's rows went out in 2 NP dependent round trips
      {
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          li[p] = live[p] ? l_n[p] : 0u;
          x[p] = (has_x && live[p]) ? x_n[p] : 1.f;
          ok[p] = live[p] && li[p] < vocab[p];
        }
        if (lane == 0) y_lds = y_n;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          row[p] = load_row_sc1<LAYOUT, RULE>(a.rows + (size_t)(ok[p] ? lo[p] + li[p] : 0) * a.stride, q, kp, a.zoff);
          bad = bad || (live[p] && !ok[p]);
        }
        fetch_inputs(i + 1);
      }
      float4 s = splat(0.f), ss = splat(0.f);
      float fo = 0.f;
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        if (ok[p]) {
          const float4 e = x[p] * row[p].v;
          s = s + e;
          ss = ss + e * e;
          fo += row[p].fo.x * x[p];
        }
      }
      fm_field_sums<LPR>(s, ss, fo, lane);
      S = s;
      float sbi;
      const float4 bi = fm_bi<LPR>(s, ss, sbi);
      fo = __shfl(fo, 0);
      const float bias_w = bias_weight<LAYOUT>(b0, b1, a.h);
      if (lane < LPR) {
        bi_lds[4 * q] = bi.x;
        bi_lds[4 * q + 1] = bi.y;
        bi_lds[4 * q + 2] = bi.z;
        bi_lds[4 * q + 3] = bi.w;
      }
      if (lane == 0) base_lds = a.fm_term ? fo + sbi + bias_w : fo + bias_w;
    }
    __syncthreads();
    // ---- the MLP step of k_mlp_small on LDS-resident parameters ----
    MlpArgs m{};
    m.params = p_lds;
    m.bi = bi_lds;
    m.base = &base_lds;
    m.y = &y_lds;
    m.pred_out = a.pred + i;
    m.h = a.h;
    m.inv_b = 1.0f;
    m.B = 1;
    m.k = a.k;
    m.kp = kp;
    m.hidden = a.hidden;
    m.n_layers = a.n_layers;
    if (a.hedge) {
      m.alpha = alpha_lds;
      m.hedge_b = a.hedge_b;
      m.hedge_s = a.hedge_s;
      m.mode = MLP_MODE_HEDGE;
    } else {
      m.dz_out = &dz_lds;
      m.gbi_out = gbi_lds;
      m.mode = MLP_MODE_FIT;
      m.rule = a.rule;
      m.loss_kind = a.loss_kind;
      if (net_rule == FMX_RULE_SGD) {  // (mlp_small_set_opt)
        m.rule = FMX_RULE_SGD;
        m.h.lr = a.opt.lr;
      } else if (net_adaptive) {
        m.opt_rule = net_rule;
        m.m = m_lds;
        m.v = v_lds;
        m.oh.lr = net_adam ? uniform_f(kc[3]) : a.opt.lr;
        m.oh.eps = net_adam ? uniform_f(kc[6]) : a.opt.eps;
        m.oh.beta1 = net_adam ? uniform_f(kc[4]) : 0.f;
        m.oh.beta2 = net_adam ? uniform_f(kc[5]) : 0.f;
      }
    }
    mlp_small_body<false>(m);
    __syncthreads();
    if (wave == 0 && !a.hedge) {
      // ---- the table update of k_fm_update at B = 1: every row is a run of one occurrence, G = dz [+ dL/dbi] ----
      const float dz = dz_lds;
      const float4 g4 = {gbi_lds[4 * q], gbi_lds[4 * q + 1], gbi_lds[4 * q + 2], gbi_lds[4 * q + 3]};
      const float4 G = splat(a.fm_term ? dz : 0.f) + g4;
      fmx_hyper_t h = a.h;
      if (RULE == FMX_RULE_ADAM) {  // the sample's constants, as update_impl derives them for a launch
        h.lr = uniform_f(kc[0]);
        h.beta1 = uniform_f(kc[1]);
        h.beta2 = uniform_f(kc[2]);
      }
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        if (ok[p]) {
          const float4 xG = x[p] * G;
          update_row<LAYOUT, RULE>(a.rows + (size_t)(lo[p] + li[p]) * a.stride, q, kp, a.zoff, row[p], xG * S, x[p] * xG, x[p] * dz,
                                   h);
        }
      }
      bias_step<LAYOUT, RULE>(b0, b1, b2, dz, h);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the row stores are acknowledged before the next sample's loads
    }
    __syncthreads();
  }
  for (int i = tid; i < a.n_params; i += blockDim.x) a.params[i] = p_lds[i];
  if (net_adaptive)
    for (int i = tid; i < a.n_params; i += blockDim.x) a.opt.v[i] = v_lds[i];
  if (net_adam)
    for (int i = tid; i < a.n_params; i += blockDim.x) a.opt.m[i] = m_lds[i];
  if (a.hedge && tid < a.n_layers) a.alpha[tid] = alpha_lds[tid];
  if (wave == 0) {
    const bool any_bad = __ballot(bad) != 0ull;
    if (lane == 0) {
      if (!a.hedge) {
        a.bias[0] = b0;
        if (LAYOUT == FMX_LAYOUT_FTRL || (MOM && RULE == FMX_RULE_ADAM)) a.bias[1] = b1;
        if (MOM) a.bias[2] = b2;
      }
      if (any_bad && a.error) *a.error = 1;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------
// k_online_mlp_pair: k_online_mlp for pairs (fmx_online_run_mlp_pair): one workgroup walks N pairs, predict (z_pos > z_neg through
// the whole network) then one pair step on that pair
// ------------------------------------------------------------------------------------------------------------
// Per pair: wave 0 holds BOTH samples' rows (as k_fm_pair_online does) and evaluates both FM parts with k_fm_forward's
// arithmetic, leaving bi [2, kp] and base [2] in LDS; the whole workgroup runs mlp_small_body<true> at B = 2 on parameters (and
// moments) that stay in LDS for the length of the stream; wave 0 then applies k_fm_update at B = 2 from the rows it still holds,
// with k_fm_pair_online's run logic: a field whose two samples name the same valid row is ONE run of two occurrences summed in
// sample order, (0 + c_pos) + c_neg, and takes one update_row; otherwise two runs of one, each 0 + c.  The bias gradient
// dz[0] + dz[1] is exactly +0 and still goes through bias_step.  has_opt is a run-time word here (the weights rules take both
// forms), so one instantiation per (kp, table rule) serves fmx_online_run_mlp_pair with and without opt.
struct OnlineMlpPairArgs {
  float *rows;
  const int64_t *foff;
  float *bias;
  const int32_t *idx;  // [2N, F]: rows 2i (positive) and 2i + 1 (negative) of pair i
  const float *xv;     // [2N, F] or null
  uint8_t *pred;       // [N] z_pos > z_neg BEFORE the pair's update
  float *logit;        // [2N] or null
  float *loss;         // [N] or null
  int32_t *error;
  float *params;       // global: copied into LDS, written back at the end
  fmx_hyper_t h;       // alpha already inverted (table rule); lr / eps also drive the MLP rule when has_opt == 0
  int32_t N, F, stride, zoff, n_params;
  int32_t k, hidden, n_layers, fm_term, rule;
  int32_t has_opt;     // the network under opt (m, v global: copied into LDS, written back at the end)
  float margin;
  fmx_mlp_opt_t opt;
};

template <int LPR, int LAYOUT, int RULE>
__global__ __launch_bounds__(256) void k_online_mlp_pair(OnlineMlpPairArgs a) {
  constexpr int SLOTS = WAVE / LPR, NP = 4;
  constexpr bool MOM = LAYOUT == FMX_LAYOUT_MOMENTS;
  extern __shared__ float p_lds[];  // [n_params] the MLP's parameters; then v [n_params] (ADAGRAD, ADAM), then m [n_params] (ADAM)
  __shared__ float kc[8];           // ADAM's constants of the pair, as in k_online_mlp
  __shared__ float bi_lds[2 * MLP_MAX_W], gbi_lds[2 * MLP_MAX_W];  // [2, kp]
  __shared__ float base_lds[2], dz_lds[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int slot = lane / LPR, q = lane % LPR;
  const int kp = LPR * 4;
  for (int i = tid; i < a.n_params; i += blockDim.x) p_lds[i] = a.params[i];
  const int net_rule = a.has_opt ? a.opt.rule : -1;  // workgroup-uniform
  const bool net_adaptive = net_rule == FMX_RULE_ADAGRAD || net_rule == FMX_RULE_ADAM, net_adam = net_rule == FMX_RULE_ADAM;
  float *v_lds = p_lds + a.n_params, *m_lds = v_lds + a.n_params;
  if (net_adaptive)
    for (int i = tid; i < a.n_params; i += blockDim.x) v_lds[i] = a.opt.v[i];
  if (net_adam)
    for (int i = tid; i < a.n_params; i += blockDim.x) m_lds[i] = a.opt.m[i];
  // the bias (or its (b, m_b, v_b)) stays in wave 0's registers
  float b0 = a.bias[0], b1 = LAYOUT != FMX_LAYOUT_WEIGHTS ? a.bias[1] : 0.f, b2 = MOM ? a.bias[2] : 0.f;
  int64_t lo[NP];
  uint32_t vocab[NP];
  bool live[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int f = p * SLOTS + slot;
    live[p] = f < a.F;
    lo[p] = live[p] ? a.foff[f] : 0;
    vocab[p] = live[p] ? (uint32_t)(a.foff[f + 1] - lo[p]) : 0u;
  }
  bool bad = false;
  // wave 0: the NEXT pair's indices (and values), sample t = 0 (positive), 1 (negative); branch-free, as in k_fm_pair_online
  const float *xsrc = a.xv ? a.xv : reinterpret_cast<const float *>(a.idx);
  const bool has_x = a.xv != nullptr;
  uint32_t l_n[2][NP];
  float x_n[2][NP];
  auto fetch_inputs = [&](int i) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        const size_t o = (live[p] && i < a.N) ? ((size_t)2 * i + t) * a.F + p * SLOTS + slot : (size_t)0;
        l_n[t][p] = (uint32_t)a.idx[o];
        x_n[t][p] = xsrc[o];
      }
    }
  };
  if (wave == 0) fetch_inputs(0);
  __syncthreads();
  for (int i = 0; i < a.N; ++i) {
    uint32_t li[2][NP];
    float x[2][NP];
    RowRegs row[2][NP];
    bool ok[2][NP];
    float4 S[2] = {splat(0.f), splat(0.f)};
    if (tid == WAVE && (RULE == FMX_RULE_ADAM || net_adam)) {  // one lane of wave 1, idle until the MLP step
      if (RULE == FMX_RULE_ADAM) adam_consts(a.h.lr, a.h.beta1, a.h.beta2, a.h.step + i + 1, kc[0], kc[1], kc[2]);
      if (net_adam) adam_consts(a.opt.lr, a.opt.beta1, a.opt.beta2, a.opt.step + i + 1, kc[3], kc[4], kc[5], a.opt.eps, &kc[6]);
    }
    if (wave == 0) {
      // ---- the FM part of both samples: the arithmetic of k_fm_forward; all row loads together ----
#pragma unroll
      for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          li[t][p] = live[p] ? l_n[t][p] : 0u;
          x[t][p] = (has_x && live[p]) ? x_n[t][p] : 1.f;
          ok[t][p] = live[p] && li[t][p] < vocab[p];
        }
      }
#pragma unroll
      for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          row[t][p] = load_row_sc1<LAYOUT, RULE>(a.rows + (size_t)(ok[t][p] ? lo[p] + li[t][p] : 0) * a.stride, q, kp, a.zoff);
          bad = bad || (live[p] && !ok[t][p]);
        }
      }
      fetch_inputs(i + 1);
      const float bias_w = bias_weight<LAYOUT>(b0, b1, a.h);
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        float4 s = splat(0.f), ss = splat(0.f);
        float fo = 0.f;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          if (ok[t][p]) {
            const float4 e = x[t][p] * row[t][p].v;
            s = s + e;
            ss = ss + e * e;
            fo += row[t][p].fo.x * x[t][p];
          }
        }
        fm_field_sums<LPR>(s, ss, fo, lane);
        S[t] = s;
        float sbi;
        const float4 bi = fm_bi<LPR>(s, ss, sbi);
        fo = __shfl(fo, 0);
        if (lane < LPR) {
          bi_lds[t * kp + 4 * q] = bi.x;
          bi_lds[t * kp + 4 * q + 1] = bi.y;
          bi_lds[t * kp + 4 * q + 2] = bi.z;
          bi_lds[t * kp + 4 * q + 3] = bi.w;
        }
        if (lane == 0) base_lds[t] = a.fm_term ? fo + sbi + bias_w : fo + bias_w;
      }
    }
    __syncthreads();
    // ---- the pair step of k_mlp_small_pair at B = 2 on LDS-resident parameters ----
    MlpArgs m{};
    m.params = p_lds;
    m.bi = bi_lds;
    m.base = base_lds;
    m.pred_out = a.logit ? a.logit + 2 * (size_t)i : nullptr;
    m.out = a.loss ? a.loss + i : nullptr;
    m.pair_pred = a.pred + i;
    m.margin = a.margin;
    m.h = a.h;
    m.inv_b = 1.0f;
    m.B = 2;
    m.k = a.k;
    m.kp = kp;
    m.hidden = a.hidden;
    m.n_layers = a.n_layers;
    m.dz_out = dz_lds;
    m.gbi_out = gbi_lds;
    m.mode = MLP_MODE_FIT;
    m.rule = a.rule;
    if (net_rule == FMX_RULE_SGD) {  // (mlp_small_set_opt)
      m.rule = FMX_RULE_SGD;
      m.h.lr = a.opt.lr;
    } else if (net_adaptive) {
      m.opt_rule = net_rule;
      m.m = m_lds;
      m.v = v_lds;
      m.oh.lr = net_adam ? uniform_f(kc[3]) : a.opt.lr;
      m.oh.eps = net_adam ? uniform_f(kc[6]) : a.opt.eps;
      m.oh.beta1 = net_adam ? uniform_f(kc[4]) : 0.f;
      m.oh.beta2 = net_adam ? uniform_f(kc[5]) : 0.f;
    }
    mlp_small_body<true>(m);
    __syncthreads();
    if (wave == 0) {
      // ---- the table update of k_fm_update at B = 2: G_t = dz_t [+ dL/dbi_t], runs as in k_fm_pair_online ----
      const float dz[2] = {dz_lds[0], dz_lds[1]};
      float4 G[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const float4 g4 = {gbi_lds[t * kp + 4 * q], gbi_lds[t * kp + 4 * q + 1], gbi_lds[t * kp + 4 * q + 2], gbi_lds[t * kp + 4 * q + 3]};
        G[t] = splat(a.fm_term ? dz[t] : 0.f) + g4;
      }
      fmx_hyper_t h = a.h;
      if (RULE == FMX_RULE_ADAM) {  // the pair's constants, as update_impl derives them for a launch
        h.lr = uniform_f(kc[0]);
        h.beta1 = uniform_f(kc[1]);
        h.beta2 = uniform_f(kc[2]);
      }
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        float4 cV[2], cA[2];
        float cw[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {  // the occurrence's terms as update_body forms them with gbi
          const float4 xG = x[t][p] * G[t];
          cV[t] = xG * S[t];
          cA[t] = x[t][p] * xG;
          cw[t] = x[t][p] * dz[t];
        }
        float *rp0 = a.rows + (size_t)(lo[p] + li[0][p]) * a.stride, *rp1 = a.rows + (size_t)(lo[p] + li[1][p]) * a.stride;
        if (ok[0][p] && ok[1][p] && li[0][p] == li[1][p]) {  // one run of two occurrences, in sample order
          update_row<LAYOUT, RULE>(rp0, q, kp, a.zoff, row[0][p], (splat(0.f) + cV[0]) + cV[1], (splat(0.f) + cA[0]) + cA[1],
                                   (0.f + cw[0]) + cw[1], h);
        } else {
          if (ok[0][p]) update_row<LAYOUT, RULE>(rp0, q, kp, a.zoff, row[0][p], splat(0.f) + cV[0], splat(0.f) + cA[0], 0.f + cw[0], h);
          if (ok[1][p]) update_row<LAYOUT, RULE>(rp1, q, kp, a.zoff, row[1][p], splat(0.f) + cV[1], splat(0.f) + cA[1], 0.f + cw[1], h);
        }
      }
      bias_step<LAYOUT, RULE>(b0, b1, b2, dz[0] + dz[1], h);           // exactly +0
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the row stores are acknowledged before the next pair's loads
    }
    __syncthreads();
  }
  for (int i = tid; i < a.n_params; i += blockDim.x) a.params[i] = p_lds[i];
  if (net_adaptive)
    for (int i = tid; i < a.n_params; i += blockDim.x) a.opt.v[i] = v_lds[i];
  if (net_adam)
    for (int i = tid; i < a.n_params; i += blockDim.x) a.opt.m[i] = m_lds[i];
  if (wave == 0) {
    const bool any_bad = __ballot(bad) != 0ull;
    if (lane == 0) {
      a.bias[0] = b0;
      if (MOM && RULE == FMX_RULE_ADAM) a.bias[1] = b1;
      if (MOM) a.bias[2] = b2;
      if (any_bad && a.error) *a.error = 1;
    }
  }
}

template <int LPR, int LAYOUT, int RULE>
void launch_online_np(const OnlineArgs &a, int np, hipStream_t st) {
  auto launch = [&](auto NP) { hipLaunchKernelGGL((k_fm_online<LPR, LAYOUT, RULE, NP>), dim3(1), dim3(64), 0, st, a); };
  if (!with_one_of<1, 2, 3>(np, launch)) launch(std::integral_constant<int, 4>{});
}

constexpr int ONLINE_MLP_MAX_PARAMS = 8192;  // floats of MLP parameters kept in LDS by k_online_mlp
// ... and with the network's moments beside them (fmx_online_run_mlp_opt): the same cap -- params, v and m are then 96 KB of
// dynamic LDS next to the kernel's 47 KB of static arrays, of the CU's 160 KiB
constexpr int ONLINE_MLP_OPT_MAX_PARAMS = 8192;

// the parameter arrays k_online_mlp keeps in LDS: params, v under the network's ADAGRAD / ADAM, m under its ADAM
inline int online_mlp_arrays(const OnlineMlpArgs &a) {
  if (!a.has_opt || a.opt.rule == FMX_RULE_SGD) return 1;
  return a.opt.rule == FMX_RULE_ADAM ? 3 : 2;
}

template <int LPR, int LAYOUT, int RULE, bool OPT>
void launch_online_mlp_k(const OnlineMlpArgs &a, hipStream_t st) {
  static int raised = 0;  // arrays of ONLINE_MLP_MAX_PARAMS floats the kernel may ask for so far
  const int arrays = online_mlp_arrays(a);
  if (raised < arrays) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_online_mlp<LPR, LAYOUT, RULE, OPT>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, arrays * ONLINE_MLP_MAX_PARAMS * 4);
    raised = arrays;
  }
  hipLaunchKernelGGL((k_online_mlp<LPR, LAYOUT, RULE, OPT>), dim3(1), dim3(256), (size_t)arrays * a.n_params * 4, st, a);
}

template <int LPR, int LAYOUT, int RULE>
void launch_online_mlp_pair_k(const OnlineMlpPairArgs &a, hipStream_t st) {
  static int raised = 0;  // (launch_online_mlp_k)
  const int arrays = !a.has_opt || a.opt.rule == FMX_RULE_SGD ? 1 : a.opt.rule == FMX_RULE_ADAM ? 3 : 2;
  if (raised < arrays) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_online_mlp_pair<LPR, LAYOUT, RULE>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, arrays * ONLINE_MLP_MAX_PARAMS * 4);
    raised = arrays;
  }
  hipLaunchKernelGGL((k_online_mlp_pair<LPR, LAYOUT, RULE>), dim3(1), dim3(256), (size_t)arrays * a.n_params * 4, st, a);
}

}  // namespace

extern "C" {

int fmx_fm_online_run(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, int32_t loss_kind,
                      const int32_t *idx, const float *xv, const float *y, int32_t N, uint8_t *pred_out, float *loss_out,
                      int32_t *error, fmx_stream_t stream) {
  if (int rc = check_table(table)) return rc;
  if (int rc = check_rule(table, rule)) return rc;
  if (mapped(table)) return fail(FMX_ERR_UNSUPPORTED, "fmx_fm_online_run: tables whose fields are pieces of index columns are not taken");
  if (N < 0) return fail(FMX_ERR_ARG, "fmx_fm_online_run: N must be >= 0");
  if (N == 0) return FMX_OK;  // an empty stream (its buffers may be null)
  if (!hyper || !idx || !y || !pred_out) return fail(FMX_ERR_ARG, "fmx_fm_online_run: null argument");
  if (int rc = check_adam(hyper, rule, N)) return rc;
  if (loss_kind != FMX_LOSS_BCE_LOGITS && loss_kind != FMX_LOSS_BCE_SIGMOID) return fail(FMX_ERR_ARG, "fit needs a loss");
  const int lpr = lpr_of(table->kp), slots = WAVE / lpr;
  const int np = (table->n_fields + slots - 1) / slots;
  if (np > 4)
    return fail(FMX_ERR_UNSUPPORTED, "fmx_fm_online_run: %d fields at kp = %d exceed the %d rows one wavefront holds", table->n_fields,
                table->kp, 4 * slots);
  OnlineArgs a;
  a.rows = table->rows;
  a.foff = table->field_offsets;
  a.bias = table->bias;
  a.idx = idx;
  a.xv = xv;
  a.y = y;
  a.pred = pred_out;
  a.loss = loss_out;
  a.error = error;
  a.h = kernel_hyper(hyper, rule);  // ADAM: the kernel derives each sample's constants from lr, beta1, beta2, step
  a.N = N;
  a.F = table->n_fields;
  a.stride = table->row_stride;
  a.zoff = table->z_offset;
  a.loss_kind = loss_kind;
  hipStream_t st = static_cast<hipStream_t>(stream);
  with_lpr(table->kp, [&](auto LPR) {
    with_rule(rule, [&](auto LAYOUT, auto RULE) { launch_online_np<LPR, LAYOUT, RULE>(a, np, st); });
  });
  return check_launch("k_fm_online");
}

int fmx_fm_pair_online_run(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const int32_t *idx, const float *xv,
                           int32_t N, float margin, uint8_t *pred_out, float *logit_out, float *loss_out, int32_t *error,
                           fmx_stream_t stream) {
  const char *who = "fmx_fm_pair_online_run";
  if (int rc = check_pair_args(table, hyper, idx, N, "N", margin, who)) return rc;
  if (int rc = check_rule(table, rule)) return named(rc, who);
  if (!pred_out) return fail(FMX_ERR_ARG, "%s: pred_out is null", who);
  if (N > INT32_MAX / 2) return fail(FMX_ERR_ARG, "%s: N = %d: 2 * N rows exceed int32", who, N);
  if (int rc = check_adam(hyper, rule, N)) return named(rc, who);
  // two samples' rows in registers: 2 x 4 passes of RowRegs fit the wavefront's 512 registers, so the limit is fmx_fm_online_run's
  const int lpr = lpr_of(table->kp), slots = WAVE / lpr;
  const int np = (table->n_fields + slots - 1) / slots;
  if (np > 4)
    return fail(FMX_ERR_UNSUPPORTED, "%s: %d fields at kp = %d exceed the %d rows per sample one wavefront holds", who, table->n_fields,
                table->kp, 4 * slots);
  PairOnlineArgs a;
  a.rows = table->rows;
  a.foff = table->field_offsets;
  a.bias = table->bias;
  a.idx = idx;
  a.xv = xv;
  a.pred = pred_out;
  a.logit = logit_out;
  a.loss = loss_out;
  a.error = error;
  a.h = kernel_hyper(hyper, rule);  // ADAM: the kernel derives each pair's constants from lr, beta1, beta2, step
  a.N = N;
  a.F = table->n_fields;
  a.stride = table->row_stride;
  a.zoff = table->z_offset;
  a.margin = margin;
  with_lpr(table->kp, [&](auto LPR) {
    with_rule(rule, [&](auto LAYOUT, auto RULE) { launch_pair_online_np<LPR, LAYOUT, RULE>(a, np, static_cast<hipStream_t>(stream)); });
  });
  return check_launch("k_fm_pair_online");
}

static int mlp_launch(const fmx_mlp_t *mlp, MlpArgs &a, int32_t B, int32_t kp, fmx_stream_t stream, const char *who, bool pair = false) {
  if (!mlp || !mlp->params) return fail(FMX_ERR_ARG, "%s: null mlp", who);
  if (mlp->n_layers < 1 || mlp->n_layers > MLP_MAX_L || mlp->hidden < 1 || mlp->hidden > MLP_MAX_W || mlp->k < 1 ||
      mlp->k > MLP_MAX_W || B < 1 || B > MLP_MAX_B || kp < mlp->k)
    return fail(FMX_ERR_UNSUPPORTED, "%s: needs B <= %d, k <= %d, hidden <= %d, layers <= %d (got B=%d k=%d hidden=%d layers=%d)", who,
                MLP_MAX_B, MLP_MAX_W, MLP_MAX_W, MLP_MAX_L, B, mlp->k, mlp->hidden, mlp->n_layers);
  a.params = mlp->params;
  a.B = B;
  a.k = mlp->k;
  a.kp = kp;
  a.hidden = mlp->hidden;
  a.n_layers = mlp->n_layers;
  if (pair) {
    hipLaunchKernelGGL(k_mlp_small_pair, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return check_launch("k_mlp_small_pair");
  }
  hipLaunchKernelGGL(k_mlp_small, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  return check_launch("k_mlp_small");
}

// the network's optimizer state for a call of n_steps steps (fmx_mlp_fit_opt, fmx_online_run_mlp_opt): mlp_opt_check's checks of opt
static int mlp_small_opt_check(const fmx_mlp_t *mlp, const fmx_mlp_opt_t *opt, int64_t n_steps, const char *who) {
  if (!opt) return fail(FMX_ERR_ARG, "%s: opt is null", who);
  if (int rc = mlp_opt_state_check(opt, n_steps, who)) return rc;
  if (!aligned16(mlp->params) || !aligned16(opt->v) || (opt->m && !aligned16(opt->m)))
    return fail(FMX_ERR_ALIGN, "%s: mlp->params, opt->m and opt->v must be 16-byte aligned", who);
  return FMX_OK;
}

// fmx_online_run_mlp (opt null) and fmx_online_run_mlp_opt (fit mode with the network under opt's rule, the tables under any rule)
static int online_run_mlp_impl(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, int32_t loss_kind, const fmx_mlp_t *mlp,
                               int32_t hedge, int32_t fm_term, float hedge_b, float hedge_s, float *alpha, const int32_t *idx,
                               const float *xv, const float *y, int32_t N, void *workspace, int64_t workspace_bytes,
                               const fmx_fwd_out_t *fwd, float *scratch, float *pred_out, const fmx_mlp_opt_t *opt, bool with_opt,
                               fmx_stream_t stream, const char *who) {
  if (int rc = check_table(table)) return with_opt ? named(rc, who) : rc;
  if (!hyper || !mlp || !idx || !y || !workspace || !fwd || !scratch || !pred_out) return fail(FMX_ERR_ARG, "%s: null argument", who);
  if (mapped(table)) return fail(FMX_ERR_UNSUPPORTED, "%s: tables whose fields are pieces of index columns are not taken", who);
  if (!fwd->S || !fwd->bi || !fwd->sfirst || !fwd->logit) return fail(FMX_ERR_ARG, "%s: fwd needs S, bi, sfirst, logit", who);
  if (!aligned16(workspace) || !aligned16(scratch)) return fail(FMX_ERR_ALIGN, "%s: workspace and scratch must be 16-byte aligned", who);
  if (hedge && !alpha) return fail(FMX_ERR_ARG, "%s: Hedge needs alpha", who);
  if (with_opt) {
    if (!mlp->params) return fail(FMX_ERR_ARG, "%s: null mlp", who);
    if (int rc = mlp_small_opt_check(mlp, opt, N > 0 ? N : 0, who)) return rc;
    if (int rc = check_rule(table, rule)) return named(rc, who);
    if (int rc = check_adam(hyper, rule, N > 0 ? N : 0)) return named(rc, who);
    if (!fm_term && table->layout == FMX_LAYOUT_FTRL)
      return fail(FMX_ERR_UNSUPPORTED, "%s: fm_term = 0 (NFM) needs a table in the weights or the moments layout", who);
  }
  if (!hedge) {
    if (!with_opt) {
      if (adaptive_rule(rule)) return refuse_adaptive(rule, "fmx_online_run_mlp (fit mode)");
      if (int rc = check_rule(table, rule)) return rc;
      if (rule != FMX_RULE_SIGNADAM && rule != FMX_RULE_SGD) return fail(FMX_ERR_ARG, "%s: rule must be SIGNADAM or SGD", who);
    }
    if (loss_kind != FMX_LOSS_BCE_LOGITS && loss_kind != FMX_LOSS_BCE_SIGMOID) return fail(FMX_ERR_ARG, "%s: fit needs a loss", who);
    if (mlp->k > MLP_MAX_W - 1) return fail(FMX_ERR_UNSUPPORTED, "%s: k <= %d", who, MLP_MAX_W - 1);
    if (int rc = check_sort_geometry(table, 1)) return with_opt ? named(rc, who) : rc;
  } else if (mlp->k + mlp->n_layers > MLP_MAX_W) {
    return fail(FMX_ERR_UNSUPPORTED, "%s: k + layers <= %d", who, MLP_MAX_W);
  }
  if (N < 0) return fail(FMX_ERR_ARG, "%s: N must be >= 0", who);
  hipStream_t st = static_cast<hipStream_t>(stream);
  {  // one workgroup walks the stream when the network fits in LDS and the fields fit one wavefront (k_online_mlp)
    long long n_params = 0;
    for (int l = 0; l < mlp->n_layers; ++l) n_params += (long long)mlp->hidden * (l == 0 ? mlp->k : mlp->hidden) + mlp->hidden;
    const int lpr = lpr_of(table->kp), slots = WAVE / lpr;
    // a fit step on FTRL tables keeps the queued launches; the MOMENTS rules are instantiated for the _opt call alone
    const bool tables_ok = hedge || table->layout == FMX_LAYOUT_WEIGHTS || (with_opt && table->layout == FMX_LAYOUT_MOMENTS);
    if (tune().online_persistent && n_params <= (with_opt ? ONLINE_MLP_OPT_MAX_PARAMS : ONLINE_MLP_MAX_PARAMS) &&
        table->n_fields <= 4 * slots && tables_ok && mlp->hidden <= MLP_MAX_W && mlp->n_layers <= MLP_MAX_L &&
        mlp->k <= MLP_MAX_W - 1 && N > 0) {
      OnlineMlpArgs a;
      memset(&a, 0, sizeof(a));
      a.rows = table->rows;
      a.foff = table->field_offsets;
      a.bias = table->bias;
      a.idx = idx;
      a.xv = xv;
      a.y = y;
      a.pred = pred_out;
      a.error = fwd->error;
      a.params = mlp->params;
      a.alpha = alpha;
      a.h = kernel_hyper(hyper, with_opt ? rule : -1);  // ADAM tables: the kernel derives each sample's constants from lr, beta1, beta2, step
      a.hedge_b = hedge_b;
      a.hedge_s = hedge_s;
      a.N = N;
      a.F = table->n_fields;
      a.stride = table->row_stride;
      a.zoff = table->z_offset;
      a.n_params = (int32_t)n_params;
      a.k = mlp->k;
      a.hidden = mlp->hidden;
      a.n_layers = mlp->n_layers;
      a.hedge = hedge;
      a.fm_term = fm_term;
      a.rule = rule;
      a.loss_kind = loss_kind;
      if (with_opt) {
        a.has_opt = 1;
        a.opt = *opt;
        with_lpr(table->kp, [&](auto LPR) {
          with_rule(rule, [&](auto LAYOUT, auto RULE) {
            if constexpr (LAYOUT != FMX_LAYOUT_FTRL) launch_online_mlp_k<LPR, LAYOUT, RULE, true>(a, st);  // (tables_ok: never FTRL)
          });
        });
        return check_launch("k_online_mlp");
      }
      // FTRL-layout tables are read only (Hedge): FTRL pairs with that layout alone, any rule but SGD takes SIGNADAM (a MOMENTS
      // table, read only too, is read as a weights one)
      const int kernel_rule = table->layout == FMX_LAYOUT_FTRL ? FMX_RULE_FTRL : rule == FMX_RULE_SGD ? FMX_RULE_SGD : FMX_RULE_SIGNADAM;
      with_lpr(table->kp, [&](auto LPR) {
        with_rule_wf(kernel_rule, [&](auto LAYOUT, auto RULE) { launch_online_mlp_k<LPR, LAYOUT, RULE, false>(a, st); });
      });
      return check_launch("k_online_mlp");
    }
  }
  if (int rc = check_workspace(table, 1, workspace, workspace_bytes, who)) return rc;
  const Workspace w = carve(table, 1, workspace);
  const size_t F = (size_t)table->n_fields;
  fmx_fwd_out_t f1 = *fwd;  // one sample: dense outputs
  f1.sample_ld = 0;
  float *dz = scratch, *gbi = scratch + 8;
  for (int i = 0; i < N; ++i) {
    const int32_t *idx_i = idx + (size_t)i * F;
    const float *xv_i = xv ? xv + (size_t)i * F : nullptr;
    if (int rc = forward_impl(table, hyper, idx_i, xv_i, nullptr, 1, FMX_LOSS_NONE, 1.0f, &f1, st)) return rc;
    MlpArgs a{};
    a.bi = fwd->bi;
    a.base = fm_term ? fwd->logit : fwd->sfirst;
    if (!fm_term) {  // NFM: the logit without the MLP term is the first-order sum plus the bias weight
      a.base_bias = table->bias;
      a.base_bias_ftrl = table->layout == FMX_LAYOUT_FTRL;
      a.h_table = kernel_hyper(hyper, -1);
    }
    a.y = y + i;
    a.pred_out = pred_out + i;
    a.h = hyper_for(hyper, -1);
    a.inv_b = 1.0f;
    if (hedge) {
      a.alpha = alpha;
      a.hedge_b = hedge_b;
      a.hedge_s = hedge_s;
      a.mode = MLP_MODE_HEDGE;
    } else {
      a.dz_out = dz;
      a.gbi_out = gbi;
      a.mode = MLP_MODE_FIT;
      a.rule = rule;
      a.loss_kind = loss_kind;
      if (with_opt) mlp_small_set_opt(a, *opt, opt->step + i + 1);  // sample i of the call is step t = opt->step + i + 1 of the network
    }
    if (int rc = mlp_launch(mlp, a, 1, table->kp, stream, who)) return rc;
    if (hedge) continue;  // Hedge trains the hidden layers and alpha only (reference deepfm_onn.py:109-154)
    if (int rc = sort_impl(table, idx_i, 1, w.sorted, w.runs, fwd->error, st)) return rc;
    const fmx_hyper_t hs = hyper_at_step(hyper, with_opt ? rule : -1, i);  // ... and step t = hyper->step + i + 1 of the tables
    if (int rc = update_impl(table, &hs, rule, w, w.sorted, xv_i, fwd->S, dz, fm_term ? dz : nullptr, gbi, 1, nullptr, 1.0f, nullptr,
                             st, nullptr, 0, fwd->error))
      return rc;
  }
  return FMX_OK;
}

int fmx_online_run_mlp(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, int32_t loss_kind,
                       const fmx_mlp_t *mlp, int32_t hedge, int32_t fm_term, float hedge_b, float hedge_s, float *alpha,
                       const int32_t *idx, const float *xv, const float *y, int32_t N, void *workspace, int64_t workspace_bytes,
                       const fmx_fwd_out_t *fwd, float *scratch, float *pred_out, fmx_stream_t stream) {
  return online_run_mlp_impl(table, hyper, rule, loss_kind, mlp, hedge, fm_term, hedge_b, hedge_s, alpha, idx, xv, y, N, workspace,
                             workspace_bytes, fwd, scratch, pred_out, nullptr, false, stream, "fmx_online_run_mlp");
}

int fmx_online_run_mlp_opt(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, int32_t loss_kind, const fmx_mlp_t *mlp,
                           int32_t fm_term, const int32_t *idx, const float *xv, const float *y, int32_t N, void *workspace,
                           int64_t workspace_bytes, const fmx_fwd_out_t *fwd, float *scratch, float *pred_out,
                           const fmx_mlp_opt_t *opt, fmx_stream_t stream) {
  return online_run_mlp_impl(table, hyper, rule, loss_kind, mlp, 0, fm_term, 0.f, 0.f, nullptr, idx, xv, y, N, workspace, workspace_bytes,
                             fwd, scratch, pred_out, opt, true, stream, "fmx_online_run_mlp_opt");
}

int fmx_mlp_forward(const fmx_mlp_t *mlp, const float *bi, int32_t kp, const float *base, int32_t B, float *out,
                    float *layers_out, fmx_stream_t stream) {
  if (!bi || !base || (!out && !layers_out)) return fail(FMX_ERR_ARG, "fmx_mlp_forward: null argument");
  MlpArgs a{};
  a.bi = bi;
  a.base = base;
  a.out = out;
  a.layers_out = layers_out;
  a.mode = MLP_MODE_FORWARD;
  return mlp_launch(mlp, a, B, kp, stream, "fmx_mlp_forward");
}

// fmx_mlp_fit (opt null) and fmx_mlp_fit_opt (the hidden layers under opt's rule; `hyper` and `rule` are then not read)
static int mlp_fit_impl(const fmx_mlp_t *mlp, const fmx_hyper_t *hyper, int32_t rule, int32_t loss_kind, const float *bi, int32_t kp,
                        const float *base, const float *y, int32_t B, float inv_b, float *dz_out, float *gbi_out, float *loss_out,
                        const fmx_mlp_opt_t *opt, bool with_opt, fmx_stream_t stream, const char *who) {
  if (!with_opt && adaptive_rule(rule)) return refuse_adaptive(rule, who);
  if ((!with_opt && !hyper) || !bi || !base || !y || !dz_out || !gbi_out) return fail(FMX_ERR_ARG, "%s: null argument", who);
  if (with_opt) {
    if (!mlp || !mlp->params) return fail(FMX_ERR_ARG, "%s: null mlp", who);
    if (int rc = mlp_small_opt_check(mlp, opt, 1, who)) return rc;
  } else if (rule != FMX_RULE_SIGNADAM && rule != FMX_RULE_SGD) {
    return fail(FMX_ERR_ARG, "%s: rule must be SIGNADAM or SGD", who);
  }
  if (loss_kind != FMX_LOSS_BCE_LOGITS && loss_kind != FMX_LOSS_BCE_SIGMOID) return fail(FMX_ERR_ARG, "%s needs a loss", who);
  if (mlp && mlp->k > MLP_MAX_W - 1) return fail(FMX_ERR_UNSUPPORTED, "%s: k <= %d", who, MLP_MAX_W - 1);
  MlpArgs a{};
  a.bi = bi;
  a.base = base;
  a.y = y;
  a.dz_out = dz_out;
  a.gbi_out = gbi_out;
  a.out = loss_out;
  if (hyper) a.h = hyper_for(hyper, -1);
  a.mode = MLP_MODE_FIT;
  a.rule = rule;
  a.loss_kind = loss_kind;
  a.inv_b = inv_b;
  if (with_opt) mlp_small_set_opt(a, *opt, opt->step + 1);
  return mlp_launch(mlp, a, B, kp, stream, who);
}

int fmx_mlp_fit(const fmx_mlp_t *mlp, const fmx_hyper_t *hyper, int32_t rule, int32_t loss_kind, const float *bi, int32_t kp,
                const float *base, const float *y, int32_t B, float inv_b, float *dz_out, float *gbi_out, float *loss_out,
                fmx_stream_t stream) {
  return mlp_fit_impl(mlp, hyper, rule, loss_kind, bi, kp, base, y, B, inv_b, dz_out, gbi_out, loss_out, nullptr, false, stream, "fmx_mlp_fit");
}

int fmx_mlp_fit_opt(const fmx_mlp_t *mlp, const fmx_hyper_t *hyper, int32_t loss_kind, const float *bi, int32_t kp, const float *base,
                    const float *y, int32_t B, float inv_b, float *dz_out, float *gbi_out, float *loss_out, const fmx_mlp_opt_t *opt,
                    fmx_stream_t stream) {
  return mlp_fit_impl(mlp, hyper, FMX_RULE_SGD, loss_kind, bi, kp, base, y, B, inv_b, dz_out, gbi_out, loss_out, opt, true, stream,
                      "fmx_mlp_fit_opt");
}


// what fmx_mlp_pair_fit refuses, and fmx_online_run_mlp_pair of its network: fmx_mlp_fit's limits on 2 * B_pairs rows, the pair
// arguments, and with opt what fmx_mlp_fit_opt refuses (n_steps steps of the network)
static int mlp_pair_fit_check(const fmx_mlp_t *mlp, const fmx_hyper_t *hyper, int32_t rule, int32_t kp, int32_t B_pairs, float margin,
                              const fmx_mlp_opt_t *opt, int64_t n_steps, const char *who) {
  if (B_pairs < 1) return fail(FMX_ERR_ARG, "%s: B_pairs = %d must be >= 1", who, B_pairs);
  if (!(margin >= 0.f) || !std::isfinite(margin)) return fail(FMX_ERR_ARG, "%s: margin = %g must be finite and >= 0", who, (double)margin);
  if (!mlp || !mlp->params) return fail(FMX_ERR_ARG, "%s: null mlp", who);
  if (opt) {
    if (int rc = mlp_small_opt_check(mlp, opt, n_steps, who)) return rc;
  } else {
    if (adaptive_rule(rule)) return refuse_adaptive(rule, who);
    if (!hyper) return fail(FMX_ERR_ARG, "%s: null argument (hyper)", who);
    if (rule != FMX_RULE_SIGNADAM && rule != FMX_RULE_SGD) return fail(FMX_ERR_ARG, "%s: rule must be SIGNADAM or SGD", who);
  }
  if (mlp->n_layers < 1 || mlp->n_layers > MLP_MAX_L || mlp->hidden < 1 || mlp->hidden > MLP_MAX_W || mlp->k < 1 ||
      mlp->k > MLP_MAX_W - 1 || B_pairs > MLP_MAX_B / 2 || kp < mlp->k)
    return fail(FMX_ERR_UNSUPPORTED, "%s: needs B_pairs <= %d, k <= %d, hidden <= %d, layers <= %d (got B_pairs=%d k=%d hidden=%d layers=%d)",
                who, MLP_MAX_B / 2, MLP_MAX_W - 1, MLP_MAX_W, MLP_MAX_L, B_pairs, mlp->k, mlp->hidden, mlp->n_layers);
  return FMX_OK;
}

// the pair step's arguments as k_mlp_small_pair takes them; the network's step t (1-based) under opt
static void mlp_pair_fit_args(MlpArgs &a, const fmx_hyper_t *hyper, int32_t rule, float margin, float inv_b, const fmx_mlp_opt_t *opt,
                              int32_t t) {
  if (hyper) a.h = hyper_for(hyper, -1);
  a.mode = MLP_MODE_FIT;
  a.rule = rule;
  a.margin = margin;
  a.inv_b = inv_b;
  if (opt) mlp_small_set_opt(a, *opt, t);
}

int fmx_mlp_pair_fit(const fmx_mlp_t *mlp, const fmx_hyper_t *hyper, int32_t rule, const float *bi, int32_t kp, const float *base,
                     int32_t B_pairs, float margin, float inv_b, float *logit_out, float *dz_out, float *gbi_out, float *loss_out,
                     const fmx_mlp_opt_t *opt, fmx_stream_t stream) {
  const char *who = "fmx_mlp_pair_fit";
  if (int rc = mlp_pair_fit_check(mlp, hyper, rule, kp, B_pairs, margin, opt, 1, who)) return rc;
  if (!bi || !base || !dz_out || !gbi_out) return fail(FMX_ERR_ARG, "%s: null argument", who);
  MlpArgs a{};
  a.bi = bi;
  a.base = base;
  a.pred_out = logit_out;
  a.dz_out = dz_out;
  a.gbi_out = gbi_out;
  a.out = loss_out;
  mlp_pair_fit_args(a, opt ? nullptr : hyper, rule, margin, inv_b, opt, opt ? opt->step + 1 : 0);
  return mlp_launch(mlp, a, 2 * B_pairs, kp, stream, who, true);
}

int fmx_online_run_mlp_pair(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_mlp_t *mlp, int32_t fm_term,
                            const int32_t *idx, const float *xv, int32_t N, float margin, void *workspace, int64_t workspace_bytes,
                            const fmx_fwd_out_t *fwd, float *scratch, uint8_t *pred_out, float *logit_out, float *loss_out,
                            const fmx_mlp_opt_t *opt, fmx_stream_t stream) {
  const char *who = "fmx_online_run_mlp_pair";
  static const int32_t no_pairs = 0;  // an empty stream's buffers may be null; everything else is checked as for one pair
  if (int rc = check_pair_args(table, hyper, N == 0 && !idx ? &no_pairs : idx, N > 0 ? N : 1, "N", margin, who)) return rc;
  if (N < 0) return fail(FMX_ERR_ARG, "%s: N = %d must be >= 0", who, N);
  if (N > INT32_MAX / 2) return fail(FMX_ERR_ARG, "%s: N = %d: 2 * N rows exceed int32", who, N);
  if (N > 0 && !pred_out) return fail(FMX_ERR_ARG, "%s: pred_out is null", who);
  if (!workspace || !fwd || !scratch) return fail(FMX_ERR_ARG, "%s: null argument", who);
  if (!fwd->S || !fwd->bi || !fwd->sfirst || !fwd->logit) return fail(FMX_ERR_ARG, "%s: fwd needs S, bi, sfirst, logit", who);
  if (!aligned16(workspace) || !aligned16(scratch)) return fail(FMX_ERR_ALIGN, "%s: workspace and scratch must be 16-byte aligned", who);
  if (int rc = mlp_pair_fit_check(mlp, hyper, rule, table->kp, 1, margin, opt, N, who)) return rc;
  if (int rc = check_rule(table, rule)) return named(rc, who);
  if (opt) {
    if (int rc = check_adam(hyper, rule, N)) return named(rc, who);
    if (!fm_term && table->layout == FMX_LAYOUT_FTRL)
      return fail(FMX_ERR_UNSUPPORTED, "%s: fm_term = 0 (NFM) needs a table in the weights or the moments layout", who);
  }
  if (int rc = check_sort_geometry(table, 2)) return named(rc, who);
  if (int rc = check_workspace(table, 2, workspace, workspace_bytes, who)) return rc;
  if (N == 0) return FMX_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  {  // one workgroup walks the stream when the network fits in LDS and both samples' fields fit one wavefront (k_online_mlp_pair)
    long long n_params = 0;
    for (int l = 0; l < mlp->n_layers; ++l) n_params += (long long)mlp->hidden * (l == 0 ? mlp->k : mlp->hidden) + mlp->hidden;
    const int slots = WAVE / lpr_of(table->kp);
    if (tune().online_persistent && n_params <= ONLINE_MLP_OPT_MAX_PARAMS && table->n_fields <= 4 * slots &&
        table->layout != FMX_LAYOUT_FTRL) {
      OnlineMlpPairArgs a;
      memset(&a, 0, sizeof(a));
      a.rows = table->rows;
      a.foff = table->field_offsets;
      a.bias = table->bias;
      a.idx = idx;
      a.xv = xv;
      a.pred = pred_out;
      a.logit = logit_out;
      a.loss = loss_out;
      a.error = fwd->error;
      a.params = mlp->params;
      a.h = kernel_hyper(hyper, opt ? rule : -1);  // ADAM tables: the kernel derives each pair's constants from lr, beta1, beta2, step
      a.N = N;
      a.F = table->n_fields;
      a.stride = table->row_stride;
      a.zoff = table->z_offset;
      a.n_params = (int32_t)n_params;
      a.k = mlp->k;
      a.hidden = mlp->hidden;
      a.n_layers = mlp->n_layers;
      a.fm_term = fm_term;
      a.rule = rule;
      a.margin = margin;
      if (opt) {
        a.has_opt = 1;
        a.opt = *opt;
      }
      with_lpr(table->kp, [&](auto LPR) {
        with_rule(rule, [&](auto LAYOUT, auto RULE) {
          if constexpr (LAYOUT != FMX_LAYOUT_FTRL) launch_online_mlp_pair_k<LPR, LAYOUT, RULE>(a, st);  // (never FTRL here)
        });
      });
      return check_launch("k_online_mlp_pair");
    }
  }
  // the queued form: per pair forward(B = 2), k_mlp_small_pair, sort(B = 2), update(B = 2), no host synchronisation
  const Workspace w = carve(table, 2, workspace);
  const size_t F = (size_t)table->n_fields;
  fmx_fwd_out_t f2 = *fwd;  // two samples: dense outputs
  f2.sample_ld = 0;
  float *dz = scratch, *gbi = scratch + 8;
  for (int i = 0; i < N; ++i) {
    const int32_t *idx_i = idx + (size_t)i * 2 * F;
    const float *xv_i = xv ? xv + (size_t)i * 2 * F : nullptr;
    if (int rc = forward_impl(table, hyper, idx_i, xv_i, nullptr, 2, FMX_LOSS_NONE, 1.0f, &f2, st)) return rc;
    MlpArgs a{};
    a.bi = fwd->bi;
    a.base = fm_term ? fwd->logit : fwd->sfirst;
    if (!fm_term) {  // NFM: the logit without the MLP term is the first-order sum plus the bias weight
      a.base_bias = table->bias;
      a.base_bias_ftrl = table->layout == FMX_LAYOUT_FTRL;
      a.h_table = kernel_hyper(hyper, -1);
    }
    a.pred_out = logit_out ? logit_out + (size_t)i * 2 : nullptr;
    a.out = loss_out ? loss_out + i : nullptr;
    a.pair_pred = pred_out + i;
    a.dz_out = dz;
    a.gbi_out = gbi;
    mlp_pair_fit_args(a, hyper, rule, margin, 1.0f, opt, opt ? opt->step + i + 1 : 0);
    if (int rc = mlp_launch(mlp, a, 2, table->kp, stream, who, true)) return rc;
    if (int rc = sort_impl(table, idx_i, 2, w.sorted, w.runs, fwd->error, st)) return rc;
    const fmx_hyper_t hs = hyper_at_step(hyper, opt ? rule : -1, i);  // pair i is step t = hyper->step + i + 1 of the tables
    if (int rc = update_impl(table, &hs, rule, w, w.sorted, xv_i, fwd->S, dz, fm_term ? dz : nullptr, gbi, 2, nullptr, 1.0f, nullptr, st,
                             nullptr, 0, fwd->error))
      return rc;
  }
  return FMX_OK;
}

int fmx_mlp_hedge_fit(const fmx_mlp_t *mlp, float lr, float hedge_b, float hedge_s, float *alpha, const float *bi, int32_t kp,
                      const float *base, const float *y, int32_t B, float *losses_out, fmx_stream_t stream) {
  if (!alpha || !bi || !base || !y) return fail(FMX_ERR_ARG, "fmx_mlp_hedge_fit: null argument");
  if (mlp && mlp->k + mlp->n_layers > MLP_MAX_W) return fail(FMX_ERR_UNSUPPORTED, "fmx_mlp_hedge_fit: k + layers <= %d", MLP_MAX_W);
  MlpArgs a{};
  a.bi = bi;
  a.base = base;
  a.y = y;
  a.alpha = alpha;
  a.layers_out = losses_out;
  a.h.lr = lr;
  a.hedge_b = hedge_b;
  a.hedge_s = hedge_s;
  a.mode = MLP_MODE_HEDGE;
  a.inv_b = 1.0f / (float)B;
  return mlp_launch(mlp, a, B, kp, stream, "fmx_mlp_hedge_fit");
}

}  // extern "C"
