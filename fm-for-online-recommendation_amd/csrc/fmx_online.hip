// fmx_online.hip -- the stream walkers, one wavefront or one workgroup walking a device-resident stream sample by sample (predict,
// then fit on that sample), and their C ABI: k_fm_online (fmx_fm_online_run), k_fm_pair_online (fmx_fm_pair_online_run), k_mlp_small
// (fmx_mlp_forward / _fit / _fit_opt / _hedge_fit), k_mlp_small_pair (fmx_mlp_pair_fit), k_online_mlp (fmx_online_run_mlp / _opt) and
// k_online_mlp_pair (fmx_online_run_mlp_pair).  The four walkers are two step loops -- fm_walk and mlp_walk, each over one or two
// samples per step -- built from the per-step pieces of fmx_walk.inc; a kernel adds its objective's label, loss and outputs.  On
// the device they use fmx_common.h alone; the queued form of fmx_online_run_mlp and fmx_online_run_mlp_pair (online_mlp_queued)
// issues the batched launches of the other units through fmx_host.h.  The list forms -- k_mlp_small_list (fmx_mlp_list_fit) and
// k_online_mlp_list (fmx_online_run_mlp_list) -- are fmx_online_list.inc, included at the end of this file.

#include "fmx_host.h"

namespace {

#include "fmx_walk.inc"

// ------------------------------------------------------------------------------------------------------------
// k_fm_online, k_fm_pair_online: the reference's online protocol on a device-resident stream (pure FM)
// ------------------------------------------------------------------------------------------------------------
// run_experiment (reference fm_adam.py:90-119): for every sample, predict (sigmoid(forward) > 0.5), then fit on that
// one sample.  Steps are inherently sequential (step i+1 reads the rows step i wrote), so ONE wavefront walks the stream
// (fm_walk): per step of T samples it gathers their rows (sc1 loads: a row may have been written by the previous step),
// evaluates the logits, stores the prediction, and applies the rule to the same rows from registers -- the arithmetic of
// k_fm_forward + k_fm_update at B = T, so the tables end bit-identical to N calls of fmx_fm_step with B = 1 (T = 1) or of
// fmx_fm_pair_step with one pair (T = 2: the pairwise-ranking loss of fmx_pair.inc, predict z_pos > z_neg).  The next step's
// indices are fetched while the current one is processed; the bias lives in registers.  Per step: one dependent gather + the
// store acknowledgement (~3 us).
struct OnlineArgs {
  WalkTable t;         // idx, xv: [N, F]
  const float *y;      // [N]
  uint8_t *pred;       // [N] sigmoid(logit) > 0.5 BEFORE the sample's update
  float *loss;         // [N] or null
  int32_t loss_kind;
};

struct PairOnlineArgs {
  WalkTable t;         // idx, xv: [2N, F], rows 2i (positive) and 2i + 1 (negative) of pair i
  uint8_t *pred;       // [N] z_pos > z_neg BEFORE the pair's update
  float *logit;        // [2N] or null
  float *loss;         // [N] or null
  float margin;
};

// label(i): the label of step i (a load, or a constant where the objective has none).  loss_dz(i, z, y, dz): the objective's
// loss of the T logits -- dz[t] = d loss / d z[t] at inv_b = 1 -- and its outputs, stored by lane 0.  The bias gradient is
// block_sum's dz[0] + .. + dz[T - 1] (a pair's is exactly +0, which still goes through bias_step: ADAM's moments decay on it).
template <int LPR, int LAYOUT, int RULE, int NP, int T, class Label, class Loss>
__device__ __forceinline__ void fm_walk(const WalkTable &a, Label label, Loss loss_dz) {
  const int lane = threadIdx.x & 63;
  const int slot = lane / LPR, q = lane % LPR;
  const int kp = LPR * 4;
  float b0, b1, b2;
  walk_bias_load<LAYOUT>(a.bias, b0, b1, b2);
  const WalkFields<NP> f = walk_fields<LPR, NP>(a.foff, a.F, slot);
  const WalkX xs = walk_x(a);
  WalkInputs<T, NP> next;
  float y_n = 0.f;
  auto fetch_inputs = [&](int i) {
    const bool in = i < a.N;
    float yy = 0.f;
    walk_fetch<LPR>(next, a, xs, f.live, slot, in, [&](int t) { return (size_t)T * i + t; }, [&] { yy = label(in ? i : 0); });
    y_n = in ? yy : 0.f;
  };
  fetch_inputs(0);
  bool bad = false;
  for (int i = 0; i < a.N; ++i) {
    const WalkInputs<T, NP> in = next;
    const float y = y_n;
    RowRegs row[T][NP];
    bool ok[T][NP];
    walk_gather<LAYOUT, RULE>(row, ok, bad, a, f, in.li, q, kp);
    fetch_inputs(i + 1);  // independent of the weights: in flight while this step is processed
    const float bias_w = bias_weight<LAYOUT>(b0, b1, a.h);
    float4 S[T];
    float z[T], dz[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      float sbi, fo;
      walk_forward<LPR>(row[t], in.x[t], ok[t], lane, S[t], sbi, fo);
      z[t] = fo + sbi + bias_w;
    }
    // ADAM: step i is step a.h.step + i + 1 -- its constants as the host derives them for a launch (same function, same bits)
    fmx_hyper_t h = a.h;
    if (RULE == FMX_RULE_ADAM) adam_consts(a.h.lr, a.h.beta1, a.h.beta2, a.h.step + i + 1, h.lr, h.beta1, h.beta2);
    loss_dz(i, z, y, dz);
    walk_fit<LAYOUT, RULE>(a, f, in.li, ok, row, q, kp, h, [&](int t, int p, float4 &cV, float4 &cA, float &cw) {
      const float xG = in.x[t][p] * dz[t];  // (dz_bi == dz_first)
      cV = xG * S[t];
      cA = splat(in.x[t][p] * xG);
      cw = xG;
    });
    float db = dz[0];
#pragma unroll
    for (int t = 1; t < T; ++t) db = db + dz[t];
    bias_step<LAYOUT, RULE>(b0, b1, b2, db, h);  // (h is a.h but under ADAM, which pairs with MOMENTS alone)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the row stores are acknowledged before the next step's loads
  }
  const bool any_bad = __ballot(bad) != 0ull;  // an out-of-range index seen by any lane group
  if (lane == 0) {
    walk_bias_store<LAYOUT, RULE>(a.bias, b0, b1, b2);
    if (any_bad && a.error) *a.error = 1;
  }
}

template <int LPR, int LAYOUT, int RULE, int NP>
__global__ __launch_bounds__(64) void k_fm_online(OnlineArgs a) {
  fm_walk<LPR, LAYOUT, RULE, NP, 1>(
      a.t, [&](int i) { return a.y[i]; },
      [&](int i, const float(&z)[1], float y, float(&dz)[1]) {
        float loss;
        bce_loss_dz(a.loss_kind, z[0], y, 1.0f, loss, dz[0]);
        if ((threadIdx.x & 63) == 0) {
          a.pred[i] = sigmoidf_(z[0]) > 0.5f ? 1 : 0;
          if (a.loss) a.loss[i] = loss;
        }
      });
}

template <int LPR, int LAYOUT, int RULE, int NP>
__global__ __launch_bounds__(64) void k_fm_pair_online(PairOnlineArgs a) {
  fm_walk<LPR, LAYOUT, RULE, NP, 2>(
      a.t, [](int) { return 0.f; },
      [&](int i, const float(&z)[2], float, float(&dz)[2]) {
        float loss;
        pair_loss_dz(z[0] - z[1], a.margin, 1.0f, loss, dz[0]);
        dz[1] = -dz[0];
        if ((threadIdx.x & 63) == 0) {
          a.pred[i] = z[0] > z[1] ? 1 : 0;
          if (a.logit) {
            a.logit[2 * (size_t)i] = z[0];
            a.logit[2 * (size_t)i + 1] = z[1];
          }
          if (a.loss) a.loss[i] = (0.f + loss) * 1.0f;  // the mean loss: (loss_i + 0) * inv_b
        }
      });
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

// the list mode of the FIT step (mlp_list_body, fmx_online_list.inc): a struct of its own beside MlpArgs, whose size the other
// kernels' descriptors carry.  The B rows are B / G lists, row G i the positive of list i
struct MlpListPart {
  const float *corr;  // [B] log Q of every row's item, subtracted in front of the softmax; null: no correction
  uint8_t *rank;      // [B / G] negatives of list i whose logit is >= its positive's, before the update; or null
  int32_t G;
};
int mlp_list_launch(const fmx_mlp_t *mlp, MlpArgs &a, const MlpListPart &lp, int32_t B, int32_t kp, fmx_stream_t stream);

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
// k_online_mlp, k_online_mlp_pair: the online predict-then-fit loop of the classes with an MLP, one workgroup walking the stream
// ------------------------------------------------------------------------------------------------------------
// Per step of T samples (mlp_walk): wave 0 gathers the samples' rows (sc1 loads: the previous step may have written them) and
// evaluates the FM parts exactly as k_fm_forward does, leaving bi [T, kp] and base [T] in LDS; the whole workgroup runs the MLP step
// of k_mlp_small (T = 1: fit or Hedge) or k_mlp_small_pair (T = 2: B = 2) on parameters that live in LDS for the length of the
// stream; wave 0 then applies the table update of k_fm_update at B = T from the rows it still holds, with fm_walk's run logic (not
// with Hedge, which leaves the tables alone).  Same arithmetic as the per-step launches (forward, k_mlp_small, sort, update), so
// the parameters end bit-identical; no launch gaps, no host in the loop.
// With opt (fmx_online_run_mlp_opt; fmx_online_run_mlp_pair with opt): the network under its own persistent rule -- its moments
// live in LDS beside the parameters (v under ADAGRAD, v and m under ADAM) and are written back at the end -- and the tables under
// any rule but FTRL, the MOMENTS rules included.  Step i is step hyper->step + i + 1 of the tables and opt.step + i + 1 of the
// network: ADAM's constants of both are derived once per step by one lane of wave 1 while wave 0 waits for the step's rows, and
// reach the other threads through LDS words.
struct OnlineMlpArgs {
  WalkTable t;      // h: lr / eps also drive the MLP rule
  const float *y;
  float *pred;      // [N] what forward() returns for the sample, before its update
  float *params;    // global: copied into LDS, written back at the end
  float *alpha;     // Hedge: global [L], same treatment
  float hedge_b, hedge_s;
  int32_t n_params;
  int32_t k, hidden, n_layers, hedge, fm_term, rule, loss_kind;
  int32_t has_opt;    // fmx_online_run_mlp_opt: the network under opt (m, v global: copied into LDS, written back at the end)
  fmx_mlp_opt_t opt;
};

struct OnlineMlpPairArgs {
  WalkTable t;         // idx, xv: [2N, F], rows 2i (positive) and 2i + 1 (negative) of pair i; h: lr / eps also drive the MLP rule when has_opt == 0
  uint8_t *pred;       // [N] z_pos > z_neg BEFORE the pair's update
  float *logit;        // [2N] or null
  float *loss;         // [N] or null
  float *params;       // global: copied into LDS, written back at the end
  int32_t n_params;
  int32_t k, hidden, n_layers, fm_term, rule;
  int32_t has_opt;     // the network under opt (m, v global: copied into LDS, written back at the end)
  float margin;
  fmx_mlp_opt_t opt;
};

// the network's rule of a fit step as mlp_small_body takes it (mlp_small_set_opt), on the LDS-resident arrays and the step's
// constants kc (walk_step_consts).  One assignment per field with the selects on the right: fields stored under branches can end
// as stores through a selected address, and MlpArgs then lives in scratch
__device__ __forceinline__ void walk_net_rule(MlpArgs &m, int net_rule, float *lds, int n_params, const float *kc, const fmx_mlp_opt_t &opt) {
  const bool sgd = net_rule == FMX_RULE_SGD, adam = net_rule == FMX_RULE_ADAM, adaptive = adam || net_rule == FMX_RULE_ADAGRAD;
  m.rule = sgd ? (int)FMX_RULE_SGD : m.rule;
  m.h.lr = sgd ? opt.lr : m.h.lr;
  m.opt_rule = adaptive ? net_rule : 0;
  m.v = adaptive ? lds + n_params : nullptr;
  m.m = adaptive ? lds + 2 * n_params : nullptr;
  m.oh.lr = adam ? uniform_f(kc[3]) : adaptive ? opt.lr : 0.f;
  m.oh.eps = adam ? uniform_f(kc[6]) : adaptive ? opt.eps : 0.f;
  m.oh.beta1 = adam ? uniform_f(kc[4]) : 0.f;
  m.oh.beta2 = adam ? uniform_f(kc[5]) : 0.f;
}

// a: the walker's arguments (what both structs above name alike).  hedge / alpha: the Hedge step, which trains the hidden layers
// and alpha (staged in LDS like the network) and leaves the tables alone.  label(i): as in fm_walk.  objective(m, i, y, alpha): the
// objective's own fields of step i's MlpArgs -- its outputs, its loss, and under Hedge the mode -- given the LDS words of the
// step's label and of alpha.  (The pair walker has neither label nor Hedge and hands in constants.  With these parts moved out to
// the pointwise kernel behind an objective object, k_online_mlp under the network's ADAM measured 3 - 4 % slower:
// profiles/walker_seam_ab.txt, D.)
template <int LPR, int LAYOUT, int RULE, int T, class Args, class Label, class Objective>
__device__ __forceinline__ void mlp_walk(const Args &a, int net_rule, bool hedge, float *alpha, Label label, Objective objective) {
  constexpr int NP = WALK_MAX_NP;
  extern __shared__ float p_lds[];  // [n_params] the MLP's parameters, then its moments (walk_net_arrays)
  __shared__ float kc[8];           // ADAM's constants of the step (walk_step_consts)
  __shared__ float bi_lds[T * MLP_MAX_W], gbi_lds[T * MLP_MAX_W], alpha_lds[MLP_MAX_L];  // [T, kp]
  __shared__ float base_lds[T], dz_lds[T];
  __shared__ float y_lds;  // the step's label, for the MLP step (its own load of y would be one more exposed round trip)
  const WalkTable &t = a.t;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int slot = lane / LPR, q = lane % LPR;
  const int kp = LPR * 4;
  walk_net_stage<false>(p_lds, a.params, a.opt, a.n_params, net_rule);
  if (hedge && tid < a.n_layers) alpha_lds[tid] = alpha[tid];
  float b0, b1, b2;  // in wave 0's registers
  walk_bias_load<LAYOUT>(t.bias, b0, b1, b2);
  const WalkFields<NP> f = walk_fields<LPR, NP>(t.foff, t.F, slot);
  bool bad = false;
  // wave 0: the NEXT step's indices (and values) are requested while this one is processed, as in fm_walk.  This prefetch is
  // mlp_walk's OWN, not walk_fetch: the words are kept as loaded and selected at the start of their step.  walk_fetch's selects
  // stand behind its loads, inside wave 0's branch, and the values leave that branch only once loaded: wave 0 then waited for the
  // prefetch (vmcnt(0)) before the MLP step's first barrier instead of leaving it in flight across the step.  With walk_fetch
  // here k_online_mlp_pair at 5 x 10 under signadam measured 13.09 us per pair against the parent's 12.81, with this copy
  // 12.86 against 12.88 (profiles/walker_seam_ab.txt, C)
  constexpr int SLOTS = WAVE / LPR;
  const WalkX xs = walk_x(t);
  WalkInputs<T, NP> next;  // as loaded
  float y_n = 0.f;
  auto fetch_inputs = [&](int i) {
#pragma unroll
    for (int s = 0; s < T; ++s) {
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        const size_t o = (f.live[p] && i < t.N) ? ((size_t)T * i + s) * t.F + p * SLOTS + slot : (size_t)0;
        next.li[s][p] = (uint32_t)t.idx[o];
        next.x[s][p] = xs.src[o];
      }
    }
    y_n = label(i < t.N ? i : 0);
  };
  if (wave == 0) fetch_inputs(0);
  __syncthreads();
  for (int i = 0; i < t.N; ++i) {
    WalkInputs<T, NP> in;
    RowRegs row[T][NP];
    bool ok[T][NP];
    float4 S[T];
#pragma unroll
    for (int s = 0; s < T; ++s) S[s] = splat(0.f);
    // one lane of wave 1, idle until the MLP step
    if (tid == WAVE && (RULE == FMX_RULE_ADAM || net_rule == FMX_RULE_ADAM)) walk_step_consts<RULE>(kc, t.h, a.opt, net_rule, i);
    if (wave == 0) {
      // ---- the FM part of the step's samples ----
#pragma unroll
      for (int s = 0; s < T; ++s) {
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          in.li[s][p] = f.live[p] ? next.li[s][p] : 0u;
          in.x[s][p] = (xs.has && f.live[p]) ? next.x[s][p] : 1.f;
        }
      }
      if (lane == 0) y_lds = y_n;
      walk_gather<LAYOUT, RULE>(row, ok, bad, t, f, in.li, q, kp);
      fetch_inputs(i + 1);
      const float bias_w = bias_weight<LAYOUT>(b0, b1, t.h);
#pragma unroll
      for (int s = 0; s < T; ++s) {
        float sbi, fo;
        const float4 bi = walk_forward<LPR>(row[s], in.x[s], ok[s], lane, S[s], sbi, fo);
        if (lane < LPR) {
          bi_lds[s * kp + 4 * q] = bi.x;
          bi_lds[s * kp + 4 * q + 1] = bi.y;
          bi_lds[s * kp + 4 * q + 2] = bi.z;
          bi_lds[s * kp + 4 * q + 3] = bi.w;
        }
        if (lane == 0) base_lds[s] = a.fm_term ? fo + sbi + bias_w : fo + bias_w;
      }
    }
    __syncthreads();
    // ---- the step of k_mlp_small (B = 1) or k_mlp_small_pair (B = 2) on LDS-resident parameters ----
    MlpArgs m{};
    m.params = p_lds;
    m.bi = bi_lds;
    m.base = base_lds;
    m.h = t.h;
    m.inv_b = 1.0f;
    m.B = T;
    m.k = a.k;
    m.kp = kp;
    m.hidden = a.hidden;
    m.n_layers = a.n_layers;
    objective(m, i, &y_lds, alpha_lds);
    if (!hedge) {
      m.dz_out = dz_lds;
      m.gbi_out = gbi_lds;
      m.mode = MLP_MODE_FIT;
      m.rule = a.rule;
      walk_net_rule(m, net_rule, p_lds, a.n_params, kc, a.opt);
    }
    mlp_small_body<T == 2>(m);
    __syncthreads();
    if (wave == 0 && !hedge) {
      // ---- the table update of k_fm_update at B = T: G_s = dz_s [+ dL/dbi_s] ----
      float dz[T];
      float4 G[T];
#pragma unroll
      for (int s = 0; s < T; ++s) {
        dz[s] = dz_lds[s];
        const float4 g4 = {gbi_lds[s * kp + 4 * q], gbi_lds[s * kp + 4 * q + 1], gbi_lds[s * kp + 4 * q + 2], gbi_lds[s * kp + 4 * q + 3]};
        G[s] = splat(a.fm_term ? dz[s] : 0.f) + g4;
      }
      fmx_hyper_t h = t.h;
      if (RULE == FMX_RULE_ADAM) {  // the step's constants, as update_impl derives them for a launch
        h.lr = uniform_f(kc[0]);
        h.beta1 = uniform_f(kc[1]);
        h.beta2 = uniform_f(kc[2]);
      }
      walk_fit<LAYOUT, RULE>(t, f, in.li, ok, row, q, kp, h, [&](int s, int p, float4 &cV, float4 &cA, float &cw) {
        const float4 xG = in.x[s][p] * G[s];  // the occurrence's terms as update_body forms them with gbi
        cV = xG * S[s];
        cA = in.x[s][p] * xG;
        cw = in.x[s][p] * dz[s];
      });
      float db = dz[0];
#pragma unroll
      for (int s = 1; s < T; ++s) db = db + dz[s];  // (a pair's: exactly +0)
      bias_step<LAYOUT, RULE>(b0, b1, b2, db, h);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the row stores are acknowledged before the next step's loads
    }
    __syncthreads();
  }
  walk_net_stage<true>(p_lds, a.params, a.opt, a.n_params, net_rule);
  if (hedge && tid < a.n_layers) alpha[tid] = alpha_lds[tid];
  if (wave == 0) {
    const bool any_bad = __ballot(bad) != 0ull;
    if (lane == 0) {
      if (!hedge) walk_bias_store<LAYOUT, RULE>(t.bias, b0, b1, b2);
      if (any_bad && t.error) *t.error = 1;
    }
  }
}

// OPT: the instantiations of fmx_online_run_mlp_opt (has_opt); fmx_online_run_mlp's own carry none of it
template <int LPR, int LAYOUT, int RULE, bool OPT>
__global__ __launch_bounds__(256) void k_online_mlp(OnlineMlpArgs a) {
  mlp_walk<LPR, LAYOUT, RULE, 1>(
      a, OPT ? a.opt.rule : -1, a.hedge != 0, a.alpha, [&](int i) { return a.y[i]; },
      [&](MlpArgs &m, int i, const float *y, float *alpha) {
        m.y = y;
        m.pred_out = a.pred + i;
        if (a.hedge) {
          m.alpha = alpha;
          m.hedge_b = a.hedge_b;
          m.hedge_s = a.hedge_s;
          m.mode = MLP_MODE_HEDGE;
        } else {
          m.loss_kind = a.loss_kind;
        }
      });
}

// has_opt is a run-time word here (the weights rules take both forms), so one instantiation per (kp, table rule) serves
// fmx_online_run_mlp_pair with and without opt
template <int LPR, int LAYOUT, int RULE>
__global__ __launch_bounds__(256) void k_online_mlp_pair(OnlineMlpPairArgs a) {
  mlp_walk<LPR, LAYOUT, RULE, 2>(
      a, a.has_opt ? a.opt.rule : -1, false, nullptr, [](int) { return 0.f; },
      [&](MlpArgs &m, int i, const float *, float *) {
        m.pred_out = a.logit ? a.logit + 2 * (size_t)i : nullptr;
        m.out = a.loss ? a.loss + i : nullptr;
        m.pair_pred = a.pred + i;
        m.margin = a.margin;
      });
}

constexpr int ONLINE_MLP_MAX_PARAMS = 8192;  // floats of MLP parameters kept in LDS by k_online_mlp
// ... and with the network's moments beside them (fmx_online_run_mlp_opt): the same cap -- params, v and m are then 96 KB of
// dynamic LDS next to the kernel's 47 KB of static arrays, of the CU's 160 KiB
constexpr int ONLINE_MLP_OPT_MAX_PARAMS = 8192;
constexpr int ONLINE_MLP_LDS_BYTES = 3 * ONLINE_MLP_MAX_PARAMS * 4;  // the most a launch asks for: the limit of every instantiation

template <class Args>
size_t online_mlp_lds(const Args &a) { return (size_t)walk_net_arrays(a.has_opt ? a.opt.rule : -1) * a.n_params * 4; }

template <int LPR, int LAYOUT, int RULE, bool OPT>
int launch_online_mlp_k(const OnlineMlpArgs &a, hipStream_t st) {
  if (int rc = raise_lds_limit<k_online_mlp<LPR, LAYOUT, RULE, OPT>>(ONLINE_MLP_LDS_BYTES, "k_online_mlp")) return rc;
  hipLaunchKernelGGL((k_online_mlp<LPR, LAYOUT, RULE, OPT>), dim3(1), dim3(256), online_mlp_lds(a), st, a);
  return check_launch("k_online_mlp");
}

template <int LPR, int LAYOUT, int RULE>
int launch_online_mlp_pair_k(const OnlineMlpPairArgs &a, hipStream_t st) {
  if (int rc = raise_lds_limit<k_online_mlp_pair<LPR, LAYOUT, RULE>>(ONLINE_MLP_LDS_BYTES, "k_online_mlp_pair")) return rc;
  hipLaunchKernelGGL((k_online_mlp_pair<LPR, LAYOUT, RULE>), dim3(1), dim3(256), online_mlp_lds(a), st, a);
  return check_launch("k_online_mlp_pair");
}

// the table part of the network walkers' arguments and what both name alike; false: the call keeps the queued launches (the
// network does not fit in LDS, or a sample's fields do not fit one wavefront)
template <class Args>
bool online_mlp_args(Args &a, const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_mlp_t *mlp, int32_t fm_term,
                     const int32_t *idx, const float *xv, int32_t *error, int32_t N, const fmx_mlp_opt_t *opt) {
  const long long n_params = mlp_n_params(mlp);
  if (!tune().online_persistent || n_params > (opt ? ONLINE_MLP_OPT_MAX_PARAMS : ONLINE_MLP_MAX_PARAMS) ||
      walk_passes(table) > WALK_MAX_NP)
    return false;
  memset(&a, 0, sizeof(a));
  a.t = walk_table(table, hyper, opt ? rule : -1, idx, xv, error, N);  // ADAM tables come with opt alone
  a.params = mlp->params;
  a.n_params = (int32_t)n_params;
  a.k = mlp->k;
  a.hidden = mlp->hidden;
  a.n_layers = mlp->n_layers;
  a.fm_term = fm_term;
  a.rule = rule;
  if (opt) {
    a.has_opt = 1;
    a.opt = *opt;
  }
  return true;
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

// The queued form of the network walkers: per step of R rows forward(B = R), k_mlp_small (or _pair), sort(B = R), update(B = R), no
// host synchronisation.  set_mode(m, i): the mode's fields of step i's MlpArgs; no_update: Hedge trains the hidden layers and alpha
// only (reference deepfm_onn.py:109-154).  rule_t: the rule whose step count the tables' hyper-parameters follow (-1: none).
// scratch: dz [R] at 0, gbi [R, kp] at gbi_at.  list (fmx_online_run_mlp_list): the R rows are ONE list -- k_mlp_small_list with row
// R i of list->corr (or null) and list->rank + i, and the update on the list steps' copy of the table, whose bias rule runs on the
// LIST_BIAS_SCRATCH bytes behind the step workspace (fmx_list.inc).
template <class Mode>
int online_mlp_queued(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, int rule_t, const fmx_mlp_t *mlp, int32_t fm_term,
                      const int32_t *idx, const float *xv, int32_t N, int R, void *workspace, const fmx_fwd_out_t *fwd, float *scratch,
                      bool no_update, fmx_stream_t stream, const char *who, Mode set_mode, int gbi_at = 8,
                      const MlpListPart *list = nullptr) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  const Workspace w = carve(table, R, workspace);
  const fmx_table_t tu = list ? list_update_table(table, workspace, w.bytes) : *table;
  const size_t F = (size_t)table->n_fields;
  fmx_fwd_out_t f1 = *fwd;  // R samples: dense outputs
  f1.sample_ld = 0;
  float *dz = scratch, *gbi = scratch + gbi_at;
  for (int i = 0; i < N; ++i) {
    const int32_t *idx_i = idx + (size_t)i * R * F;
    const float *xv_i = xv ? xv + (size_t)i * R * F : nullptr;
    if (int rc = forward_impl(table, hyper, idx_i, xv_i, nullptr, R, FMX_LOSS_NONE, 1.0f, &f1, st)) return rc;
    MlpArgs a{};
    a.bi = fwd->bi;
    a.base = fm_term ? fwd->logit : fwd->sfirst;
    if (!fm_term) {  // NFM: the logit without the MLP term is the first-order sum plus the bias weight
      a.base_bias = table->bias;
      a.base_bias_ftrl = table->layout == FMX_LAYOUT_FTRL;
      a.h_table = kernel_hyper(hyper, -1);
    }
    a.dz_out = dz;
    a.gbi_out = gbi;
    set_mode(a, i);
    if (list) {
      const MlpListPart lp = {list->corr ? list->corr + (size_t)i * R : nullptr, list->rank + i, R};
      if (int rc = mlp_list_launch(mlp, a, lp, R, table->kp, stream)) return rc;
    } else if (int rc = mlp_launch(mlp, a, R, table->kp, stream, who, R == 2)) {
      return rc;
    }
    if (no_update) continue;
    if (int rc = sort_impl(table, idx_i, R, w.sorted, w.runs, fwd->error, st)) return rc;
    const fmx_hyper_t hs = hyper_at_step(hyper, rule_t, i);  // step i is step t = hyper->step + i + 1 of the tables
    if (int rc = update_impl(&tu, &hs, rule, w, w.sorted, xv_i, fwd->S, dz, fm_term ? dz : nullptr, gbi, R, nullptr, 1.0f, nullptr, st,
                             nullptr, 0, fwd->error))
      return rc;
  }
  return FMX_OK;
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
  int max_fields;
  const int np = walk_passes(table, &max_fields);
  if (np > WALK_MAX_NP)
    return fail(FMX_ERR_UNSUPPORTED, "fmx_fm_online_run: %d fields at kp = %d exceed the %d rows one wavefront holds", table->n_fields,
                table->kp, max_fields);
  OnlineArgs a;
  a.t = walk_table(table, hyper, rule, idx, xv, error, N);
  a.y = y;
  a.pred = pred_out;
  a.loss = loss_out;
  a.loss_kind = loss_kind;
  hipStream_t st = static_cast<hipStream_t>(stream);
  with_lpr(table->kp, [&](auto LPR) {
    with_rule(rule, [&](auto LAYOUT, auto RULE) {
      with_walk_np(np, [&](auto NP) { hipLaunchKernelGGL((k_fm_online<LPR, LAYOUT, RULE, NP>), dim3(1), dim3(64), 0, st, a); });
    });
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
  int max_fields;
  const int np = walk_passes(table, &max_fields);
  if (np > WALK_MAX_NP)
    return fail(FMX_ERR_UNSUPPORTED, "%s: %d fields at kp = %d exceed the %d rows per sample one wavefront holds", who, table->n_fields,
                table->kp, max_fields);
  PairOnlineArgs a;
  a.t = walk_table(table, hyper, rule, idx, xv, error, N);
  a.pred = pred_out;
  a.logit = logit_out;
  a.loss = loss_out;
  a.margin = margin;
  hipStream_t st = static_cast<hipStream_t>(stream);
  with_lpr(table->kp, [&](auto LPR) {
    with_rule(rule, [&](auto LAYOUT, auto RULE) {
      with_walk_np(np, [&](auto NP) { hipLaunchKernelGGL((k_fm_pair_online<LPR, LAYOUT, RULE, NP>), dim3(1), dim3(64), 0, st, a); });
    });
  });
  return check_launch("k_fm_pair_online");
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
  // one workgroup walks the stream when the network fits in LDS and the fields fit one wavefront (k_online_mlp).  A fit step on
  // FTRL tables keeps the queued launches; the MOMENTS rules are instantiated for the _opt call alone
  const bool tables_ok = hedge || table->layout == FMX_LAYOUT_WEIGHTS || (with_opt && table->layout == FMX_LAYOUT_MOMENTS);
  OnlineMlpArgs a;
  if (tables_ok && mlp->hidden <= MLP_MAX_W && mlp->n_layers <= MLP_MAX_L && mlp->k <= MLP_MAX_W - 1 && N > 0 &&
      online_mlp_args(a, table, hyper, rule, mlp, fm_term, idx, xv, fwd->error, N, opt)) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    a.y = y;
    a.pred = pred_out;
    a.alpha = alpha;
    a.hedge_b = hedge_b;
    a.hedge_s = hedge_s;
    a.hedge = hedge;
    a.loss_kind = loss_kind;
    int rc = FMX_OK;
    if (with_opt) {
      with_lpr(table->kp, [&](auto LPR) {
        with_rule(rule, [&](auto LAYOUT, auto RULE) {
          if constexpr (LAYOUT != FMX_LAYOUT_FTRL) rc = launch_online_mlp_k<LPR, LAYOUT, RULE, true>(a, st);  // (tables_ok: never FTRL)
        });
      });
      return rc;
    }
    // FTRL-layout tables are read only (Hedge): FTRL pairs with that layout alone, any rule but SGD takes SIGNADAM (a MOMENTS
    // table, read only too, is read as a weights one)
    const int kernel_rule = table->layout == FMX_LAYOUT_FTRL ? FMX_RULE_FTRL : rule == FMX_RULE_SGD ? FMX_RULE_SGD : FMX_RULE_SIGNADAM;
    with_lpr(table->kp, [&](auto LPR) {
      with_rule_wf(kernel_rule, [&](auto LAYOUT, auto RULE) { rc = launch_online_mlp_k<LPR, LAYOUT, RULE, false>(a, st); });
    });
    return rc;
  }
  if (int rc = check_workspace(table, 1, workspace, workspace_bytes, who)) return rc;
  return online_mlp_queued(table, hyper, rule, with_opt ? rule : -1, mlp, fm_term, idx, xv, N, 1, workspace, fwd, scratch, hedge != 0,
                           stream, who, [&](MlpArgs &m, int i) {
                             m.y = y + i;
                             m.pred_out = pred_out + i;
                             m.h = hyper_for(hyper, -1);
                             m.inv_b = 1.0f;
                             if (hedge) {
                               m.alpha = alpha;
                               m.hedge_b = hedge_b;
                               m.hedge_s = hedge_s;
                               m.mode = MLP_MODE_HEDGE;
                               return;
                             }
                             m.mode = MLP_MODE_FIT;
                             m.rule = rule;
                             m.loss_kind = loss_kind;
                             // sample i of the call is step t = opt->step + i + 1 of the network
                             if (with_opt) mlp_small_set_opt(m, *opt, opt->step + i + 1);
                           });
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
  // one workgroup walks the stream when the network fits in LDS and both samples' fields fit one wavefront (k_online_mlp_pair)
  OnlineMlpPairArgs a;
  if (table->layout != FMX_LAYOUT_FTRL && online_mlp_args(a, table, hyper, rule, mlp, fm_term, idx, xv, fwd->error, N, opt)) {
    a.pred = pred_out;
    a.logit = logit_out;
    a.loss = loss_out;
    a.margin = margin;
    int rc = FMX_OK;
    with_lpr(table->kp, [&](auto LPR) {
      with_rule(rule, [&](auto LAYOUT, auto RULE) {
        if constexpr (LAYOUT != FMX_LAYOUT_FTRL)  // (never FTRL here)
          rc = launch_online_mlp_pair_k<LPR, LAYOUT, RULE>(a, static_cast<hipStream_t>(stream));
      });
    });
    return rc;
  }
  return online_mlp_queued(table, hyper, rule, opt ? rule : -1, mlp, fm_term, idx, xv, N, 2, workspace, fwd, scratch, false, stream, who,
                           [&](MlpArgs &m, int i) {
                             m.pred_out = logit_out ? logit_out + (size_t)i * 2 : nullptr;
                             m.out = loss_out ? loss_out + i : nullptr;
                             m.pair_pred = pred_out + i;
                             mlp_pair_fit_args(m, hyper, rule, margin, 1.0f, opt, opt ? opt->step + i + 1 : 0);
                           });
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

#include "fmx_online_list.inc"
