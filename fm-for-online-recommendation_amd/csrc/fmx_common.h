// fmx_common.h -- what the translation units of libfmx.so share: the error plumbing and the tuning switches (one copy, defined
// in fmx_kernels.hip), and the device helpers every kernel file uses (per-unit copies in an anonymous namespace).  The host-side
// vocabulary of the units that take a table (checks, dispatchers, workspace) is fmx_host.h.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <mutex>

#include "fmx.h"

// No floating-point contraction: every kernel evaluates the expressions as written (one rounding per operation), so two
// kernels that state the same arithmetic -- k_fm_forward + k_fm_update at B = 1 and k_fm_online, the update with and
// without the in-launch hand-off, ... -- give the same bits whatever the surrounding code looks like.  The kernels are
// bound by memory round trips, not by VALU issue; fused multiply-adds are written explicitly where they are wanted.
#pragma clang fp contract(off)

// ------------------------------------------------------------------------------------------------------------
// host-side error plumbing
// ------------------------------------------------------------------------------------------------------------
namespace fmxd {  // defined in fmx_kernels.hip
extern thread_local char g_err[512];
int fail(int code, const char *fmt, ...);
int check_launch(const char *what);

// ---- launch geometry knobs (waves per workgroup), overridable from the environment for experiments ----
struct Tune {
  int wpb_fwd = 4, wpb_upd = 2;  // waves per workgroup (FMX_WPB_FWD / FMX_WPB_UPD: 1, 2 or 4).  The forward's first wave evaluates
                                 // the workgroup's loss epilogues together: 4 (19.85-19.89 us per loop step; 2: 20.24-20.46)
  int sort_e = 0;     // FMX_SORT_E: elements per thread of the bitonic sort (0 = default)
  int inline_fixup = 1;  // FMX_INLINE_FIXUP=0 / fmx_set_option("inline_fixup", 0): partial records are combined by a second
                         // launch (k_fm_fixup) instead of the in-launch hand-off; both give identical bits
  int upd_order = 1;  // FMX_UPD_ORDER / fmx_set_option("upd_order", v): the order in which k_fm_update's grid takes the sort fields.
                      // 0: index order; 1: ascending row count (the small fields' hand-off chains ahead of the large fields' row
                      // burst); 2: descending (the adversarial order, for tests).  Identical bits (fmx_host.h, upd_order_of)
  int online_persistent = 1;  // FMX_ONLINE_PERSISTENT=0 / fmx_set_option("online_persistent", 0): fmx_online_run_mlp as per-sample launches
  int afm_online_persistent = 1;  // fmx_set_option("afm_online_persistent", 0): fmx_afm_online_run as per-sample launches (same bits)
  int afm_pair_online_persistent = 1;  // fmx_set_option("afm_pair_online_persistent", 0): fmx_afm_pair_online_run as queued pair steps (same bits)
  int sort_ahead = 16;  // FMX_SORT_AHEAD: batches per side-stream sort launch in fmx_fm_stream (1..16)
  int sort_resident = -1;  // FMX_SORT_RESIDENT / fmx_set_option("sort_resident", v): most workgroups of a side-stream group sort of
                           // the online loop from the call's third group on (k_sort_occ_resident, at most one per CU); 0: one
                           // workgroup per (batch, field) as everywhere else; -1: the library's default for the device
                           // (sort_resident_cap, fmx_kernels.hip).  Identical lists
  int mlp_chain = 1;          // FMX_MLP_CHAIN=0 / fmx_set_option("mlp_chain", 0): fmx_mlp_section as separate GEMM launches
                              // (forward x L, loss, dgrad x L) instead of k_mlp_chain; same results up to summation order
  int sort_chunked = 1;  // FMX_SORT_CHUNKED / fmx_set_option("sort_chunked", v): 0: one workgroup per field (k_sort_occ) at
                         // every width; 1: k_sort_chunk + k_sort_merge from 8,192 composites per field on; 2: from 2,048 on.
                         // Identical lists either way
};
Tune &tune();

// Sort fields whose dispatch order k_fm_update carries BY VALUE in its kernel arguments, one byte each (UpdArgs::order).  A table
// with more sort fields is updated in index order.
constexpr int UPD_ORDER_MAX = 128;

// ---- the library's RCCL communicator for the field-owner step (fmx_comm.hip) ----
constexpr int FMX_COMM_SLOTS = 4;  // batches whose indices may be gathered + sorted ahead of their step
struct Comm {
  int rank = 0, world = 1, n_blocks = 1;
  bool force = false;            // issue the collectives even with one rank (tests: the RCCL calls of a step on a one-GPU box)
  int block_count[FMX_COMM_MAX_WORLD] = {0}, block_first[FMX_COMM_MAX_WORLD] = {0};  // tree blocks per rank (fmx/plan.py)
  void *main = nullptr, *pf = nullptr;  // ncclComm_t of the step's stream / of the prefetch stream; null: one rank, nothing to exchange
  hipStream_t pf_stream = nullptr;      // the prefetch stream (library-owned)
  hipEvent_t fork = nullptr, ready[FMX_COMM_SLOTS] = {nullptr}, free_[FMX_COMM_SLOTS] = {nullptr};
  bool used[FMX_COMM_SLOTS] = {false};  // free_[s] has been recorded at least once
};
int comm_all_gather(Comm *c, int which, const void *send, void *recv, size_t count, hipStream_t st);
int comm_exchange_blocks(Comm *c, const float *send, float *recv, size_t per, hipStream_t st);

// ---- the fixed-order reduction of the MLP's partial weight gradients (k_mlp_reduce, or carried by k_fm_update_rider) ----
constexpr int MLP_BIG_MAX_L = 8;
struct MlpReduceArgs {
  const float *parts[MLP_BIG_MAX_L];  // [n_split, out_l, ldp_l]
  int out_dim[MLP_BIG_MAX_L], in_dim[MLP_BIG_MAX_L], ldp[MLP_BIG_MAX_L];
  long long grad_off[MLP_BIG_MAX_L];  // offset of W_l in the flat buffer; b_l follows W_l
  float *grads;
  float *params;  // with lr != 0: params -= lr * grad in the same pass (single-rank SGD)
  float lr;
  // the network's rule (fmx_mlp_opt_t; mlp_reduce_set_opt): FMX_RULE_SGD as above, or FMX_RULE_ADAGRAD / FMX_RULE_ADAM on the flat
  // moments m, v (the layout of params), applied in the same pass whatever lr is.  Under them lr, eps, c1, c2 are what
  // moments_upd reads as h.lr, h.eps, h.beta1, h.beta2: the step's step size, eps (ADAM: eps sqrt(1 - beta2^t)), 1 - beta1, 1 - beta2
  int rule;
  float *m, *v;
  float eps, c1, c2;
  int n_split[MLP_BIG_MAX_L], n_layers;
  const float *loss_b;
  float *loss_out;
  int B;
  float inv_b;
};
// fmx_mlp_section without its last launch: `deferred` receives the arguments of the reduction instead, for a caller that carries
// its blocks in another launch of the same stream (fmx_deepfm_stream: inside the table update's) or launches it itself
// (mlp_launch_reduce).  Defined in fmx_mlp.hip.
// pair_margin >= 0: the pair mode (fmx_mlp_pair_section, fmx_deepfm_pair_stream) -- the B rows are B / 2 pairs, row 2 i the positive
// and row 2 i + 1 the negative, the loss is pair_loss_dz of their logits' difference under that margin; y and loss_kind are not read.
int mlp_section_deferred_reduce(const fmx_mlp_t *mlp, int32_t loss_kind, const float *bi, int32_t ld_bi, const float *base, const float *y, int32_t B,
                                float inv_b, void *workspace, float *logit_out, float *dz_out, float *gbi_out, int32_t ld_gbi, float *grads,
                                float lr_apply, float *loss_out, hipStream_t st, MlpReduceArgs *deferred, const char *who = "fmx_mlp_section",
                                float pair_margin = -1.f);
void mlp_launch_reduce(const MlpReduceArgs &a, hipStream_t st);
// the host-side checks of fmx_mlp_section_opt / fmx_deepfm_stream_opt on the network, its buffers and its optimizer state for a
// call of n_steps steps; `who` names the entry point in the message.  Defined in fmx_mlp.hip.
int mlp_opt_check(const fmx_mlp_t *mlp, int32_t B, const void *workspace, int64_t workspace_bytes, const float *grads, const fmx_mlp_opt_t *opt,
                  int64_t n_steps, const char *who);
// ... its checks of a non-null opt alone (rule, m / v given, betas, step count), shared with the one-workgroup kernel's _opt calls
int mlp_opt_state_check(const fmx_mlp_opt_t *opt, int64_t n_steps, const char *who);
int mlp_reduce_blocks_per_layer(const MlpReduceArgs &a, int threads);
}  // namespace fmxd
using namespace fmxd;

namespace {

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

constexpr uint32_t SENT = 0xFFFFFFFFu;
constexpr int WAVE = 64;
constexpr int LIST_MAX_G = 16;  // rows per list of the listwise losses, every model family (k_fm_forward_list: one wave per row of a workgroup)
constexpr int MAX_SORT_WIDTH = 32768;  // 128 KiB of the 160 KiB LDS
constexpr int SORT_CHUNK = 1024;       // composites per chunk of the chunked sort (fmx_sort.inc); the workspace holds its runs from 2 chunks on

// ------------------------------------------------------------------------------------------------------------
// device helpers
// ------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ float4 operator+(float4 a, float4 b) { return {a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w}; }
__device__ __forceinline__ float4 operator-(float4 a, float4 b) { return {a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w}; }
__device__ __forceinline__ float4 operator*(float4 a, float4 b) { return {a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w}; }
__device__ __forceinline__ float4 operator*(float a, float4 b) { return {a * b.x, a * b.y, a * b.z, a * b.w}; }
__device__ __forceinline__ float4 splat(float a) { return {a, a, a, a}; }

__device__ __forceinline__ float4 shfl_xor4(float4 v, int m) {
  return {__shfl_xor(v.x, m), __shfl_xor(v.y, m), __shfl_xor(v.z, m), __shfl_xor(v.w, m)};
}
__device__ __forceinline__ float4 shfl_up4(float4 v, int d) {
  return {__shfl_up(v.x, d), __shfl_up(v.y, d), __shfl_up(v.z, d), __shfl_up(v.w, d)};
}
__device__ __forceinline__ float4 shfl4(float4 v, int src) {
  return {__shfl(v.x, src), __shfl(v.y, src), __shfl(v.z, src), __shfl(v.w, src)};
}

// v_rcp_f32 / v_sqrt_f32 are 1-ulp instructions; the IEEE-exact expansions hipcc emits for `/` and sqrtf cost 10-14
// VALU instructions each and made the FTRL kernels VALU-bound (profiles/r01_*).  1 ulp is ~1e-7 relative, two orders
// below the 1e-5 parity tolerance.
__device__ __forceinline__ float rcp_(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float sqrt_(float x) { return __builtin_amdgcn_sqrtf(x); }

// FTRL-proximal weight from (z, n)  (McMahan et al. 2013, Algorithm 1); h.alpha holds 1/alpha on the device
__device__ __forceinline__ float ftrl_w(float z, float n, const fmx_hyper_t &h) {
  const float denom = fmaf(h.beta + sqrt_(n), h.alpha, h.l2);
  const float w = -(z - copysignf(h.l1, z)) * rcp_(denom);
  return fabsf(z) <= h.l1 ? 0.f : w;
}
__device__ __forceinline__ float4 ftrl_w4(float4 z, float4 n, const fmx_hyper_t &h) {
  return {ftrl_w(z.x, n.x, h), ftrl_w(z.y, n.y, h), ftrl_w(z.z, n.z, h), ftrl_w(z.w, n.w, h)};
}
// one FTRL-proximal update of (z, n) by gradient g; w is the weight derived from the OLD (z, n)
__device__ __forceinline__ void ftrl_upd(float &z, float &n, float w, float g, const fmx_hyper_t &h) {
  const float n2 = fmaf(g, g, n);
  const float sigma = (sqrt_(n2) - sqrt_(n)) * h.alpha;
  z = fmaf(-sigma, w, z + g);
  n = n2;
}

template <int RULE>
__device__ __forceinline__ float apply_rule(float p, float g, const fmx_hyper_t &h) {
  if (RULE == FMX_RULE_SIGNADAM) return p - h.lr * g * rcp_(fabsf(g) + h.eps);
  return p - h.lr * g;  // FMX_RULE_SGD
}
template <int RULE>
__device__ __forceinline__ float4 apply_rule4(float4 p, float4 g, const fmx_hyper_t &h) {
  return {apply_rule<RULE>(p.x, g.x, h), apply_rule<RULE>(p.y, g.y, h), apply_rule<RULE>(p.z, g.z, h),
          apply_rule<RULE>(p.w, g.w, h)};
}

// ---- the persistent adaptive rules (FMX_LAYOUT_MOMENTS).  On the device h.lr holds the step's step size (ADAM: lr sqrt(1 -
//      beta2^t) / (1 - beta1^t), ADAGRAD: lr), h.beta1 / h.beta2 hold 1 - beta1 / 1 - beta2: adam_consts, in double, once per
//      step on the host (k_fm_online: once per sample on the device, with the same function and the same bits) ----
// b^t by squaring: the same multiplications in the same order on the host and on the device
__host__ __device__ inline double pow_step(double b, int32_t t) {
  double r = 1.0, p = b;
  for (uint32_t e = (uint32_t)t; e; e >>= 1) {
    if (e & 1u) r = r * p;
    p = p * p;
  }
  return r;
}
// the device-side constants of ADAM's step t (1-based) from the caller's hyper-parameters; eps_dense, when asked for, receives
// eps sqrt(1 - beta2^t): what stands in eps' place when torch.optim.Adam's denominator sqrt(v) / sqrt(1 - beta2^t) + eps is
// multiplied through by sqrt(1 - beta2^t) (the network's rule, fmx_mlp_opt_t)
__host__ __device__ inline void adam_consts(float lr, float beta1, float beta2, int32_t t, float &step_size, float &c1, float &c2,
                                            float eps = 0.f, float *eps_dense = nullptr) {
  const double b1 = beta1, b2 = beta2;
  const double s2 = sqrt(1.0 - pow_step(b2, t));
  step_size = (float)((double)lr * s2 / (1.0 - pow_step(b1, t)));
  c1 = (float)(1.0 - b1);
  c2 = (float)(1.0 - b2);
  if (eps_dense) *eps_dense = (float)((double)eps * s2);
}
// one coordinate: p, m, v by gradient g (h as above)
template <int RULE>
__device__ __forceinline__ void moments_upd(float &p, float &m, float &v, float g, const fmx_hyper_t &h) {
  if (RULE == FMX_RULE_ADAM) {
    m = m + h.beta1 * (g - m);
    v = v + h.beta2 * (g * g - v);
    p = p - h.lr * (m * rcp_(sqrt_(v) + h.eps));
  } else {  // FMX_RULE_ADAGRAD: G in the v slot
    v = v + g * g;
    p = p - h.lr * (g * rcp_(sqrt_(v) + h.eps));
  }
}
template <int RULE>
__device__ __forceinline__ void moments_upd4(float4 &p, float4 &m, float4 &v, float4 g, const fmx_hyper_t &h) {
  moments_upd<RULE>(p.x, m.x, v.x, g.x, h);
  moments_upd<RULE>(p.y, m.y, v.y, g.y, h);
  moments_upd<RULE>(p.z, m.z, v.z, g.z, h);
  moments_upd<RULE>(p.w, m.w, v.w, g.w, h);
}

// ---- the table's bias, held as the words (b0, b1, b2) of fmx_table_t.bias: WEIGHTS (b, -, -), FTRL (z, n, -), MOMENTS (b, m, v) ----
// the bias weight the logit adds
template <int LAYOUT>
__device__ __forceinline__ float bias_weight(float b0, float b1, const fmx_hyper_t &h) {
  return LAYOUT == FMX_LAYOUT_FTRL ? ftrl_w(b0, b1, h) : b0;
}
// one step of the rule by the bias gradient g
template <int LAYOUT, int RULE>
__device__ __forceinline__ void bias_step(float &b0, float &b1, float &b2, float g, const fmx_hyper_t &h) {
  if (LAYOUT == FMX_LAYOUT_WEIGHTS) {
    b0 = apply_rule<RULE>(b0, g, h);
  } else if (LAYOUT == FMX_LAYOUT_MOMENTS) {
    moments_upd<RULE>(b0, b1, b2, g, h);
  } else {
    const float w = ftrl_w(b0, b1, h);
    ftrl_upd(b0, b1, w, g, h);
  }
}

__device__ __forceinline__ float sigmoidf_(float z) { return 1.f / (1.f + expf(-z)); }
// F.binary_cross_entropy_with_logits per element
__device__ __forceinline__ float bcewl(float z, float y) {
  return (1.f - y) * z + log1pf(expf(-fabsf(z))) + fmaxf(-z, 0.f);
}
// the loss of logit z against label y and its gradient d loss / d z scaled by inv_b (1 / batch): FMX_LOSS_BCE_LOGITS, or
// FMX_LOSS_BCE_SIGMOID (the reference's BCEWithLogits applied to sigmoid(z))
__device__ __forceinline__ void bce_loss_dz(int loss_kind, float z, float y, float inv_b, float &loss, float &dz) {
  if (loss_kind == FMX_LOSS_BCE_LOGITS) {
    loss = bcewl(z, y);
    dz = (sigmoidf_(z) - y) * inv_b;
  } else {
    const float p = sigmoidf_(z);
    loss = bcewl(p, y);
    dz = (sigmoidf_(p) - y) * p * (1.f - p) * inv_b;
  }
}

// The pairwise-ranking loss of a logit difference d = z_pos - z_neg: loss = -log(sigmoid(d) + margin), margin >= 0, and its
// gradient d loss / d d = -sigmoid(d) sigmoid(-d) / (sigmoid(d) + margin), scaled by inv_b.  margin == 0 (BPR) in the stable
// softplus form, where the gradient is -sigmoid(-d); sigmoid(-d) is evaluated as such, not as 1 - sigmoid(d), which loses its
// digits once d is large.  Finite for every finite d.
__device__ __forceinline__ void pair_loss_dz(float d, float margin, float inv_b, float &loss, float &dz) {
  const float sn = 1.f / (1.f + expf(d));  // sigmoid(-d)
  float g;
  if (margin == 0.f) {
    loss = log1pf(expf(-fabsf(d))) + fmaxf(-d, 0.f);
    g = -sn;
  } else {
    const float sp = sigmoidf_(d);
    loss = -logf(sp + margin);
    g = -(sp * sn) / (sp + margin);
  }
  dz = g * inv_b;
}

// The listwise (sampled-softmax) loss of a list of G logits held on G consecutive lanes of a wave, the positive's first:
// lane `lane` holds z of position lane % G, every lane of the list is active.  With m = max_j z_j, e_j = exp(z_j - m) and
// s = e_0 + e_1 + ... + e_{G-1} added in that order: loss = log(s) - (z_0 - m) (softmax cross-entropy against position 0),
// dz_j = e_j / s inv_b for a negative and dz_0 = -((e_1 + ... + e_{G-1}) / s) inv_b -- the negatives' mass itself, not 1 - p_0,
// which loses its digits as p_0 -> 1 (as pair_loss_dz evaluates sigmoid(-d)).  Every lane of the list walks the G logits by
// lane reads in the order j = 0 .. G-1 and evaluates the same operands in the same order, so the result depends on the logits
// and G alone.  exp's argument is <= 0 and s >= 1: finite for finite logits.  `loss` is the list's on every lane.
__device__ __forceinline__ void list_loss_dz(float z, int lane, int G, float inv_b, float &loss, float &dz) {
  const int pos = lane % G, first = lane - pos;
  const float z0 = __shfl(z, first);
  float m = z0;
  for (int j = 1; j < G; ++j) m = fmaxf(m, __shfl(z, first + j));
  float s = expf(z0 - m), neg = 0.f;  // neg: e_1 + ... + e_{G-1}, in that order
  for (int j = 1; j < G; ++j) {
    const float e = expf(__shfl(z, first + j) - m);
    s += e;
    neg += e;
  }
  loss = logf(s) - (z0 - m);
  dz = pos == 0 ? -(neg / s) * inv_b : (expf(z - m) / s) * inv_b;
}
// ... and the same formula over zj(j) = the logit of position j read from anywhere (k_fm_list_online, fmx_list_online.hip: from
// LDS), for the caller at position `pos` whose own logit is z: the operands and the order above, so the same bits.  (The lines are
// repeated: with list_loss_dz routed through this function -- a lambda by reference or by value, a functor struct, a stateless
// reader, z_0 handed in -- 16 of k_fm_forward_list's 50 instantiations came out with another schedule, and their code is to stay what
// it was, tools/isa_diff.py; as with k_fm_forward_list's own six lines.)
template <class ReadLogit>
__device__ __forceinline__ void list_loss_dz_of(ReadLogit zj, float z, int pos, int G, float inv_b, float &loss, float &dz) {
  const float z0 = zj(0);
  float m = z0;
  for (int j = 1; j < G; ++j) m = fmaxf(m, zj(j));
  float s = expf(z0 - m), neg = 0.f;  // neg: e_1 + ... + e_{G-1}, in that order
  for (int j = 1; j < G; ++j) {
    const float e = expf(zj(j) - m);
    s += e;
    neg += e;
  }
  loss = logf(s) - (z0 - m);
  dz = pos == 0 ? -(neg / s) * inv_b : (expf(z - m) / s) * inv_b;
}

// lane ^ M exchanges without the LDS crossbar (ds_bpermute made the sort LDS-pipe bound): DPP for M = 1, 2, 4, 8,
// v_permlane16/32_swap for M = 16, 32.
template <int M>
__device__ __forceinline__ uint32_t xor_lane(uint32_t v, int lane) {
  if constexpr (M == 1) {
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, true);  // quad_perm [1,0,3,2]
  } else if constexpr (M == 2) {
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, true);  // quad_perm [2,3,0,1]
  } else if constexpr (M == 4) {
    const int t = __builtin_amdgcn_mov_dpp((int)v, 0x141, 0xF, 0xF, true);     // row_half_mirror: i -> 7 - i
    return (uint32_t)__builtin_amdgcn_mov_dpp(t, 0x1B, 0xF, 0xF, true);         // quad_perm [3,2,1,0]: together i ^ 4
  } else if constexpr (M == 8) {
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x128, 0xF, 0xF, true);  // row_ror:8
  } else if constexpr (M == 16) {
    const auto sw = __builtin_amdgcn_permlane16_swap(v, v, false, false);  // {[r0,r0,r2,r2], [r1,r1,r3,r3]}
    return (lane & 16) ? sw[0] : sw[1];
  } else {
    const auto sw = __builtin_amdgcn_permlane32_swap(v, v, false, false);  // {[lo,lo], [hi,hi]}
    return (lane & 32) ? sw[0] : sw[1];
  }
}

template <int M>
__device__ __forceinline__ float xor_lane_f(float v, int lane) {
  return __uint_as_float(xor_lane<M>(__float_as_uint(v), lane));
}
template <int M>
__device__ __forceinline__ float4 xor_lane_f4(float4 v, int lane) {
  return {xor_lane_f<M>(v.x, lane), xor_lane_f<M>(v.y, lane), xor_lane_f<M>(v.z, lane), xor_lane_f<M>(v.w, lane)};
}

// ---- the FM's per-sample sums: lane group `slot` (LPR lanes, lane q owns coordinates 4q..4q+3) holds the partial sums s, ss, fo
//      of e = x V, e * e and x w over ITS fields ----
template <int M, int LPR>
__device__ __forceinline__ void fm_sums_level(float4 &s, float4 &ss, float &fo, int lane, int groups) {
  if (LPR <= M && M / LPR < groups) {
    s = s + xor_lane_f4<M>(s, lane);
    ss = ss + xor_lane_f4<M>(ss, lane);
    fo += xor_lane_f<M>(fo, lane);
  }
}
// the field sums: a butterfly over the lane groups (lanes with equal q; slot ^ 1, ^ 2, ^ 4, ...), DPP / permlane exchanges (no LDS
// crossbar).  `groups` (a power of two) stops it inside runs of that many lane groups (k_fm_forward_part: an owner's block); by
// default every lane group of the wave ends with the sums of all of them.
template <int LPR>
__device__ __forceinline__ void fm_field_sums(float4 &s, float4 &ss, float &fo, int lane, int groups = WAVE) {
  fm_sums_level<1, LPR>(s, ss, fo, lane, groups);
  fm_sums_level<2, LPR>(s, ss, fo, lane, groups);
  fm_sums_level<4, LPR>(s, ss, fo, lane, groups);
  fm_sums_level<8, LPR>(s, ss, fo, lane, groups);
  fm_sums_level<16, LPR>(s, ss, fo, lane, groups);
  fm_sums_level<32, LPR>(s, ss, fo, lane, groups);
}
// the bi-interaction vector from the field sums, and its sum over the LPR lanes of a group (every lane of the group gets it)
template <int LPR>
__device__ __forceinline__ float4 fm_bi(float4 s, float4 ss, float &sbi) {
  const float4 bi = 0.5f * (s * s - ss);
  sbi = (bi.x + bi.y) + (bi.z + bi.w);
#pragma unroll
  for (int m = 1; m < LPR; m <<= 1) sbi += __shfl_xor(sbi, m);
  return bi;
}
// ... with the exchanges of the LPR lanes by DPP instead of the LDS crossbar: the same operands added in the same order, the
// same bits (k_fm_forward; the other kernels keep the form above)
template <int LPR>
__device__ __forceinline__ float4 fm_bi_dpp(float4 s, float4 ss, float &sbi) {
  const float4 bi = 0.5f * (s * s - ss);
  sbi = (bi.x + bi.y) + (bi.z + bi.w);
  if (LPR > 1) sbi += xor_lane_f<1>(sbi, 0);
  if (LPR > 2) sbi += xor_lane_f<2>(sbi, 0);
  if (LPR > 4) sbi += xor_lane_f<4>(sbi, 0);
  if (LPR > 8) sbi += xor_lane_f<8>(sbi, 0);
  return bi;
}

// deterministic block reduction of src[0..n): every thread sums a strided set of elements (16-byte groups when dense),
// 16 independent loads in flight per round -- at B = 16,384 with 128 threads a 4-deep unroll left 32 dependent rounds of
// HBM latency per sum and the one workgroup that owns the bias became the longest path of the launch -- then an LDS tree.
// The order of the additions depends only on (n, ld == 1, min(blockDim, 128)): at most 128 threads take part, so that
// workgroups of any width give identical bits.
__device__ float block_sum(const float *src, int n, int ld, float *sm) {
  constexpr int U = 16;
  const int tid = threadIdx.x, nt = blockDim.x < 128 ? blockDim.x : 128;
  float acc = 0.f;
  if (tid >= nt) {  // bystanders of a wider workgroup: only the barriers
    __syncthreads();
    for (int w = nt >> 1; w > 0; w >>= 1) __syncthreads();
    const float r = sm[0];
    __syncthreads();
    return r;
  }
  if (ld == 1) {
    const int n4 = n >> 2;
    const float4 *src4 = reinterpret_cast<const float4 *>(src);
    for (int i0 = tid; i0 < n4; i0 += U * nt) {
      float4 v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {  // branch-free: a group beyond the end reads group 0 and counts as zeros (a branch per
        const int i = i0 + u * nt;   // load made the compiler wait for every load before it issued the next)
        v[u] = src4[i < n4 ? i : 0];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool in = i0 + u * nt < n4;
        acc += in ? (v[u].x + v[u].y) + (v[u].z + v[u].w) : 0.f;
      }
    }
    for (int i = (n4 << 2) + tid; i < n; i += nt) acc += src[i];
  } else {  // strided sample records: the SAME order of additions as the dense form (groups of four elements, then the
            // tail), so a step over gathered records and a step over dense arrays give identical bits
    constexpr int V = 4;
    const int n4 = n >> 2;
    for (int i0 = tid; i0 < n4; i0 += V * nt) {
      float4 v[V];
#pragma unroll
      for (int u = 0; u < V; ++u) {
        const int i = i0 + u * nt;
        const float *p = src + (size_t)(4 * (i < n4 ? i : 0)) * ld;
        v[u] = float4{p[0], p[ld], p[2 * (size_t)ld], p[3 * (size_t)ld]};
      }
#pragma unroll
      for (int u = 0; u < V; ++u) {
        const bool in = i0 + u * nt < n4;
        acc += in ? (v[u].x + v[u].y) + (v[u].z + v[u].w) : 0.f;
      }
    }
    for (int i = (n4 << 2) + tid; i < n; i += nt) acc += src[(size_t)i * ld];
  }
  sm[tid] = acc;
  __syncthreads();
  for (int w = nt >> 1; w > 0; w >>= 1) {
    if (tid < w) sm[tid] += sm[tid + w];
    __syncthreads();
  }
  const float r = sm[0];
  __syncthreads();
  return r;
}

// ---- the table rows as the kernels hold and update them (k_fm_update, k_fm_online, k_online_mlp, k_afm_online) ----
// Agent-scope relaxed atomic loads compile to `global_load ... sc1` (L1-bypassing): a row another wave stored earlier in the
// same launch is read as stored
__device__ __forceinline__ float ld_sc1(const float *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float4 ld_sc1_4(const float *p) { return {ld_sc1(p), ld_sc1(p + 1), ld_sc1(p + 2), ld_sc1(p + 3)}; }

// Row stores are nontemporal: the lines go out while the launch runs instead of staying dirty in L2 for the write-back at its end
// (same-box A/B of the online loop, tools/ab_old_new.sh: 21.51 / 21.60 against 21.90 / 21.83 us per step).
__device__ __forceinline__ void st16(float *p, float4 v) {
  typedef float f4v __attribute__((ext_vector_type(4)));
  __builtin_nontemporal_store(f4v{v.x, v.y, v.z, v.w}, reinterpret_cast<f4v *>(p));
}
__device__ __forceinline__ void st4(float *p, float v) { __builtin_nontemporal_store(v, p); }

// The state of one row as LPR lanes hold it: lane q owns coordinates 4q..4q+3; lane 0 also the first-order part.
//   WEIGHTS row  [ V(kp) | w | pad ]
//   FTRL row     [ V(kp) | w, zw, nw, pad | ... | zV(kp) | nV(kp) ]   zV starts at float `zoff`;
//                V and w are the weights derived from (z, n), re-derived and stored by every update
//   MOMENTS row  [ V(kp) | w, mw, vw, pad | ... | mV(kp) | vV(kp) ]   the FTRL geometry; V and w are the parameters
//                (ADAGRAD neither loads nor stores the m slots: z stays zero in the registers)
struct RowRegs {
  float4 v;       // V
  float4 z, n;    // FTRL: (z, n); MOMENTS: (m, v)
  float4 fo;      // lane 0: (w, zw, nw, -) / (w, mw, vw, -)
};

template <int LAYOUT, int RULE>
__device__ __forceinline__ RowRegs load_row(const float *rp, int q, int kp, int zoff) {
  RowRegs r;
  r.v = *reinterpret_cast<const float4 *>(rp + 4 * q);
  r.z = splat(0.f);
  r.n = splat(0.f);
  r.fo = splat(0.f);
  // the first-order part is used by lane 0 of the group only, but every lane requests it (same address: one request): a
  // load under `if (q == 0)` is a branch, and the compiler's wait counts fall back to vmcnt(0) around it
  if (LAYOUT == FMX_LAYOUT_WEIGHTS) {
    r.fo.x = rp[kp];
  } else {
    if (LAYOUT == FMX_LAYOUT_FTRL || RULE == FMX_RULE_ADAM) r.z = *reinterpret_cast<const float4 *>(rp + zoff + 4 * q);
    r.n = *reinterpret_cast<const float4 *>(rp + zoff + kp + 4 * q);
    r.fo = *reinterpret_cast<const float4 *>(rp + kp);
  }
  return r;
}

// gradient of the row from the run sums (dV = cV - V * cA, dw = cw), one application of the rule, store
template <int LAYOUT, int RULE>
__device__ __forceinline__ void update_row(float *rp, int q, int kp, int zoff, RowRegs r, float4 cV, float4 cA, float cw,
                                           const fmx_hyper_t &h) {
  // two roundings on purpose (no fma): where a sample is the row's only contribution to S (x = 1), cV = dz * V and
  // V * cA = V * dz round alike and the gradient is exactly 0, as in the reference's dz * x * (S - e)
  const float4 gr = cV - r.v * cA;
  if (LAYOUT == FMX_LAYOUT_WEIGHTS) {
    st16(rp + 4 * q, apply_rule4<RULE>(r.v, gr, h));
    if (q == 0) st4(rp + kp, apply_rule<RULE>(r.fo.x, cw, h));
  } else if (LAYOUT == FMX_LAYOUT_MOMENTS) {
    float4 p4 = r.v, m4 = r.z, v4 = r.n;
    moments_upd4<RULE>(p4, m4, v4, gr, h);
    // the (m, v) half is read by nobody but the next update of this row (a later launch): plain stores
    if (RULE == FMX_RULE_ADAM) *reinterpret_cast<float4 *>(rp + zoff + 4 * q) = m4;
    *reinterpret_cast<float4 *>(rp + zoff + kp + 4 * q) = v4;
    st16(rp + 4 * q, p4);
    if (q == 0) {
      float4 fo = r.fo;
      moments_upd<RULE>(fo.x, fo.y, fo.z, cw, h);
      st16(rp + kp, fo);
    }
  } else {
    float4 z4 = r.z, n4 = r.n;
    ftrl_upd(z4.x, n4.x, r.v.x, gr.x, h);
    ftrl_upd(z4.y, n4.y, r.v.y, gr.y, h);
    ftrl_upd(z4.z, n4.z, r.v.z, gr.z, h);
    ftrl_upd(z4.w, n4.w, r.v.w, gr.w, h);
    // the (z, n) half is read by nobody but the next update of this row (a later launch): plain stores
    *reinterpret_cast<float4 *>(rp + zoff + 4 * q) = z4;
    *reinterpret_cast<float4 *>(rp + zoff + kp + 4 * q) = n4;
    st16(rp + 4 * q, ftrl_w4(z4, n4, h));
    if (q == 0) {
      float4 fo = r.fo;
      ftrl_upd(fo.y, fo.z, fo.x, cw, h);
      fo.x = ftrl_w(fo.y, fo.z, h);
      st16(rp + kp, fo);
    }
  }
}

// ... with every load sc1: the row may have been written earlier in this launch (the online kernels)
template <int LAYOUT, int RULE>
__device__ __forceinline__ RowRegs load_row_sc1(const float *rp, int q, int kp, int zoff) {
  RowRegs r;
  r.v = ld_sc1_4(rp + 4 * q);
  r.z = splat(0.f);
  r.n = splat(0.f);
  r.fo = splat(0.f);
  if (LAYOUT == FMX_LAYOUT_WEIGHTS) {  // (every lane, as in load_row: no branch around a load)
    r.fo.x = ld_sc1(rp + kp);
  } else {
    if (LAYOUT == FMX_LAYOUT_FTRL || RULE == FMX_RULE_ADAM) r.z = ld_sc1_4(rp + zoff + 4 * q);
    r.n = ld_sc1_4(rp + zoff + kp + 4 * q);
    r.fo = ld_sc1_4(rp + kp);
  }
  return r;
}

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// the network's rule for its step t (1-based) into the reduction's arguments: ADAM's constants in double, once per step
inline void mlp_reduce_set_opt(MlpReduceArgs &a, const fmx_mlp_opt_t &o, int32_t t) {
  a.rule = o.rule;
  a.m = o.m;
  a.v = o.v;
  a.lr = o.lr;
  a.eps = o.eps;
  a.c1 = a.c2 = 0.f;
  if (o.rule == FMX_RULE_ADAM) adam_consts(o.lr, o.beta1, o.beta2, t, a.lr, a.c1, a.c2, o.eps, &a.eps);
}

// Block `block` of `n_blocks` of layer l: one thread per 4 consecutive columns of one row of the layer's partial [out, ldp] (ldp a
// multiple of 4: the weight columns, the bias column `in`, padding): 16-byte loads of up to 16 splits in flight, summed in the
// order z = 0, 1, ...; block 0 of layer 0 also reduces the loss.  Any workgroup width (the table update's is 64 or 128 or 256).
// The thread that sums a group also applies the network's rule to it (MlpReduceArgs.rule) and stores params (and m, v).
__device__ __forceinline__ void mlp_reduce_block(const MlpReduceArgs &a, int l, int block, int n_blocks) {
  const int out = a.out_dim[l], in = a.in_dim[l], ldp = a.ldp[l], ns = a.n_split[l];
  const int groups = ldp >> 2;
  const long long n = (long long)out * groups;
  const float *p = a.parts[l];
  const size_t zs = (size_t)out * ldp;
  // the network's rule: a wave-uniform run-time branch (a template parameter would multiply the rider's instantiations)
  const bool adaptive = a.rule != FMX_RULE_SGD, apply = adaptive || a.lr != 0.f;
  fmx_hyper_t h;
  h.lr = a.lr;
  h.eps = a.eps;
  h.beta1 = a.c1;
  h.beta2 = a.c2;
  for (long long i = (long long)block * blockDim.x + threadIdx.x; i < n; i += (long long)n_blocks * blockDim.x) {
    const int m = (int)(i / groups), c = (int)(i - (long long)m * groups) * 4;
    const float *q = p + (size_t)m * ldp + c;
    // the parameters this thread updates, requested with the partials instead of behind their sum (a dependent round trip less);
    // a group of four weight columns is 16 contiguous, 16-byte aligned bytes of W_l when in % 4 == 0 (else the scalar path below)
    const bool vec4 = apply && c + 3 < in && (in & 3) == 0 && (a.grad_off[l] & 3) == 0;
    float4 pv = {0.f, 0.f, 0.f, 0.f}, mv = pv, vv = pv;
    if (vec4) {
      const long long o = a.grad_off[l] + (long long)m * in + c;
      pv = *reinterpret_cast<const float4 *>(a.params + o);
      if (adaptive) vv = *reinterpret_cast<const float4 *>(a.v + o);
      if (a.rule == FMX_RULE_ADAM) mv = *reinterpret_cast<const float4 *>(a.m + o);
    }
    float4 s = {0.f, 0.f, 0.f, 0.f};
    for (int z0 = 0; z0 < ns; z0 += 16) {
      float4 r[16];
#pragma unroll
      for (int z = 0; z < 16; ++z)
        if (z0 + z < ns) r[z] = *reinterpret_cast<const float4 *>(q + (size_t)(z0 + z) * zs);
#pragma unroll
      for (int z = 0; z < 16; ++z)
        if (z0 + z < ns) {
          s.x += r[z].x;
          s.y += r[z].y;
          s.z += r[z].z;
          s.w += r[z].w;
        }
    }
    if (vec4) {
      const long long o = a.grad_off[l] + (long long)m * in + c;
      *reinterpret_cast<float4 *>(a.grads + o) = s;
      if (a.rule == FMX_RULE_ADAM) {
        moments_upd4<FMX_RULE_ADAM>(pv, mv, vv, s, h);
        *reinterpret_cast<float4 *>(a.m + o) = mv;
        *reinterpret_cast<float4 *>(a.v + o) = vv;
      } else if (adaptive) {
        moments_upd4<FMX_RULE_ADAGRAD>(pv, mv, vv, s, h);
        *reinterpret_cast<float4 *>(a.v + o) = vv;
      } else {
        pv = float4{pv.x - a.lr * s.x, pv.y - a.lr * s.y, pv.z - a.lr * s.z, pv.w - a.lr * s.w};
      }
      *reinterpret_cast<float4 *>(a.params + o) = pv;
      continue;
    }
    const float v[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (c + j > in) break;  // padding
      const long long o = c + j < in ? a.grad_off[l] + (long long)m * in + c + j : a.grad_off[l] + (long long)out * in + m;
      a.grads[o] = v[j];
      if (!apply) continue;
      if (!adaptive) {
        a.params[o] -= a.lr * v[j];
      } else if (a.rule == FMX_RULE_ADAM) {
        moments_upd<FMX_RULE_ADAM>(a.params[o], a.m[o], a.v[o], v[j], h);
      } else {
        float unused = 0.f;
        moments_upd<FMX_RULE_ADAGRAD>(a.params[o], unused, a.v[o], v[j], h);
      }
    }
  }
  if (block == 0 && l == 0 && a.loss_out) {
    __shared__ float sm[256];
    const float ls = block_sum(a.loss_b, a.B, 1, sm);
    if (threadIdx.x == 0) a.loss_out[0] = ls * a.inv_b;
  }
}

}  // namespace
