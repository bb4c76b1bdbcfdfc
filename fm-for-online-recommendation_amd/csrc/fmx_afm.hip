// fmx_afm.hip -- gfx950 kernels of the attentional factorization machine (AFM; Xiao et al. 2017) and its C ABI.  The device code is
// fmx_afm_device.inc (shared with fmx_afm_pair_online.hip); the host side and the C ABI follow it here.
//
// The model (include/fmx.h, DESIGN.md section 3 "AFM"): per sample, e_f = x_f V[row_f], the P = F (F - 1) / 2 pairs in the fixed
// order i = 0 .. F-2, j = i+1 .. F-1, q_ij = e_i (.) e_j, s_ij = h . relu(W q_ij + b), a = softmax(s), and
//     logit = bias + sum_f w_f x_f + p . sum_ij a_ij q_ij.
//
//   k_afm<KP, FTRL, BWD>  one wavefront per workgroup; a workgroup walks the samples blockIdx.x, blockIdx.x + gridDim.x, ...
//                         The sample's F x kp embeddings go to LDS once (lane f gathers field f's row).  The pairs are cut into
//                         TILES of whole pair rows i (at most 64 pairs: one per lane); each lane evaluates its pair's W q + b,
//                         relu, h and p products from LDS (the attention parameters sit in LDS for the whole launch) and leaves
//                         (s, p . q) in LDS.  The softmax then runs over the sample's P scores in LDS: max, exp, sums.
//                         BWD (the training step) walks the tiles again: every lane recomputes its pair's terms and leaves
//                         dL/dq, q and the per-unit coefficients of the tile in LDS; the lanes then add the tile into
//                         accumulators they OWN -- dW / db / dh / dp entries, and the (field, coordinate) entries of dL/de --
//                         in pair order.  dL/dV_row = x dL/de goes to E [B, F, kp]; the attention accumulators leave the
//                         launch as one partial per workgroup.
//   k_afm_reduce          the partials of the workgroups summed in workgroup order into [ dW | db | dh | dp ].
//   k_afm_reduce_opt<RULE> the same sums (afm_reduce_column); the thread that finishes column g also applies the attention
//                         parameters' rule to (params[g], m[g], v[g]) and stores them (fmx_afm_step_opt, fmx_afm_stream).
//
//   k_afm_online<KP>      one workgroup of 8 waves walks a stream one sample at a time (fmx_afm_online_run): k_afm's sample spread over
//                         the waves, the table update and the attention rule in the same launch; the bits of B = 1 steps.  It is
//                         afm_walk<KP, 1> of fmx_afm_device.inc (the comment in front of the online section there).
//
//   k_afm_pair_online<KP> (fmx_afm_pair_online.hip, a unit of its own) k_afm_online for pairs, afm_walk<KP, 2>: one workgroup walks a stream of
//                         (positive, negative) pairs (fmx_afm_pair_online_run); the bits of B_pairs = 1 pair steps.
//
//   k_afm_pair<KP, FTRL, BWD>  (fmx_afm_pair.inc) pairwise-ranking training: a workgroup walks PAIRS of rows (positive, negative) and
//                         runs k_afm's row forward and backward under the pair loss of the two logits (fmx_afm_pair_*).
//
//   k_afm_list<KP, FTRL, BWD>  (fmx_afm_list.inc) listwise training: a workgroup walks LISTS of G rows (a positive, G - 1 negatives) and
//                         runs the same row forward and backward under the softmax loss of the G logits (fmx_afm_list_*).
//
// The host side defines once what the three objectives (BCE on y, pairs, lists) share: afm_step_launches, one step's launches under
// an AfmObjective (the kind, the rows per unit, the margin); afm_steps_run, the ONE queue of steps behind every stream and every
// queued online run; check_afm_unit_steps, the step check of the objectives that read no labels.  The two online walkers share
// launch_afm_walk_k and the form decision afm_online_form (fmx_afm_device.inc), each under its own option.  Every launcher raises its
// kernel's dynamic-LDS limit through raise_lds_limit (fmx_host.h).  The entry points keep their own checks in their own order.
//
// No float is accumulated with atomics and every sum has one fixed order that depends on (B, F, t, k) alone: results are
// bit-identical run to run.  The table update between the two launches is fmx_fm_update_occ (fmx_kernels.hip).

#include "fmx_host.h"

namespace {

#include "fmx_afm_device.inc"

// ------------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------------
// the shared table check (FTRL and MOMENTS rows: z_offset and the row stride that covers both halves included), then what the
// AFM kernels add to it
int check_afm(const fmx_table_t *t, const fmx_afm_t *afm, const char *who) {
  if (int rc = named(check_table(t), who)) return rc;
  if (!afm || !afm->params) return fail(FMX_ERR_ARG, "%s: null attention parameters", who);
  if (mapped(t)) return fail(FMX_ERR_UNSUPPORTED, "%s: tables whose fields are pieces of index columns are not supported", who);
  if (t->n_fields < 2 || t->n_fields > AFM_MAX_F)
    return fail(FMX_ERR_UNSUPPORTED, "%s: %d fields; the AFM kernels take 2 <= F <= %d", who, t->n_fields, AFM_MAX_F);
  if (afm->k != t->k) return fail(FMX_ERR_SHAPE, "%s: afm->k=%d differs from the table's k=%d", who, afm->k, t->k);
  if (afm->t < 1 || afm->t > AFM_MAX_T) return fail(FMX_ERR_UNSUPPORTED, "%s: attention size t=%d; the AFM kernels take 1 <= t <= %d", who, afm->t, AFM_MAX_T);
  return FMX_OK;
}

template <int KP, bool FTRL, bool BWD>
int launch_afm_k(const AfmArgs &a, hipStream_t st) {
  const size_t lds = (size_t)afm_lds(a.F, KP, a.t, BWD).total * 4;
  if (int rc = raise_lds_limit<k_afm<KP, FTRL, BWD>>((int)(afm_lds(AFM_MAX_F, KP, AFM_MAX_T, BWD).total * 4), "k_afm")) return rc;
  hipLaunchKernelGGL((k_afm<KP, FTRL, BWD>), dim3(afm_grid(a.B)), dim3(64), lds, st, a);
  return check_launch("k_afm");
}

template <int KP, bool FTRL>
int launch_afm_side_k(const AfmSideArgs &a, hipStream_t st) {
  const size_t lds = (size_t)afm_lds(a.n, KP, a.t, false).total * 4;
  if (int rc = raise_lds_limit<k_afm_side<KP, FTRL>>((int)(afm_lds(AFM_MAX_F, KP, AFM_MAX_T, false).total * 4), "k_afm_side")) return rc;
  hipLaunchKernelGGL((k_afm_side<KP, FTRL>), dim3(afm_grid(a.R)), dim3(64), lds, st, a);
  return check_launch("k_afm_side");
}

template <bool BWD>
int launch_afm(const AfmArgs &a, int kp, bool ftrl, hipStream_t st) {
  return with_kp(kp, [&](auto KP) { return ftrl ? launch_afm_k<KP, true, BWD>(a, st) : launch_afm_k<KP, false, BWD>(a, st); });
}

AfmArgs fill_afm(const fmx_table_t *table, const fmx_afm_t *afm, const fmx_hyper_t *hyper, const int32_t *idx, const float *xv,
                 const float *y, int32_t B, int32_t loss_kind, float inv_b, int32_t *error) {
  AfmArgs a;
  memset(&a, 0, sizeof(a));
  a.rows = table->rows;
  a.foff = table->field_offsets;
  a.bias = table->bias;
  a.idx = idx;
  a.xv = xv;
  a.y = y;
  a.params = afm->params;
  a.error = error;
  a.h = kernel_hyper(hyper, -1);
  a.B = B;
  a.F = table->n_fields;
  a.k = afm->k;
  a.t = afm->t;
  a.stride = table->row_stride;
  a.loss_kind = loss_kind;
  a.G = afm->t * afm->k + 2 * afm->t + afm->k;
  a.inv_b = inv_b;
  return a;
}

// the step's workspace: [ the table's step workspace | dz [B] | loss [B] | E [B, F, kp] | partials [grid, G] ], 256-byte sections
struct AfmWs {
  int64_t table_bytes;
  float *dz, *loss, *E, *part;
  int64_t bytes;
};
AfmWs carve_afm(const fmx_table_t *table, const fmx_afm_t *afm, int B, void *base) {
  AfmWs w;
  w.table_bytes = fmx_workspace_bytes(table, B);
  char *p = static_cast<char *>(base);
  size_t o = align_up((size_t)(w.table_bytes > 0 ? w.table_bytes : 0), 256);
  w.dz = reinterpret_cast<float *>(p + o);
  o += align_up((size_t)B * 4, 256);
  w.loss = reinterpret_cast<float *>(p + o);
  o += align_up((size_t)B * 4, 256);
  w.E = reinterpret_cast<float *>(p + o);
  o += align_up((size_t)B * table->n_fields * table->kp * 4, 256);
  w.part = reinterpret_cast<float *>(p + o);
  o += align_up((size_t)afm_grid(B) * (afm->t * afm->k + 2 * afm->t + afm->k) * 4, 256);
  w.bytes = (int64_t)o;
  return w;
}

// the rule and the caller's workspace for a step of B rows (fmx_afm_step; the pair steps with B = 2 B_pairs); w receives the
// carved workspace
int check_afm_ws(const fmx_table_t *table, int32_t rule, const fmx_afm_t *afm, int32_t B, void *workspace, int64_t workspace_bytes, AfmWs &w,
                 const char *who) {
  if (int rc = named(check_rule(table, rule), who)) return rc;
  if (!aligned16(workspace)) return fail(FMX_ERR_ALIGN, "%s: workspace must be 16-byte aligned", who);
  w = carve_afm(table, afm, B, workspace);
  if (w.table_bytes < 0) return (int)w.table_bytes;
  if (workspace_bytes < w.bytes)
    return fail(FMX_ERR_SHAPE, "%s: workspace of %lld bytes, %lld needed (fmx_afm_workspace_bytes)", who, (long long)workspace_bytes,
                (long long)w.bytes);
  return FMX_OK;
}

// fmx_afm_step's own checks
int check_afm_step(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_afm_t *afm, const int32_t *idx, const float *y,
                   int32_t B, void *workspace, int64_t workspace_bytes, const float *attn_grad_out, AfmWs &w, const char *who) {
  if (int rc = check_afm(table, afm, who)) return rc;
  if (!hyper || !idx || !y || !workspace || !attn_grad_out) return fail(FMX_ERR_ARG, "%s: null argument", who);
  if (B < 1) return fail(FMX_ERR_ARG, "%s: B must be >= 1", who);
  return check_afm_ws(table, rule, afm, B, workspace, workspace_bytes, w, who);
}

// the attention parameters take one of four rules (fmx_mlp_opt_t's three and FMX_RULE_SIGNADAM)
int check_attn_rule(int r, const char *who) {
  if (r != FMX_RULE_SIGNADAM && r != FMX_RULE_SGD && r != FMX_RULE_ADAGRAD && r != FMX_RULE_ADAM)
    return fail(FMX_ERR_ARG, "%s: the attention rule %d is not FMX_RULE_SIGNADAM, FMX_RULE_SGD, FMX_RULE_ADAGRAD or FMX_RULE_ADAM", who, r);
  return FMX_OK;
}

// the attention parameters' optimizer state for a call of n_steps steps (fmx_mlp_opt_t with FMX_RULE_SIGNADAM accepted), and
// what the steps' other calls would refuse after the first launch: the tables' FMX_RULE_ADAM hyper-parameters and the sort's
// geometry.  Everything here is decided before anything is launched.
int check_afm_opt(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_afm_t *afm, int32_t B, const fmx_mlp_opt_t *opt,
                  int64_t n_steps, const char *who) {
  if (!opt) return fail(FMX_ERR_ARG, "%s: null argument (opt)", who);
  const int r = opt->rule;
  if (int rc = check_attn_rule(r, who)) return rc;
  if (((r == FMX_RULE_ADAGRAD || r == FMX_RULE_ADAM) && !opt->v) || (r == FMX_RULE_ADAM && !opt->m))
    return fail(FMX_ERR_ARG, "%s: opt->v (FMX_RULE_ADAGRAD, FMX_RULE_ADAM) and opt->m (FMX_RULE_ADAM) must be given", who);
  if (r == FMX_RULE_ADAM && !(opt->beta1 >= 0.f && opt->beta1 < 1.f && opt->beta2 >= 0.f && opt->beta2 < 1.f))
    return fail(FMX_ERR_ARG, "%s: opt->beta1 = %g and opt->beta2 = %g must lie in [0, 1)", who, opt->beta1, opt->beta2);
  if (opt->step < 0 || (int64_t)opt->step + n_steps > INT32_MAX)
    return fail(FMX_ERR_ARG, "%s: opt->step = %d must be >= 0 and step + steps of the call <= 2^31 - 1", who, opt->step);
  if (!aligned16(afm->params) || (opt->m && !aligned16(opt->m)) || (opt->v && !aligned16(opt->v)))
    return fail(FMX_ERR_ALIGN, "%s: afm->params, opt->m and opt->v must be 16-byte aligned", who);
  if (int rc = named(check_adam(hyper, rule, n_steps), who)) return rc;
  return named(check_sort_geometry(table, B), who);
}

// what apply_rule / moments_upd read for step t (1-based) of the attention parameters: ADAM's constants in double, once per step
AfmOptArgs afm_opt_args(const fmx_afm_t *afm, const fmx_mlp_opt_t &o, int32_t t) {
  AfmOptArgs a;
  memset(&a, 0, sizeof(a));
  a.params = afm->params;
  a.m = o.m;
  a.v = o.v;
  a.h.lr = o.lr;
  a.h.eps = o.eps;
  if (o.rule == FMX_RULE_ADAM) adam_consts(o.lr, o.beta1, o.beta2, t, a.h.lr, a.h.beta1, a.h.beta2, o.eps, &a.h.eps);
  return a;
}

// The refusals of a call of n_steps steps of n_rows rows that reads no labels (the pair and the list steps), behind its objective's
// own: the workspace and the rule (check_afm_ws), then the attention rule's state (check_afm_opt) or, without one, what it
// decides for the tables (ADAM's hyper-parameters, the sort's geometry)
int check_afm_unit_steps(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_afm_t *afm, int32_t n_rows,
                         void *workspace, int64_t workspace_bytes, const float *attn_grad_out, const fmx_mlp_opt_t *opt, bool with_opt,
                         int64_t n_steps, AfmWs &w, const char *who) {
  if (!workspace || !attn_grad_out) return fail(FMX_ERR_ARG, "%s: null argument", who);
  if (int rc = check_afm_ws(table, rule, afm, n_rows, workspace, workspace_bytes, w, who)) return rc;
  if (with_opt) return check_afm_opt(table, hyper, rule, afm, n_rows, opt, n_steps, who);
  if (int rc = named(check_adam(hyper, rule, n_steps), who)) return rc;
  return named(check_sort_geometry(table, n_rows), who);
}

// What a step trains on.  Its rows are UNITS of `rows` rows each: samples under BCE on y (POINT); pairs, row 2 i the positive and
// row 2 i + 1 the negative, under the pair loss with `margin` (PAIR, fmx_afm_pair_*); lists of G rows, row G i the positive of list
// i, under the softmax loss (LIST, fmx_afm_list_*).  PAIR and LIST read no y.
struct AfmObjective {
  enum Kind { POINT, PAIR, LIST } kind;
  int32_t rows;  // per unit: 1, 2 or G
  float margin;  // PAIR
};
constexpr AfmObjective AFM_POINTWISE = {AfmObjective::POINT, 1, 0.f};
inline AfmObjective afm_pairs(float margin) { return {AfmObjective::PAIR, 2, margin}; }
inline AfmObjective afm_lists(int32_t G) { return {AfmObjective::LIST, G, 0.f}; }

// k_afm_pair (fmx_afm_pair.inc) over the a.B PAIRS of the 2 a.B rows of a.idx
template <bool BWD>
int launch_afm_pair(const AfmArgs &a, float margin, int kp, bool ftrl, hipStream_t st);
// k_afm_list (fmx_afm_list.inc) over the a.B LISTS of the G a.B rows of a.idx
template <bool BWD>
int launch_afm_list(const AfmArgs &a, int G, int kp, bool ftrl, hipStream_t st);

// One step of B rows on `st`: sort -> forward + backward -> table update (its last workgroups reduce the bias gradient and the
// loss) -> attention gradient, with the attention parameters' rule for their step opt_t when opt is given.  The arguments have
// been checked.  The objective decides the forward + backward: k_afm over the B samples, or k_afm_pair / k_afm_list over the
// B / obj.rows units (one workgroup per unit: that many partials at most).  LIST: the update's bias rule runs on the scratch behind
// the workspace (list_update_table: w.bytes + LIST_BIAS_SCRATCH bytes have been checked).
// logit_out: [B] or null (fmx_afm_step and fmx_afm_stream keep no logits).
int afm_step_launches(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_afm_t *afm, const AfmObjective &obj,
                      const int32_t *idx, const float *xv, const float *y, int32_t B, float inv_b, void *workspace, const AfmWs &w,
                      float *attn_grad_out, float *logit_out, float *loss_out, int32_t *error, const fmx_mlp_opt_t *opt, int32_t opt_t,
                      hipStream_t st) {
  const bool list = obj.kind == AfmObjective::LIST;
  if (int rc = fmx_sort_occurrences(table, idx, B, workspace, w.table_bytes, error, st)) return rc;
  AfmArgs a = fill_afm(table, afm, hyper, idx, xv, y, B / obj.rows, FMX_LOSS_BCE_LOGITS, inv_b, error);
  a.logit = logit_out;
  a.dz = w.dz;
  a.loss = w.loss;
  a.E = w.E;
  a.part = w.part;
  const bool ftrl = table->layout == FMX_LAYOUT_FTRL;
  if (int rc = obj.kind == AfmObjective::PAIR ? launch_afm_pair<true>(a, obj.margin, table->kp, ftrl, st)
               : list                         ? launch_afm_list<true>(a, obj.rows, table->kp, ftrl, st)
                                              : launch_afm<true>(a, table->kp, ftrl, st))
    return rc;
  const fmx_table_t tu = list ? list_update_table(table, workspace, (size_t)w.bytes) : *table;
  if (int rc = fmx_fm_update_occ(&tu, hyper, rule, workspace, w.table_bytes, xv, w.dz, w.E, table->n_fields * table->kp, B, w.loss,
                                 inv_b, loss_out, st))
    return rc;
  const dim3 grid((a.G + 63) / 64), block(256);
  const int n = afm_grid(a.B);
  if (!opt) {
    hipLaunchKernelGGL(k_afm_reduce, grid, block, 0, st, w.part, n, a.G, attn_grad_out);
    return check_launch("k_afm_reduce");
  }
  const AfmOptArgs o = afm_opt_args(afm, *opt, opt_t);
  with_one_of<FMX_RULE_SIGNADAM, FMX_RULE_SGD, FMX_RULE_ADAGRAD, FMX_RULE_ADAM>(opt->rule, [&](auto RULE) {  // (check_afm_opt: one of these)
    hipLaunchKernelGGL(k_afm_reduce_opt<RULE>, grid, block, 0, st, w.part, n, a.G, attn_grad_out, o);
  });
  return check_launch("k_afm_reduce_opt");
}

// n_steps steps of `rows` rows each as ONE plain queue of launches on `st`: every batch is sorted in front of its step, as
// fmx_afm_step does it (no side stream, no events, no host synchronisation; the sort-ahead loop of fmx_fm_stream is not used).
// Step s takes batch s mod n_pool of the pools (idx [n_pool, rows, F]; xv the same or null; y [n_pool, rows], or null where the
// objective reads none) under the tables' hyper-parameters of step s and, with opt, the attention parameters' step
// opt->step + s + 1; its mean loss goes to loss_out[s] and its logits to logit_out + s logit_stride (either may be null).
// The streams pass logit_stride 0; the online runs walk N units once (n_pool = n_steps = N, rows = obj.rows, inv_b = 1) and keep
// every unit's logits before its update: logit_stride = rows.
int afm_steps_run(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_afm_t *afm, const AfmObjective &obj,
                  const int32_t *idx_pool, const float *xv_pool, const float *y_pool, int32_t n_pool, int32_t rows, float inv_b,
                  int32_t n_steps, void *workspace, const AfmWs &w, float *attn_grad_out, const fmx_mlp_opt_t *opt, float *logit_out,
                  int32_t logit_stride, float *loss_out, int32_t *error, hipStream_t st) {
  const size_t F = (size_t)table->n_fields;
  for (int s = 0; s < n_steps; ++s) {
    const fmx_hyper_t hs = hyper_at_step(hyper, rule, s);
    const size_t j = (size_t)(s % n_pool);
    if (int rc = afm_step_launches(table, &hs, rule, afm, obj, idx_pool + j * rows * F, xv_pool ? xv_pool + j * rows * F : nullptr,
                                   y_pool ? y_pool + j * rows : nullptr, rows, inv_b, workspace, w, attn_grad_out,
                                   logit_out ? logit_out + (size_t)s * logit_stride : nullptr, loss_out ? loss_out + s : nullptr, error, opt,
                                   opt ? opt->step + s + 1 : 0, st))
      return rc;
  }
  return FMX_OK;
}

#include "fmx_afm_pair.inc"
#include "fmx_afm_list.inc"

}  // namespace

extern "C" {

int fmx_afm_forward(const fmx_table_t *table, const fmx_afm_t *afm, const fmx_hyper_t *hyper, const int32_t *idx, const float *xv,
                    const float *y, int32_t B, int32_t loss_kind, float inv_b, float *logit_out, float *loss_out, int32_t *error,
                    fmx_stream_t stream) {
  if (int rc = check_afm(table, afm, "fmx_afm_forward")) return rc;
  if (!hyper || !idx) return fail(FMX_ERR_ARG, "fmx_afm_forward: null argument");
  if (B < 1) return fail(FMX_ERR_ARG, "fmx_afm_forward: B must be >= 1");
  if (loss_kind < FMX_LOSS_NONE || loss_kind > FMX_LOSS_BCE_SIGMOID) return fail(FMX_ERR_ARG, "unknown loss %d", loss_kind);
  if (loss_kind != FMX_LOSS_NONE && !y) return fail(FMX_ERR_ARG, "fmx_afm_forward: a loss needs labels y");
  AfmArgs a = fill_afm(table, afm, hyper, idx, xv, y, B, loss_kind, inv_b, error);
  a.logit = logit_out;
  a.loss = loss_kind != FMX_LOSS_NONE ? loss_out : nullptr;
  return launch_afm<false>(a, table->kp, table->layout == FMX_LAYOUT_FTRL, static_cast<hipStream_t>(stream));
}

int64_t fmx_afm_workspace_bytes(const fmx_table_t *table, const fmx_afm_t *afm, int32_t B) {
  if (int rc = check_afm(table, afm, "fmx_afm_workspace_bytes")) return rc;
  if (B < 1) return fail(FMX_ERR_ARG, "fmx_afm_workspace_bytes: B must be >= 1");
  const AfmWs w = carve_afm(table, afm, B, nullptr);
  if (w.table_bytes < 0) return w.table_bytes;
  return w.bytes;
}

int fmx_afm_step(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_afm_t *afm, const int32_t *idx,
                 const float *xv, const float *y, int32_t B, float inv_b, void *workspace, int64_t workspace_bytes,
                 float *attn_grad_out, float *loss_out, int32_t *error, fmx_stream_t stream) {
  const char *who = "fmx_afm_step";
  AfmWs w;
  if (int rc = check_afm_step(table, hyper, rule, afm, idx, y, B, workspace, workspace_bytes, attn_grad_out, w, who)) return rc;
  return afm_step_launches(table, hyper, rule, afm, AFM_POINTWISE, idx, xv, y, B, inv_b, workspace, w, attn_grad_out, nullptr, loss_out,
                           error, nullptr, 0, static_cast<hipStream_t>(stream));
}

int fmx_afm_step_opt(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_afm_t *afm, const int32_t *idx,
                     const float *xv, const float *y, int32_t B, float inv_b, void *workspace, int64_t workspace_bytes,
                     float *attn_grad_out, const fmx_mlp_opt_t *opt, float *loss_out, int32_t *error, fmx_stream_t stream) {
  const char *who = "fmx_afm_step_opt";
  AfmWs w;
  if (int rc = check_afm_step(table, hyper, rule, afm, idx, y, B, workspace, workspace_bytes, attn_grad_out, w, who)) return rc;
  if (int rc = check_afm_opt(table, hyper, rule, afm, B, opt, 1, who)) return rc;
  return afm_step_launches(table, hyper, rule, afm, AFM_POINTWISE, idx, xv, y, B, inv_b, workspace, w, attn_grad_out, nullptr, loss_out,
                           error, opt, opt->step + 1, static_cast<hipStream_t>(stream));
}

int fmx_afm_stream(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_afm_t *afm, const int32_t *idx_pool,
                   const float *xv_pool, const float *y_pool, int32_t n_pool, int32_t B, float inv_b, int32_t n_steps, void *workspace,
                   int64_t workspace_bytes, float *attn_grad_out, const fmx_mlp_opt_t *opt, float *loss_out, int32_t *error,
                   fmx_stream_t stream) {
  const char *who = "fmx_afm_stream";
  AfmWs w;
  if (int rc = check_afm_step(table, hyper, rule, afm, idx_pool, y_pool, B, workspace, workspace_bytes, attn_grad_out, w, who)) return rc;
  if (n_pool < 1 || n_steps < 0) return fail(FMX_ERR_ARG, "%s: n_pool = %d must be >= 1 and n_steps = %d >= 0", who, n_pool, n_steps);
  if (int rc = check_afm_opt(table, hyper, rule, afm, B, opt, n_steps, who)) return rc;
  return afm_steps_run(table, hyper, rule, afm, AFM_POINTWISE, idx_pool, xv_pool, y_pool, n_pool, B, inv_b, n_steps, workspace, w,
                       attn_grad_out, opt, nullptr, 0, loss_out, error, static_cast<hipStream_t>(stream));
}

int fmx_afm_online_run(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_afm_t *afm, const int32_t *idx,
                       const float *xv, const float *y, int32_t N, void *workspace, int64_t workspace_bytes, float *attn_grad_out,
                       const fmx_mlp_opt_t *opt, float *logit_out, float *loss_out, int32_t *error, fmx_stream_t stream) {
  const char *who = "fmx_afm_online_run";
  AfmWs w;
  if (int rc = check_afm_step(table, hyper, rule, afm, idx, y, 1, workspace, workspace_bytes, attn_grad_out, w, who)) return rc;
  if (N < 0) return fail(FMX_ERR_ARG, "%s: N = %d must be >= 0", who, N);
  if (int rc = check_afm_opt(table, hyper, rule, afm, 1, opt, N, who)) return rc;
  if (N == 0) return FMX_OK;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  bool mom = false;
  const int nb = afm_online_form(tune().afm_online_persistent, table->n_fields, afm->k, table->kp, afm->t, opt->rule, mom);
  if (nb == 0)  // the per-sample launches of fmx_afm_step_opt(B = 1, inv_b = 1), queued
    return afm_steps_run(table, hyper, rule, afm, AFM_POINTWISE, idx, xv, y, N, 1, 1.0f, N, workspace, w, attn_grad_out, opt, logit_out, 1,
                         loss_out, error, st);
  const AfmOnlArgs a = fill_afm_online(table, hyper, rule, afm, opt, idx, xv, y, N, attn_grad_out, logit_out, loss_out, error, nb, mom);
  return with_kp(table->kp, [&](auto KP) { return launch_afm_walk_k<KP, k_afm_online<KP>>(a, a, "k_afm_online", st); });
}

int fmx_afm_side(const fmx_table_t *table, const fmx_afm_t *afm, const fmx_hyper_t *hyper, const int32_t *idx, const float *xv,
                 int32_t R, const int32_t *fields, int32_t n_sel, int32_t with_bias, float *E_out, float *stats_out, int32_t *error,
                 fmx_stream_t stream) {
  if (int rc = check_afm(table, afm, "fmx_afm_side")) return rc;
  if (!hyper || !idx || !fields || !E_out || !stats_out) return fail(FMX_ERR_ARG, "fmx_afm_side: null argument");
  if (R < 1) return fail(FMX_ERR_ARG, "fmx_afm_side: R must be >= 1");
  if (with_bias != 0 && with_bias != 1) return fail(FMX_ERR_ARG, "fmx_afm_side: with_bias=%d must be 0 or 1", with_bias);
  const int F = table->n_fields;
  if (n_sel < 1 || n_sel > F) return fail(FMX_ERR_SHAPE, "fmx_afm_side: n_sel=%d must lie in [1, %d]", n_sel, F);
  for (int l = 0; l < n_sel; ++l)
    if (fields[l] < 0 || fields[l] >= F || (l > 0 && fields[l] <= fields[l - 1]))
      return fail(FMX_ERR_ARG, "fmx_afm_side: fields must be ascending field numbers of 0 .. %d", F - 1);
  if (!aligned16(E_out) || !aligned16(stats_out)) return fail(FMX_ERR_ALIGN, "fmx_afm_side: E_out and stats_out must be 16-byte aligned");
  AfmSideArgs a;
  memset(&a, 0, sizeof(a));
  const AfmArgs f = fill_afm(table, afm, hyper, idx, xv, nullptr, R, FMX_LOSS_NONE, 1.f, error);
  a.rows = f.rows;
  a.foff = f.foff;
  a.bias = f.bias;
  a.idx = idx;
  a.xv = xv;
  a.params = afm->params;
  a.E = E_out;
  a.stats = stats_out;
  a.error = error;
  a.h = f.h;
  a.R = R;
  a.F = F;
  a.n = n_sel;
  a.k = afm->k;
  a.t = afm->t;
  a.stride = table->row_stride;
  a.with_bias = with_bias;
  for (int l = 0; l < n_sel; ++l) a.fields[l] = (int8_t)fields[l];
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const bool ftrl = table->layout == FMX_LAYOUT_FTRL;
  return with_kp(table->kp, [&](auto KP) { return ftrl ? launch_afm_side_k<KP, true>(a, st) : launch_afm_side_k<KP, false>(a, st); });
}

// ---- pairwise-ranking (BPR) training: fmx_afm_pair.inc ----
int fmx_afm_pair_forward(const fmx_table_t *table, const fmx_afm_t *afm, const fmx_hyper_t *hyper, const int32_t *idx, const float *xv,
                         int32_t B_pairs, float margin, float inv_b, float *logit_out, float *loss_out, float *dz_out, int32_t *error,
                         fmx_stream_t stream) {
  return afm_pair_forward_call(table, afm, hyper, idx, xv, B_pairs, margin, inv_b, logit_out, loss_out, dz_out, error,
                               static_cast<hipStream_t>(stream));
}

int fmx_afm_pair_step(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_afm_t *afm, const int32_t *idx,
                      const float *xv, int32_t B_pairs, float margin, float inv_b, void *workspace, int64_t workspace_bytes,
                      float *attn_grad_out, float *logit_out, float *loss_out, int32_t *error, fmx_stream_t stream) {
  return afm_pair_steps_call("fmx_afm_pair_step", table, hyper, rule, afm, idx, xv, 1, B_pairs, margin, inv_b, 1, workspace,
                             workspace_bytes, attn_grad_out, nullptr, false, logit_out, loss_out, error, static_cast<hipStream_t>(stream));
}

int fmx_afm_pair_step_opt(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_afm_t *afm, const int32_t *idx,
                          const float *xv, int32_t B_pairs, float margin, float inv_b, void *workspace, int64_t workspace_bytes,
                          float *attn_grad_out, const fmx_mlp_opt_t *opt, float *logit_out, float *loss_out, int32_t *error,
                          fmx_stream_t stream) {
  return afm_pair_steps_call("fmx_afm_pair_step_opt", table, hyper, rule, afm, idx, xv, 1, B_pairs, margin, inv_b, 1, workspace,
                             workspace_bytes, attn_grad_out, opt, true, logit_out, loss_out, error, static_cast<hipStream_t>(stream));
}

int fmx_afm_pair_stream(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_afm_t *afm, const int32_t *idx_pool,
                        const float *xv_pool, int32_t n_pool, int32_t B_pairs, float margin, float inv_b, int32_t n_steps,
                        void *workspace, int64_t workspace_bytes, float *attn_grad_out, const fmx_mlp_opt_t *opt, float *loss_out,
                        int32_t *error, fmx_stream_t stream) {
  return afm_pair_steps_call("fmx_afm_pair_stream", table, hyper, rule, afm, idx_pool, xv_pool, n_pool, B_pairs, margin, inv_b, n_steps,
                             workspace, workspace_bytes, attn_grad_out, opt, true, nullptr, loss_out, error,
                             static_cast<hipStream_t>(stream));
}

int fmx_afm_pair_online_run(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_afm_t *afm, const int32_t *idx,
                            const float *xv, int32_t N_pairs, float margin, void *workspace, int64_t workspace_bytes,
                            float *attn_grad_out, const fmx_mlp_opt_t *opt, float *logit_out, float *loss_out, int32_t *error,
                            fmx_stream_t stream) {
  return afm_pair_online_call(table, hyper, rule, afm, idx, xv, N_pairs, margin, workspace, workspace_bytes, attn_grad_out, opt,
                              logit_out, loss_out, error, static_cast<hipStream_t>(stream));
}

int fmx_afm_pair_online_form(const fmx_table_t *table, const fmx_afm_t *afm, int32_t attn_rule, int32_t *moments_in_lds) {
  return afm_pair_online_form_call(table, afm, attn_rule, moments_in_lds);
}

// ---- listwise (sampled-softmax) training: fmx_afm_list.inc ----
int64_t fmx_afm_list_workspace_bytes(const fmx_table_t *table, const fmx_afm_t *afm, int32_t B_lists, int32_t G) {
  const char *who = "fmx_afm_list_workspace_bytes";
  if (int rc = check_afm(table, afm, who)) return rc;
  if (B_lists < 1 || G < 2 || G > LIST_MAX_G || (int64_t)B_lists * G > INT32_MAX)
    return fail(FMX_ERR_ARG, "%s: B_lists >= 1, 2 <= G <= %d and B_lists * G within int32", who, LIST_MAX_G);
  const AfmWs w = carve_afm(table, afm, B_lists * G, nullptr);
  if (w.table_bytes < 0) return w.table_bytes;
  return w.bytes + LIST_BIAS_SCRATCH;
}

int fmx_afm_list_forward(const fmx_table_t *table, const fmx_afm_t *afm, const fmx_hyper_t *hyper, const int32_t *idx, const float *xv,
                         int32_t B_lists, int32_t G, float inv_b, float *logit_out, float *loss_out, float *dz_out, int32_t *error,
                         fmx_stream_t stream) {
  return afm_list_forward_call(table, afm, hyper, idx, xv, B_lists, G, inv_b, logit_out, loss_out, dz_out, error,
                               static_cast<hipStream_t>(stream));
}

int fmx_afm_list_step(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_afm_t *afm, const int32_t *idx,
                      const float *xv, int32_t B_lists, int32_t G, float inv_b, void *workspace, int64_t workspace_bytes,
                      float *attn_grad_out, float *logit_out, float *loss_out, int32_t *error, fmx_stream_t stream) {
  return afm_list_steps_call("fmx_afm_list_step", table, hyper, rule, afm, idx, xv, 1, B_lists, G, inv_b, 1, workspace, workspace_bytes,
                             attn_grad_out, nullptr, false, logit_out, loss_out, error, static_cast<hipStream_t>(stream));
}

int fmx_afm_list_step_opt(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_afm_t *afm, const int32_t *idx,
                          const float *xv, int32_t B_lists, int32_t G, float inv_b, void *workspace, int64_t workspace_bytes,
                          float *attn_grad_out, const fmx_mlp_opt_t *opt, float *logit_out, float *loss_out, int32_t *error,
                          fmx_stream_t stream) {
  return afm_list_steps_call("fmx_afm_list_step_opt", table, hyper, rule, afm, idx, xv, 1, B_lists, G, inv_b, 1, workspace,
                             workspace_bytes, attn_grad_out, opt, true, logit_out, loss_out, error, static_cast<hipStream_t>(stream));
}

int fmx_afm_list_stream(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_afm_t *afm, const int32_t *idx_pool,
                        const float *xv_pool, int32_t n_pool, int32_t B_lists, int32_t G, float inv_b, int32_t n_steps, void *workspace,
                        int64_t workspace_bytes, float *attn_grad_out, const fmx_mlp_opt_t *opt, float *loss_out, int32_t *error,
                        fmx_stream_t stream) {
  return afm_list_steps_call("fmx_afm_list_stream", table, hyper, rule, afm, idx_pool, xv_pool, n_pool, B_lists, G, inv_b, n_steps,
                             workspace, workspace_bytes, attn_grad_out, opt, true, nullptr, loss_out, error,
                             static_cast<hipStream_t>(stream));
}

int fmx_afm_list_online_run(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_afm_t *afm, const int32_t *idx,
                            const float *xv, int32_t N, int32_t G, void *workspace, int64_t workspace_bytes, float *attn_grad_out,
                            const fmx_mlp_opt_t *opt, float *logit_out, float *loss_out, int32_t *error, fmx_stream_t stream) {
  return afm_list_online_call(table, hyper, rule, afm, idx, xv, N, G, workspace, workspace_bytes, attn_grad_out, opt, logit_out, loss_out,
                              error, static_cast<hipStream_t>(stream));
}

}  // extern "C"
