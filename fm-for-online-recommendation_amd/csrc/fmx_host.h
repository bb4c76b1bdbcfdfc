// fmx_host.h -- the host-side vocabulary of the translation units that take an fmx_table_t: the kp / rule dispatchers, the
// table's derived sizes, the hyper-parameters as the launches take them, the step workspace, and the shared checks and the
// launch seams between the units (one definition each; the comment at a declaration names its home).  Host-only.
#pragma once
#include <type_traits>

#include "fmx_common.h"

namespace fmxd {

// the step workspace: [ sorted u32 F*Bp (x 2*SORT_AHEAD_MAX: the online loop sorts a group of batches ahead) |
//                       meta i32 F*tiles*2 | counter | parts f32 F*tiles*2*REC ], each 256-byte aligned (carve)
struct Workspace {
  uint32_t *sorted;       // buffer 0 of a ring of 2 * SORT_AHEAD_MAX buffers, `sorted_stride` elements apart
  size_t sorted_stride;
  uint32_t *runs;         // SORT_AHEAD_MAX buffers of the same shape: the chunk-sorted intermediate of k_sort_chunk / k_sort_merge
  int32_t *meta;
  int32_t *counter;  // step counter (one int32 in its own 256-byte slot; unused by the current loop)
  float *parts;
  size_t bytes;
};

struct SortBatch {  // several batches of a pool in one launch
  int n_pool = 1, first = 0, n_batches = 1;
  int64_t pool_stride = 0, sorted_stride = 0;
  int resident = 0;  // > 0: at most this many workgroups, one per CU at the most, each walking several (batch, field) units
                     // (k_sort_occ_resident: the online loop's side-stream launches); 0: one workgroup per unit
};

// ---- the shared checks (fmx_kernels.hip).  Each leaves its message in g_err; named() puts the entry point in front ----
int check_table(const fmx_table_t *t);
int check_rule(const fmx_table_t *t, int rule);
// ADAM's hyper-parameters for a call of n_steps steps: betas in [0, 1) (torch's bounds) and t = step + n_steps in int32
int check_adam(const fmx_hyper_t *h, int rule, int64_t n_steps);
int check_sort_geometry(const fmx_table_t *t, int B);
// the caller's workspace against what a step of B samples on this table needs NOW (the table's sort fields may have been
// split since the buffer was sized: fmx_workspace_bytes grows with them)
int check_workspace(const fmx_table_t *t, int B, const void *workspace, int64_t workspace_bytes, const char *who);
// what every pair entry point refuses before it looks further: each message names the argument
int check_pair_args(const fmx_table_t *table, const fmx_hyper_t *hyper, const int32_t *idx, int64_t n_pairs, const char *count_name,
                    float margin, const char *who);
// what every list entry point refuses before it looks further (check_pair_args' refusals under the count's name B_lists, then G
// and B_lists * G); *rows = B_lists * G
int check_list_args(const fmx_table_t *table, const fmx_hyper_t *hyper, const int32_t *idx, int32_t B_lists, int32_t G, int32_t *rows,
                    const char *who);
// a shared check's refusal, with the entry point in front of its message
int named(int rc, const char *who);
// the entry points outside the pure-FM table steps: a refusal that names the rule
int refuse_adaptive(int rule, const char *who);

// ---- the launches one unit issues for another; the arguments have been checked ----
// fmx_kernels.hip.  `runs`: the workspace's chunk-sort intermediate (Workspace::runs; used when Bp >= 2 * SORT_CHUNK)
int forward_impl(const fmx_table_t *table, const fmx_hyper_t *hyper, const int32_t *idx, const float *xv, const float *y,
                 int32_t B, int32_t loss_kind, float inv_b, const fmx_fwd_out_t *out, hipStream_t st);
int sort_impl(const fmx_table_t *table, const int32_t *idx, int32_t B, uint32_t *sorted, uint32_t *runs, int32_t *error,
              hipStream_t st, const SortBatch *mb = nullptr);
// fmx_kernels.hip: the dispatch order of k_fm_update's tiles for this table under tune().upd_order, packed four sort fields to a
// word (UpdArgs::order); false: index order (upd_order = 0, more than UPD_ORDER_MAX sort fields, or the table's row counts are
// not known).  The row counts come from a per-device cache keyed by (offsets pointer, sort fields, n_rows, largest sort field);
// a table seen for the first time is entered with ONE blocking copy of its offsets, and only when `may_fill` (the caller's
// stream is not capturing).  A stale entry -- another table at the same address with the same key -- or a missing one gives
// another order of the same tiles: it can cost time, never correctness.
bool update_order(const fmx_table_t *table, bool may_fill, uint32_t *order_words);
// ... the order in which a resident-capped group sort walks the sort fields (k_sort_occ_resident): descending row count from the
// same cache, never filled from here (a table's first update has filled it by the time a call's third group is sorted);
// false: index order
bool sort_walk_order(const fmx_table_t *table, uint32_t *order_words);
// fmx_update.hip
int update_impl(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const Workspace &w,
                const uint32_t *sorted, const float *xv, const float *S, const float *dz_first, const float *dz_bi, const float *gbi,
                int32_t B, const float *loss_b, float inv_b, float *loss_out, hipStream_t st, int32_t *step_counter = nullptr,
                int32_t sample_ld = 0, int32_t *err_flag = nullptr, const MlpReduceArgs *rider = nullptr);
// occ [B, ld_occ]: sample b's gradients of its fields' rows, field f's kp floats at b * ld_occ + f * kp (update_body's OCC)
int update_occ_impl(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const Workspace &w, const float *xv,
                    const float *dz_first, const float *occ, int32_t ld_occ, int32_t B, const float *loss_b, float inv_b,
                    float *loss_out, hipStream_t st);
// fmx_afm_pair_online.hip: the form fmx_afm_pair_online_run takes at this shape under this attention rule -- the tile buffers of
// k_afm_pair_online, or 0 for the queued pair steps (the option "afm_pair_online_persistent" off, or not even min(2, tiles) buffers
// fit beside a sample); *moments_in_lds (or null): whether the attention moments stay in LDS.  Then the launch in that form
int afm_pair_online_buffers(int F, int k, int kp, int t, int attn_rule, bool *moments_in_lds);
int afm_pair_online_launch(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_afm_t *afm, const int32_t *idx,
                           const float *xv, int32_t N_pairs, float margin, float *attn_grad_out, const fmx_mlp_opt_t *opt,
                           float *logit_out, float *loss_out, int32_t *error, int nb, bool moments_in_lds, hipStream_t st);
// fmx_list_online.hip: k_fm_list_online, one workgroup of G waves walking N lists (fmx_fm_list_online_run; list_online_call in
// fmx_list.inc has checked the arguments)
int list_online_launch(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const int32_t *idx, const float *xv, int32_t N,
                       int32_t G, uint8_t *rank_out, float *logit_out, float *loss_out, int32_t *error, hipStream_t st);
// fmx_mlp.hip (fmx_mlp_list.inc): fmx_mlp_list_section without its last launch -- `deferred` receives the arguments of the reduction
// (mlp_section_deferred_reduce's contract; null: launched here).  B_lists lists of G rows, row G i the positive; corr [B_lists G] or
// null.  It checks its own arguments, workspace_bytes included, in front of any launch, and never launches k_mlp_chain
int mlp_list_section_deferred_reduce(const fmx_mlp_t *mlp, const float *bi, int32_t ld_bi, const float *base, const float *corr,
                                     int32_t B_lists, int32_t G, float inv_b, void *workspace, int64_t workspace_bytes, float *logit_out,
                                     float *dz_out, float *gbi_out, int32_t ld_gbi, float *grads, float lr_apply, float *loss_out,
                                     hipStream_t st, MlpReduceArgs *deferred, const char *who);

}  // namespace fmxd

namespace {

inline int lpr_of(int kp) {
  switch (kp) {
    case 4: return 1;
    case 8: return 2;
    case 16: return 4;
    case 32: return 8;
    case 64: return 16;
    default: return 0;
  }
}

// f(std::integral_constant<int, LPR>{}) for a table's kp (anything lpr_of rejects takes the widest)
template <class Fn>
decltype(auto) with_lpr(int kp, Fn &&f) {
  switch (lpr_of(kp)) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 8: return f(std::integral_constant<int, 8>{});
    default: return f(std::integral_constant<int, 16>{});
  }
}

// ... the same with KP = 4 LPR, for the kernels that take the row width itself
template <class Fn>
decltype(auto) with_kp(int kp, Fn &&f) {
  return with_lpr(kp, [&](auto LPR) { return f(std::integral_constant<int, 4 * LPR>{}); });
}

// f(std::integral_constant<int, V>{}) for the V of VS that equals v; false (and no call) when none does
template <int... VS, class Fn>
bool with_one_of(int v, Fn &&f) {
  return ((v == VS && (f(std::integral_constant<int, VS>{}), true)) || ...);
}

// f(LAYOUT, RULE) as integral constants for an update rule and the layout it pairs with (check_rule); false, and no call,
// for a rule it does not know.  with_rule_wf: the rules of the weights and FTRL layouts only (the launches the adaptive
// rules do not take -- fmx_online_run_mlp's k_online_mlp -- are not instantiated for them).
template <bool MOMENTS_RULES, class Fn>
bool with_rule_impl(int rule, Fn &&f) {
  using Weights = std::integral_constant<int, FMX_LAYOUT_WEIGHTS>;
  using Moments = std::integral_constant<int, FMX_LAYOUT_MOMENTS>;
  switch (rule) {
    case FMX_RULE_SIGNADAM: f(Weights{}, std::integral_constant<int, FMX_RULE_SIGNADAM>{}); return true;
    case FMX_RULE_SGD: f(Weights{}, std::integral_constant<int, FMX_RULE_SGD>{}); return true;
    case FMX_RULE_FTRL: f(std::integral_constant<int, FMX_LAYOUT_FTRL>{}, std::integral_constant<int, FMX_RULE_FTRL>{}); return true;
    case FMX_RULE_ADAGRAD:
      if constexpr (MOMENTS_RULES) {
        f(Moments{}, std::integral_constant<int, FMX_RULE_ADAGRAD>{});
        return true;
      }
      return false;
    case FMX_RULE_ADAM:
      if constexpr (MOMENTS_RULES) {
        f(Moments{}, std::integral_constant<int, FMX_RULE_ADAM>{});
        return true;
      }
      return false;
    default: return false;
  }
}
template <class Fn>
bool with_rule(int rule, Fn &&f) { return with_rule_impl<true>(rule, f); }
template <class Fn>
bool with_rule_wf(int rule, Fn &&f) { return with_rule_impl<false>(rule, f); }

inline bool adaptive_rule(int rule) { return rule == FMX_RULE_ADAGRAD || rule == FMX_RULE_ADAM; }
inline const char *rule_name(int rule) { return rule == FMX_RULE_ADAM ? "FMX_RULE_ADAM" : "FMX_RULE_ADAGRAD"; }

// the SORT fields of a table: its fields, or the finer partition fmx_table_t.sort_offsets describes
inline bool mapped(const fmx_table_t *t) { return t->field_cols || t->field_base; }  // fields are pieces of index columns
inline int n_cols(const fmx_table_t *t) { return t->n_cols > 0 ? t->n_cols : t->n_fields; }
inline int n_sort_fields(const fmx_table_t *t) { return t->n_sort_fields > 0 ? t->n_sort_fields : t->n_fields; }
inline const int64_t *sort_offsets(const fmx_table_t *t) { return t->n_sort_fields > 0 ? t->sort_offsets : t->field_offsets; }
inline const int32_t *sort_cols(const fmx_table_t *t) { return t->n_sort_fields > 0 ? t->sort_cols : nullptr; }
inline int64_t max_sort_rows(const fmx_table_t *t) { return t->n_sort_fields > 0 ? t->max_sort_field_rows : t->max_field_rows; }

// The order in which k_fm_update's grid takes n sort fields of rows[i] rows each (fmx_update_order states the contract): a
// permutation in ascending (mode 1) or descending (mode 2) row count, ties in index order; mode 0: the identity.  Returns n, or
// 0 with nothing written when the launch carries no order for so many fields (n > UPD_ORDER_MAX) or the mode is unknown.
inline int upd_order_of(const int64_t *rows, int n, int mode, uint8_t *order) {
  if (n < 1 || n > UPD_ORDER_MAX || mode < 0 || mode > 2) return 0;
  for (int i = 0; i < n; ++i) order[i] = (uint8_t)i;
  if (mode == 0) return n;
  for (int i = 1; i < n; ++i) {  // insertion sort: stable, and n is small
    const uint8_t f = order[i];
    int j = i;
    for (; j > 0 && (mode == 1 ? rows[order[j - 1]] > rows[f] : rows[order[j - 1]] < rows[f]); --j) order[j] = order[j - 1];
    order[j] = f;
  }
  return n;
}

// The caller's hyper-parameters as the launches take them: the six floats every rule reads, and the fields appended after
// them (beta1, beta2, step) for FMX_RULE_ADAM only -- a caller built against the six-float struct passes a shorter struct and
// keeps working with the other rules; nothing past its end is read.  Appended fields not read are zero.
static_assert(sizeof(fmx_hyper_t) == 40, "hyper_for copies fmx_hyper_t field by field: add the new field to the copy");
inline fmx_hyper_t hyper_for(const fmx_hyper_t *h, int rule) {
  fmx_hyper_t r;
  memset(&r, 0, sizeof(r));
  r.lr = h->lr;
  r.eps = h->eps;
  r.alpha = h->alpha;
  r.beta = h->beta;
  r.l1 = h->l1;
  r.l2 = h->l2;
  if (rule == FMX_RULE_ADAM) {
    r.beta1 = h->beta1;
    r.beta2 = h->beta2;
    r.step = h->step;
  }
  return r;
}

// ... for step s of a call of several: step t = h->step + s + 1 of the tables (ADAM's bias correction; the others read no step)
inline fmx_hyper_t hyper_at_step(const fmx_hyper_t *h, int rule, int s) {
  fmx_hyper_t r = hyper_for(h, rule);
  r.step += s;
  return r;
}

// ... and as a kernel's argument: the kernels multiply by 1/alpha
inline fmx_hyper_t kernel_hyper(const fmx_hyper_t *h, int rule) {
  fmx_hyper_t r = hyper_for(h, rule);
  r.alpha = 1.0f / h->alpha;
  return r;
}

// Raise kernel K's dynamic-LDS limit to `bytes` ONCE per process (K is one instantiation: its own flag), and report a failure
// of that one attempt on every call, under the kernel's name: FMX_OK, or FMX_ERR_LAUNCH "hipFuncSetAttribute(<name>): ..."
template <auto K>
int raise_lds_limit(int bytes, const char *name) {
  static std::once_flag once;
  static hipError_t raised = hipSuccess;
  std::call_once(once, [bytes] {
    raised = hipFuncSetAttribute(reinterpret_cast<const void *>(K), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  });
  if (raised != hipSuccess) return fail(FMX_ERR_LAUNCH, "hipFuncSetAttribute(%s): %s", name, hipGetErrorString(raised));
  return FMX_OK;
}

constexpr int SORT_AHEAD_MAX = 16;  // batches sorted per side-stream launch in fmx_fm_stream (r3: 16, was 8 -- every group boundary puts a
                                    // cross-stream wait of 5 - 6 us on the step's stream: 21.33 - 21.39 against 21.53 - 21.79 us per step)

// The list steps' bias scratch (fmx_list.inc's header says why): bytes behind the step workspace of `step_bytes` bytes, and the table
// as the update of a list step takes it -- the bias rule runs on that scratch
constexpr int64_t LIST_BIAS_SCRATCH = 16;  // >= the 3 floats the bias rule of a moments table reads and writes; keeps 16-byte alignment
inline fmx_table_t list_update_table(const fmx_table_t *table, void *workspace, size_t step_bytes) {
  fmx_table_t t = *table;
  t.bias = reinterpret_cast<float *>(static_cast<char *>(workspace) + step_bytes);
  return t;
}

// the shape of a batch of lists, as check_list_args (fmx_kernels.hip) refuses it for the list calls on a table: the network's list
// calls, which take no table (fmx_mlp_list_section in fmx_mlp_list.inc, fmx_mlp_list_fit in fmx_online.hip)
inline int mlp_list_shape(int32_t B_lists, int32_t G, const char *who) {
  if (B_lists < 1) return fail(FMX_ERR_ARG, "%s: B_lists = %d must be >= 1", who, B_lists);
  if (G < 2) return fail(FMX_ERR_ARG, "%s: G = %d: a list is a positive and at least one negative (G >= 2)", who, G);
  if (G > LIST_MAX_G) return fail(FMX_ERR_UNSUPPORTED, "%s: G = %d: at most %d rows per list", who, G, LIST_MAX_G);
  if ((int64_t)B_lists * G > INT32_MAX) return fail(FMX_ERR_ARG, "%s: B_lists = %d, G = %d: B_lists * G rows exceed int32", who, B_lists, G);
  return FMX_OK;
}

inline Workspace carve(const fmx_table_t *t, int B, void *base) {
  const size_t F = (size_t)n_sort_fields(t), Bp = (size_t)fmx_sorted_width(B), tiles = Bp >> 6;
  const size_t rec = 2 * (size_t)t->kp + 4;
  const size_t o_sorted1 = align_up(F * Bp * 4, 256);
  const size_t o_runs = 2 * SORT_AHEAD_MAX * o_sorted1;
  const size_t o_meta = o_runs + (Bp >= 2 * SORT_CHUNK ? SORT_AHEAD_MAX * o_sorted1 : 0);
  const size_t o_counter = o_meta + align_up(F * tiles * 2 * 4, 256);
  const size_t o_parts = o_counter + 256;
  Workspace w;
  char *p = static_cast<char *>(base);
  w.sorted = reinterpret_cast<uint32_t *>(p);
  w.sorted_stride = o_sorted1 / 4;
  w.runs = reinterpret_cast<uint32_t *>(p + o_runs);
  w.meta = reinterpret_cast<int32_t *>(p + o_meta);
  w.counter = reinterpret_cast<int32_t *>(p + o_counter);
  w.parts = reinterpret_cast<float *>(p + o_parts);
  w.bytes = o_parts + align_up(F * tiles * 2 * rec * 4, 256);
  return w;
}

}  // namespace
