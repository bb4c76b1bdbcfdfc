// fmx_list.inc -- listwise (sampled-softmax) training of the pure FM, the batched calls: fmx_fm_list_forward / _step / _stream and
// their log-Q corrected forms fmx_fm_list_forward_q / _step_q / _stream_q (corr: one float per row, subtracted from the row's logit in
// front of the softmax; it rides where the pointwise objective's label rides -- FwdArgs.y, step_run's y, stream_run's y_pool --
// and corr == nullptr is the uncorrected call: one set of checks and one step for both).
// Included by fmx_kernels.hip inside its anonymous namespace, behind fmx_pair.inc, whose checks it shares.
// The online form (fmx_fm_list_online_run) has its checks at the end of this file and its kernel, k_fm_list_online, in a unit of its
// own, fmx_list_online.hip.
//
// A batch of B_lists lists of G rows is B_lists G full-width rows: row G i the positive sample of list i, rows G i + 1 .. G i + G - 1
// its negatives.  The forward's epilogue (forward_finish<LIST>, list_loss_dz in fmx_common.h) leaves the softmax cross-entropy of
// every list against its positive in loss[G i] (0 in the negatives' slots) and its gradient in dz, so k_fm_update on the rows with
// dz_first = dz_bi = dz performs the step of inv_b sum_i loss_i.  Nothing of the update changes.
//
// The bias: a softmax does not move under a shift of all its logits, so the bias has no gradient -- but the dz of a list sum to
// zero only up to rounding, and under signadam g / (|g| + eps) would turn that rounding into a step.  The update is therefore
// handed a copy of the (host) table struct whose bias points at LIST_BIAS_SCRATCH bytes behind the ordinary step workspace: the
// bias rule runs on scratch, the table's bias and its state stay bit-unchanged, the forward reads the real bias.  No such device
// exists for the first-order weights of columns every row of a list shares (the context): their gradient is zero in exact
// arithmetic and rounding-level here, and signadam normalises such a gradient like any other.

inline int64_t list_workspace_bytes(const fmx_table_t *table, int32_t rows) { return (int64_t)carve(table, rows, nullptr).bytes + LIST_BIAS_SCRATCH; }

int list_forward_impl(const fmx_table_t *table, const fmx_hyper_t *hyper, const int32_t *idx, const float *xv, const float *corr,
                      int32_t rows, int32_t G, float inv_b, const fmx_fwd_out_t *out, hipStream_t st) {
  FwdArgs a = fill_fwd(table, hyper, idx, xv, corr, rows, FMX_LOSS_NONE, inv_b, out);
  a.list_g = G;
  if (corr) {
    with_lpr(table->kp, [&](auto LPR) { launch_forward_list<LPR, true>(a, table->layout, st); });
    return check_launch("k_fm_forward_listq");
  }
  with_lpr(table->kp, [&](auto LPR) { launch_forward_list<LPR>(a, table->layout, st); });
  return check_launch("k_fm_forward_list");
}

int list_forward_call(const fmx_table_t *table, const fmx_hyper_t *hyper, const int32_t *idx, const float *xv, const float *corr,
                      int32_t B_lists, int32_t G, float inv_b, const fmx_fwd_out_t *out, hipStream_t st, const char *who) {
  int32_t rows = 0;
  if (int rc = check_list_args(table, hyper, idx, B_lists, G, &rows, who)) return rc;
  if (int rc = check_pair_out(table, out, "out", false, who)) return rc;
  return list_forward_impl(table, hyper, idx, xv, corr, rows, G, inv_b, out, st);
}

// the checks of a step (n_steps = 1) or a stream of them, in front of the first launch
int check_list_step(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const int32_t *idx, int32_t B_lists, int32_t G,
                    const void *workspace, int64_t workspace_bytes, const fmx_fwd_out_t *fwd, int64_t n_steps, int32_t *rows, const char *who) {
  if (int rc = check_list_args(table, hyper, idx, B_lists, G, rows, who)) return rc;
  if (int rc = check_rule(table, rule)) return named(rc, who);
  if (int rc = check_adam(hyper, rule, n_steps)) return named(rc, who);
  if (int rc = check_pair_out(table, fwd, "fwd", true, who)) return rc;
  if (int rc = check_sort_geometry(table, *rows)) return rc;  // (as fmx_sort_occurrences reports it)
  if (int rc = check_workspace(table, *rows, workspace, workspace_bytes, who)) return rc;
  const int64_t need = list_workspace_bytes(table, *rows);
  if (workspace_bytes < need)
    return fail(FMX_ERR_SHAPE, "%s: workspace of %lld bytes, %lld needed: the step's and %lld bytes behind it (fmx_fm_list_workspace_bytes)", who,
                (long long)workspace_bytes, (long long)need, (long long)LIST_BIAS_SCRATCH);
  return FMX_OK;
}

// the list objective's forward, as step_run and stream_run call it: their per-step float pointer (the pointwise label's place) is the
// step's corr, null for the uncorrected calls
inline auto list_forward(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rows, int32_t G, float inv_b, const fmx_fwd_out_t *fwd) {
  return [=](const int32_t *idx, const float *xv, const float *corr, hipStream_t st) {
    return list_forward_impl(table, hyper, idx, xv, corr, rows, G, inv_b, fwd, st);
  };
}

int list_step_call(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const int32_t *idx, const float *xv, const float *corr,
                   int32_t B_lists, int32_t G, float inv_b, void *workspace, int64_t workspace_bytes, const fmx_fwd_out_t *fwd,
                   float *loss_out, hipStream_t st, const char *who) {
  int32_t rows = 0;
  if (int rc = check_list_step(table, hyper, rule, idx, B_lists, G, workspace, workspace_bytes, fwd, 1, &rows, who)) return rc;
  const Workspace w = carve(table, rows, workspace);
  const fmx_table_t tu = list_update_table(table, workspace, w.bytes);
  return step_run(table, &tu, hyper, rule, idx, xv, corr, rows, inv_b, w, fwd, loss_out, st, list_forward(table, hyper, rows, G, inv_b, fwd));
}

int list_stream_call(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const int32_t *idx_pool, const float *corr_pool,
                     int32_t n_pool, int32_t B_lists, int32_t G, float inv_b, int32_t n_steps, void *workspace, int64_t workspace_bytes,
                     const fmx_fwd_out_t *fwd, float *loss_out, hipStream_t st, const char *who) {
  int32_t rows = 0;
  if (int rc = check_list_step(table, hyper, rule, idx_pool, B_lists, G, workspace, workspace_bytes, fwd, n_steps > 0 ? n_steps : 0, &rows, who))
    return rc;
  if (int rc = check_pool_steps(n_pool, n_steps, who)) return rc;
  const Workspace w = carve(table, rows, workspace);
  const fmx_table_t tu = list_update_table(table, workspace, w.bytes);
  return stream_run(table, &tu, hyper, rule, idx_pool, corr_pool, n_pool, rows, inv_b, n_steps, w, fwd, loss_out, st,
                    list_forward(table, hyper, rows, G, inv_b, fwd));
}

// fmx_fm_list_online_run: the checks, all on the host and in front of the launch; the kernel is k_fm_list_online (fmx_list_online.hip)
int list_online_call(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const int32_t *idx, const float *xv, int32_t N,
                     int32_t G, uint8_t *rank_out, float *logit_out, float *loss_out, int32_t *error, hipStream_t st) {
  const char *who = "fmx_fm_list_online_run";
  if (!table) return fail(FMX_ERR_ARG, "%s: table is null", who);
  if (int rc = check_table(table)) return named(rc, who);
  if (int rc = check_rule(table, rule)) return named(rc, who);
  if (N < 0) return fail(FMX_ERR_ARG, "%s: N = %d must be >= 0", who, N);
  if (N == 0) return FMX_OK;  // an empty stream (its buffers may be null)
  int32_t rows = 0;
  if (int rc = check_list_args(table, hyper, idx, N, G, &rows, who)) return rc;
  if (int rc = check_adam(hyper, rule, N)) return named(rc, who);
  if (!rank_out) return fail(FMX_ERR_ARG, "%s: rank_out is null", who);
  // a wave holds its row of the list as k_fm_online holds a sample: 4 passes of RowRegs
  const int slots = WAVE / lpr_of(table->kp);
  if (table->n_fields > 4 * slots)
    return fail(FMX_ERR_UNSUPPORTED, "%s: %d fields at kp = %d exceed the %d rows one wavefront holds", who, table->n_fields, table->kp,
                4 * slots);
  // the order of a run's additions follows its positions in the sort field's list; a split field's are counted per piece
  if (table->n_sort_fields > 0)
    return fail(FMX_ERR_UNSUPPORTED, "%s: tables with a sort split (n_sort_fields = %d) are not taken: walk the lists with fmx_fm_list_step", who,
                table->n_sort_fields);
  return list_online_launch(table, hyper, rule, idx, xv, N, G, rank_out, logit_out, loss_out, error, st);
}
