// fmx_pair.inc -- pairwise-ranking (BPR) training of the pure FM, the batched calls: fmx_fm_pair_forward / _step / _stream.
// Included by fmx_kernels.hip inside its anonymous namespace, behind the kernels and the host helpers it builds on.
//
// A batch of B pairs is 2B full-width rows: row 2i the positive sample of pair i, row 2i + 1 the negative.  With
// d_i = z[2i] - z[2i + 1] the loss is -log(sigmoid(d_i) + margin) (pair_loss_dz, fmx_common.h; margin 0 is BPR, the reference
// model's meta_fm.py:145-169 uses 0.1) and the forward's epilogue (forward_finish<PAIR>) leaves
//   dz[2i] = g_i inv_b, dz[2i + 1] = -dz[2i], loss[2i] = loss_i, loss[2i + 1] = 0,
// so k_fm_update on the 2B rows with dz_first = dz_bi = dz performs the exact step of inv_b sum_i loss_i: it sums duplicate rows
// per run, the two occurrences of a row both samples of a pair name included (their cA terms cancel exactly), and the bias
// gradient is sum dz = exactly 0.  Nothing of the update changes.
//
// The online form (fmx_fm_pair_online_run, k_fm_pair_online) is with the other stream walkers in fmx_online.hip.

// ------------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------------
// 2 * B_pairs as the sort and the update take it; beyond int32 it is clamped, which the sort's width check then refuses
inline int32_t pair_rows(int32_t B_pairs) { return B_pairs > INT32_MAX / 2 ? INT32_MAX : 2 * B_pairs; }

int check_pair_out(const fmx_table_t *table, const fmx_fwd_out_t *out, const char *name, bool step, const char *who) {
  if (!out) return fail(FMX_ERR_ARG, "%s: %s is null", who, name);
  if (step) {
    if (!out->S) return fail(FMX_ERR_ARG, "%s: %s->S is required", who, name);
    if (!out->loss) return fail(FMX_ERR_ARG, "%s: %s->loss is required", who, name);
    if (!out->dz) return fail(FMX_ERR_ARG, "%s: %s->dz is required", who, name);
    if (!aligned16(out->dz) || !aligned16(out->loss)) return fail(FMX_ERR_ALIGN, "%s: %s->dz and %s->loss must be 16-byte aligned", who, name, name);
  }
  if ((out->S && !aligned16(out->S)) || (out->bi && !aligned16(out->bi)))
    return fail(FMX_ERR_ALIGN, "%s: %s->S and %s->bi must be 16-byte aligned", who, name, name);
  if (out->sample_ld != 0 && (out->sample_ld < table->kp || out->sample_ld % 4))
    return fail(FMX_ERR_SHAPE, "%s: %s->sample_ld = %d must be 0 or a multiple of 4 that is >= kp", who, name, out->sample_ld);
  return FMX_OK;
}

int pair_forward_impl(const fmx_table_t *table, const fmx_hyper_t *hyper, const int32_t *idx, const float *xv, int32_t B2, float margin,
                      float inv_b, const fmx_fwd_out_t *out, hipStream_t st) {
  FwdArgs a = fill_fwd(table, hyper, idx, xv, nullptr, B2, FMX_LOSS_NONE, inv_b, out);
  a.margin = margin;
  with_lpr(table->kp, [&](auto LPR) { launch_forward<LPR, true>(a, table->layout, st); });
  return check_launch("k_fm_forward (pair)");
}

int pair_forward_call(const fmx_table_t *table, const fmx_hyper_t *hyper, const int32_t *idx, const float *xv, int32_t B_pairs, float margin,
                      float inv_b, const fmx_fwd_out_t *out, hipStream_t st) {
  const char *who = "fmx_fm_pair_forward";
  if (int rc = check_pair_args(table, hyper, idx, B_pairs, "B_pairs", margin, who)) return rc;
  if (B_pairs > INT32_MAX / 2) return fail(FMX_ERR_ARG, "%s: B_pairs = %d: 2 * B_pairs rows exceed int32", who, B_pairs);
  if (int rc = check_pair_out(table, out, "out", false, who)) return rc;
  return pair_forward_impl(table, hyper, idx, xv, 2 * B_pairs, margin, inv_b, out, st);
}

// the checks of a step (n_steps = 1) or a stream of them, in front of the first launch
int check_pair_step(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const int32_t *idx, int32_t B_pairs, float margin,
                    const void *workspace, int64_t workspace_bytes, const fmx_fwd_out_t *fwd, int64_t n_steps, const char *who) {
  if (int rc = check_pair_args(table, hyper, idx, B_pairs, "B_pairs", margin, who)) return rc;
  if (int rc = check_rule(table, rule)) return named(rc, who);
  if (int rc = check_adam(hyper, rule, n_steps)) return named(rc, who);
  if (int rc = check_pair_out(table, fwd, "fwd", true, who)) return rc;
  if (int rc = check_sort_geometry(table, pair_rows(B_pairs))) return rc;  // (as fmx_sort_occurrences reports it)
  return check_workspace(table, pair_rows(B_pairs), workspace, workspace_bytes, who);
}

// the pair objective's forward, as step_run and stream_run call it
inline auto pair_forward(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t B2, float margin, float inv_b, const fmx_fwd_out_t *fwd) {
  return [=](const int32_t *idx, const float *xv, const float *, hipStream_t st) {
    return pair_forward_impl(table, hyper, idx, xv, B2, margin, inv_b, fwd, st);
  };
}

int pair_step_call(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const int32_t *idx, const float *xv, int32_t B_pairs,
                   float margin, float inv_b, void *workspace, int64_t workspace_bytes, const fmx_fwd_out_t *fwd, float *loss_out,
                   hipStream_t st) {
  if (int rc = check_pair_step(table, hyper, rule, idx, B_pairs, margin, workspace, workspace_bytes, fwd, 1, "fmx_fm_pair_step")) return rc;
  const int32_t B2 = 2 * B_pairs;
  return step_run(table, table, hyper, rule, idx, xv, nullptr, B2, inv_b, carve(table, B2, workspace), fwd, loss_out, st,
                  pair_forward(table, hyper, B2, margin, inv_b, fwd));
}

int pair_stream_call(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const int32_t *idx_pool, int32_t n_pool,
                     int32_t B_pairs, float margin, float inv_b, int32_t n_steps, void *workspace, int64_t workspace_bytes,
                     const fmx_fwd_out_t *fwd, float *loss_out, hipStream_t st) {
  const char *who = "fmx_fm_pair_stream";
  if (int rc = check_pair_step(table, hyper, rule, idx_pool, B_pairs, margin, workspace, workspace_bytes, fwd, n_steps > 0 ? n_steps : 0, who))
    return rc;
  if (int rc = check_pool_steps(n_pool, n_steps, who)) return rc;
  const int32_t B2 = 2 * B_pairs;
  return stream_run(table, table, hyper, rule, idx_pool, nullptr, n_pool, B2, inv_b, n_steps, carve(table, B2, workspace), fwd, loss_out, st,
                    pair_forward(table, hyper, B2, margin, inv_b, fwd));
}
