// fmx_pair.inc -- pairwise-ranking (BPR) training of the pure FM: fmx_fm_pair_forward / _step / _stream / _online_run.
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
// k_fm_pair_online is k_fm_online for pairs: one wavefront walks N pairs, predict (z_pos > z_neg) then fit on that pair.

// ------------------------------------------------------------------------------------------------------------
// k_fm_pair_online
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
// host side
// ------------------------------------------------------------------------------------------------------------
// what every pair entry point refuses before it looks further: each message names the argument
int check_pair_args(const fmx_table_t *table, const fmx_hyper_t *hyper, const int32_t *idx, int64_t n_pairs, const char *count_name,
                    float margin, const char *who) {
  if (!table) return fail(FMX_ERR_ARG, "%s: table is null", who);
  if (int rc = check_table(table)) return named(rc, who);
  if (!hyper) return fail(FMX_ERR_ARG, "%s: hyper is null", who);
  if (!idx) return fail(FMX_ERR_ARG, "%s: idx is null", who);
  if (n_pairs < 1) return fail(FMX_ERR_ARG, "%s: %s = %lld must be >= 1", who, count_name, (long long)n_pairs);
  if (!(margin >= 0.f) || !std::isfinite(margin)) return fail(FMX_ERR_ARG, "%s: margin = %g must be finite and >= 0", who, (double)margin);
  if (mapped(table))
    return fail(FMX_ERR_UNSUPPORTED, "%s: tables whose fields are pieces of index columns (field_cols / field_base) are not taken", who);
  return FMX_OK;
}

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

int pair_step_call(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const int32_t *idx, const float *xv, int32_t B_pairs,
                   float margin, float inv_b, void *workspace, int64_t workspace_bytes, const fmx_fwd_out_t *fwd, float *loss_out,
                   hipStream_t st) {
  if (int rc = check_pair_step(table, hyper, rule, idx, B_pairs, margin, workspace, workspace_bytes, fwd, 1, "fmx_fm_pair_step")) return rc;
  const int32_t B2 = 2 * B_pairs;
  const Workspace w = carve(table, B2, workspace);
  // one stream: sort -> pair forward -> update, as fmx_fm_step
  if (int rc = sort_impl(table, idx, B2, w.sorted, w.runs, fwd->error, st)) return rc;
  if (int rc = pair_forward_impl(table, hyper, idx, xv, B2, margin, inv_b, fwd, st)) return rc;
  return update_impl(table, hyper, rule, w, w.sorted, xv, fwd->S, fwd->dz, fwd->dz, nullptr, B2, fwd->loss, inv_b, loss_out, st, nullptr,
                     fwd->sample_ld, fwd->error);
}

int pair_stream_call(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const int32_t *idx_pool, int32_t n_pool,
                     int32_t B_pairs, float margin, float inv_b, int32_t n_steps, void *workspace, int64_t workspace_bytes,
                     const fmx_fwd_out_t *fwd, float *loss_out, hipStream_t st) {
  const char *who = "fmx_fm_pair_stream";
  if (int rc = check_pair_step(table, hyper, rule, idx_pool, B_pairs, margin, workspace, workspace_bytes, fwd, n_steps > 0 ? n_steps : 0, who))
    return rc;
  if (n_pool < 1) return fail(FMX_ERR_ARG, "%s: n_pool = %d must be >= 1", who, n_pool);
  if (n_steps < 0) return fail(FMX_ERR_ARG, "%s: n_steps = %d must be >= 0", who, n_steps);
  const int32_t B2 = 2 * B_pairs;
  const Workspace w = carve(table, B2, workspace);
  // fmx_fm_stream's loop on the 2B rows of a step (pool_loop: the sorts of a group of steps in one launch, ahead of them)
  auto forward = [&](int, const int32_t *idx, const float *, hipStream_t s_) {
    return pair_forward_impl(table, hyper, idx, nullptr, B2, margin, inv_b, fwd, s_);
  };
  auto update = [&](int s, const uint32_t *sorted, hipStream_t s_) {
    fmx_hyper_t hs = hyper_for(hyper, rule);  // step s of the call is step t = hyper->step + s + 1 of the table
    hs.step += s;
    return update_impl(table, &hs, rule, w, sorted, nullptr, fwd->S, fwd->dz, fwd->dz, nullptr, B2, fwd->loss, inv_b,
                       loss_out ? loss_out + s : nullptr, s_, nullptr, fwd->sample_ld, fwd->error);
  };
  return pool_loop(table, idx_pool, nullptr, n_pool, B2, n_steps, w, fwd->error, st, forward, update);
}

int pair_online_call(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const int32_t *idx, const float *xv, int32_t N,
                     float margin, uint8_t *pred_out, float *logit_out, float *loss_out, int32_t *error, hipStream_t st) {
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
  a.h = hyper_for(hyper, rule);  // ADAM: the kernel derives each pair's constants from lr, beta1, beta2, step
  a.h.alpha = 1.0f / hyper->alpha;  // the kernels multiply by 1/alpha
  a.N = N;
  a.F = table->n_fields;
  a.stride = table->row_stride;
  a.zoff = table->z_offset;
  a.margin = margin;
  with_lpr(table->kp, [&](auto LPR) {
    with_rule(rule, [&](auto LAYOUT, auto RULE) { launch_pair_online_np<LPR, LAYOUT, RULE>(a, np, st); });
  });
  return check_launch("k_fm_pair_online");
}
