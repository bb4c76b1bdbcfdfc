// fmx_afm_list.inc -- listwise (sampled-softmax) training of the attentional FM: k_afm_list and the host code of fmx_afm_list_*
// (included by fmx_afm.hip inside its unnamed namespace, behind fmx_afm_pair.inc, whose row helpers it shares; the step's launches, the
// queue of steps and the step checks the objectives share -- afm_step_launches, afm_steps_run, check_afm_unit_steps -- are fmx_afm.hip's).
//
// A batch of B_lists lists of G rows is idx [B_lists G, F] in fmx_fm_list_forward's layout: row G i the positive of list i, rows
// G i + 1 .. G i + G - 1 its negatives.  With z_j the full AFM logit of row G i + j the loss is the softmax cross-entropy against
// position 0 (list_loss_dz_of, fmx_common.h: the FM family's formula, called, not restated).  dL/dlogit of a row depends on every
// logit of its list, so -- as k_afm_pair owns the pair -- the workgroup owns the LIST:
//
//   k_afm_list<KP, FTRL, BWD>  one wavefront per workgroup; a workgroup walks the lists blockIdx.x, blockIdx.x + gridDim.x, ...  Per list:
//       1  the forwards of rows G-1, G-2, .., 1 (afm_row_forward)  -> z_j, wave-uniform, kept in a strip of LIST_MAX_G floats of LDS
//          BEHIND afm_lds(..).total (the carving the pinned kernels share is not touched; the launch asks for total + 16 floats)
//       2  the positive's forward, last                            -> z_0; its e, exponentials, Z, att stay in LDS
//       3  list_loss_dz_of over the strip: lane j < G evaluates position j on operands every lane reads identically, and writes
//          logit[G i + j], loss[G i + j] (the list's loss at j = 0, +0 behind it) and dz[G i + j] -- one vector store each
//       4  BWD: the positive's pass B with dz_0 (afm_row_backward)  -> E[G i]; then, for j = 1 .. G-1, row j's forward AGAIN (the
//          bits of 1) and its pass B with dz_j                      -> E[G i + j]
//     Step 4 recomputes for k_afm_pair's reason: at F = kp = t = 64 the BWD carving is 37,248 of the 40,960 floats and one row's
//     e | s | r is all that fits.  One code path for every shape.
//     The attention accumulators [ dW | db | dh | dp ] take a list's positive tiles first, then its negatives' in row order, each in
//     add_tile's pair order; lists in the workgroup's walk order; the partials in workgroup order (k_afm_reduce / k_afm_reduce_opt).
//
// A row's logit has the bits of fmx_afm_forward.  No float atomics; every sum has one fixed order that depends on
// (B_lists, G, F, t, k) alone.
//
// The bias: a softmax has no bias gradient, but a list's dz sum to zero only up to rounding -- the table update is handed
// list_update_table's copy of the table struct (fmx_host.h), whose bias points at LIST_BIAS_SCRATCH bytes behind the AFM step
// workspace.  The forward reads the real bias; it and its state keep their bits under every rule.

struct AfmListArgs {
  AfmArgs a;  // B: the number of LISTS; y and loss_kind are not read.  (a.G is the attention gradient's length, as everywhere)
  int32_t g;  // rows per list
};

template <int KP, bool FTRL, bool BWD>
__global__ __launch_bounds__(64) void k_afm_list(AfmListArgs la) {
  extern __shared__ float4 lds4[];
  float *sm = reinterpret_cast<float *>(lds4);
  const AfmArgs &a = la.a;
  const int lane = threadIdx.x;
  const int F = a.F, t = a.t, P = F * (F - 1) / 2, G = la.g;
  const AfmLds L = afm_lds(F, KP, t, BWD);
  float *zs = sm + L.total;  // the list's logits, LIST_MAX_G floats
  const float bias_w = afm_begin<KP, FTRL, BWD>(sm, L, a, lane);

  for (int p = blockIdx.x; p < a.B; p += gridDim.x) {
    const int b0 = p * G;
    float Z, att;
    for (int j = G - 1; j >= 0; --j) {  // the positive last: its e, exponentials, Z and att stay
      const float z = afm_row_forward<KP>(sm, L, a, F, t, P, lane, bias_w, b0 + j, Z, att);
      if (lane == 0) zs[j] = z;
      __syncthreads();  // the next row's gather overwrites e; the strip is read below
    }
    const int pos = lane < G ? lane : 0;
    float loss, g;
    list_loss_dz_of([&](int j) { return zs[j]; }, zs[pos], pos, G, a.inv_b, loss, g);
    if (lane < G) {
      if (a.logit) a.logit[b0 + lane] = zs[lane];
      if (a.loss) a.loss[b0 + lane] = lane == 0 ? loss : 0.f;
      if (a.dz) a.dz[b0 + lane] = g;
    }
    if (!BWD) {
      __syncthreads();  // the next list's first row writes the strip
      continue;
    }
    afm_row_backward<KP>(sm, L, a, F, t, lane, b0, Z, __shfl(g, 0), att);
    for (int j = 1; j < G; ++j) {
      afm_row_forward<KP>(sm, L, a, F, t, P, lane, bias_w, b0 + j, Z, att);  // row j again: the same bits as above
      afm_row_backward<KP>(sm, L, a, F, t, lane, b0 + j, Z, __shfl(g, j), att);
    }
  }
  if (BWD) afm_store_partial<KP>(sm, L, a, lane);
}

template <int KP, bool FTRL, bool BWD>
int launch_afm_list_k(const AfmListArgs &la, hipStream_t st) {
  const size_t lds = (size_t)(afm_lds(la.a.F, KP, la.a.t, BWD).total + LIST_MAX_G) * 4;
  if (int rc = raise_lds_limit<k_afm_list<KP, FTRL, BWD>>((int)((afm_lds(AFM_MAX_F, KP, AFM_MAX_T, BWD).total + LIST_MAX_G) * 4), "k_afm_list"))
    return rc;
  hipLaunchKernelGGL((k_afm_list<KP, FTRL, BWD>), dim3(afm_grid(la.a.B)), dim3(64), lds, st, la);
  return check_launch("k_afm_list");
}

template <bool BWD>
int launch_afm_list(const AfmArgs &a, int G, int kp, bool ftrl, hipStream_t st) {
  AfmListArgs la;
  la.a = a;
  la.g = G;
  return with_kp(kp, [&](auto KP) { return ftrl ? launch_afm_list_k<KP, true, BWD>(la, st) : launch_afm_list_k<KP, false, BWD>(la, st); });
}

// what every fmx_afm_list_* call refuses first: the list entry points' shared refusals (check_list_args; *rows = B_lists G), then
// the AFM's (check_afm)
int check_afm_list(const fmx_table_t *table, const fmx_afm_t *afm, const fmx_hyper_t *hyper, const int32_t *idx, int32_t B_lists, int32_t G,
                   int32_t *rows, const char *who) {
  if (int rc = check_list_args(table, hyper, idx, B_lists, G, rows, who)) return rc;
  return check_afm(table, afm, who);
}

int afm_list_forward_call(const fmx_table_t *table, const fmx_afm_t *afm, const fmx_hyper_t *hyper, const int32_t *idx, const float *xv,
                          int32_t B_lists, int32_t G, float inv_b, float *logit_out, float *loss_out, float *dz_out, int32_t *error,
                          hipStream_t st) {
  int32_t rows = 0;
  if (int rc = check_afm_list(table, afm, hyper, idx, B_lists, G, &rows, "fmx_afm_list_forward")) return rc;
  AfmArgs a = fill_afm(table, afm, hyper, idx, xv, nullptr, B_lists, FMX_LOSS_NONE, inv_b, error);
  a.logit = logit_out;
  a.loss = loss_out;
  a.dz = dz_out;
  return launch_afm_list<false>(a, G, table->kp, table->layout == FMX_LAYOUT_FTRL, st);
}

// the list steps' refusals behind check_afm_list: check_afm_unit_steps' for steps of `rows` rows, then the bias scratch behind them
int check_afm_list_steps(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_afm_t *afm, int32_t rows, void *workspace,
                         int64_t workspace_bytes, const float *attn_grad_out, const fmx_mlp_opt_t *opt, bool with_opt, int64_t n_steps,
                         AfmWs &w, const char *who) {
  if (int rc = check_afm_unit_steps(table, hyper, rule, afm, rows, workspace, workspace_bytes, attn_grad_out, opt, with_opt, n_steps, w, who))
    return rc;
  if (workspace_bytes < w.bytes + LIST_BIAS_SCRATCH)
    return fail(FMX_ERR_SHAPE, "%s: workspace of %lld bytes, %lld needed: the step's and %lld bytes behind it (fmx_afm_list_workspace_bytes)", who,
                (long long)workspace_bytes, (long long)(w.bytes + LIST_BIAS_SCRATCH), (long long)LIST_BIAS_SCRATCH);
  return FMX_OK;
}

// fmx_afm_list_step (n_pool = n_steps = 1, no opt; its logits kept), fmx_afm_list_step_opt (the same with opt) and
// fmx_afm_list_stream: afm_steps_run's queue of list steps
int afm_list_steps_call(const char *who, const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_afm_t *afm,
                        const int32_t *idx_pool, const float *xv_pool, int32_t n_pool, int32_t B_lists, int32_t G, float inv_b,
                        int32_t n_steps, void *workspace, int64_t workspace_bytes, float *attn_grad_out, const fmx_mlp_opt_t *opt,
                        bool with_opt, float *logit_out, float *loss_out, int32_t *error, hipStream_t st) {
  int32_t rows = 0;
  if (int rc = check_afm_list(table, afm, hyper, idx_pool, B_lists, G, &rows, who)) return rc;
  if (n_pool < 1 || n_steps < 0) return fail(FMX_ERR_ARG, "%s: n_pool = %d must be >= 1 and n_steps = %d >= 0", who, n_pool, n_steps);
  AfmWs w;
  if (int rc = check_afm_list_steps(table, hyper, rule, afm, rows, workspace, workspace_bytes, attn_grad_out, opt, with_opt, n_steps, w, who))
    return rc;
  return afm_steps_run(table, hyper, rule, afm, afm_lists(G), idx_pool, xv_pool, nullptr, n_pool, rows, inv_b, n_steps, workspace, w,
                       attn_grad_out, with_opt ? opt : nullptr, logit_out, 0, loss_out, error, st);
}

// fmx_afm_list_online_run, the queued form: for every list, fmx_afm_list_step_opt(B_lists = 1, inv_b = 1) -- its own forward gives the
// list's logits before its update -- as afm_steps_run's walk of the N lists
int afm_list_online_call(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_afm_t *afm, const int32_t *idx,
                         const float *xv, int32_t N, int32_t G, void *workspace, int64_t workspace_bytes, float *attn_grad_out,
                         const fmx_mlp_opt_t *opt, float *logit_out, float *loss_out, int32_t *error, hipStream_t st) {
  const char *who = "fmx_afm_list_online_run";
  if (!table) return fail(FMX_ERR_ARG, "%s: table is null", who);
  if (int rc = check_afm(table, afm, who)) return rc;
  if (N < 0) return fail(FMX_ERR_ARG, "%s: N = %d must be >= 0", who, N);
  if (N == 0) return FMX_OK;  // an empty stream (its buffers may be null)
  int32_t rows = 0;
  if (int rc = check_afm_list(table, afm, hyper, idx, N, G, &rows, who)) return rc;
  AfmWs w;
  if (int rc = check_afm_list_steps(table, hyper, rule, afm, G, workspace, workspace_bytes, attn_grad_out, opt, true, N, w, who)) return rc;
  return afm_steps_run(table, hyper, rule, afm, afm_lists(G), idx, xv, nullptr, N, G, 1.0f, N, workspace, w, attn_grad_out, opt, logit_out, G,
                       loss_out, error, st);
}
