// fmx_afm_pair.inc -- pairwise-ranking (BPR) training of the attentional FM: k_afm_pair and the host code of fmx_afm_pair_*
// (included by fmx_afm.hip inside its unnamed namespace, behind the host code the objectives share: the step's launches under an
// AfmObjective, afm_step_launches; the one queue of steps, afm_steps_run; the label-free step check, check_afm_unit_steps).
//
// A batch of B_pairs pairs is idx [2 B_pairs, F] in fmx_fm_pair_forward's layout: row 2 i the positive, row 2 i + 1 the negative.  With
// d_i = z[2i] - z[2i + 1] over the full AFM logit the loss is -log(sigmoid(d_i) + margin) (pair_loss_dz, fmx_common.h; margin 0 is
// BPR, the reference's meta_fm.py:145-169).  dL/dlogit of a row depends on its partner's logit, and k_afm runs a row's forward and
// backward in one loop iteration of one wavefront -- so here the workgroup owns the PAIR:
//
//   k_afm_pair<KP, FTRL, BWD>  one wavefront per workgroup; a workgroup walks the pairs blockIdx.x, blockIdx.x + gridDim.x, ...  Per pair:
//       1  the negative's forward (afm_row_forward: k_afm's gather, pass A and softmax)  -> z_neg, kept in a register
//       2  the positive's forward                                                       -> z_pos; its e, exponentials, Z, att in LDS
//       3  pair_loss_dz(z_pos - z_neg) once, on operands every lane holds identically; lane 0 writes both logits,
//          loss[2p] = loss, loss[2p + 1] = +0, dz[2p] = g, dz[2p + 1] = -g (the same float negated)
//       4  BWD: the positive's pass B with g (afm_row_backward)                          -> E[2p]
//       5  BWD: the negative's forward AGAIN (the bits of 1), then its pass B with -g    -> E[2p + 1]
//     Step 5 recomputes because the LDS has no room for two rows at every shape the kernel takes: at F = kp = t = 64 the BWD carving
//     is 37,248 of the 40,960 floats and a second copy of e | s | r is 8,128.  One code path for every shape.
//     The attention accumulators [ dW | db | dh | dp ] take a pair's positive tiles first, then its negative tiles, each in
//     add_tile's pair order; pairs in the workgroup's walk order; the partials in workgroup order (k_afm_reduce / k_afm_reduce_opt).
//
// A row's device code is k_afm's, statement for statement (afm_row_forward / afm_row_backward below): a row's logit has the bits of
// fmx_afm_forward.
// No float atomics; every sum has one fixed order that depends on (B_pairs, F, t, k) alone.

// The halves of k_afm's walk of one row, restated statement for statement (k_afm keeps its own text: folding it onto these helpers
// reorders its instruction stream, and its instantiations are pinned -- DESIGN.md section 3).
// Forward half of row b: the gather (lane f loads field f's row; an index outside its field: the row is absent,
// the error word says so), pass A (every pair's score s and p . q) and the max-subtracted softmax over the row's pairs.  e, the
// exponentials (in L.s) and p . q (L.r) stay in LDS for afm_row_backward; Z and att = p . sum_ij a_ij q_ij go back in registers
// and the logit is returned.  Every lane ends with the same Z, att and logit.
template <int KP>
__device__ __forceinline__ float afm_row_forward(float *sm, const AfmLds &L, const AfmArgs &a, int F, int t, int P, int lane, float bias_w,
                                                 int b, float &Z, float &att) {
  float fo = 0.f;
  if (lane < F) fo = gather_field<KP>(a.rows, a.foff, a.idx, a.xv, a.error, a.stride, F, b, lane, sm + L.e + lane * KP);
  fo = wave_sum(fo);
  __syncthreads();

  score_pairs<KP>(sm, L, F, t, lane);
  __syncthreads();

  float mx = -INFINITY;
  for (int l = lane; l < P; l += WAVE) mx = fmaxf(mx, sm[L.s + l]);
  mx = wave_max(mx);
  float N = 0.f;
  Z = 0.f;
  for (int l = lane; l < P; l += WAVE) {
    const float ex = expf(sm[L.s + l] - mx);
    sm[L.s + l] = ex;  // (this lane's own slots: read by the other lanes after the barrier in afm_row_backward)
    Z += ex;
    N += ex * sm[L.r + l];
  }
  Z = wave_sum(Z);
  N = wave_sum(N);
  att = N / Z;
  return (bias_w + fo) + att;
}

// ... backward half (pass B) with g = dL/dlogit of the row afm_row_forward left in LDS: every tile's pairs recomputed, then the tile
// added into the owned accumulators in pair order; dL/dV_row = x dL/de goes to E[b]
template <int KP>
__device__ __forceinline__ void afm_row_backward(float *sm, const AfmLds &L, const AfmArgs &a, int F, int t, int lane, int b, float Z, float g,
                                                 float att) {
  for (int l = lane; l < F * KP; l += WAVE) sm[L.Ea + l] = 0.f;
  __syncthreads();
  const AfmTileBuf T = {L.q, L.c, L.co, L.hr, L.ga};
  for (int i0 = 0, pb = 0; i0 < F - 1;) {
    int n;
    const int i1 = next_tile(F, i0, n);
    if (lane < n) {
      int i, j;
      tile_pair(F, i0, lane, i, j);
      pair_backward<KP>(sm, L, T, t, i, j, lane, sm[L.s + pb + lane], Z, g, att);
    }
    __syncthreads();
    add_tile<KP>(sm, L, T, F, t, i0, i1, n, lane, WAVE);
    __syncthreads();
    pb += n;
    i0 = i1;
  }
  float *Eb = a.E + (size_t)b * F * KP;
  for (int l = lane * 4; l < F * KP; l += WAVE * 4) {
    const int f = l / KP;
    const float x = a.xv ? a.xv[(size_t)b * F + f] : 1.f;
    *reinterpret_cast<float4 *>(Eb + l) = x * *reinterpret_cast<const float4 *>(sm + L.Ea + l);
  }
  __syncthreads();
}

// the launch's prologue (the attention parameters staged, BWD: the accumulators zeroed; returns the bias weight) and BWD's
// epilogue (the workgroup's partial [ dW | db | dh | dp ] out)
template <int KP, bool FTRL, bool BWD>
__device__ __forceinline__ float afm_begin(float *sm, const AfmLds &L, const AfmArgs &a, int lane) {
  const int k = a.k, t = a.t;
  stage_params<KP>(sm, L, a.params, k, t, lane);
  if (BWD) {
    for (int i = lane; i < t * KP; i += WAVE) sm[L.aW + i] = 0.f;
    for (int u = lane; u < t; u += WAVE) sm[L.ab + u] = sm[L.ah + u] = 0.f;
    for (int d = lane; d < KP; d += WAVE) sm[L.ap + d] = 0.f;
  }
  return FTRL ? ftrl_w(a.bias[0], a.bias[1], a.h) : a.bias[0];
}
template <int KP>
__device__ __forceinline__ void afm_store_partial(const float *sm, const AfmLds &L, const AfmArgs &a, int lane) {
  const int k = a.k, t = a.t;
  float *part = a.part + (size_t)blockIdx.x * a.G;
  for (int l = lane; l < t * k; l += WAVE) {
    const int u = l / k, d = l - u * k;
    part[l] = sm[L.aW + u * KP + d];
  }
  for (int u = lane; u < t; u += WAVE) {
    part[t * k + u] = sm[L.ab + u];
    part[t * k + t + u] = sm[L.ah + u];
  }
  for (int d = lane; d < k; d += WAVE) part[t * k + 2 * t + d] = sm[L.ap + d];
}

struct AfmPairArgs {
  AfmArgs a;  // B: the number of PAIRS; y and loss_kind are not read
  float margin;
};

template <int KP, bool FTRL, bool BWD>
__global__ __launch_bounds__(64) void k_afm_pair(AfmPairArgs pa) {
  extern __shared__ float4 lds4[];
  float *sm = reinterpret_cast<float *>(lds4);
  const AfmArgs &a = pa.a;
  const int lane = threadIdx.x;
  const int F = a.F, t = a.t, P = F * (F - 1) / 2;
  const AfmLds L = afm_lds(F, KP, t, BWD);
  const float bias_w = afm_begin<KP, FTRL, BWD>(sm, L, a, lane);

  for (int p = blockIdx.x; p < a.B; p += gridDim.x) {
    const int bp = 2 * p, bn = 2 * p + 1;
    float Z, att;
    const float zn = afm_row_forward<KP>(sm, L, a, F, t, P, lane, bias_w, bn, Z, att);
    __syncthreads();  // the positive's gather overwrites e
    const float zp = afm_row_forward<KP>(sm, L, a, F, t, P, lane, bias_w, bp, Z, att);
    float loss, g;
    pair_loss_dz(zp - zn, pa.margin, a.inv_b, loss, g);
    if (lane == 0) {
      if (a.logit) {
        a.logit[bp] = zp;
        a.logit[bn] = zn;
      }
      if (a.loss) {
        a.loss[bp] = loss;
        a.loss[bn] = 0.f;
      }
      if (a.dz) {
        a.dz[bp] = g;
        a.dz[bn] = -g;
      }
    }
    if (!BWD) {
      __syncthreads();  // the next pair's gather overwrites e
      continue;
    }
    afm_row_backward<KP>(sm, L, a, F, t, lane, bp, Z, g, att);
    afm_row_forward<KP>(sm, L, a, F, t, P, lane, bias_w, bn, Z, att);  // the negative again: the same bits as above
    afm_row_backward<KP>(sm, L, a, F, t, lane, bn, Z, -g, att);
  }
  if (BWD) afm_store_partial<KP>(sm, L, a, lane);
}

template <int KP, bool FTRL, bool BWD>
int launch_afm_pair_k(const AfmPairArgs &pa, hipStream_t st) {
  const size_t lds = (size_t)afm_lds(pa.a.F, KP, pa.a.t, BWD).total * 4;
  if (int rc = raise_lds_limit<k_afm_pair<KP, FTRL, BWD>>((int)(afm_lds(AFM_MAX_F, KP, AFM_MAX_T, BWD).total * 4), "k_afm_pair")) return rc;
  hipLaunchKernelGGL((k_afm_pair<KP, FTRL, BWD>), dim3(afm_grid(pa.a.B)), dim3(64), lds, st, pa);
  return check_launch("k_afm_pair");
}

template <bool BWD>
int launch_afm_pair(const AfmArgs &a, float margin, int kp, bool ftrl, hipStream_t st) {
  AfmPairArgs pa;
  pa.a = a;
  pa.margin = margin;
  return with_kp(kp, [&](auto KP) { return ftrl ? launch_afm_pair_k<KP, true, BWD>(pa, st) : launch_afm_pair_k<KP, false, BWD>(pa, st); });
}

// what every fmx_afm_pair_* call refuses first: the pair entry points' shared refusals (check_pair_args), the AFM's (check_afm),
// and a row count 2 n_pairs beyond int32
int check_afm_pair(const fmx_table_t *table, const fmx_afm_t *afm, const fmx_hyper_t *hyper, const int32_t *idx, int64_t n_pairs,
                   const char *count_name, float margin, const char *who) {
  if (int rc = check_pair_args(table, hyper, idx, n_pairs, count_name, margin, who)) return rc;
  if (int rc = check_afm(table, afm, who)) return rc;
  if (n_pairs > INT32_MAX / 2) return fail(FMX_ERR_ARG, "%s: %s = %lld: 2 * %s rows exceed int32", who, count_name, (long long)n_pairs, count_name);
  return FMX_OK;
}

int afm_pair_forward_call(const fmx_table_t *table, const fmx_afm_t *afm, const fmx_hyper_t *hyper, const int32_t *idx, const float *xv,
                          int32_t B_pairs, float margin, float inv_b, float *logit_out, float *loss_out, float *dz_out, int32_t *error,
                          hipStream_t st) {
  if (int rc = check_afm_pair(table, afm, hyper, idx, B_pairs, "B_pairs", margin, "fmx_afm_pair_forward")) return rc;
  AfmArgs a = fill_afm(table, afm, hyper, idx, xv, nullptr, B_pairs, FMX_LOSS_NONE, inv_b, error);
  a.logit = logit_out;
  a.loss = loss_out;
  a.dz = dz_out;
  return launch_afm_pair<false>(a, margin, table->kp, table->layout == FMX_LAYOUT_FTRL, st);
}

// fmx_afm_pair_step (n_pool = n_steps = 1, no opt; its logits kept), fmx_afm_pair_step_opt (the same with opt) and
// fmx_afm_pair_stream: afm_steps_run's queue of pair steps
int afm_pair_steps_call(const char *who, const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_afm_t *afm,
                        const int32_t *idx_pool, const float *xv_pool, int32_t n_pool, int32_t B_pairs, float margin, float inv_b,
                        int32_t n_steps, void *workspace, int64_t workspace_bytes, float *attn_grad_out, const fmx_mlp_opt_t *opt,
                        bool with_opt, float *logit_out, float *loss_out, int32_t *error, hipStream_t st) {
  if (int rc = check_afm_pair(table, afm, hyper, idx_pool, B_pairs, "B_pairs", margin, who)) return rc;
  if (n_pool < 1 || n_steps < 0) return fail(FMX_ERR_ARG, "%s: n_pool = %d must be >= 1 and n_steps = %d >= 0", who, n_pool, n_steps);
  const int32_t B2 = 2 * B_pairs;
  AfmWs w;
  if (int rc = check_afm_unit_steps(table, hyper, rule, afm, B2, workspace, workspace_bytes, attn_grad_out, opt, with_opt, n_steps, w, who))
    return rc;
  return afm_steps_run(table, hyper, rule, afm, afm_pairs(margin), idx_pool, xv_pool, nullptr, n_pool, B2, inv_b, n_steps, workspace, w,
                       attn_grad_out, with_opt ? opt : nullptr, logit_out, 0, loss_out, error, st);
}

// fmx_afm_pair_online_run.  Two forms, the same bits: k_afm_pair_online (fmx_afm_pair_online.hip), one workgroup walking the
// stream, where afm_pair_online_buffers gives it tile buffers; otherwise, for every pair, fmx_afm_pair_step_opt(B_pairs = 1,
// inv_b = 1) -- its own forward gives the pair's logits before its update -- as afm_steps_run's walk of the N pairs (the form
// fmx_afm_online_run falls back to)
int afm_pair_online_call(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_afm_t *afm, const int32_t *idx,
                         const float *xv, int32_t N_pairs, float margin, void *workspace, int64_t workspace_bytes, float *attn_grad_out,
                         const fmx_mlp_opt_t *opt, float *logit_out, float *loss_out, int32_t *error, hipStream_t st) {
  const char *who = "fmx_afm_pair_online_run";
  if (int rc = check_afm_pair(table, afm, hyper, idx, N_pairs > 0 ? N_pairs : 1, "N_pairs", margin, who)) return rc;
  if (N_pairs < 0) return fail(FMX_ERR_ARG, "%s: N_pairs = %d must be >= 0", who, N_pairs);
  AfmWs w;
  if (int rc = check_afm_unit_steps(table, hyper, rule, afm, 2, workspace, workspace_bytes, attn_grad_out, opt, true, N_pairs, w, who)) return rc;
  if (N_pairs == 0) return FMX_OK;
  bool mom = false;
  if (const int nb = afm_pair_online_buffers(table->n_fields, afm->k, table->kp, afm->t, opt->rule, &mom))
    return afm_pair_online_launch(table, hyper, rule, afm, idx, xv, N_pairs, margin, attn_grad_out, opt, logit_out, loss_out, error, nb, mom, st);
  return afm_steps_run(table, hyper, rule, afm, afm_pairs(margin), idx, xv, nullptr, N_pairs, 2, 1.0f, N_pairs, workspace, w, attn_grad_out,
                       opt, logit_out, 2, loss_out, error, st);
}

// fmx_afm_pair_online_form: which of the two forms fmx_afm_pair_online_run takes at this shape -- the structs are read, nothing
// is launched
int afm_pair_online_form_call(const fmx_table_t *table, const fmx_afm_t *afm, int32_t attn_rule, int32_t *moments_in_lds) {
  const char *who = "fmx_afm_pair_online_form";
  if (int rc = check_afm(table, afm, who)) return rc;
  if (int rc = check_attn_rule(attn_rule, who)) return rc;
  bool mom = false;
  const int nb = afm_pair_online_buffers(table->n_fields, afm->k, table->kp, afm->t, attn_rule, &mom);
  if (moments_in_lds) *moments_in_lds = mom ? 1 : 0;
  return nb;
}
