// fmx_afm_pair_online.hip -- k_afm_pair_online: the attentional FM's online PAIR loop (predict z_pos > z_neg, then fit on that pair)
// in one workgroup (fmx_afm_pair_online_run; the host code that decides between this kernel and the queued pair steps is
// afm_pair_online_call in fmx_afm_pair.inc).  The launch takes k_afm_online's arguments, filled by the same fill_afm_online
// (fmx_afm_device.inc) with y null, and the margin beside them.
//
// A unit of its own, built from fmx_afm_device.inc: the kernel calls the device functions of k_afm / k_afm_online (stage_params,
// score_pairs, pair_backward, add_tile, ...) and restates none of their arithmetic.  Compiled inside fmx_afm.hip, where it shares those
// template instantiations with the other kernels, every kernel of the same kp came out of the compiler with its instructions
// reordered (tools/isa_diff.py: 55 of 60 listings differed; an empty kernel body, or the kernel at the end of the unit, changed
// nothing about that); here fmx_afm.hip's listings are the parent's, instruction for instruction.
//
// The sibling of k_afm_online for pairs: ONE workgroup of AFM_ONL_WAVES waves walks the stream, the work inside a pair is spread
// over the waves, the attention parameters (and their moments where they fit) stay in LDS.  Every float is the one
// fmx_afm_pair_step_opt gives at B_pairs = 1, inv_b = 1 -- the sort of two rows, k_afm_pair<BWD>, k_fm_update_occ, k_afm_reduce_opt
// over one partial.  Per pair i (row 2 i the positive, row 2 i + 1 the negative):
//   gather    a row slot is (sample, field, quarter): a thread holds BOTH samples' slices of its (field, quarter), loaded by sc1 loads
//             before either sample's update; they stay in registers for the whole pair.  The next pair's inputs are requested behind
//             them.
//   forwards  the negative's, then the positive's (pair_forward below: e = x V and x w from the row registers to LDS, pass A over the
//             waves, k_afm_online's softmax: every wave evaluates the one-wave reductions itself); every wave holds z_neg and z_pos
//             and evaluates pair_loss_dz once on identical operands.
//   backward  the positive's pass B with g in rounds of nb tile buffers; its x dL/de slices go to the registers of the threads that
//             hold the rows.  Then the negative: its e is rebuilt from the row registers (k_afm_pair regathers; the rows have not
//             moved, so the bits are the same), pass A and the softmax re-run, pass B with -g.  dL/de is zeroed before each row, the
//             attention accumulators once per pair: they take the positive's tiles, then the negative's (k_afm_pair's order).
//   update    the attention parameters as in k_afm_online (0 + accumulator, the rule, in LDS).  The tables with the run logic of
//             k_fm_pair_online: a valid row both samples name in a field is ONE run of two occurrences, positive first; otherwise
//             each valid row is a run of one.  The bias gradient (0 + g) + (-g) = +0 still goes through onl_bias_step.
// One code path for every shape; the field sums x w are rewritten with e by each forward, so the LDS carving is afm_online_lds'
// without a word added and the buffer decision is afm_online_buffers' itself.

#include "fmx_host.h"

namespace {

#define FMX_AFM_SHARED_ONLY
#include "fmx_afm_device.inc"

struct AfmPairOnlArgs {
  AfmOnlArgs o;  // N: the number of PAIRS; idx / xv [2 N, F]; logit [2 N]; loss [N]; y is not read
  float margin;
};

template <int KP>
__global__ __launch_bounds__(AFM_ONL_THREADS) void k_afm_pair_online(AfmPairOnlArgs pa) {
  constexpr int NT = AFM_ONL_THREADS, NW = AFM_ONL_WAVES, LPR = KP / 4;
  constexpr int NP = (AFM_MAX_F * LPR + NT - 1) / NT;  // (field, quarter) slots a thread holds, each for both samples
  extern __shared__ float4 lds4[];
  float *sm = reinterpret_cast<float *>(lds4);
  const AfmOnlArgs &a = pa.o;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int F = a.F, k = a.k, t = a.t, P = F * (F - 1) / 2, G = a.G, nb = a.nb;
  const AfmOnlLds O = afm_online_lds(F, KP, t, G, nb, a.mom_lds != 0);
  const AfmLds &L = O.L;
  const bool ftrl = a.rule == FMX_RULE_FTRL, mom_rule = a.rule == FMX_RULE_ADAGRAD || a.rule == FMX_RULE_ADAM;
  const bool o_v = a.o_rule == FMX_RULE_ADAGRAD || a.o_rule == FMX_RULE_ADAM, o_m = a.o_rule == FMX_RULE_ADAM;

  stage_params<KP>(sm, L, a.params, k, t, tid, NT);
  if (tid < WAVE) sm[O.fo + tid] = 0.f;
  if (tid < ONL_MISC) sm[O.misc + tid] = 0.f;
  __syncthreads();
  if (tid == 0) {
    sm[O.misc] = a.bias[0];
    if (ftrl || mom_rule) sm[O.misc + 1] = a.bias[1];
    if (mom_rule) sm[O.misc + 2] = a.bias[2];
  }
  // the moments: in LDS for the whole stream, or left in global memory (the same code through a generic pointer)
  float *mm = a.mom_lds ? sm + O.m : a.m, *vv = a.mom_lds ? sm + O.v : a.v;
  if (a.mom_lds) {
    for (int g = tid; g < G; g += NT) {
      if (o_m) mm[g] = a.m[g];
      if (o_v) vv[g] = a.v[g];
    }
  }

  // the slots this thread gathers and updates: slot rr = tid + p NT is lanes q of field f, for the positive and the negative
  int fld[NP], qq[NP];
  int64_t lo[NP];
  uint32_t vocab[NP];
  bool live[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int rr = tid + p * NT;
    fld[p] = rr / LPR;
    qq[p] = rr - fld[p] * LPR;
    live[p] = fld[p] < F;
    lo[p] = live[p] ? a.foff[fld[p]] : 0;
    vocab[p] = live[p] ? (uint32_t)(a.foff[fld[p] + 1] - lo[p]) : 0u;
  }
  // the next pair's indices and values, sample s = 0 (positive), 1 (negative); branch-free, as in k_afm_online
  uint32_t li_n[2][NP];
  float x_n[2][NP];
  const float *xsrc = a.xv ? a.xv : reinterpret_cast<const float *>(a.idx);
  const bool has_x = a.xv != nullptr;
  auto fetch_inputs = [&](int i) {
    const bool in = i < a.N;
    uint32_t l_[2][NP];
    float x_[2][NP];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        const size_t o = (live[p] && in) ? ((size_t)2 * i + s) * F + fld[p] : (size_t)0;
        l_[s][p] = (uint32_t)a.idx[o];
        x_[s][p] = xsrc[o];
      }
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        li_n[s][p] = (live[p] && in) ? l_[s][p] : 0u;
        x_n[s][p] = (has_x && live[p] && in) ? x_[s][p] : 1.f;
      }
    }
  };
  fetch_inputs(0);
  bool bad = false;
  __syncthreads();

  for (int i = 0; i < a.N; ++i) {
    // ---- gather: both samples' rows by sc1 loads; the next pair's inputs behind them ----
    uint32_t li[2][NP];
    float x[2][NP];
    RowRegs row[2][NP];
    bool ok[2][NP];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        li[s][p] = li_n[s][p];
        x[s][p] = x_n[s][p];
        ok[s][p] = live[p] && li[s][p] < vocab[p];  // (a negative index is a large unsigned one)
        row[s][p] = onl_load_row(a.rule, a.rows + (size_t)(ok[s][p] ? lo[p] + li[s][p] : 0) * a.stride, qq[p], KP, a.zoff);
        bad = bad || (live[p] && !ok[s][p]);
      }
    }
    fetch_inputs(i + 1);
    if (tid == WAVE) {  // ADAM's constants of this pair: [0..2] the tables', [3..6] the attention parameters'
      float *kc = sm + O.misc + ONL_KC;
      if (a.rule == FMX_RULE_ADAM) adam_consts(a.h.lr, a.h.beta1, a.h.beta2, a.h.step + i + 1, kc[0], kc[1], kc[2]);
      if (o_m) adam_consts(a.o_lr, a.o_beta1, a.o_beta2, a.o_step + i + 1, kc[3], kc[4], kc[5], a.o_eps, &kc[6]);
    }
    // dL/de and the attention accumulators [ dW | db | dh | dp ] (one run in LDS): zero before the pair's first pass B
    for (int l = tid; l < O.acc_len; l += NT) sm[L.Ea + l] = 0.f;

    // the forward of sample s from the row registers: e = x V and x w to LDS (gather_field's products; an absent row is zeros),
    // pass A over the waves, k_afm_online's softmax.  The exponentials stay in O.x, p . q in L.r; returns the logit, in every wave
    auto pair_forward = [&](int s, float &Z, float &att) {
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        if (live[p]) {
          const bool okp = s ? ok[1][p] : ok[0][p];
          const float xp = s ? x[1][p] : x[0][p];
          const float4 v = s ? row[1][p].v : row[0][p].v;
          const float w = s ? row[1][p].fo.x : row[0][p].fo.x;
          *reinterpret_cast<float4 *>(sm + L.e + fld[p] * KP + 4 * qq[p]) = okp ? xp * v : splat(0.f);
          if (qq[p] == 0) sm[O.fo + fld[p]] = okp ? w * xp : 0.f;
        }
      }
      __syncthreads();
      score_pairs<KP>(sm, L, F, t, lane, wv, NW);
      __syncthreads();
      float mx = -INFINITY;
      for (int l = lane; l < P; l += WAVE) mx = fmaxf(mx, sm[L.s + l]);
      mx = wave_max(mx);
      for (int l = tid; l < P; l += NT) sm[O.x + l] = expf(sm[L.s + l] - mx);
      const float fo = wave_sum(sm[O.fo + lane]);
      __syncthreads();
      float N = 0.f;
      Z = 0.f;
      for (int l = lane; l < P; l += WAVE) {
        const float ex = sm[O.x + l];
        Z += ex;
        N += ex * sm[L.r + l];
      }
      Z = wave_sum(Z);
      N = wave_sum(N);
      att = N / Z;
      const float bias_w = ftrl ? ftrl_w(sm[O.misc], sm[O.misc + 1], a.h) : sm[O.misc];
      return (bias_w + fo) + att;
    };
    // pass B of the sample whose forward is in LDS, under dlogit g: rounds of nb tiles, as in k_afm_online.  Ends behind a barrier
    auto pair_pass_b = [&](float Z, float g, float att) {
      for (int i0r = 0, pbr = 0; i0r < F - 1;) {
        int i0 = i0r, pb = pbr, cnt = 0;
        for (; cnt < nb && i0 < F - 1; ++cnt) {
          int n;
          const int i1 = next_tile(F, i0, n);
          if (cnt == wv && lane < n) {
            int pi, pj;
            tile_pair(F, i0, lane, pi, pj);
            pair_backward<KP>(sm, L, tile_buf(O, KP, t, cnt), t, pi, pj, lane, sm[O.x + pb + lane], Z, g, att);
          }
          pb += n;
          i0 = i1;
        }
        __syncthreads();
        i0 = i0r;
        for (int c = 0; c < cnt; ++c) {
          int n;
          const int i1 = next_tile(F, i0, n);
          add_tile<KP>(sm, L, tile_buf(O, KP, t, c), F, t, i0, i1, n, tid, NT);
          i0 = i1;
        }
        __syncthreads();
        i0r = i0;
        pbr = pb;
      }
    };

    // ---- forwards: the negative, then the positive; the pair's loss and dlogit in every wave ----
    float Z, att;
    const float zn = pair_forward(1, Z, att);
    const float zp = pair_forward(0, Z, att);  // (its writes of e and x w lie behind the barrier every wave passed after reading them)
    float loss, g;
    pair_loss_dz(zp - zn, pa.margin, 1.0f, loss, g);
    if (tid == 0) {
      if (a.logit) {
        a.logit[2 * (size_t)i] = zp;
        a.logit[2 * (size_t)i + 1] = zn;
      }
      if (a.loss) a.loss[i] = (0.f + loss) + 0.f;  // the update's block_sum over the two rows: the pair's loss, then +0
    }

    // ---- the positive's pass B; its dL/dV_row = x dL/de slices to registers (k_afm's products), its dL/de slots zeroed by their
    //      holders for the negative ----
    pair_pass_b(Z, g, att);
    float4 EP[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      EP[p] = splat(0.f);
      if (live[p]) {
        float4 *ea = reinterpret_cast<float4 *>(sm + L.Ea + fld[p] * KP + 4 * qq[p]);
        EP[p] = x[0][p] * *ea;
        *ea = splat(0.f);
      }
    }
    // ---- the negative again from the row registers (the same bits: the rows have not moved), then its pass B with -g ----
    pair_forward(1, Z, att);
    pair_pass_b(Z, -g, att);

    // ---- the attention parameters: column c's gradient is 0 + the one workgroup's partial (afm_reduce_column), then the rule ----
    {
      fmx_hyper_t ho;
      ho.lr = a.o_lr;
      ho.eps = a.o_eps;
      if (o_m) {
        const float *kc = sm + O.misc + ONL_KC;
        ho.lr = kc[3];
        ho.beta1 = kc[4];
        ho.beta2 = kc[5];
        ho.eps = kc[6];
      }
      for (int c = tid; c < G; c += NT) {
        int par, acc;
        onl_column(L, c, k, t, KP, par, acc);
        const float s = 0.f + sm[acc];
        if (i == a.N - 1) a.grad[c] = s;
        float p = sm[par], m = 0.f, v = 0.f;
        if (o_v) v = vv[c];
        if (o_m) m = mm[c];
        switch (a.o_rule) {
          case FMX_RULE_SIGNADAM: afm_opt_column<FMX_RULE_SIGNADAM>(p, m, v, s, ho); break;
          case FMX_RULE_SGD: afm_opt_column<FMX_RULE_SGD>(p, m, v, s, ho); break;
          case FMX_RULE_ADAGRAD: afm_opt_column<FMX_RULE_ADAGRAD>(p, m, v, s, ho); break;
          default: afm_opt_column<FMX_RULE_ADAM>(p, m, v, s, ho); break;
        }
        if (o_v) vv[c] = v;
        if (o_m) mm[c] = m;
        sm[par] = p;
      }
    }
    // ---- the tables: k_fm_update_occ on the two rows.  The same valid row in a field: one run of two occurrences, positive
    //      first; otherwise each valid row is a run of one ----
    fmx_hyper_t ht = a.h;
    if (a.rule == FMX_RULE_ADAM) {
      const float *kc = sm + O.misc + ONL_KC;
      ht.lr = kc[0];
      ht.beta1 = kc[1];
      ht.beta2 = kc[2];
    }
    const float gn = -g;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      if (live[p]) {
        const float4 EN = x[1][p] * *reinterpret_cast<const float4 *>(sm + L.Ea + fld[p] * KP + 4 * qq[p]);
        const float cwp = x[0][p] * g, cwn = x[1][p] * gn;
        float *rp0 = a.rows + (size_t)(lo[p] + li[0][p]) * a.stride, *rp1 = a.rows + (size_t)(lo[p] + li[1][p]) * a.stride;
        if (ok[0][p] && ok[1][p] && li[0][p] == li[1][p]) {
          onl_update_row(a.rule, rp0, qq[p], KP, a.zoff, row[0][p], (splat(0.f) + EP[p]) + EN, (0.f + cwp) + cwn, ht);
        } else {
          if (ok[0][p]) onl_update_row(a.rule, rp0, qq[p], KP, a.zoff, row[0][p], splat(0.f) + EP[p], 0.f + cwp, ht);
          if (ok[1][p]) onl_update_row(a.rule, rp1, qq[p], KP, a.zoff, row[1][p], splat(0.f) + EN, 0.f + cwn, ht);
        }
      }
    }
    if (tid == 0) {
      float b0 = sm[O.misc], b1 = sm[O.misc + 1], b2 = sm[O.misc + 2];
      onl_bias_step(a.rule, b0, b1, b2, (0.f + g) + gn, ht);  // exactly +0: the moments still decay
      sm[O.misc] = b0;
      sm[O.misc + 1] = b1;
      sm[O.misc + 2] = b2;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the row stores are acknowledged ...
    __syncthreads();                                   // ... before any thread's next gather
  }

  // ---- the state back to global memory ----
  if (bad) sm[O.misc + ONL_FLAG] = 1.f;
  for (int c = tid; c < G; c += NT) {
    int par, acc;
    onl_column(L, c, k, t, KP, par, acc);
    a.params[c] = sm[par];
    if (a.mom_lds) {
      if (o_m) a.m[c] = mm[c];
      if (o_v) a.v[c] = vv[c];
    }
  }
  __syncthreads();
  if (tid == 0) {
    a.bias[0] = sm[O.misc];
    if (ftrl || a.rule == FMX_RULE_ADAM) a.bias[1] = sm[O.misc + 1];
    if (mom_rule) a.bias[2] = sm[O.misc + 2];
    if (sm[O.misc + ONL_FLAG] != 0.f && a.error) *a.error = 1;
  }
}

template <int KP>
int launch_afm_pair_online_k(const AfmPairOnlArgs &pa, hipStream_t st) {
  const AfmOnlArgs &a = pa.o;
  const size_t lds = (size_t)afm_online_lds(a.F, KP, a.t, a.G, a.nb, a.mom_lds != 0).total * 4;
  if (int rc = raise_lds_limit<k_afm_pair_online<KP>>(AFM_LDS_BYTES, "k_afm_pair_online")) return rc;
  hipLaunchKernelGGL((k_afm_pair_online<KP>), dim3(1), dim3(AFM_ONL_THREADS), lds, st, pa);
  return check_launch("k_afm_pair_online");
}

}  // namespace

namespace fmxd {

int afm_pair_online_buffers(int F, int k, int kp, int t, int attn_rule, bool *moments_in_lds) {
  bool mom = false;
  const int nb = !tune().afm_pair_online_persistent
                     ? 0
                     : afm_online_buffers(F, kp, t, t * k + 2 * t + k, attn_rule == FMX_RULE_ADAGRAD || attn_rule == FMX_RULE_ADAM, mom);
  if (moments_in_lds) *moments_in_lds = nb > 0 && mom;
  return nb;
}

int afm_pair_online_launch(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_afm_t *afm, const int32_t *idx,
                           const float *xv, int32_t N_pairs, float margin, float *attn_grad_out, const fmx_mlp_opt_t *opt,
                           float *logit_out, float *loss_out, int32_t *error, int nb, bool moments_in_lds, hipStream_t st) {
  AfmPairOnlArgs pa;
  memset(&pa, 0, sizeof(pa));
  pa.o = fill_afm_online(table, hyper, rule, afm, opt, idx, xv, nullptr, N_pairs, attn_grad_out, logit_out, loss_out, error, nb, moments_in_lds);
  pa.margin = margin;
  return with_kp(table->kp, [&](auto KP) { return launch_afm_pair_online_k<KP>(pa, st); });
}

}  // namespace fmxd
