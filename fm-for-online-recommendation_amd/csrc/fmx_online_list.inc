// fmx_online_list.inc -- the list (sampled-softmax) forms of the one-workgroup MLP step and of the network walkers:
// k_mlp_small_list (fmx_mlp_list_fit), the list sibling of k_mlp_small_pair, and k_online_mlp_list (fmx_online_run_mlp_list), the
// list sibling of k_online_mlp_pair, with its queued form (online_mlp_queued).  Included by fmx_online.hip at file scope behind
// everything else of the unit: it adds code beside the pointwise and the pair forms and changes none of theirs.  The step has its
// OWN text (mlp_list_body) instead of a third instantiation of mlp_small_body: MlpArgs, whose size the other kernels'
// descriptors carry, and their listings stay what they were (tools/isa_diff.py).

namespace {

// ------------------------------------------------------------------------------------------------------------
// k_mlp_small_list: mlp_small_body's FIT step under the list loss
// ------------------------------------------------------------------------------------------------------------
// The B rows are B / G lists, row G i the positive of list i.  Forward, backward and the update are mlp_small_body's FIT mode line
// for line: every output element is ONE thread's serial sum, so the results do not depend on blockDim.  The loss site is the
// list's own.  In mlp_small_body row b of the last layer is thread (L - 1) B + b, and the pair form exchanges logits by lane
// reads; the rows of a list can sit in two wavefronts there (L = 8, B = 9: threads 63 .. 71), so here thread b < B takes row b and
// the logits go through LDS behind a barrier: z_b = base_b + sum_j x_L[b, j] (the sum of the other modes: fmx_mlp_forward's bits),
// the softmax's operand z_b - corr_b, then list_loss_dz_of over the list's operands in the order j = 0 .. G - 1 on every thread of
// the list -- k_mlp_list_loss's operands in its order.  The logit stored is the uncorrected z; z - (+0) is z bit for bit, so
// corr == nullptr and a corr of +0 agree in every bit.  The list's loss is parked in its positive's slot, +0 in the negatives',
// for the FIT mode's ordered sum over the rows times inv_b.  rank[i]: the negatives with z_j >= z_0 on the uncorrected logits
// (k_fm_list_online's definition).
__device__ __forceinline__ void mlp_list_body(const MlpArgs &a, const MlpListPart &lp) {
  __shared__ float acts[(MLP_MAX_L + 1) * MLP_MAX_B * MLP_MAX_W];  // x_0 .. x_L, [l][b][j]
  __shared__ float dA[MLP_MAX_B * MLP_MAX_W], dB[MLP_MAX_B * MLP_MAX_W];  // d x_l (ping-pong); dA is reused as d pre
  __shared__ float dout[MLP_MAX_B];  // d loss / d z_b
  __shared__ float z_l[MLP_MAX_B], zc_l[MLP_MAX_B];  // the logits, and the softmax's operands
  const int tid = threadIdx.x, nt = blockDim.x;
  const int B = a.B, H = a.hidden, L = a.n_layers, G = lp.G;
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
  // ---- the logits ----
  if (tid < B) {
    const int b = tid;
    float s = 0.f;
    for (int j = 0; j < H; ++j) s += X(L, b, j);
    float base_b = a.base[b];
    if (a.base_bias) base_b += a.base_bias_ftrl ? ftrl_w(a.base_bias[0], a.base_bias[1], a.h_table) : a.base_bias[0];
    const float z = base_b + s;
    if (a.pred_out) a.pred_out[b] = z;
    z_l[b] = z;
    zc_l[b] = lp.corr ? z - lp.corr[b] : z;
  }
  __syncthreads();
  // ---- the lists' loss and d loss / d z ----
  if (tid < B) {
    const int b = tid, pos = b % G, first = b - pos;
    float loss, g;
    list_loss_dz_of([&](int j) { return zc_l[first + j]; }, zc_l[b], pos, G, a.inv_b, loss, g);
    a.dz_out[b] = g;
    dout[b] = g;
    X(0, b, MLP_MAX_W - 1) = pos == 0 ? loss : 0.f;  // parked for the ordered sum below (k <= 63 is host-checked)
    if (pos == 0 && lp.rank) {
      int r = 0;
      for (int j = 1; j < G; ++j) r += z_l[first + j] >= z_l[first] ? 1 : 0;
      lp.rank[b / G] = (uint8_t)r;
    }
  }
  __syncthreads();
  if (tid == 0 && a.out) {
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += X(0, b, MLP_MAX_W - 1);
    a.out[0] = s * a.inv_b;
  }
  // ---- backward + update, top layer first ----
  float *dcur = dA, *dnext = dB;
  for (int i = tid; i < B * H; i += nt) dcur[(i / H) * MLP_MAX_W + (i % H)] = dout[i / H];
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
    // d x_l = W^T d pre, with the OLD weights
    for (int i = tid; i < B * in; i += nt) {
      const int b = i / in, c = i % in;
      float s = 0.f;
      for (int j = 0; j < H; ++j) s += W[(size_t)j * in + c] * dcur[b * MLP_MAX_W + j];
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
      if (a.opt_rule != 0) {  // the network's persistent rule: a workgroup-uniform run-time branch
        const size_t o = (size_t)(p - a.params);
        if (a.opt_rule == FMX_RULE_ADAM) {
          moments_upd<FMX_RULE_ADAM>(*p, a.m[o], a.v[o], g, a.oh);
        } else {  // ADAGRAD: m is neither loaded nor stored
          float unused = 0.f;
          moments_upd<FMX_RULE_ADAGRAD>(*p, unused, a.v[o], g, a.oh);
        }
      } else if (a.rule == FMX_RULE_SGD) *p = *p - a.h.lr * g;
      else *p = *p - a.h.lr * g * rcp_(fabsf(g) + a.h.eps);
    }
    __syncthreads();
    float *t = dcur;
    dcur = dnext;
    dnext = t;
  }
  for (int i = tid; i < B * a.kp; i += nt) {
    const int b = i / a.kp, c = i % a.kp;
    a.gbi_out[i] = c < a.k ? dcur[b * MLP_MAX_W + c] : 0.f;
  }
}

__global__ __launch_bounds__(256) void k_mlp_small_list(MlpArgs a, MlpListPart lp) { mlp_list_body(a, lp); }

// the launch of online_mlp_queued and fmx_mlp_list_fit; the callers have checked the shapes (mlp_list_fit_check)
int mlp_list_launch(const fmx_mlp_t *mlp, MlpArgs &a, const MlpListPart &lp, int32_t B, int32_t kp, fmx_stream_t stream) {
  a.params = mlp->params;
  a.B = B;
  a.k = mlp->k;
  a.kp = kp;
  a.hidden = mlp->hidden;
  a.n_layers = mlp->n_layers;
  hipLaunchKernelGGL(k_mlp_small_list, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), a, lp);
  return check_launch("k_mlp_small_list");
}

// ------------------------------------------------------------------------------------------------------------
// k_online_mlp_list: the online list loop of the classes with an MLP, one workgroup walking the stream
// ------------------------------------------------------------------------------------------------------------
// k_fm_list_online's walk around mlp_walk's network step.  A workgroup of 64 max(G, 4) threads walks N lists of G <= 8 rows; wave j < G owns row
// j of the current list (the waves from G on, where G < 4, serve the network's step alone).  Per list every owning wave gathers
// its row's table rows (sc1 loads; the next list's indices, values and corr are requested behind them), evaluates the FM part
// with k_fm_forward's arithmetic (walk_forward) and leaves bi, base, corr, S and the row's (index, value) per field in LDS; the
// whole workgroup runs mlp_list_body at B = G, inv_b = 1 on parameters -- and under opt moments -- that live in LDS for the length
// of the stream (walk_net_stage, walk_net_rule, walk_step_consts: mlp_walk's pieces), which stores the list's logits, loss and
// rank; the fit follows field by field as in k_fm_list_online -- the head of a run adds its members' terms in k_fm_update's order
// (PlainSum / RunSum) and applies one update_row -- on the terms update_body forms with gbi (mlp_walk's): with
// G_j = splat(fm_term ? dz_j : 0) + gbi_j, xG = x G_j, cV = xG S_j, cA = x xG (a float4), cw = x dz_j.  s_waitcnt vmcnt(0) and a
// barrier close the list.  The bias is read once and never written.  Tables, network, moments, logits, ranks and losses end
// bit-identical to N times fmx_fm_forward(B = G), fmx_mlp_list_fit(B_lists = 1, inv_b = 1), fmx_sort_occurrences, fmx_fm_update on
// the list steps' copy of the table.
// G <= 8 ONLY (ONLINE_LIST_MAX_G): eight waves have 256 registers each and keep their rows across the network's step.  A
// 16-wave form (128 registers per wave) was built -- the rows requested again at the fit, the fit walked pass by pass from LDS,
// the step's index arithmetic kept inside the loop, the run walks split, then without the prefetch and specialised on the
// table's passes -- and every instantiation with more than one pass still spilled registers to scratch (1 to 40 per lane: the
// run sums of the fit carry a float4 A-term); no kernel here uses scratch, so longer lists take the queued form.
// LDS: mlp_list_body's 45,248 bytes of static arrays and this kernel's -- bi, gbi, S [8, kp], (index, value) [8, MAXF], the
// fields' offsets: 50,744 to 55,368 bytes in all over the five widths -- and the 96 KB of dynamic LDS the other network walkers
// ask for (ONLINE_MLP_LDS_BYTES) are 153,672 bytes at the most of the CU's 163,840: the parameter cap is theirs, 8,192 with or
// without moments.  MAXF, the fields whose (index, value) are kept, is capped at ONLINE_LIST_MAX_F = 128 (kp = 4 alone would
// reach 256); a table with more fields takes the queued form.
constexpr int ONLINE_LIST_MAX_F = 128, ONLINE_LIST_MAX_G = 8;

struct OnlineMlpListArgs {
  WalkTable t;         // idx, xv: [N G, F], row G i the positive of list i; h: lr / eps also drive the MLP rule when has_opt == 0
  const float *corr;   // [N G] or null
  uint8_t *rank;       // [N] negatives of list i whose logit is >= the positive's, BEFORE the list's update
  float *logit;        // [N G] or null
  float *loss;         // [N] or null
  float *params;       // global: copied into LDS, written back at the end
  int32_t n_params;
  int32_t k, hidden, n_layers, fm_term, rule;
  int32_t has_opt;     // the network under opt (m, v global: copied into LDS, written back at the end)
  int32_t G;
  fmx_mlp_opt_t opt;
};

// the terms one occurrence adds to its run's sums, as update_body carries them with gbi: cV, and (cA, cw) apart
struct NetAW {
  float4 A;
  float w;
};
__device__ __forceinline__ NetAW operator+(NetAW a, NetAW b) { return {a.A + b.A, a.w + b.w}; }
template <>
__device__ __forceinline__ NetAW no_terms<NetAW>() { return {splat(0.f), 0.f}; }
struct NetTerms {
  float4 V;
  NetAW S;
};
__device__ __forceinline__ NetTerms operator+(NetTerms a, NetTerms b) { return {a.V + b.V, a.S + b.S}; }
template <>
__device__ __forceinline__ NetTerms no_terms<NetTerms>() { return {splat(0.f), {splat(0.f), 0.f}}; }

template <int LPR, int LAYOUT, int RULE>
__global__ __launch_bounds__(WAVE * ONLINE_LIST_MAX_G) void k_online_mlp_list(OnlineMlpListArgs la) {
  const WalkTable &a = la.t;
  constexpr int NP = WALK_MAX_NP;
  constexpr int SLOTS = WAVE / LPR, MAXF = NP * SLOTS < ONLINE_LIST_MAX_F ? NP * SLOTS : ONLINE_LIST_MAX_F, MAXG = ONLINE_LIST_MAX_G;
  constexpr int kp = LPR * 4;
  extern __shared__ float p_lds[];  // [n_params] the MLP's parameters, then its moments (walk_net_arrays)
  __shared__ float kc[8];           // ADAM's constants of the list's step (walk_step_consts)
  __shared__ float bi_lds[MAXG * kp], gbi_lds[MAXG * kp];  // [G, kp]
  __shared__ float base_lds[MAXG], corr_lds[MAXG], dz_lds[MAXG];
  __shared__ float S_lds[MAXG][kp];
  __shared__ uint32_t li_lds[MAXG][MAXF];  // the row of field f that list position j names, SENT where it is out of range
  __shared__ float x_lds[MAXG][MAXF];
  __shared__ int64_t foff_lds[MAXF + 1];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);  // (w: wave-uniform, in a scalar register)
  const int slot = lane / LPR, q = lane % LPR;
  const int G = la.G;
  const bool mine = w < G;  // this wave owns row w of every list
  const int net_rule = la.has_opt ? la.opt.rule : -1;
  walk_net_stage<false>(p_lds, la.params, la.opt, la.n_params, net_rule);
  const float bias_w = bias_weight<LAYOUT>(a.bias[0], LAYOUT != FMX_LAYOUT_WEIGHTS ? a.bias[1] : 0.f, a.h);
  // the lane group's field of pass p: fi[p] (the host keeps F <= MAXF, so a live field's arrays are within bounds; a dead lane
  // group reads the last slot and writes none)
  bool live[NP];
  int fi[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    live[p] = p * SLOTS + slot < a.F;
    fi[p] = p * SLOTS + slot < MAXF ? p * SLOTS + slot : MAXF - 1;
  }
  for (int f = tid; f <= MAXF; f += blockDim.x) foff_lds[f] = a.foff[f < a.F ? f : a.F];
  // this wave's row of the next list, and its corr (without corr the index array is loaded in its place and dropped: +0)
  const WalkX xs = walk_x(a);
  walk_gfloat *csrc = (walk_gfloat *)(la.corr ? la.corr : reinterpret_cast<const float *>(a.idx));
  WalkInputs<1, NP> next;
  float c_n = 0.f;
  auto fetch_inputs = [&](int i) {
    const bool in = i < a.N;
    float cc = 0.f;
    walk_fetch<LPR>(next, a, xs, live, slot, in, [&](int) { return (size_t)G * i + w; }, [&] { cc = csrc[in ? (size_t)G * i + w : (size_t)0]; });
    c_n = (la.corr && in) ? cc : 0.f;
  };
  if (mine) fetch_inputs(0);
  __syncthreads();
  bool bad = false;
  for (int i = 0; i < a.N; ++i) {
    uint32_t li[NP];
    float x[NP];
    RowRegs row[NP];
    bool ok[NP];
    float4 s = splat(0.f);
    float c = 0.f;
    if (mine) {
      // ---- the FM part of this wave's row: the gather ----
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        li[p] = next.li[0][p];
        x[p] = next.x[0][p];
        const int64_t lo = foff_lds[fi[p]];
        ok[p] = live[p] && li[p] < (uint32_t)(foff_lds[fi[p] + 1] - lo);
        row[p] = load_row_sc1<LAYOUT, RULE>(a.rows + (size_t)(ok[p] ? lo + li[p] : 0) * a.stride, q, kp, a.zoff);
        bad = bad || (live[p] && !ok[p]);
      }
      c = c_n;
      fetch_inputs(i + 1);  // independent of the weights: in flight while this list is processed
    }
    // one lane of the last wave (idle until the network's step where G < 4), under its gather's latency
    if (tid == (int)blockDim.x - WAVE && (RULE == FMX_RULE_ADAM || net_rule == FMX_RULE_ADAM)) walk_step_consts<RULE>(kc, a.h, la.opt, net_rule, i);
    if (mine) {
      float sbi, fo;
      const float4 bi = walk_forward<LPR>(row, x, ok, lane, s, sbi, fo);
      if (lane < LPR) {
        *reinterpret_cast<float4 *>(&bi_lds[w * kp + 4 * q]) = bi;
        *reinterpret_cast<float4 *>(&S_lds[w][4 * q]) = s;
      }
      if (lane == 0) {
        base_lds[w] = la.fm_term ? fo + sbi + bias_w : fo + bias_w;
        corr_lds[w] = c;
      }
      if (q == 0) {
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          if (live[p]) {
            li_lds[w][fi[p]] = ok[p] ? li[p] : SENT;
            x_lds[w][fi[p]] = x[p];
          }
        }
      }
    }
    __syncthreads();
    // ---- the step of k_mlp_small_list (B = G, inv_b = 1) on LDS-resident parameters ----
    MlpArgs m{};
    m.params = p_lds;
    m.bi = bi_lds;
    m.base = base_lds;
    m.h = a.h;
    m.inv_b = 1.0f;
    m.B = G;
    m.k = la.k;
    m.kp = kp;
    m.hidden = la.hidden;
    m.n_layers = la.n_layers;
    m.pred_out = la.logit ? la.logit + (size_t)G * i : nullptr;
    m.out = la.loss ? la.loss + i : nullptr;
    m.dz_out = dz_lds;
    m.gbi_out = gbi_lds;
    m.mode = MLP_MODE_FIT;
    m.rule = la.rule;
    walk_net_rule(m, net_rule, p_lds, la.n_params, kc, la.opt);
    const MlpListPart lp = {corr_lds, la.rank + i, G};
    mlp_list_body(m, lp);
    __syncthreads();
    if (mine) {
      // ---- fit: k_fm_update on the G rows of the list with dz, dz again where fm_term, and gbi (inv_b = 1) ----
      const float dz_all = dz_lds[lane < G ? lane : 0];  // lane j: the dz of position j (lanes beyond the list are not read)
      const float dz = lane_f(dz_all, w);
      const bool fm = la.fm_term != 0;
      auto g_of = [&](int j, float dzj) { return splat(fm ? dzj : 0.f) + *reinterpret_cast<const float4 *>(&gbi_lds[j * kp + 4 * q]); };
      const float4 Gw = g_of(w, dz);
      fmx_hyper_t h = a.h;
      if (RULE == FMX_RULE_ADAM) {  // the step's constants, as update_impl derives them for a launch
        h.lr = uniform_f(kc[0]);
        h.beta1 = uniform_f(kc[1]);
        h.beta2 = uniform_f(kc[2]);
      }
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        const int f = fi[p];
        const uint32_t my = ok[p] ? li[p] : SENT;
        float *rp = a.rows + (size_t)(ok[p] ? foff_lds[f] + li[p] : 0) * a.stride;
        int before = 0, L = 0;  // valid occurrences of the field with a smaller row; members of this row's run
        bool head = ok[p];
        constexpr int U = 4;  // positions whose LDS reads are in flight together
        for (int j0 = 0; j0 < G; j0 += U) {    // (a position beyond the list repeats the last one, uncounted)
          uint32_t lj[U];
#pragma unroll
          for (int u = 0; u < U; ++u) lj[u] = li_lds[j0 + u < G ? j0 + u : G - 1][f];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const bool in = j0 + u < G;
            before += in && lj[u] < my ? 1 : 0;
            L += in && lj[u] == my ? 1 : 0;
            head = head && !(in && lj[u] == my && j0 + u < w);
          }
        }
        // the occurrence's terms as update_body forms them with gbi
        const float4 xG = x[p] * Gw;
        const float4 ownV = xG * s;
        const NetAW ownS = {x[p] * xG, x[p] * dz};
        float4 rV = splat(0.f) + ownV;
        NetAW rS = no_terms<NetAW>() + ownS;
        if (__ballot(head && L > 1) != 0ull) {  // (wave-uniform) some lane group heads a run of several rows
          // the members behind the head in list order, each read from LDS where it is used
          auto walk = [&](auto rs, auto own, auto term) {
            rs.add(own, head);
            for (int j = w + 1; j < G; ++j) {
              const uint32_t lj = li_lds[j][f];
              const float xj = x_lds[j][f];
              const float4 Sj = *reinterpret_cast<const float4 *>(&S_lds[j][4 * q]);
              const float dzj = lane_f(dz_all, j);
              rs.add(term(xj, dzj, Sj, g_of(j, dzj)), head && lj == my);
            }
            return rs.g;
          };
          auto all_terms = [](float xj, float dzj, float4 Sj, float4 Gj) {
            const float4 xGj = xj * Gj;
            return NetTerms{xGj * Sj, NetAW{xj * xGj, xj * dzj}};
          };
          auto machine = [&](auto zero) {
            RunSum<LPR, decltype(zero)> rs;
            rs.init(before, L);
            return rs;
          };
          const bool wide = head && L > 1 && (before + L - 1) / LPR - before / LPR > 1;  // the run goes over three lane groups or more
          // (the scan's order: the vector's walk, then (cA, cw)'s -- half the registers of one walk for all the sums)
          auto v_terms = [](float xj, float, float4 Sj, float4 Gj) { return (xj * Gj) * Sj; };
          auto s_terms = [](float xj, float dzj, float4, float4 Gj) { return NetAW{xj * (xj * Gj), xj * dzj}; };
          if (__ballot(wide) != 0ull) {  // (wave-uniform) a run of this wave needs the scan's order
            rV = walk(machine(splat(0.f)), ownV, v_terms);
            rS = walk(machine(no_terms<NetAW>()), ownS, s_terms);
          } else {  // the common case, one walk for all the sums
            const NetTerms r1 = walk(PlainSum<NetTerms>{no_terms<NetTerms>()}, NetTerms{ownV, ownS}, all_terms);
            rV = r1.V;
            rS = r1.S;
          }
        }
        if (head) update_row<LAYOUT, RULE>(rp, q, kp, a.zoff, row[p], rV, rS.A, rS.w, h);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the row stores are acknowledged before any wave loads the next list's rows
    }
    __syncthreads();
  }
  walk_net_stage<true>(p_lds, la.params, la.opt, la.n_params, net_rule);
  if (mine) {
    const bool any_bad = __ballot(bad) != 0ull;
    if (lane == 0 && any_bad && a.error) *a.error = 1;
  }
}

template <int LPR, int LAYOUT, int RULE>
int launch_online_mlp_list_k(const OnlineMlpListArgs &a, hipStream_t st) {
  if (int rc = raise_lds_limit<k_online_mlp_list<LPR, LAYOUT, RULE>>(ONLINE_MLP_LDS_BYTES, "k_online_mlp_list")) return rc;
  hipLaunchKernelGGL((k_online_mlp_list<LPR, LAYOUT, RULE>), dim3(1), dim3(WAVE * (a.G > 4 ? a.G : 4)), online_mlp_lds(a), st, a);
  return check_launch("k_online_mlp_list");
}

// what fmx_mlp_list_fit refuses, and fmx_online_run_mlp_list of its network: the list's shape (mlp_list_shape), fmx_mlp_fit's limits
// on B_lists * G rows, and the rule's or opt's checks as mlp_pair_fit_check makes them (n_steps steps of the network)
int mlp_list_fit_check(const fmx_mlp_t *mlp, const fmx_hyper_t *hyper, int32_t rule, int32_t kp, int32_t B_lists, int32_t G,
                       const fmx_mlp_opt_t *opt, int64_t n_steps, const char *who) {
  if (int rc = mlp_list_shape(B_lists, G, who)) return rc;
  if (!mlp || !mlp->params) return fail(FMX_ERR_ARG, "%s: null mlp", who);
  if (opt) {
    if (int rc = mlp_small_opt_check(mlp, opt, n_steps, who)) return rc;
  } else {
    if (adaptive_rule(rule)) return refuse_adaptive(rule, who);
    if (!hyper) return fail(FMX_ERR_ARG, "%s: null argument (hyper)", who);
    if (rule != FMX_RULE_SIGNADAM && rule != FMX_RULE_SGD) return fail(FMX_ERR_ARG, "%s: rule must be SIGNADAM or SGD", who);
  }
  if (mlp->n_layers < 1 || mlp->n_layers > MLP_MAX_L || mlp->hidden < 1 || mlp->hidden > MLP_MAX_W || mlp->k < 1 ||
      mlp->k > MLP_MAX_W - 1 || (int64_t)B_lists * G > MLP_MAX_B || kp < mlp->k)
    return fail(FMX_ERR_UNSUPPORTED,
                "%s: needs B_lists * G <= %d, k <= %d, hidden <= %d, layers <= %d (got B_lists=%d G=%d k=%d hidden=%d layers=%d)", who,
                MLP_MAX_B, MLP_MAX_W - 1, MLP_MAX_W, MLP_MAX_L, B_lists, G, mlp->k, mlp->hidden, mlp->n_layers);
  return FMX_OK;
}

// the list step's arguments as k_mlp_small_list takes them; the network's step t (1-based) under opt
void mlp_list_fit_args(MlpArgs &a, const fmx_hyper_t *hyper, int32_t rule, float inv_b, const fmx_mlp_opt_t *opt, int32_t t) {
  if (hyper) a.h = hyper_for(hyper, -1);
  a.mode = MLP_MODE_FIT;
  a.rule = rule;
  a.inv_b = inv_b;
  if (opt) mlp_small_set_opt(a, *opt, t);
}

}  // namespace

extern "C" {

int fmx_mlp_list_fit(const fmx_mlp_t *mlp, const fmx_hyper_t *hyper, int32_t rule, const float *bi, int32_t kp, const float *base,
                     const float *corr, int32_t B_lists, int32_t G, float inv_b, float *logit_out, float *dz_out, float *gbi_out,
                     float *loss_out, uint8_t *rank_out, const fmx_mlp_opt_t *opt, fmx_stream_t stream) {
  const char *who = "fmx_mlp_list_fit";
  if (int rc = mlp_list_fit_check(mlp, hyper, rule, kp, B_lists, G, opt, 1, who)) return rc;
  if (!bi || !base || !dz_out || !gbi_out) return fail(FMX_ERR_ARG, "%s: null argument", who);
  MlpArgs a{};
  a.bi = bi;
  a.base = base;
  a.pred_out = logit_out;
  a.dz_out = dz_out;
  a.gbi_out = gbi_out;
  a.out = loss_out;
  mlp_list_fit_args(a, opt ? nullptr : hyper, rule, inv_b, opt, opt ? opt->step + 1 : 0);
  const MlpListPart lp = {corr, rank_out, G};
  return mlp_list_launch(mlp, a, lp, B_lists * G, kp, stream);
}

int fmx_online_run_mlp_list(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_mlp_t *mlp, int32_t fm_term,
                            const int32_t *idx, const float *xv, const float *corr, int32_t N, int32_t G, void *workspace,
                            int64_t workspace_bytes, const fmx_fwd_out_t *fwd, float *scratch, uint8_t *rank_out, float *logit_out,
                            float *loss_out, const fmx_mlp_opt_t *opt, fmx_stream_t stream) {
  const char *who = "fmx_online_run_mlp_list";
  static const int32_t no_lists = 0;  // an empty stream's buffers may be null; everything else is checked as for one list
  int32_t rows = 0;
  if (int rc = check_list_args(table, hyper, N == 0 && !idx ? &no_lists : idx, N > 0 ? N : 1, G, &rows, who)) return rc;
  if (N < 0) return fail(FMX_ERR_ARG, "%s: N = %d must be >= 0", who, N);
  if (N > 0 && !rank_out) return fail(FMX_ERR_ARG, "%s: rank_out is null", who);
  // the order of a run's additions follows its positions in the sort field's list; a split field's are counted per piece
  if (table->n_sort_fields > 0)
    return fail(FMX_ERR_UNSUPPORTED, "%s: tables with a sort split (n_sort_fields = %d) are not taken", who, table->n_sort_fields);
  if (!workspace || !fwd || !scratch) return fail(FMX_ERR_ARG, "%s: null argument", who);
  if (!fwd->S || !fwd->bi || !fwd->sfirst || !fwd->logit) return fail(FMX_ERR_ARG, "%s: fwd needs S, bi, sfirst, logit", who);
  if (!aligned16(workspace) || !aligned16(scratch)) return fail(FMX_ERR_ALIGN, "%s: workspace and scratch must be 16-byte aligned", who);
  if (int rc = mlp_list_fit_check(mlp, hyper, rule, table->kp, 1, G, opt, N, who)) return rc;
  if (int rc = check_rule(table, rule)) return named(rc, who);
  if (opt) {
    if (int rc = check_adam(hyper, rule, N)) return named(rc, who);
    if (!fm_term && table->layout == FMX_LAYOUT_FTRL)
      return fail(FMX_ERR_UNSUPPORTED, "%s: fm_term = 0 (NFM) needs a table in the weights or the moments layout", who);
  }
  if (int rc = check_sort_geometry(table, G)) return named(rc, who);
  if (int rc = check_workspace(table, G, workspace, workspace_bytes, who)) return rc;
  const int64_t need = (int64_t)carve(table, G, nullptr).bytes + LIST_BIAS_SCRATCH;
  if (workspace_bytes < need)
    return fail(FMX_ERR_SHAPE, "%s: workspace of %lld bytes, %lld needed: the step's and %lld bytes behind it (fmx_fm_list_workspace_bytes)", who,
                (long long)workspace_bytes, (long long)need, (long long)LIST_BIAS_SCRATCH);
  if (N == 0) return FMX_OK;
  // one workgroup walks the stream when the list fits its waves, the network fits in LDS and a row's fields fit one wavefront
  // (k_online_mlp_list)
  OnlineMlpListArgs a;
  if (G <= ONLINE_LIST_MAX_G && table->layout != FMX_LAYOUT_FTRL && table->n_fields <= ONLINE_LIST_MAX_F &&
      online_mlp_args(a, table, hyper, rule, mlp, fm_term, idx, xv, fwd->error, N, opt)) {
    a.corr = corr;
    a.rank = rank_out;
    a.logit = logit_out;
    a.loss = loss_out;
    a.G = G;
    int rc = FMX_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    with_lpr(table->kp, [&](auto LPR) {
      with_rule(rule, [&](auto LAYOUT, auto RULE) {
        if constexpr (LAYOUT != FMX_LAYOUT_FTRL)  // (never FTRL here)
          rc = launch_online_mlp_list_k<LPR, LAYOUT, RULE>(a, st);
      });
    });
    return rc;
  }
  const MlpListPart list = {corr, rank_out, G};
  return online_mlp_queued(
      table, hyper, rule, opt ? rule : -1, mlp, fm_term, idx, xv, N, G, workspace, fwd, scratch, false, stream, who,
      [&](MlpArgs &m, int i) {
        m.pred_out = logit_out ? logit_out + (size_t)i * G : nullptr;
        m.out = loss_out ? loss_out + i : nullptr;
        mlp_list_fit_args(m, hyper, rule, 1.0f, opt, opt ? opt->step + i + 1 : 0);
      },
      LIST_MAX_G, &list);
}

}  // extern "C"
