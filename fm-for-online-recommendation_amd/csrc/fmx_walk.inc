// fmx_walk.inc -- what the stream walkers of fmx_online.hip and fmx_list_online.hip have in common, each piece stated once: the
// table part of their arguments and the host helpers that fill and size it, and the force-inlined device pieces of one step -- the
// lane group's field table, the branch-free prefetch of the next step's inputs, the sc1 gather, the FM forward from registers, the
// fit of one or two samples from the rows held, the bias words, and for the walkers with a network its LDS staging and its per-step
// constants.  Included inside the unit's anonymous namespace, after fmx_host.h.  A walker is bit-identical to the
// batched launches it stands for: a change here changes every walker, and the tests that pin them run them all.

// ------------------------------------------------------------------------------------------------------------
// host: the table part of a walker's arguments (the first member of each argument struct)
// ------------------------------------------------------------------------------------------------------------
struct WalkTable {
  float *rows;
  const int64_t *foff;
  float *bias;
  const int32_t *idx;  // [rows of the stream, F]
  const float *xv;     // the same shape, or null
  int32_t *error;
  fmx_hyper_t h;       // alpha already inverted; ADAM: the kernel derives each step's constants from lr, beta1, beta2, step
  int32_t N, F, stride, zoff;
};

inline WalkTable walk_table(const fmx_table_t *table, const fmx_hyper_t *hyper, int rule, const int32_t *idx, const float *xv,
                            int32_t *error, int32_t N) {
  WalkTable t;
  t.rows = table->rows;
  t.foff = table->field_offsets;
  t.bias = table->bias;
  t.idx = idx;
  t.xv = xv;
  t.error = error;
  t.h = kernel_hyper(hyper, rule);
  t.N = N;
  t.F = table->n_fields;
  t.stride = table->row_stride;
  t.zoff = table->z_offset;
  return t;
}

// the passes a wavefront makes over a sample's fields (WAVE / lpr lane groups take one field each per pass); a walker holds the
// rows of at most WALK_MAX_NP passes in registers, *max_fields fields
constexpr int WALK_MAX_NP = 4;
inline int walk_passes(const fmx_table_t *table, int *max_fields = nullptr) {
  const int slots = WAVE / lpr_of(table->kp);
  if (max_fields) *max_fields = WALK_MAX_NP * slots;
  return (table->n_fields + slots - 1) / slots;
}
// f(std::integral_constant<int, NP>{}) for np passes (1 .. WALK_MAX_NP; the callers have refused more)
template <class Fn>
void with_walk_np(int np, Fn &&f) {
  if (!with_one_of<1, 2, 3>(np, f)) f(std::integral_constant<int, WALK_MAX_NP>{});
}

// ------------------------------------------------------------------------------------------------------------
// device: the pieces of one step
// ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float uniform_f(float x) { return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(x))); }

// the fields of a lane group, one per pass: field p * SLOTS + slot, its first row and its rows (a dead lane group: 0 rows)
template <int NP>
struct WalkFields {
  int64_t lo[NP];
  uint32_t vocab[NP];
  bool live[NP];
};
template <int LPR, int NP>
__device__ __forceinline__ WalkFields<NP> walk_fields(const int64_t *foff, int F, int slot) {
  constexpr int SLOTS = WAVE / LPR;
  WalkFields<NP> f;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int fi = p * SLOTS + slot;
    f.live[p] = fi < F;
    f.lo[p] = f.live[p] ? foff[fi] : 0;
    f.vocab[p] = f.live[p] ? (uint32_t)(foff[fi + 1] - f.lo[p]) : 0u;
  }
  return f;
}

// the (index, value) of R rows of the stream per lane group
template <int R, int NP>
struct WalkInputs {
  uint32_t li[R][NP];
  float x[R][NP];
};
// The values' source: without xv the index itself is loaded in their place and dropped (x = 1).  It is a pointer to GLOBAL memory
// by type, so that the prefetch is global loads whatever the compiler can see of the select: a flat load counts on both wait
// counters, and every wait of the step would then cover the prefetch as well (profiles/walker_seam_ab.txt has what that costs).
typedef const __attribute__((address_space(1))) float walk_gfloat;
struct WalkX {
  walk_gfloat *src;
  bool has;
};
__device__ __forceinline__ WalkX walk_x(const WalkTable &t) {
  return {(walk_gfloat *)(t.xv ? t.xv : reinterpret_cast<const float *>(t.idx)), t.xv != nullptr};
}
// The next step's inputs: rows row_of(0) .. row_of(R - 1) of the stream.  They do not depend on the weights, so a walker requests
// them behind its row loads and they are in flight while the step is processed.  Branch-free (see forward_sample): beyond the
// stream (`in` false) or the last field the loads read element 0 and are dropped.  mid() stands between the loads and the selects:
// a walker's other load of the next step (the label) goes there.
template <int LPR, int R, int NP, class RowOf, class Mid>
__device__ __forceinline__ void walk_fetch(WalkInputs<R, NP> &n, const WalkTable &t, WalkX xs, const bool (&live)[NP], int slot, bool in,
                                           RowOf row_of, Mid mid) {
  constexpr int SLOTS = WAVE / LPR;
  uint32_t l_[R][NP];
  float x_[R][NP];
#pragma unroll
  for (int r = 0; r < R; ++r) {
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const size_t o = (live[p] && in) ? (size_t)row_of(r) * t.F + p * SLOTS + slot : (size_t)0;
      l_[r][p] = (uint32_t)t.idx[o];
      x_[r][p] = xs.src[o];
    }
  }
  mid();
#pragma unroll
  for (int r = 0; r < R; ++r) {
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      n.li[r][p] = (live[p] && in) ? l_[r][p] : 0u;
      n.x[r][p] = (xs.has && live[p] && in) ? x_[r][p] : 1.f;
    }
  }
}

// The gather: the table rows the R samples name, all requested together (sc1: the previous step may have written them).
// Branch-free: a dead lane group or a bad index requests the table's first row and drops it -- with a branch per pass the rows of
// a sample went out in NP dependent round trips.
template <int LAYOUT, int RULE, int R, int NP>
__device__ __forceinline__ void walk_gather(RowRegs (&row)[R][NP], bool (&ok)[R][NP], bool &bad, const WalkTable &t,
                                            const WalkFields<NP> &f, const uint32_t (&li)[R][NP], int q, int kp) {
#pragma unroll
  for (int r = 0; r < R; ++r) {
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      ok[r][p] = f.live[p] && li[r][p] < f.vocab[p];
      row[r][p] = load_row_sc1<LAYOUT, RULE>(t.rows + (size_t)(ok[r][p] ? f.lo[p] + li[r][p] : 0) * t.stride, q, kp, t.zoff);
      bad = bad || (f.live[p] && !ok[r][p]);
    }
  }
}

// The FM forward of one sample from the rows held -- the arithmetic of k_fm_forward: S (every lane group ends with it), the
// bi-interaction vector (returned) and its sum sbi, and the first-order sum fo
template <int LPR, int NP>
__device__ __forceinline__ float4 walk_forward(const RowRegs (&row)[NP], const float (&x)[NP], const bool (&ok)[NP], int lane, float4 &S,
                                               float &sbi, float &fo) {
  float4 s = splat(0.f), ss = splat(0.f);
  fo = 0.f;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    if (ok[p]) {
      const float4 e = x[p] * row[p].v;
      s = s + e;
      ss = ss + e * e;
      fo += row[p].fo.x * x[p];
    }
  }
  fm_field_sums<LPR>(s, ss, fo, lane);
  const float4 bi = fm_bi<LPR>(s, ss, sbi);
  fo = __shfl(fo, 0);
  S = s;
  return bi;
}

// The fit of a step of T samples from the rows held: k_fm_update on a batch of T (inv_b = 1).  terms(t, p, cV, cA, cw) gives the
// terms the occurrence of sample t in the lane group's field of pass p adds to its run's sums, as update_body forms them.
// T = 1: every row is a run of one occurrence and takes its terms as they are.  T = 2: per field the sorted list holds the two
// occurrences by (row, sample); the same valid row is ONE run summed from zero in sample order, (0 + c_0) + c_1, and takes one
// update_row; otherwise two runs of one, each 0 + c.  (c and 0 + c differ where c is -0, and apply_rule hands the sign of a zero
// gradient on to a zero parameter: each T keeps the form of the batched launch it stands for.)
template <int LAYOUT, int RULE, int T, int NP, class Terms>
__device__ __forceinline__ void walk_fit(const WalkTable &t, const WalkFields<NP> &f, const uint32_t (&li)[T][NP], const bool (&ok)[T][NP],
                                         const RowRegs (&row)[T][NP], int q, int kp, const fmx_hyper_t &h, Terms terms) {
  static_assert(T == 1 || T == 2, "a step of one or two samples");
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    float4 cV[T], cA[T];
    float cw[T];
    float *rp[T];
#pragma unroll
    for (int s = 0; s < T; ++s) {
      terms(s, p, cV[s], cA[s], cw[s]);
      rp[s] = t.rows + (size_t)(f.lo[p] + li[s][p]) * t.stride;
    }
    if constexpr (T == 1) {
      if (ok[0][p]) update_row<LAYOUT, RULE>(rp[0], q, kp, t.zoff, row[0][p], cV[0], cA[0], cw[0], h);
    } else if (ok[0][p] && ok[1][p] && li[0][p] == li[1][p]) {  // one run of two occurrences, in sample order
      update_row<LAYOUT, RULE>(rp[0], q, kp, t.zoff, row[0][p], (splat(0.f) + cV[0]) + cV[1], (splat(0.f) + cA[0]) + cA[1],
                               (0.f + cw[0]) + cw[1], h);
    } else {
#pragma unroll
      for (int s = 0; s < T; ++s)
        if (ok[s][p]) update_row<LAYOUT, RULE>(rp[s], q, kp, t.zoff, row[s][p], splat(0.f) + cV[s], splat(0.f) + cA[s], 0.f + cw[s], h);
    }
  }
}

// the bias (or its (z, n), or (b, m_b, v_b)) stays in registers for the length of the stream; one lane writes it back
template <int LAYOUT>
__device__ __forceinline__ void walk_bias_load(const float *bias, float &b0, float &b1, float &b2) {
  b0 = bias[0];
  b1 = LAYOUT != FMX_LAYOUT_WEIGHTS ? bias[1] : 0.f;
  b2 = LAYOUT == FMX_LAYOUT_MOMENTS ? bias[2] : 0.f;
}
template <int LAYOUT, int RULE>
__device__ __forceinline__ void walk_bias_store(float *bias, float b0, float b1, float b2) {
  constexpr bool MOM = LAYOUT == FMX_LAYOUT_MOMENTS;
  bias[0] = b0;
  if (LAYOUT == FMX_LAYOUT_FTRL || (MOM && RULE == FMX_RULE_ADAM)) bias[1] = b1;
  if (MOM) bias[2] = b2;
}

// ---- the list walkers (k_fm_list_online, k_online_mlp_list): the sums of a run of a single-list step ----
// no_terms<T>(): the zero a run's sums of terms T start from (a kernel specialises it for its own terms)
template <class T>
__device__ __forceinline__ T no_terms();
template <>
__device__ __forceinline__ float4 no_terms<float4>() { return splat(0.f); }

// The sums of ONE run of a field's sorted list of a single-list step, added in k_fm_update's order (update_body, fmx_update.hip).
// There the list of G <= 16 occurrences is one tile; EPG consecutive positions are a lane group, which sums its part of a run one
// term after the other from zero.  A run inside one group is that sum.  A run over the groups g0 .. g1 takes, as the carry into
// g1, the segmented Hillis-Steele scan of the partials v_0 .. v_D of the groups g0 .. g1 - 1 (for off = 1, 2, 4, ...: a group at
// distance d >= off from g0 adds the OLD value of the group at d - off), and g1 adds its own terms onto that carry one by one.
// What the scan leaves at distance D is F(D) with F(0) = v_0, F(d) = B(d, h) + F(d - h), h the highest power of two <= d, and
// B(e, h) = B(e, h/2) + B(e - h/2, h/2) the balanced sum of the h partials ending at e: the blocks are the set bits of D, the
// lowest first.  add() is handed the members in list order and builds exactly that: `g` the group's sum, `s` a binary counter
// for the block under way, `F` the carry so far.  NLVL = log2 of the largest block: positions stay below 16, so D <= 16 / EPG - 2.
// T: all the terms (Terms), or the vector cV and the scalars (cA, cw) apart -- at 16 waves the kernel walks a run once for each,
// which halves the registers the walk holds.
template <int EPG, class T>
struct RunSum {
  static constexpr int NLVL = EPG == 1 ? 3 : EPG == 2 ? 2 : EPG == 4 ? 1 : 0;
  T g, F, s[NLVL > 0 ? NLVL : 1];
  int pos, first, g0, g1, D, bstart;
  // a run of L members whose first stands at position a of the sorted list
  __device__ __forceinline__ void init(int a, int L) {
    g = F = no_terms<T>();
#pragma unroll
    for (int l = 0; l < (NLVL > 0 ? NLVL : 1); ++l) s[l] = no_terms<T>();
    pos = first = a;
    g0 = a / EPG;
    g1 = (a + L - 1) / EPG;
    D = g1 - 1 - g0;
    bstart = 1;
  }
  __device__ __forceinline__ void leaf(int rel, T v) {
    if (rel == 0) {
      F = v;
      return;
    }
    const int rem = D - (bstart - 1), h = rem & -rem, n = rel - bstart;
    T carry = v;
    bool go = true;
#pragma unroll
    for (int l = 0; l < NLVL; ++l) {
      const bool bit = ((n >> l) & 1) != 0;
      if (go && bit) carry = s[l] + carry;
      if (go && !bit) {
        s[l] = carry;
        go = false;
      }
    }
    if (n == h - 1) {
      F = carry + F;
      bstart += h;
    }
  }
  __device__ __forceinline__ void add(T c, bool member) {
    if (!member) return;
    const int gi = pos / EPG;
    if (pos % EPG == 0 || pos == first) g = (gi == g1 && g1 > g0) ? F : no_terms<T>();
    g = g + c;
    if ((pos + 1) % EPG == 0 && gi < g1) leaf(gi - g0, g);
    ++pos;
  }
};

// ... and the same interface for a run that lies in one lane group or in two neighbouring ones (D <= 0 above): its terms add up
// one after the other from zero -- the group's sum, which is also the carry the second group goes on adding to
template <class T>
struct PlainSum {
  T g;
  __device__ __forceinline__ void add(T c, bool member) {
    if (member) g = g + c;
  }
};

// lane j's value for a wave-uniform j: a lane read into a scalar register, no LDS round trip
__device__ __forceinline__ float lane_f(float x, int j) { return __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(x), j)); }

// ---- the walkers with a network (k_online_mlp, k_online_mlp_pair): it lives in LDS for the length of the stream ----
// net_rule: the network's persistent rule (fmx_mlp_opt_t.rule), or -1 where the table's rule drives it; workgroup-uniform

// the network's floats per array: what the layers of an fmx_mlp_t hold
inline long long mlp_n_params(const fmx_mlp_t *mlp) {
  long long n = 0;
  for (int l = 0; l < mlp->n_layers; ++l) n += (long long)mlp->hidden * (l == 0 ? mlp->k : mlp->hidden) + mlp->hidden;
  return n;
}
// the arrays of n_params floats a walker keeps in LDS: params, then v under the network's ADAGRAD / ADAM, then m under its ADAM
__host__ __device__ inline int walk_net_arrays(int net_rule) {
  return net_rule == FMX_RULE_ADAM ? 3 : net_rule == FMX_RULE_ADAGRAD ? 2 : 1;
}
// ... copied in before the first step (OUT false) and written back after the last (OUT true), by the whole workgroup
template <bool OUT>
__device__ __forceinline__ void walk_net_stage(float *lds, float *params, const fmx_mlp_opt_t &opt, int n_params, int net_rule) {
  auto copy = [&](float *l, float *g) {
    for (int i = threadIdx.x; i < n_params; i += blockDim.x) {
      if (OUT) g[i] = l[i];
      else l[i] = g[i];
    }
  };
  copy(lds, params);
  if (walk_net_arrays(net_rule) >= 2) copy(lds + n_params, opt.v);
  if (walk_net_arrays(net_rule) >= 3) copy(lds + 2 * n_params, opt.m);
}
// ADAM's constants of step i of the call, derived by ONE lane (adam_consts, the function the host uses for a launch: same bits)
// into kc[8]: the tables' (step size, 1 - beta1, 1 - beta2), then the network's (the same and eps sqrt(1 - beta2^t))
template <int RULE>
__device__ __forceinline__ void walk_step_consts(float *kc, const fmx_hyper_t &h, const fmx_mlp_opt_t &opt, int net_rule, int i) {
  if (RULE == FMX_RULE_ADAM) adam_consts(h.lr, h.beta1, h.beta2, h.step + i + 1, kc[0], kc[1], kc[2]);
  if (net_rule == FMX_RULE_ADAM) adam_consts(opt.lr, opt.beta1, opt.beta2, opt.step + i + 1, kc[3], kc[4], kc[5], opt.eps, &kc[6]);
}
