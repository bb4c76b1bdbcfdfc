// fmx_afm_device.inc -- the device code of the attentional FM: the LDS carvings, the per-pair and per-tile device functions and the
// kernels k_afm, k_afm_reduce, k_afm_reduce_opt, k_afm_side and k_afm_online (fmx_afm.hip's header describes them), and the online
// walk afm_walk<KP, T> with its onl_ pieces, the body of k_afm_online (T = 1) and of k_afm_pair_online (T = 2).  Included inside the
// unnamed namespace of fmx_afm.hip, which launches these kernels, and of fmx_afm_pair_online.hip, whose kernel is the same walk
// in a unit of its own (with FMX_AFM_SHARED_ONLY; why: that file's header).

constexpr int AFM_TILE = 64;       // pairs per tile at most: one per lane of the wavefront
constexpr int AFM_MAX_WG = 1024;   // workgroups of a launch; with fewer samples, one workgroup per sample
constexpr int AFM_MAX_F = 64, AFM_MAX_T = 64;

inline int afm_grid(int B) { return B < AFM_MAX_WG ? B : AFM_MAX_WG; }
__host__ __device__ inline int r4(int x) { return (x + 3) & ~3; }

// LDS carving in floats (every section starts on 16 bytes): the sample's embeddings, the attention parameters (W rows padded to kp
// with zeros), the pair scores; BWD: the tile's q, dL/dq, unit coefficients and dlogit x a, the sample's dL/de, the accumulators
struct AfmLds {
  int e, W, bW, h, p, s, r, q, c, co, hr, ga, Ea, aW, ab, ah, ap, total;
};
__host__ __device__ inline AfmLds afm_lds(int F, int kp, int t, bool bwd) {
  AfmLds L;
  const int P = F * (F - 1) / 2;
  int o = 0;
  L.e = o; o += F * kp;
  L.W = o; o += t * kp;
  L.bW = o; o += r4(t);
  L.h = o; o += r4(t);
  L.p = o; o += kp;
  L.s = o; o += r4(P);
  L.r = o; o += r4(P);
  L.q = L.c = L.co = L.hr = L.ga = L.Ea = L.aW = L.ab = L.ah = L.ap = o;
  if (bwd) {
    L.q = o; o += AFM_TILE * kp;
    L.c = o; o += AFM_TILE * kp;
    L.co = o; o += r4(AFM_TILE * t);
    L.hr = o; o += r4(AFM_TILE * t);
    L.ga = o; o += AFM_TILE;
    L.Ea = o; o += F * kp;
    L.aW = o; o += t * kp;
    L.ab = o; o += r4(t);
    L.ah = o; o += r4(t);
    L.ap = o; o += kp;
  }
  L.total = o;
  return L;
}

struct AfmArgs {
  const float *rows;
  const int64_t *foff;
  const float *bias;
  const int32_t *idx;
  const float *xv;
  const float *y;
  const float *params;  // [ W (t x k) | b (t) | h (t) | p (k) ]
  float *logit, *loss, *dz;  // [B] each or null
  float *E;                  // BWD: [B, F * kp]
  float *part;               // BWD: [gridDim.x, G]
  int32_t *error;
  fmx_hyper_t h;
  int32_t B, F, k, t, stride, loss_kind, G;
  float inv_b;
};

// butterfly over the wavefront: every lane ends with the same bits (a + b == b + a at every level)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int m = 1; m < WAVE; m <<= 1) v += __shfl_xor(v, m);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int m = 1; m < WAVE; m <<= 1) v = fmaxf(v, __shfl_xor(v, m));
  return v;
}

// the next tile: pair rows [i0, i1) holding n <= AFM_TILE pairs (a row has F - 1 - i <= 63 pairs: at least one row fits)
__host__ __device__ __forceinline__ int next_tile(int F, int i0, int &n) {
  int i1 = i0;
  n = 0;
  while (i1 < F - 1 && n + (F - 1 - i1) <= AFM_TILE) {
    n += F - 1 - i1;
    ++i1;
  }
  return i1;
}

// pair `l` of the tile starting at row i0 -> (i, j)
__device__ __forceinline__ void tile_pair(int F, int i0, int l, int &i, int &j) {
  i = i0;
  while (l >= F - 1 - i) {
    l -= F - 1 - i;
    ++i;
  }
  j = i + 1 + l;
}

// the attention parameters into LDS for the whole launch, W rows and p padded to kp with zeros (thread `lane` of `nt`)
template <int KP>
__device__ __forceinline__ void stage_params(float *sm, const AfmLds &L, const float *params, int k, int t, int lane, int nt = WAVE) {
  for (int i = lane; i < t * KP; i += nt) {
    const int u = i / KP, d = i - u * KP;
    sm[L.W + i] = d < k ? params[u * k + d] : 0.f;
  }
  for (int u = lane; u < t; u += nt) {
    sm[L.bW + u] = params[t * k + u];
    sm[L.h + u] = params[t * k + t + u];
  }
  for (int d = lane; d < KP; d += nt) sm[L.p + d] = d < k ? params[t * k + 2 * t + d] : 0.f;
}

// field f of sample b (full-width rows [B, F]): x V[row] (kp floats) to dst, returns x w[row]; an index outside its field is
// an absent row (zeros) and sets the error word
template <int KP>
__device__ __forceinline__ float gather_field(const float *rows, const int64_t *foff, const int32_t *idx, const float *xv, int32_t *error,
                                              int stride, int F, int b, int f, float *dst) {
  const int64_t base = foff[f], rows_f = foff[f + 1] - base;
  const int ix = idx[(size_t)b * F + f];
  const float x = xv ? xv[(size_t)b * F + f] : 1.f;
  const bool ok = ix >= 0 && (int64_t)ix < rows_f;
  if (!ok && error) *error = 1;
  const float *rp = rows + (size_t)(base + (ok ? ix : 0)) * stride;
#pragma unroll
  for (int d = 0; d < KP; d += 4) {
    const float4 v = ok ? *reinterpret_cast<const float4 *>(rp + d) : splat(0.f);
    *reinterpret_cast<float4 *>(dst + d) = x * v;
  }
  return ok ? rp[KP] * x : 0.f;
}

// q = e_i (.) e_j; r = p . q (d ascending); s = h . relu(W q + b) (u ascending, each unit's sum d ascending from b_u)
template <int KP>
__device__ __forceinline__ void pair_terms(const float *sm, const AfmLds &L, int t, int i, int j, float (&q)[KP], float &r, float &s) {
#pragma unroll
  for (int d = 0; d < KP; d += 4) {
    const float4 a = *reinterpret_cast<const float4 *>(sm + L.e + i * KP + d);
    const float4 b = *reinterpret_cast<const float4 *>(sm + L.e + j * KP + d);
    q[d] = a.x * b.x;
    q[d + 1] = a.y * b.y;
    q[d + 2] = a.z * b.z;
    q[d + 3] = a.w * b.w;
  }
  r = 0.f;
#pragma unroll
  for (int d = 0; d < KP; ++d) r = fmaf(sm[L.p + d], q[d], r);
  s = 0.f;
  for (int u = 0; u < t; ++u) {
    float z = sm[L.bW + u];
#pragma unroll
    for (int d = 0; d < KP; ++d) z = fmaf(sm[L.W + u * KP + d], q[d], z);
    s = fmaf(sm[L.h + u], fmaxf(z, 0.f), s);
  }
}

// every pair's s and p . q of the F embeddings in LDS, tile by tile, into L.s / L.r in pair order; wave `wv` of `nw` takes the
// tiles wv, wv + nw, ... (a pair's terms depend on nothing but the pair)
template <int KP>
__device__ __forceinline__ void score_pairs(float *sm, const AfmLds &L, int F, int t, int lane, int wv = 0, int nw = 1) {
  for (int i0 = 0, pb = 0, tile = 0; i0 < F - 1; ++tile) {
    int n;
    const int i1 = next_tile(F, i0, n);
    if (tile % nw == wv && lane < n) {
      int i, j;
      tile_pair(F, i0, lane, i, j);
      float q[KP], r, s;
      pair_terms<KP>(sm, L, t, i, j, q, r, s);
      sm[L.s + pb + lane] = s;
      sm[L.r + pb + lane] = r;
    }
    pb += n;
    i0 = i1;
  }
}

// where one tile's backward terms lie in LDS: q and dL/dq [64, kp], the unit coefficients dL/dz and dL/dh's terms [64, t], dL/dr [64]
struct AfmTileBuf {
  int q, c, co, hr, ga;
};

// the backward of pair (i, j), slot `lane` of its tile: ex = exp(s_ij - max), Z the softmax's sum, g = dlogit, att = p . sum a q.
// The pair's terms are recomputed and q, dL/dq and the per-unit coefficients go to the tile's buffers T
template <int KP>
__device__ __forceinline__ void pair_backward(float *sm, const AfmLds &L, const AfmTileBuf &T, int t, int i, int j, int lane, float ex,
                                              float Z, float g, float att) {
  float q[KP], r, s;
  pair_terms<KP>(sm, L, t, i, j, q, r, s);
  const float ai = ex / Z;
  const float ga = g * ai;              // dL/dr_ij
  const float delta = ga * (r - att);   // dL/ds_ij
  float dq[KP];
#pragma unroll
  for (int d = 0; d < KP; ++d) dq[d] = ga * sm[L.p + d];
  for (int u = 0; u < t; ++u) {
    float z = sm[L.bW + u];
#pragma unroll
    for (int d = 0; d < KP; ++d) z = fmaf(sm[L.W + u * KP + d], q[d], z);
    const float co = z > 0.f ? delta * sm[L.h + u] : 0.f;  // dL/dz_u
    sm[T.co + lane * t + u] = co;
    sm[T.hr + lane * t + u] = delta * fmaxf(z, 0.f);       // dL/dh_u's term
#pragma unroll
    for (int d = 0; d < KP; ++d) dq[d] = fmaf(co, sm[L.W + u * KP + d], dq[d]);
  }
#pragma unroll
  for (int d = 0; d < KP; d += 4) {
    *reinterpret_cast<float4 *>(sm + T.q + lane * KP + d) = float4{q[d], q[d + 1], q[d + 2], q[d + 3]};
    *reinterpret_cast<float4 *>(sm + T.c + lane * KP + d) = float4{dq[d], dq[d + 1], dq[d + 2], dq[d + 3]};
  }
  sm[T.ga + lane] = ga;
}

// the tile of pair rows [i0, i1) (n pairs, its terms in T) added into the accumulators in pair order; thread `tid` of `nt` owns the
// accumulators tid, tid + nt, ... of each kind, so an accumulator's terms arrive in the same order whatever nt is
template <int KP>
__device__ __forceinline__ void add_tile(float *sm, const AfmLds &L, const AfmTileBuf &T, int F, int t, int i0, int i1, int n, int tid,
                                         int nt) {
  for (int l = tid; l < t * KP; l += nt) {  // dW[u][d] += sum_pairs dL/dz_u q_d
    const int u = l / KP, d = l - u * KP;
    float acc = sm[L.aW + l];
    for (int m = 0; m < n; ++m) acc = fmaf(sm[T.co + m * t + u], sm[T.q + m * KP + d], acc);
    sm[L.aW + l] = acc;
  }
  for (int u = tid; u < t; u += nt) {
    float ab = sm[L.ab + u], ah = sm[L.ah + u];
    for (int m = 0; m < n; ++m) {
      ab += sm[T.co + m * t + u];
      ah += sm[T.hr + m * t + u];
    }
    sm[L.ab + u] = ab;
    sm[L.ah + u] = ah;
  }
  for (int d = tid; d < KP; d += nt) {
    float ap = sm[L.ap + d];
    for (int m = 0; m < n; ++m) ap = fmaf(sm[T.ga + m], sm[T.q + m * KP + d], ap);
    sm[L.ap + d] = ap;
  }
  // dL/de_f[d]: the pairs (i, f), i < f, then (f, j), j > f -- the pair order, whatever the tiling
  for (int l = tid; l < F * KP; l += nt) {
    const int f = l / KP, d = l - f * KP;
    float acc = sm[L.Ea + l];
    int lb = 0;  // tile-local index of row i's first pair
    for (int i = i0; i < i1 && i <= f; lb += F - 1 - i, ++i) {
      if (i < f) {
        acc = fmaf(sm[T.c + (lb + f - i - 1) * KP + d], sm[L.e + i * KP + d], acc);
      } else {
        for (int jj = i + 1; jj < F; ++jj) acc = fmaf(sm[T.c + (lb + jj - i - 1) * KP + d], sm[L.e + jj * KP + d], acc);
      }
    }
    sm[L.Ea + l] = acc;
  }
}

template <int KP, bool FTRL, bool BWD>
__global__ __launch_bounds__(64) void k_afm(AfmArgs a) {
  extern __shared__ float4 lds4[];
  float *sm = reinterpret_cast<float *>(lds4);
  const int lane = threadIdx.x;
  const int F = a.F, k = a.k, t = a.t, P = F * (F - 1) / 2;
  const AfmLds L = afm_lds(F, KP, t, BWD);
  stage_params<KP>(sm, L, a.params, k, t, lane);
  if (BWD) {
    for (int i = lane; i < t * KP; i += WAVE) sm[L.aW + i] = 0.f;
    for (int u = lane; u < t; u += WAVE) sm[L.ab + u] = sm[L.ah + u] = 0.f;
    for (int d = lane; d < KP; d += WAVE) sm[L.ap + d] = 0.f;
  }
  const float bias_w = FTRL ? ftrl_w(a.bias[0], a.bias[1], a.h) : a.bias[0];

  for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
    // ---- gather: lane f loads field f's row (an index outside its field: the row is absent, the error word says so) ----
    float fo = 0.f;
    if (lane < F) fo = gather_field<KP>(a.rows, a.foff, a.idx, a.xv, a.error, a.stride, F, b, lane, sm + L.e + lane * KP);
    fo = wave_sum(fo);
    __syncthreads();

    // ---- pass A: every pair's score s and p . q ----
    score_pairs<KP>(sm, L, F, t, lane);
    __syncthreads();

    // ---- softmax over the sample's pairs (max-subtracted); the logit, loss and dlogit ----
    float mx = -INFINITY;
    for (int l = lane; l < P; l += WAVE) mx = fmaxf(mx, sm[L.s + l]);
    mx = wave_max(mx);
    float Z = 0.f, N = 0.f;
    for (int l = lane; l < P; l += WAVE) {
      const float ex = expf(sm[L.s + l] - mx);
      sm[L.s + l] = ex;  // (this lane's own slots: read by the other lanes after the barrier below)
      Z += ex;
      N += ex * sm[L.r + l];
    }
    Z = wave_sum(Z);
    N = wave_sum(N);
    const float att = N / Z;  // p . sum_ij a_ij q_ij
    const float logit = (bias_w + fo) + att;
    float loss = 0.f, g = 0.f;
    if (a.loss_kind != FMX_LOSS_NONE) bce_loss_dz(a.loss_kind, logit, a.y[b], a.inv_b, loss, g);
    if (lane == 0) {
      if (a.logit) a.logit[b] = logit;
      if (a.loss) a.loss[b] = loss;
      if (a.dz) a.dz[b] = g;
    }
    if (!BWD) {
      __syncthreads();  // the next sample's gather overwrites e
      continue;
    }

    // ---- pass B: recompute every tile's pairs, then add the tile into the owned accumulators in pair order ----
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
    // dL/dV_row = x dL/de
    float *Eb = a.E + (size_t)b * F * KP;
    for (int l = lane * 4; l < F * KP; l += WAVE * 4) {
      const int f = l / KP;
      const float x = a.xv ? a.xv[(size_t)b * F + f] : 1.f;
      *reinterpret_cast<float4 *>(Eb + l) = x * *reinterpret_cast<const float4 *>(sm + L.Ea + l);
    }
    __syncthreads();
  }
  if (!BWD) return;
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

// column g's sum over the n workgroups' partials, workgroup order: 4 quarters of 64 columns per workgroup, then the quarters in
// order; the value is returned to the threads of quarter 0 with g < G (the others return 0)
__device__ __forceinline__ float afm_reduce_column(const float *part, int n, int G, float (&sm)[4][64]) {
  const int c = threadIdx.x & 63, qt = threadIdx.x >> 6;
  const int g = blockIdx.x * 64 + c;
  float acc = 0.f;
  if (g < G) {
    constexpr int U = 8;
    for (int w0 = qt; w0 < n; w0 += 4 * U) {
      float v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int w = w0 + 4 * u;
        v[u] = w < n ? part[(size_t)w * G + g] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) acc += v[u];
    }
  }
  sm[qt][c] = acc;
  __syncthreads();
  return qt == 0 && g < G ? ((sm[0][c] + sm[1][c]) + sm[2][c]) + sm[3][c] : 0.f;
}

#ifndef FMX_AFM_SHARED_ONLY  // (the one kernel here that is no template: emitted by fmx_afm.hip alone)
// grad[g] = column g's sum
__global__ __launch_bounds__(256) void k_afm_reduce(const float *part, int n, int G, float *grad) {
  __shared__ float sm[4][64];
  const int g = blockIdx.x * 64 + (threadIdx.x & 63);
  const float s = afm_reduce_column(part, n, G, sm);
  if ((threadIdx.x >> 6) == 0 && g < G) grad[g] = s;
}
#endif

// ... and the attention parameters under their rule in the same pass: the thread that holds column g's sum applies RULE to
// (params[g], m[g], v[g]), requested ahead of the sum, and stores them.  Every parameter moves on every step, a zero gradient
// included (dense Adam: the moments keep decaying).  h: what apply_rule / moments_upd read (afm_opt_args).
struct AfmOptArgs {
  float *params, *m, *v;
  fmx_hyper_t h;
};
// the attention parameters' rule on one column: (p, m, v) by its gradient s
template <int RULE>
__device__ __forceinline__ void afm_opt_column(float &p, float &m, float &v, float s, const fmx_hyper_t &h) {
  if (RULE == FMX_RULE_ADAGRAD || RULE == FMX_RULE_ADAM) moments_upd<RULE>(p, m, v, s, h);
  else p = apply_rule<RULE>(p, s, h);
}
template <int RULE>
__global__ __launch_bounds__(256) void k_afm_reduce_opt(const float *part, int n, int G, float *grad, AfmOptArgs o) {
  __shared__ float sm[4][64];
  const int g = blockIdx.x * 64 + (threadIdx.x & 63);
  const bool mine = (threadIdx.x >> 6) == 0 && g < G;
  float p = 0.f, m = 0.f, v = 0.f;
  if (mine) {
    p = o.params[g];
    if (RULE == FMX_RULE_ADAGRAD || RULE == FMX_RULE_ADAM) v = o.v[g];
    if (RULE == FMX_RULE_ADAM) m = o.m[g];
  }
  const float s = afm_reduce_column(part, n, G, sm);
  if (!mine) return;
  grad[g] = s;
  afm_opt_column<RULE>(p, m, v, s, o.h);
  if (RULE == FMX_RULE_ADAGRAD || RULE == FMX_RULE_ADAM) o.v[g] = v;
  if (RULE == FMX_RULE_ADAM) o.m[g] = m;
  o.params[g] = p;
}

// fmx_afm_side: one side of a recommendation (the context fields or the item fields of full-width rows)
struct AfmSideArgs {
  const float *rows;
  const int64_t *foff;
  const float *bias;
  const int32_t *idx;
  const float *xv;
  const float *params;
  float *E;      // [R, n, kp]
  float *stats;  // [R, 4]: (lin, m, Z, R)
  int32_t *error;
  fmx_hyper_t h;
  int32_t R, F, n, k, t, stride, with_bias;
  int8_t fields[AFM_MAX_F];
};

// k_afm's forward on the n selected fields of each row alone: lane l gathers field fields[l] (k_afm's gather), pass A over the
// n (n - 1) / 2 pairs of the selected fields in pair order, then the max-subtracted sums of k_afm's softmax.  One wavefront per
// row and nothing shared between rows: a row's results do not depend on R or on the other rows.
template <int KP, bool FTRL>
__global__ __launch_bounds__(64) void k_afm_side(AfmSideArgs a) {
  extern __shared__ float4 lds4[];
  float *sm = reinterpret_cast<float *>(lds4);
  const int lane = threadIdx.x;
  const int n = a.n, t = a.t, P = n * (n - 1) / 2;
  const AfmLds L = afm_lds(n, KP, t, false);
  stage_params<KP>(sm, L, a.params, a.k, t, lane);
  const float bias_w = !a.with_bias ? 0.f : FTRL ? ftrl_w(a.bias[0], a.bias[1], a.h) : a.bias[0];
  for (int b = blockIdx.x; b < a.R; b += gridDim.x) {
    float fo = 0.f;
    if (lane < n) fo = gather_field<KP>(a.rows, a.foff, a.idx, a.xv, a.error, a.stride, a.F, b, a.fields[lane], sm + L.e + lane * KP);
    fo = wave_sum(fo);
    __syncthreads();
    score_pairs<KP>(sm, L, n, t, lane);
    __syncthreads();
    float mx = -INFINITY;
    for (int l = lane; l < P; l += WAVE) mx = fmaxf(mx, sm[L.s + l]);
    mx = wave_max(mx);
    float Z = 0.f, N = 0.f;
    for (int l = lane; l < P; l += WAVE) {
      const float ex = expf(sm[L.s + l] - mx);
      Z += ex;
      N += ex * sm[L.r + l];
    }
    Z = wave_sum(Z);
    N = wave_sum(N);
    if (lane == 0)
      *reinterpret_cast<float4 *>(a.stats + (size_t)b * 4) = float4{a.with_bias ? bias_w + fo : fo, mx, Z, N};
    float *Eb = a.E + (size_t)b * n * KP;
    for (int l = lane * 4; l < n * KP; l += WAVE * 4) *reinterpret_cast<float4 *>(Eb + l) = *reinterpret_cast<const float4 *>(sm + L.e + l);
    __syncthreads();  // the next row's gather overwrites e
  }
}

// ------------------------------------------------------------------------------------------------------------
// k_afm_online: the online predict-then-fit loop of the AFM on a device-resident stream (fmx_afm_online_run)
// ------------------------------------------------------------------------------------------------------------
// Steps of one sample are sequential (sample i + 1 reads the rows and the attention parameters sample i wrote), so ONE workgroup
// walks the stream and the work INSIDE a sample is spread over its AFM_ONL_WAVES waves; every float is the one fmx_afm_step_opt
// gives at B = 1, inv_b = 1 (k_afm on one sample, k_fm_update_occ on F runs of one occurrence, k_afm_reduce_opt over one partial):
//   gather   LPR = kp / 4 threads per field: the row by sc1 loads (the previous sample may have written it) into registers, where
//            it stays for the update; e = x V and x w to LDS
//   pass A   the pair tiles dealt over the waves (score_pairs)
//   softmax  every wave evaluates k_afm's one-wave max and sums itself (the same lanes, the same order) and so holds the logit,
//            the loss and dlogit without a broadcast; the exponentials are shared out over all threads in between
//   pass B   rounds of nb tiles: wave w recomputes tile w of the round into tile buffer w (pair_backward), then every thread adds
//            the round's tiles, in tile order, into the accumulators it owns (add_tile: the t kp + 2 t + kp attention entries and
//            the F kp entries of dL/de over all the threads instead of k_afm's 64 lanes; an accumulator's terms still arrive in
//            pair order)
//   update   the attention parameters live in LDS for the whole stream (their moments too where they fit, else in global memory,
//            touched by the owning thread alone): column g's owner applies the rule to 0 + its accumulator -- afm_reduce_column
//            over ONE workgroup's partial, which turns a -0 into +0 -- and the threads that hold the rows apply the tables' rule
//            to dL/dV = 0 + x dL/de, dL/dw = 0 + x dlogit (update_body's run of one occurrence); thread 0 steps the bias words,
//            which stay in LDS.  The stores are acknowledged (vmcnt(0)) and a barrier passed before the next sample's gather.
// ADAM's constants of sample i -- step hyper.step + i + 1 of the tables, opt.step + i + 1 of the attention parameters -- are
// derived by one thread per sample with adam_consts, the function the host uses for a launch (same bits), as in k_online_mlp.
// The kernel is afm_walk<KP, 1> below; k_afm_pair_online (fmx_afm_pair_online.hip) is afm_walk<KP, 2>, the same walk with two rows
// in every slot.  What the two share -- prologue, fetch, ADAM's constants, forward and softmax, pass B, the attention rule, the bias
// step, the epilogue -- is one onl_ function each; the objective and the table update's run logic are the walk's `if constexpr` parts.
constexpr int AFM_ONL_WAVES = 8, AFM_ONL_THREADS = AFM_ONL_WAVES * WAVE;  // 2 waves per SIMD: 256 VGPRs each (pair_backward at
                                                                          // kp = 64 holds q and dL/dq: 128 registers)
constexpr int AFM_LDS_BYTES = 160 * 1024;

// LDS carving in floats: k_afm's sections (L) with the accumulators [ dL/de | dW | db | dh | dp ] in one run, the exponentials,
// the fields' x w, (bias words | ADAM's constants | the index flag), nb tile buffers and, when they fit, the moments
struct AfmOnlLds {
  AfmLds L;
  int x, fo, misc, acc_len, tile0, tile_sz, m, v, total;
};
constexpr int ONL_KC = 4, ONL_FLAG = 12, ONL_MISC = 16;  // offsets inside misc
__host__ __device__ inline int afm_tile_floats(int kp, int t) { return 2 * AFM_TILE * kp + 2 * r4(AFM_TILE * t) + AFM_TILE; }
__host__ __device__ inline AfmOnlLds afm_online_lds(int F, int kp, int t, int G, int nb, bool mom) {
  AfmOnlLds O;
  AfmLds &L = O.L;
  const int P = F * (F - 1) / 2;
  int o = 0;
  L.e = o; o += F * kp;
  L.W = o; o += t * kp;
  L.bW = o; o += r4(t);
  L.h = o; o += r4(t);
  L.p = o; o += kp;
  L.s = o; o += r4(P);
  L.r = o; o += r4(P);
  O.x = o; o += r4(P);
  L.Ea = o; o += F * kp;
  L.aW = o; o += t * kp;
  L.ab = o; o += r4(t);
  L.ah = o; o += r4(t);
  L.ap = o; o += kp;
  O.acc_len = o - L.Ea;
  O.fo = o; o += WAVE;
  O.misc = o; o += ONL_MISC;
  O.tile0 = o;
  O.tile_sz = afm_tile_floats(kp, t);
  o += nb * O.tile_sz;
  L.q = L.c = L.co = L.hr = L.ga = O.tile0;  // (buffer 0; tile_buf gives each buffer's sections)
  O.m = O.v = o;
  if (mom) {
    O.m = o; o += r4(G);
    O.v = o; o += r4(G);
  }
  O.total = L.total = o;
  return O;
}
__device__ __forceinline__ AfmTileBuf tile_buf(const AfmOnlLds &O, int kp, int t, int b) {
  AfmTileBuf T;
  T.q = O.tile0 + b * O.tile_sz;
  T.c = T.q + AFM_TILE * kp;
  T.co = T.c + AFM_TILE * kp;
  T.hr = T.co + r4(AFM_TILE * t);
  T.ga = T.hr + r4(AFM_TILE * t);
  return T;
}
// the pair tiles of a sample
inline int afm_n_tiles(int F) {
  int nt = 0;
  for (int i0 = 0, n; i0 < F - 1; ++nt) i0 = next_tile(F, i0, n);
  return nt;
}
// tile buffers of the one-workgroup form at this shape: as many as waves, tiles and the LDS allow; the moments go to LDS too when
// that costs no buffer.  0: the form is not used -- not even two tiles' buffers fit beside the sample, so the pair work could not
// be spread over waves
inline int afm_online_buffers(int F, int kp, int t, int G, bool want_mom, bool &mom) {
  const int tiles = afm_n_tiles(F), most = tiles < AFM_ONL_WAVES ? tiles : AFM_ONL_WAVES, least = tiles < 2 ? tiles : 2;
  auto fits = [&](int nb, bool mo) { return (size_t)afm_online_lds(F, kp, t, G, nb, mo).total * 4 <= (size_t)AFM_LDS_BYTES; };
  mom = false;
  int nb = most;
  while (nb >= least && !fits(nb, false)) --nb;
  if (nb < least) return 0;
  mom = want_mom && fits(nb, true);
  return nb;
}

struct AfmOnlArgs {
  float *rows;
  const int64_t *foff;
  float *bias;
  const int32_t *idx;  // [N, F]
  const float *xv;     // [N, F] or null
  const float *y;      // [N]
  float *params, *m, *v;  // the attention parameters and their moments (m, v: as the rule needs them)
  float *grad;            // [G] the last sample's attention gradient
  float *logit, *loss;    // [N] each or null
  int32_t *error;
  fmx_hyper_t h;  // the tables' (alpha holds 1 / alpha); ADAM: lr, beta1, beta2, step as the caller gave them
  float o_lr, o_eps, o_beta1, o_beta2;  // the attention parameters' (fmx_mlp_opt_t)
  int32_t o_rule, o_step;
  int32_t N, F, k, t, stride, zoff, rule, G, nb, mom_lds;
};
// ... filled for a stream of N units in the form afm_online_buffers gave (nb > 0 tile buffers, the moments in LDS or not); y:
// null for the pairs.  ADAM: the kernel derives each unit's constants from lr, beta1, beta2, step of `hyper` and `opt`
inline AfmOnlArgs fill_afm_online(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_afm_t *afm,
                                  const fmx_mlp_opt_t *opt, const int32_t *idx, const float *xv, const float *y, int32_t N,
                                  float *attn_grad_out, float *logit_out, float *loss_out, int32_t *error, int nb, bool moments_in_lds) {
  AfmOnlArgs a;
  memset(&a, 0, sizeof(a));
  a.rows = table->rows;
  a.foff = table->field_offsets;
  a.bias = table->bias;
  a.idx = idx;
  a.xv = xv;
  a.y = y;
  a.params = afm->params;
  a.m = opt->m;
  a.v = opt->v;
  a.grad = attn_grad_out;
  a.logit = logit_out;
  a.loss = loss_out;
  a.error = error;
  a.h = kernel_hyper(hyper, rule);
  a.o_lr = opt->lr;
  a.o_eps = opt->eps;
  a.o_beta1 = opt->beta1;
  a.o_beta2 = opt->beta2;
  a.o_rule = opt->rule;
  a.o_step = opt->step;
  a.N = N;
  a.F = table->n_fields;
  a.k = afm->k;
  a.t = afm->t;
  a.stride = table->row_stride;
  a.zoff = table->z_offset;
  a.rule = rule;
  a.G = afm->t * afm->k + 2 * afm->t + afm->k;
  a.nb = nb;
  a.mom_lds = moments_in_lds ? 1 : 0;
  return a;
}
// the form an online run takes: `option` (the entry point's "..._persistent" option) on: afm_online_buffers' tile buffers for the
// one-workgroup kernel, mom: its moments in LDS; off, or 0 buffers: the queued steps
inline int afm_online_form(int option, int F, int k, int kp, int t, int attn_rule, bool &mom) {
  mom = false;
  return option ? afm_online_buffers(F, kp, t, t * k + 2 * t + k, attn_rule == FMX_RULE_ADAGRAD || attn_rule == FMX_RULE_ADAM, mom) : 0;
}
// the launch of a walker K (k_afm_online<KP> or k_afm_pair_online<KP>; o: the AfmOnlArgs of its arguments): one workgroup
template <int KP, auto K, class Args>
int launch_afm_walk_k(const Args &args, const AfmOnlArgs &o, const char *name, hipStream_t st) {
  const size_t lds = (size_t)afm_online_lds(o.F, KP, o.t, o.G, o.nb, o.mom_lds != 0).total * 4;
  if (int rc = raise_lds_limit<K>(AFM_LDS_BYTES, name)) return rc;
  hipLaunchKernelGGL(K, dim3(1), dim3(AFM_ONL_THREADS), lds, st, args);
  return check_launch(name);
}

// the tables' rule is a workgroup-uniform run-time switch around the row helpers (a template parameter would multiply the five
// kp instantiations by five for a few instructions per sample)
__device__ __forceinline__ RowRegs onl_load_row(int rule, const float *rp, int q, int kp, int zoff) {
  switch (rule) {
    case FMX_RULE_FTRL: return load_row_sc1<FMX_LAYOUT_FTRL, FMX_RULE_FTRL>(rp, q, kp, zoff);
    case FMX_RULE_ADAGRAD: return load_row_sc1<FMX_LAYOUT_MOMENTS, FMX_RULE_ADAGRAD>(rp, q, kp, zoff);
    case FMX_RULE_ADAM: return load_row_sc1<FMX_LAYOUT_MOMENTS, FMX_RULE_ADAM>(rp, q, kp, zoff);
    default: return load_row_sc1<FMX_LAYOUT_WEIGHTS, FMX_RULE_SGD>(rp, q, kp, zoff);
  }
}
__device__ __forceinline__ void onl_update_row(int rule, float *rp, int q, int kp, int zoff, const RowRegs &r, float4 cV, float cw,
                                               const fmx_hyper_t &h) {
  const float4 cA = splat(0.f);
  switch (rule) {
    case FMX_RULE_SIGNADAM: update_row<FMX_LAYOUT_WEIGHTS, FMX_RULE_SIGNADAM>(rp, q, kp, zoff, r, cV, cA, cw, h); break;
    case FMX_RULE_SGD: update_row<FMX_LAYOUT_WEIGHTS, FMX_RULE_SGD>(rp, q, kp, zoff, r, cV, cA, cw, h); break;
    case FMX_RULE_FTRL: update_row<FMX_LAYOUT_FTRL, FMX_RULE_FTRL>(rp, q, kp, zoff, r, cV, cA, cw, h); break;
    case FMX_RULE_ADAGRAD: update_row<FMX_LAYOUT_MOMENTS, FMX_RULE_ADAGRAD>(rp, q, kp, zoff, r, cV, cA, cw, h); break;
    default: update_row<FMX_LAYOUT_MOMENTS, FMX_RULE_ADAM>(rp, q, kp, zoff, r, cV, cA, cw, h); break;
  }
}
__device__ __forceinline__ void onl_bias_step(int rule, float &b0, float &b1, float &b2, float g, const fmx_hyper_t &h) {
  switch (rule) {
    case FMX_RULE_SIGNADAM: bias_step<FMX_LAYOUT_WEIGHTS, FMX_RULE_SIGNADAM>(b0, b1, b2, g, h); break;
    case FMX_RULE_SGD: bias_step<FMX_LAYOUT_WEIGHTS, FMX_RULE_SGD>(b0, b1, b2, g, h); break;
    case FMX_RULE_FTRL: bias_step<FMX_LAYOUT_FTRL, FMX_RULE_FTRL>(b0, b1, b2, g, h); break;
    case FMX_RULE_ADAGRAD: bias_step<FMX_LAYOUT_MOMENTS, FMX_RULE_ADAGRAD>(b0, b1, b2, g, h); break;
    default: bias_step<FMX_LAYOUT_MOMENTS, FMX_RULE_ADAM>(b0, b1, b2, g, h); break;
  }
}
// column g of [ W (t x k) | b | h | p ] -> its offset from L.W / L.aW's section starts (W rows are padded to kp in LDS)
__device__ __forceinline__ void onl_column(const AfmLds &L, int g, int k, int t, int kp, int &par, int &acc) {
  if (g < t * k) {
    const int u = g / k, d = g - u * k;
    par = L.W + u * kp + d;
    acc = L.aW + u * kp + d;
  } else if (g < t * k + t) {
    par = L.bW + (g - t * k);
    acc = L.ab + (g - t * k);
  } else if (g < t * k + 2 * t) {
    par = L.h + (g - t * k - t);
    acc = L.ah + (g - t * k - t);
  } else {
    par = L.p + (g - t * k - 2 * t);
    acc = L.ap + (g - t * k - 2 * t);
  }
}

// ---- the pieces of the walk (afm_walk below), each stated once for k_afm_online and k_afm_pair_online ----
constexpr int onl_slots(int kp) { return (AFM_MAX_F * (kp / 4) + AFM_ONL_THREADS - 1) / AFM_ONL_THREADS; }
// the workgroup-uniform facts of the two rules
struct OnlRules {
  bool ftrl, mom_rule;  // the tables': FTRL rows; rows with moments (ADAGRAD, ADAM)
  bool o_v, o_m;        // the attention parameters' rule keeps v; keeps m
};
__device__ __forceinline__ OnlRules onl_rules(const AfmOnlArgs &a) {
  return {a.rule == FMX_RULE_FTRL, a.rule == FMX_RULE_ADAGRAD || a.rule == FMX_RULE_ADAM,
          a.o_rule == FMX_RULE_ADAGRAD || a.o_rule == FMX_RULE_ADAM, a.o_rule == FMX_RULE_ADAM};
}
// the slots a thread gathers and updates: slot rr = tid + p NT is lanes q of field f, for each of the unit's samples (kp = 64:
// 64 fields x 16 threads over 512, two slots a thread)
template <int NP>
struct OnlSlots {
  int fld[NP], qq[NP];
  int64_t lo[NP];
  uint32_t vocab[NP];
  bool live[NP];
};
template <int KP>
__device__ __forceinline__ OnlSlots<onl_slots(KP)> onl_slot_table(const AfmOnlArgs &a) {
  constexpr int NT = AFM_ONL_THREADS, LPR = KP / 4, NP = onl_slots(KP);
  const int tid = threadIdx.x;
  OnlSlots<NP> S;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int rr = tid + p * NT;
    S.fld[p] = rr / LPR;
    S.qq[p] = rr - S.fld[p] * LPR;
    S.live[p] = S.fld[p] < a.F;
    S.lo[p] = S.live[p] ? a.foff[S.fld[p]] : 0;
    S.vocab[p] = S.live[p] ? (uint32_t)(a.foff[S.fld[p] + 1] - S.lo[p]) : 0u;
  }
  return S;
}
// the (index, value) a slot holds of each of the T samples of a unit
template <int T, int NP>
struct OnlInputs {
  uint32_t li[T][NP];
  float x[T][NP];
};

// The prologue: the attention parameters, the x w words, the bias words and (where they fit: a.mom_lds) the moments to LDS.  mm /
// vv name the moments wherever they are: in LDS for the whole stream, or left in global memory (the same code through a generic
// pointer).  (The walk builds its slot table BEHIND this call, as the kernels did.  With the table in front of it the pair walker
// at kp = 16 and the pointwise walker at kp = 64 measured 4 - 7 % slower per unit -- profiles/afm_walk_seam_ab.txt, B.)
template <int KP>
__device__ __forceinline__ void onl_open(const AfmOnlArgs &a, const OnlRules &R, const AfmOnlLds &O, float *sm, float *&mm, float *&vv) {
  constexpr int NT = AFM_ONL_THREADS;
  const int tid = threadIdx.x;
  stage_params<KP>(sm, O.L, a.params, a.k, a.t, tid, NT);
  if (tid < WAVE) sm[O.fo + tid] = 0.f;
  if (tid < ONL_MISC) sm[O.misc + tid] = 0.f;
  __syncthreads();
  if (tid == 0) {
    sm[O.misc] = a.bias[0];
    if (R.ftrl || R.mom_rule) sm[O.misc + 1] = a.bias[1];
    if (R.mom_rule) sm[O.misc + 2] = a.bias[2];
  }
  mm = a.mom_lds ? sm + O.m : a.m;
  vv = a.mom_lds ? sm + O.v : a.v;
  if (a.mom_lds) {
    for (int g = tid; g < a.G; g += NT) {
      if (R.o_m) mm[g] = a.m[g];
      if (R.o_v) vv[g] = a.v[g];
    }
  }
}

// The next unit's inputs, rows T i .. T i + T - 1 of the stream.  Branch-free (k_fm_online): beyond the stream or the last field the
// loads read element 0 and are dropped.  xsrc: the values, or without them the indices, loaded in their place and dropped (x = 1).
// mid() stands between the loads and the selects: the unit's other load (the label) goes there, as in walk_fetch
template <int T, int NP, class Mid>
__device__ __forceinline__ void onl_fetch(OnlInputs<T, NP> &n, const AfmOnlArgs &a, const OnlSlots<NP> &S, const float *xsrc, bool has_x,
                                          int i, bool in, Mid mid) {
  uint32_t l_[T][NP];
  float x_[T][NP];
#pragma unroll
  for (int s = 0; s < T; ++s) {
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const size_t o = (S.live[p] && in) ? ((size_t)T * i + s) * a.F + S.fld[p] : (size_t)0;
      l_[s][p] = (uint32_t)a.idx[o];
      x_[s][p] = xsrc[o];
    }
  }
  mid();
#pragma unroll
  for (int s = 0; s < T; ++s) {
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      n.li[s][p] = (S.live[p] && in) ? l_[s][p] : 0u;
      n.x[s][p] = (has_x && S.live[p] && in) ? x_[s][p] : 1.f;
    }
  }
}

// ADAM's constants of unit i, by one thread into misc: [0..2] the tables', [3..6] the attention parameters'
__device__ __forceinline__ void onl_unit_consts(const AfmOnlArgs &a, const OnlRules &R, const AfmOnlLds &O, float *sm, int i) {
  if (threadIdx.x == WAVE) {
    float *kc = sm + O.misc + ONL_KC;
    if (a.rule == FMX_RULE_ADAM) adam_consts(a.h.lr, a.h.beta1, a.h.beta2, a.h.step + i + 1, kc[0], kc[1], kc[2]);
    if (R.o_m) adam_consts(a.o_lr, a.o_beta1, a.o_beta2, a.o_step + i + 1, kc[3], kc[4], kc[5], a.o_eps, &kc[6]);
  }
}

// The forward of one sample from its row registers: e = x V and x w to LDS (gather_field's products; an absent row is zeros), pass A
// over the waves, then the softmax -- k_afm's one-wave reductions in every wave, the exponentials over all threads in between.
// The exponentials stay in O.x, p . q in L.r; returns the logit, which every wave holds, with Z and att for pass B.  (A second
// forward's writes of e and x w lie behind the barrier every wave passed after reading the first's.)
template <int KP, int NP>
__device__ __forceinline__ float onl_forward(const AfmOnlArgs &a, const OnlRules &R, const AfmOnlLds &O, float *sm, const OnlSlots<NP> &S,
                                             const RowRegs (&row)[NP], const float (&x)[NP], const bool (&ok)[NP], float &Z, float &att) {
  constexpr int NT = AFM_ONL_THREADS, NW = AFM_ONL_WAVES;
  const AfmLds &L = O.L;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, P = a.F * (a.F - 1) / 2;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    if (S.live[p]) {
      *reinterpret_cast<float4 *>(sm + L.e + S.fld[p] * KP + 4 * S.qq[p]) = ok[p] ? x[p] * row[p].v : splat(0.f);
      if (S.qq[p] == 0) sm[O.fo + S.fld[p]] = ok[p] ? row[p].fo.x * x[p] : 0.f;
    }
  }
  __syncthreads();
  score_pairs<KP>(sm, L, a.F, a.t, lane, wv, NW);
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
  const float bias_w = R.ftrl ? ftrl_w(sm[O.misc], sm[O.misc + 1], a.h) : sm[O.misc];
  return (bias_w + fo) + att;
}

// Pass B of the sample whose forward is in LDS, under dlogit g, in rounds of nb tiles: wave w recomputes tile w of the round into
// tile buffer w, then every thread adds the round's tiles, in tile order, into the accumulators it owns.  Ends behind a barrier
template <int KP>
__device__ __forceinline__ void onl_pass_b(const AfmOnlArgs &a, const AfmOnlLds &O, float *sm, float Z, float g, float att) {
  const AfmLds &L = O.L;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, F = a.F, t = a.t;
  for (int i0r = 0, pbr = 0; i0r < F - 1;) {
    int i0 = i0r, pb = pbr, cnt = 0;
    for (; cnt < a.nb && i0 < F - 1; ++cnt) {
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
      add_tile<KP>(sm, L, tile_buf(O, KP, t, c), F, t, i0, i1, n, tid, AFM_ONL_THREADS);
      i0 = i1;
    }
    __syncthreads();
    i0r = i0;
    pbr = pb;
  }
}

// The attention parameters' step of unit i: column c's gradient is 0 + the one workgroup's partial (afm_reduce_column), then the
// rule, on the parameters in LDS and the moments behind mm / vv.  The last unit's gradient goes to a.grad
template <int KP>
__device__ __forceinline__ void onl_attn_rule(const AfmOnlArgs &a, const OnlRules &R, const AfmOnlLds &O, float *sm, float *mm, float *vv, int i) {
  fmx_hyper_t ho;
  ho.lr = a.o_lr;
  ho.eps = a.o_eps;
  if (R.o_m) {
    const float *kc = sm + O.misc + ONL_KC;
    ho.lr = kc[3];
    ho.beta1 = kc[4];
    ho.beta2 = kc[5];
    ho.eps = kc[6];
  }
  for (int c = threadIdx.x; c < a.G; c += AFM_ONL_THREADS) {
    int par, acc;
    onl_column(O.L, c, a.k, a.t, KP, par, acc);
    const float s = 0.f + sm[acc];
    if (i == a.N - 1) a.grad[c] = s;
    float p = sm[par], m = 0.f, v = 0.f;
    if (R.o_v) v = vv[c];
    if (R.o_m) m = mm[c];
    switch (a.o_rule) {
      case FMX_RULE_SIGNADAM: afm_opt_column<FMX_RULE_SIGNADAM>(p, m, v, s, ho); break;
      case FMX_RULE_SGD: afm_opt_column<FMX_RULE_SGD>(p, m, v, s, ho); break;
      case FMX_RULE_ADAGRAD: afm_opt_column<FMX_RULE_ADAGRAD>(p, m, v, s, ho); break;
      default: afm_opt_column<FMX_RULE_ADAM>(p, m, v, s, ho); break;
    }
    if (R.o_v) vv[c] = v;
    if (R.o_m) mm[c] = m;
    sm[par] = p;
  }
}

// the tables' hyper-parameters of the unit: ADAM's constants from misc
__device__ __forceinline__ fmx_hyper_t onl_table_hyper(const AfmOnlArgs &a, const AfmOnlLds &O, const float *sm) {
  fmx_hyper_t ht = a.h;
  if (a.rule == FMX_RULE_ADAM) {
    const float *kc = sm + O.misc + ONL_KC;
    ht.lr = kc[0];
    ht.beta1 = kc[1];
    ht.beta2 = kc[2];
  }
  return ht;
}
// thread 0 steps the bias words, which stay in LDS, on the unit's bias gradient g
__device__ __forceinline__ void onl_bias_words(const AfmOnlArgs &a, const AfmOnlLds &O, float *sm, float g, const fmx_hyper_t &ht) {
  if (threadIdx.x == 0) {
    float b0 = sm[O.misc], b1 = sm[O.misc + 1], b2 = sm[O.misc + 2];
    onl_bias_step(a.rule, b0, b1, b2, g, ht);
    sm[O.misc] = b0;
    sm[O.misc + 1] = b1;
    sm[O.misc + 2] = b2;
  }
}

// The epilogue: the attention parameters, the moments that lived in LDS, the bias words and the index flag back to global memory
template <int KP>
__device__ __forceinline__ void onl_close(const AfmOnlArgs &a, const OnlRules &R, const AfmOnlLds &O, float *sm, const float *mm, const float *vv, bool bad) {
  const int tid = threadIdx.x;
  if (bad) sm[O.misc + ONL_FLAG] = 1.f;
  for (int c = tid; c < a.G; c += AFM_ONL_THREADS) {
    int par, acc;
    onl_column(O.L, c, a.k, a.t, KP, par, acc);
    a.params[c] = sm[par];
    if (a.mom_lds) {
      if (R.o_m) a.m[c] = mm[c];
      if (R.o_v) a.v[c] = vv[c];
    }
  }
  __syncthreads();
  if (tid == 0) {
    a.bias[0] = sm[O.misc];
    if (R.ftrl || a.rule == FMX_RULE_ADAM) a.bias[1] = sm[O.misc + 1];
    if (R.mom_rule) a.bias[2] = sm[O.misc + 2];
    if (sm[O.misc + ONL_FLAG] != 0.f && a.error) *a.error = 1;
  }
}

// The walk over a stream of N units of T samples: T = 1, k_afm_online's sample under BCE on its label; T = 2, k_afm_pair_online's
// (positive, negative) rows 2 i and 2 i + 1 under pair_loss_dz on z_pos - z_neg (fmx_afm_pair_online.hip's header has what the pair
// stands for).  A slot's rows of all T samples are loaded before any update and stay in registers for the unit.  Per unit:
//   T = 1   forward; loss; pass B with g; the attention rule; every valid row is a run of one occurrence
//   T = 2   the negative's forward, then the positive's; loss; the positive's pass B with g, its x dL/de slices to registers (EP)
//           and its dL/de slots zeroed by their holders; the negative again from the row registers (k_afm_pair regathers; the rows
//           have not moved, so the bits are the same), its pass B with -g -- the attention accumulators are zeroed once per unit
//           and take the positive's tiles, then the negative's; the attention rule; a valid row both samples name in a field is
//           ONE run of two occurrences, positive first (k_fm_pair_online's run logic), otherwise each valid row is a run of one.
//           The bias gradient (0 + g) + (-g) = +0 still goes through the bias step: the moments decay on it
template <int KP, int T>
__device__ __forceinline__ void afm_walk(const AfmOnlArgs &a, float margin) {
  static_assert(T == 1 || T == 2, "a unit of one or two samples");
  constexpr int NT = AFM_ONL_THREADS, NP = onl_slots(KP);
  extern __shared__ float4 lds4[];
  float *sm = reinterpret_cast<float *>(lds4);
  const int tid = threadIdx.x;
  const AfmOnlLds O = afm_online_lds(a.F, KP, a.t, a.G, a.nb, a.mom_lds != 0);
  const AfmLds &L = O.L;
  const OnlRules R = onl_rules(a);
  float *mm, *vv;
  onl_open<KP>(a, R, O, sm, mm, vv);
  const OnlSlots<NP> S = onl_slot_table<KP>(a);
  OnlInputs<T, NP> next;
  float y_n = 0.f;
  const float *xsrc = a.xv ? a.xv : reinterpret_cast<const float *>(a.idx);
  const bool has_x = a.xv != nullptr;
  auto fetch_inputs = [&](int i) {
    const bool in = i < a.N;
    float yy = 0.f;
    onl_fetch(next, a, S, xsrc, has_x, i, in, [&] {
      if constexpr (T == 1) yy = a.y[in ? i : 0];
    });
    y_n = in ? yy : 0.f;
  };
  fetch_inputs(0);
  bool bad = false;
  __syncthreads();

  for (int i = 0; i < a.N; ++i) {
    // ---- gather: the unit's rows by sc1 loads; the next unit's inputs behind them ----
    const OnlInputs<T, NP> in = next;
    [[maybe_unused]] const float y = y_n;
    RowRegs row[T][NP];
    bool ok[T][NP];
#pragma unroll
    for (int s = 0; s < T; ++s) {
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        ok[s][p] = S.live[p] && in.li[s][p] < S.vocab[p];  // (a negative index is a large unsigned one)
        row[s][p] = onl_load_row(a.rule, a.rows + (size_t)(ok[s][p] ? S.lo[p] + in.li[s][p] : 0) * a.stride, S.qq[p], KP, a.zoff);
        bad = bad || (S.live[p] && !ok[s][p]);
      }
    }
    fetch_inputs(i + 1);
    onl_unit_consts(a, R, O, sm, i);
    // dL/de and the attention accumulators [ dW | db | dh | dp ] (one run in LDS): zero before the unit's first pass B
    for (int l = tid; l < O.acc_len; l += NT) sm[L.Ea + l] = 0.f;

    // ---- forwards; the unit's loss and dlogit in every wave, on identical operands ----
    float Z, att, loss, g;
    [[maybe_unused]] float4 EP[NP];
    if constexpr (T == 1) {
      const float logit = onl_forward<KP>(a, R, O, sm, S, row[0], in.x[0], ok[0], Z, att);
      bce_loss_dz(FMX_LOSS_BCE_LOGITS, logit, y, 1.0f, loss, g);
      if (tid == 0) {
        if (a.logit) a.logit[i] = logit;
        if (a.loss) a.loss[i] = 0.f + loss;  // the update's block_sum over one sample
      }
      onl_pass_b<KP>(a, O, sm, Z, g, att);
    } else {
      const float zn = onl_forward<KP>(a, R, O, sm, S, row[1], in.x[1], ok[1], Z, att);
      const float zp = onl_forward<KP>(a, R, O, sm, S, row[0], in.x[0], ok[0], Z, att);
      pair_loss_dz(zp - zn, margin, 1.0f, loss, g);
      if (tid == 0) {
        if (a.logit) {
          a.logit[2 * (size_t)i] = zp;
          a.logit[2 * (size_t)i + 1] = zn;
        }
        if (a.loss) a.loss[i] = (0.f + loss) + 0.f;  // the update's block_sum over the two rows: the pair's loss, then +0
      }
      onl_pass_b<KP>(a, O, sm, Z, g, att);
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        EP[p] = splat(0.f);
        if (S.live[p]) {
          float4 *ea = reinterpret_cast<float4 *>(sm + L.Ea + S.fld[p] * KP + 4 * S.qq[p]);
          EP[p] = in.x[0][p] * *ea;  // k_afm's dL/dV_row
          *ea = splat(0.f);
        }
      }
      onl_forward<KP>(a, R, O, sm, S, row[1], in.x[1], ok[1], Z, att);
      onl_pass_b<KP>(a, O, sm, Z, -g, att);
    }
    onl_attn_rule<KP>(a, R, O, sm, mm, vv, i);

    // ---- the tables: k_fm_update_occ on the unit's rows, from the registers that hold them ----
    const fmx_hyper_t ht = onl_table_hyper(a, O, sm);
    if constexpr (T == 1) {
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        if (ok[0][p]) {
          const float4 E = in.x[0][p] * *reinterpret_cast<const float4 *>(sm + L.Ea + S.fld[p] * KP + 4 * S.qq[p]);  // k_afm's dL/dV_row
          onl_update_row(a.rule, a.rows + (size_t)(S.lo[p] + in.li[0][p]) * a.stride, S.qq[p], KP, a.zoff, row[0][p], splat(0.f) + E,
                         0.f + in.x[0][p] * g, ht);
        }
      }
      onl_bias_words(a, O, sm, 0.f + g, ht);
    } else {
      const float gn = -g;
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        if (S.live[p]) {
          const float4 EN = in.x[1][p] * *reinterpret_cast<const float4 *>(sm + L.Ea + S.fld[p] * KP + 4 * S.qq[p]);
          const float cwp = in.x[0][p] * g, cwn = in.x[1][p] * gn;
          float *rp0 = a.rows + (size_t)(S.lo[p] + in.li[0][p]) * a.stride, *rp1 = a.rows + (size_t)(S.lo[p] + in.li[1][p]) * a.stride;
          if (ok[0][p] && ok[1][p] && in.li[0][p] == in.li[1][p]) {
            onl_update_row(a.rule, rp0, S.qq[p], KP, a.zoff, row[0][p], (splat(0.f) + EP[p]) + EN, (0.f + cwp) + cwn, ht);
          } else {
            if (ok[0][p]) onl_update_row(a.rule, rp0, S.qq[p], KP, a.zoff, row[0][p], splat(0.f) + EP[p], 0.f + cwp, ht);
            if (ok[1][p]) onl_update_row(a.rule, rp1, S.qq[p], KP, a.zoff, row[1][p], splat(0.f) + EN, 0.f + cwn, ht);
          }
        }
      }
      onl_bias_words(a, O, sm, (0.f + g) + gn, ht);  // exactly +0: the moments still decay
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the row stores are acknowledged ...
    __syncthreads();                                   // ... before any thread's next gather
  }
  onl_close<KP>(a, R, O, sm, mm, vv, bad);
}

template <int KP>
__global__ __launch_bounds__(AFM_ONL_THREADS) void k_afm_online(AfmOnlArgs a) {
  afm_walk<KP, 1>(a, 0.f);
}
