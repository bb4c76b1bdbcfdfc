// fmx_inbatch.hip -- in-batch sampled-softmax training of the pure FM (fmx_fm_inbatch_*, include/fmx.h): every row of a batch of B
// rows takes the other rows' items as its negatives.  With the fields split into item fields and context fields, the logit of
// (context i, item j) is the serving score of fmx_fm_topk,
//     score(i, j) = (a_u[i] + a_c[j]) + fma-chain over d ascending of S_u[i, d] S_c[j, d]        (fm_score, fmx_topk.hip)
// so the B x B logits come out of two masked forward passes of B rows each and the loss and its backward are scans over two
// [B, kp] arrays; no B x B array is stored (the gradient coefficients g_ij are recomputed from the per-row (m, s, n)).
//
// The kernels, one wave per workgroup, thread t of tile T holding row 64 T + t of ONE side in its registers while the other side's
// rows arrive as wave-uniform operands, R at a time (k_topk_scan's layout):
//   k_inbatch_scan<KP, false>   grid (tiles, splits): the maximum of c_ij over the split's eligible j -> pm [splits, B]; score_out
//   k_inbatch_scan<KP, true>    the same grid: m_i = max over pm, then s / n of the split's j -> ps, pn [splits, B]
//   k_inbatch_lse<KP>           per row: (m, s, n) merged in split order, c_ii, loss_i
//   k_inbatch_bwd<KP>           grid (tiles, splits, 2): blockIdx.z = 0 a thread per context row (gSu), 1 a thread per item row
//                               (gSc, gac): ib_bwd_body instantiated twice with the roles swapped; partial sums per split
//   k_inbatch_bwd_merge<KP>     the partial sums added in split order (not launched when there is one split)
//   k_inbatch_occ<KP>           the per-occurrence table gradients in fmx_fm_update_occ's layout
//   k_inbatch_mask              the two masked copies of (idx, xv) the step's side forwards read
//   fmx_inbatch_bank.inc       the cross-batch item bank (fmx_fm_inbatch_bank_*): its scans, its backward role, its merge, its push
// The geometry (ib_geom) is a function of B alone: every sum has one fixed order, there are no float atomics.
// The score's products commute and so does a_u + a_c, so both roles of the backward evaluate the bits the forward evaluated.
#include "fmx_host.h"

#include <cmath>

namespace {

constexpr int IB_THREADS = 64;      // one wave per workgroup: a tile of 64 rows of the register side
constexpr int IB_SPLIT_MIN = 64;    // fewest rows of the uniform side per split
constexpr int IB_MAX_SPLITS = 32;
constexpr int IB_MAX_FIELDS = 512;  // the item-field mask rides in the kernel arguments, one bit per field

struct IbGeom {
  int tiles, splits, per;
};
// splits = min(32, ceil(B / 64)) ranges of per = ceil(B / splits) rows (the last one may be shorter; ranges that would be empty
// are dropped): one split up to B = 64, two from B = 65 on.  include/fmx.h states this formula (fmx_fm_inbatch_splits).
inline IbGeom ib_geom(int B) {
  IbGeom g;
  g.tiles = (B + IB_THREADS - 1) / IB_THREADS;
  const int s0 = std::min(IB_MAX_SPLITS, (B + IB_SPLIT_MIN - 1) / IB_SPLIT_MIN);
  g.per = (B + s0 - 1) / s0;
  g.splits = (B + g.per - 1) / g.per;
  return g;
}

struct IbLse {  // the lse block: the per-row state first, the partial results of the splits behind it
  float *m, *s, *n, *pm, *ps, *pn, *pgac, *pgu, *pgc;
  size_t bytes;
};
inline IbLse ib_lse(int B, int kp, void *base) {
  const IbGeom g = ib_geom(B);
  const size_t row = align_up((size_t)B * 4, 256), part = align_up((size_t)g.splits * B * 4, 256);
  const size_t partv = align_up((size_t)g.splits * B * kp * 4, 256);
  char *p = static_cast<char *>(base);
  IbLse l;
  auto take = [&](size_t n) {
    float *r = reinterpret_cast<float *>(p);
    p += n;
    return r;
  };
  l.m = take(row);
  l.s = take(row);
  l.n = take(row);
  l.pm = take(part);
  l.ps = take(part);
  l.pn = take(part);
  l.pgac = take(part);
  l.pgu = take(partv);
  l.pgc = take(partv);
  l.bytes = (size_t)(p - static_cast<char *>(base));
  return l;
}

// the bank's slots [0, M): the same formula on M (include/fmx.h: fmx_fm_inbatch_bank_splits)
struct IbBankGeom {
  int splits_q, per_q;
};
inline IbBankGeom ib_bank_geom(int M) {
  const IbGeom g = ib_geom(M);
  return {g.splits, g.per};
}

// the lse block of a bank call: ib_lse's members, the partial results that the bank's ranges add to laid behind the batch's
inline IbLse ib_bank_lse(int B, int M, int kp, void *base) {
  const int sb = ib_geom(B).splits, sa = sb + ib_bank_geom(M).splits_q;
  const size_t row = align_up((size_t)B * 4, 256);
  char *p = static_cast<char *>(base);
  IbLse l;
  auto take = [&](size_t n) {
    float *r = reinterpret_cast<float *>(p);
    p += align_up(n, 256);
    return r;
  };
  l.m = take(row);
  l.s = take(row);
  l.n = take(row);
  l.pm = take((size_t)sa * B * 4);
  l.ps = take((size_t)sa * B * 4);
  l.pn = take((size_t)sa * B * 4);
  l.pgac = take((size_t)sb * B * 4);
  l.pgu = take((size_t)sa * B * kp * 4);
  l.pgc = take((size_t)sb * B * kp * 4);
  l.bytes = (size_t)(p - static_cast<char *>(base));
  return l;
}

struct IbArgs {
  const float *Su, *au, *Sc, *ac, *ac2;  // ac2: null, or a second term of a_c (the step: a_c = sfirst + sbi, added here)
  const float *corr;
  const int32_t *key;
  float *m, *s, *n, *pm, *ps, *pn, *pgac, *pgu, *pgc;
  float *loss, *score_out, *gSu, *gSc, *gac;
  int ld_u, ld_c, B, splits, per;
  float inv_b;
};

// fm_score's arithmetic (fmx_topk.hip) with the sides interchangeable: `un` the wave-uniform side's row, v the row in the thread's
// registers, a_sum = a_u[i] + a_c[j].  Products and the sum of the two a's commute: the bits are fmx_fm_topk's top_score whichever
// side sits in the registers.
template <int KP>
__device__ __forceinline__ float ib_score(const float4 *un, const float4 (&v)[KP / 4], float a_sum) {
  float acc = un[0].x * v[0].x;
  acc = fmaf(un[0].y, v[0].y, acc);
  acc = fmaf(un[0].z, v[0].z, acc);
  acc = fmaf(un[0].w, v[0].w, acc);
#pragma unroll
  for (int q = 1; q < KP / 4; ++q) {
    const float4 sq = un[q];
    acc = fmaf(sq.x, v[q].x, acc);
    acc = fmaf(sq.y, v[q].y, acc);
    acc = fmaf(sq.z, v[q].z, acc);
    acc = fmaf(sq.w, v[q].w, acc);
  }
  return a_sum + acc;
}

__device__ __forceinline__ float ib_ac(const float *__restrict__ ac, const float *__restrict__ ac2, int j) {
  return ac2 ? ac[j] + ac2[j] : ac[j];
}

// j is in row i's softmax: itself, or an item other than row i's own (equal keys: the same item -- an accidental hit)
__device__ __forceinline__ bool ib_eligible(int i, int j, bool keyed, int ki, int kj) { return i == j || !keyed || ki != kj; }

// the rows of the uniform side taken at a time: their operands fill 32 scalar registers, R independent product chains in flight
template <int KP>
constexpr int ib_r() { return KP >= 32 ? 1 : 32 / KP; }

// SUM = false: pm[split, i] = max of c_ij over the split's eligible j (-inf: none), and the uncorrected scores where asked for.
// SUM = true: with m_i the maximum over every split's pm, ps / pn [split, i] = the sums of e_ij = exp(c_ij - m_i) over the split's
// eligible j, with and without j = i, j ascending from +0.
template <int KP, bool SUM>
__global__ __launch_bounds__(IB_THREADS) void k_inbatch_scan(IbArgs a) {
  const int i = blockIdx.x * IB_THREADS + (int)threadIdx.x;
  const bool valid = i < a.B;
  const int ir = valid ? i : a.B - 1;
  const float *__restrict__ Sc = a.Sc;
  const float *__restrict__ ac = a.ac;
  const float *__restrict__ ac2 = a.ac2;
  const float *__restrict__ corr = a.corr;
  const int32_t *__restrict__ key = a.key;
  const float4 *row = reinterpret_cast<const float4 *>(a.Su + (size_t)ir * a.ld_u);
  float4 v[KP / 4];
#pragma unroll
  for (int q = 0; q < KP / 4; ++q) v[q] = row[q];
  const float aui = a.au[ir];
  const bool keyed = key != nullptr;
  const int ki = keyed ? key[ir] : 0;
  const int j0 = blockIdx.y * a.per, j1 = min(a.B, j0 + a.per);
  float mi = 0.f;
  if constexpr (SUM) {
    mi = a.pm[ir];
    for (int p = 1; p < a.splits; ++p) mi = fmaxf(mi, a.pm[(size_t)p * a.B + ir]);
  }
  float mx = -INFINITY, s = 0.f, n = 0.f;
  constexpr int R = ib_r<KP>();
  for (int jb = j0; jb < j1; jb += R) {
    float sc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int j = min(jb + r, j1 - 1);
      sc[r] = ib_score<KP>(reinterpret_cast<const float4 *>(Sc + (size_t)j * a.ld_c), v, aui + ib_ac(ac, ac2, j));
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int j = jb + r;
      if (R > 1 && j >= j1) break;
      const float c = corr ? sc[r] - corr[j] : sc[r];
      const bool el = ib_eligible(i, j, keyed, ki, keyed ? key[j] : 0);
      if constexpr (SUM) {
        const float e = expf(c - mi);
        if (el) {
          s += e;
          if (j != i) n += e;
        }
      } else {
        if (el) mx = fmaxf(mx, c);
        if (a.score_out && valid) a.score_out[(size_t)i * a.B + j] = sc[r];
      }
    }
  }
  if (!valid) return;
  const size_t o = (size_t)blockIdx.y * a.B + i;
  if constexpr (SUM) {
    a.ps[o] = s;
    a.pn[o] = n;
  } else {
    a.pm[o] = mx;
  }
}

// per row: m = max over the splits, s and n the partial sums added in split order, loss = log(s) - (c_ii - m)
template <int KP>
__global__ __launch_bounds__(256) void k_inbatch_lse(IbArgs a) {
  const int i = blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= a.B) return;
  float m = a.pm[i], s = a.ps[i], n = a.pn[i];
  for (int p = 1; p < a.splits; ++p) {
    const size_t o = (size_t)p * a.B + i;
    m = fmaxf(m, a.pm[o]);
    s += a.ps[o];
    n += a.pn[o];
  }
  const float4 *row = reinterpret_cast<const float4 *>(a.Su + (size_t)i * a.ld_u);
  float4 v[KP / 4];
#pragma unroll
  for (int q = 0; q < KP / 4; ++q) v[q] = row[q];
  const float sc = ib_score<KP>(reinterpret_cast<const float4 *>(a.Sc + (size_t)i * a.ld_c), v, a.au[i] + ib_ac(a.ac, a.ac2, i));
  const float c = a.corr ? sc - a.corr[i] : sc;
  a.m[i] = m;
  a.s[i] = s;
  a.n[i] = n;
  a.loss[i] = logf(s) - (c - m);
}

// The backward's body.  ROLE 0: the thread holds context row i = t and walks the items j of its split: gSu[i] += g_ij S_c[j].
// ROLE 1: the thread holds item row j = t and walks the contexts i: gSc[j] += g_ij S_u[i], gac[j] += g_ij.  The walk ascends from
// +0; with one split the sums are the outputs, else partial sums per split (k_inbatch_bwd_merge).
//     g_ij = (exp(c_ij - m_i) / s_i) inv_b  for eligible j != i,    g_ii = -(n_i / s_i) inv_b,    0 for the others
template <int KP, int ROLE>
__device__ __forceinline__ void ib_bwd_body(const IbArgs &a) {
  const int t = blockIdx.x * IB_THREADS + (int)threadIdx.x;
  const bool valid = t < a.B;
  const int tr = valid ? t : a.B - 1;
  const float *__restrict__ Un = ROLE == 0 ? a.Sc : a.Su;  // the uniform side
  const int ld_un = ROLE == 0 ? a.ld_c : a.ld_u;
  const float *__restrict__ au = a.au;
  const float *__restrict__ ac = a.ac;
  const float *__restrict__ ac2 = a.ac2;
  const float *__restrict__ corr = a.corr;
  const int32_t *__restrict__ key = a.key;
  const float *__restrict__ ms = a.m;
  const float *__restrict__ ss = a.s;
  const float *__restrict__ ns = a.n;
  const float4 *row = reinterpret_cast<const float4 *>((ROLE == 0 ? a.Su + (size_t)tr * a.ld_u : a.Sc + (size_t)tr * a.ld_c));
  float4 v[KP / 4], acc[KP / 4];
#pragma unroll
  for (int q = 0; q < KP / 4; ++q) {
    v[q] = row[q];
    acc[q] = splat(0.f);
  }
  const bool keyed = key != nullptr;
  const int kt = keyed ? key[tr] : 0;
  const float at = ROLE == 0 ? au[tr] : ib_ac(ac, ac2, tr);
  const float corr_t = (ROLE == 1 && corr) ? corr[tr] : 0.f;
  const float mt = ROLE == 0 ? ms[tr] : 0.f, st = ROLE == 0 ? ss[tr] : 1.f, nt = ROLE == 0 ? ns[tr] : 0.f;
  float gsum = 0.f;
  const int o0 = blockIdx.y * a.per, o1 = min(a.B, o0 + a.per);
  constexpr int R = ib_r<KP>();
  for (int ob = o0; ob < o1; ob += R) {
    float sc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int o = min(ob + r, o1 - 1);
      const float a_sum = ROLE == 0 ? at + ib_ac(ac, ac2, o) : au[o] + at;
      sc[r] = ib_score<KP>(reinterpret_cast<const float4 *>(Un + (size_t)o * ld_un), v, a_sum);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int o = ob + r;
      if (R > 1 && o >= o1) break;
      const int i = ROLE == 0 ? t : o, j = ROLE == 0 ? o : t;
      const float cj = ROLE == 0 ? (corr ? corr[o] : 0.f) : corr_t;
      const float c = corr ? sc[r] - cj : sc[r];
      const float mi = ROLE == 0 ? mt : ms[o], si = ROLE == 0 ? st : ss[o], ni = ROLE == 0 ? nt : ns[o];
      const bool el = ib_eligible(i, j, keyed, ROLE == 0 ? kt : (keyed ? key[o] : 0), ROLE == 0 ? (keyed ? key[o] : 0) : kt);
      const float gn = (expf(c - mi) / si) * a.inv_b;
      const float gp = -(ni / si) * a.inv_b;
      const float g = i == j ? gp : (el ? gn : 0.f);
      const float4 *un = reinterpret_cast<const float4 *>(Un + (size_t)o * ld_un);
#pragma unroll
      for (int q = 0; q < KP / 4; ++q) {
        const float4 u4 = un[q];
        acc[q].x = fmaf(g, u4.x, acc[q].x);
        acc[q].y = fmaf(g, u4.y, acc[q].y);
        acc[q].z = fmaf(g, u4.z, acc[q].z);
        acc[q].w = fmaf(g, u4.w, acc[q].w);
      }
      if (ROLE == 1) gsum += g;
    }
  }
  if (!valid) return;
  const bool direct = a.splits == 1;
  float *out = ROLE == 0 ? (direct ? a.gSu : a.pgu + (size_t)blockIdx.y * a.B * KP) : (direct ? a.gSc : a.pgc + (size_t)blockIdx.y * a.B * KP);
  float4 *dst = reinterpret_cast<float4 *>(out + (size_t)t * KP);
#pragma unroll
  for (int q = 0; q < KP / 4; ++q) dst[q] = acc[q];
  if (ROLE == 1) (direct ? a.gac : a.pgac + (size_t)blockIdx.y * a.B)[t] = gsum;
}

template <int KP>
__global__ __launch_bounds__(IB_THREADS) void k_inbatch_bwd(IbArgs a) {
  if (blockIdx.z == 0) ib_bwd_body<KP, 0>(a);
  else ib_bwd_body<KP, 1>(a);
}

// the splits' partial sums in split order: thread (which, row, quad) for gSu / gSc, and B more threads for gac
template <int KP>
__global__ __launch_bounds__(256) void k_inbatch_bwd_merge(IbArgs a) {
  constexpr int LPR = KP / 4;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x, nv = (int64_t)a.B * LPR;
  if (t < 2 * nv) {
    const bool item = t >= nv;
    const int64_t e = item ? t - nv : t;
    const float4 *p = reinterpret_cast<const float4 *>(item ? a.pgc : a.pgu) + e;
    float4 acc = p[0];
    for (int s = 1; s < a.splits; ++s) acc = acc + p[(size_t)s * nv];
    reinterpret_cast<float4 *>(item ? a.gSc : a.gSu)[e] = acc;
  } else if (t < 2 * nv + a.B) {
    const int64_t j = t - 2 * nv;
    float acc = a.pgac[j];
    for (int s = 1; s < a.splits; ++s) acc += a.pgac[(size_t)s * a.B + j];
    a.gac[j] = acc;
  }
}

struct IbMask {
  uint32_t w[IB_MAX_FIELDS / 32];
  __host__ __device__ bool item(int f) const { return (w[f >> 5] >> (f & 31)) & 1u; }
};

struct IbOccArgs {
  const float *rows;
  const int64_t *foff;
  const int32_t *idx;
  const float *xv, *gSu, *gSc, *gac, *Sc;
  float *occ;
  int B, F, stride, ld_c, ld_occ;
  IbMask mask;
};

// E of sample b's row of field f, x applied (fmx_fm_update_occ's occ_grad): an item field's x (fma(gac, S_c - x v, gSc)), a
// context field's x gSu; an index outside its field (the forward dropped that row and raised the error word): +0
template <int KP>
__global__ __launch_bounds__(256) void k_inbatch_occ(IbOccArgs a) {
  constexpr int LPR = KP / 4;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)a.B * a.F * LPR) return;
  const int q = (int)(t % LPR), f = (int)((t / LPR) % a.F), b = (int)(t / ((int64_t)LPR * a.F));
  const size_t o = (size_t)b * a.F + f;
  const float x = a.xv ? a.xv[o] : 1.f;
  const int64_t lo = a.foff[f], hi = a.foff[f + 1];
  const uint32_t li = (uint32_t)a.idx[o];
  const bool ok = li < (uint32_t)(hi - lo);
  float4 E = splat(0.f);
  if (a.mask.item(f)) {
    const float4 v = *reinterpret_cast<const float4 *>(a.rows + (size_t)(lo + (ok ? li : 0u)) * a.stride + 4 * q);
    const float4 S = *reinterpret_cast<const float4 *>(a.Sc + (size_t)b * a.ld_c + 4 * q);
    const float4 G = *reinterpret_cast<const float4 *>(a.gSc + (size_t)b * KP + 4 * q);
    const float ga = a.gac[b];
    E.x = x * fmaf(ga, S.x - x * v.x, G.x);
    E.y = x * fmaf(ga, S.y - x * v.y, G.y);
    E.z = x * fmaf(ga, S.z - x * v.z, G.z);
    E.w = x * fmaf(ga, S.w - x * v.w, G.w);
  } else {
    E = x * *reinterpret_cast<const float4 *>(a.gSu + (size_t)b * KP + 4 * q);
  }
  if (!ok) E = splat(0.f);
  *reinterpret_cast<float4 *>(a.occ + (size_t)b * a.ld_occ + (size_t)f * KP + 4 * q) = E;
}

// the step's masked copies: (idx_u, xv_u) keep the context fields, (idx_c, xv_c) the item fields; the others index 0, value 0
__global__ __launch_bounds__(256) void k_inbatch_mask(const int32_t *idx, const float *xv, int64_t n, int F, IbMask mask, int32_t *idx_u,
                                                      float *xv_u, int32_t *idx_c, float *xv_c) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const bool item = mask.item((int)(t % F));
  const int32_t ix = idx[t];
  const float x = xv ? xv[t] : 1.f;
  idx_u[t] = item ? 0 : ix;
  xv_u[t] = item ? 0.f : x;
  idx_c[t] = item ? ix : 0;
  xv_c[t] = item ? x : 0.f;
}

#include "fmx_inbatch_bank.inc"

// ---- host ----

IbArgs ib_args(const float *Su, int ld_u, const float *au, const float *Sc, int ld_c, const float *ac, const float *ac2, int B, int kp,
               const float *corr, const int32_t *key, float inv_b, const IbLse &l) {
  const IbGeom g = ib_geom(B);
  IbArgs a;
  memset(&a, 0, sizeof(a));
  a.Su = Su;
  a.au = au;
  a.Sc = Sc;
  a.ac = ac;
  a.ac2 = ac2;
  a.corr = corr;
  a.key = key;
  a.m = l.m;
  a.s = l.s;
  a.n = l.n;
  a.pm = l.pm;
  a.ps = l.ps;
  a.pn = l.pn;
  a.pgac = l.pgac;
  a.pgu = l.pgu;
  a.pgc = l.pgc;
  a.ld_u = ld_u;
  a.ld_c = ld_c;
  a.B = B;
  a.splits = g.splits;
  a.per = g.per;
  a.inv_b = inv_b;
  return a;
}

int ib_forward_launch(IbArgs a, int kp, float *loss, float *score_out, hipStream_t st) {
  const IbGeom g = ib_geom(a.B);
  a.loss = loss;
  a.score_out = score_out;
  const dim3 grid(g.tiles, g.splits);
  with_kp(kp, [&](auto KP) {
    hipLaunchKernelGGL((k_inbatch_scan<KP, false>), grid, dim3(IB_THREADS), 0, st, a);
    hipLaunchKernelGGL((k_inbatch_scan<KP, true>), grid, dim3(IB_THREADS), 0, st, a);
    hipLaunchKernelGGL((k_inbatch_lse<KP>), dim3((a.B + 255) / 256), dim3(256), 0, st, a);
  });
  return check_launch("k_inbatch_scan / k_inbatch_lse");
}

int ib_backward_launch(IbArgs a, int kp, float *gSu, float *gSc, float *gac, hipStream_t st) {
  const IbGeom g = ib_geom(a.B);
  a.gSu = gSu;
  a.gSc = gSc;
  a.gac = gac;
  with_kp(kp, [&](auto KP) {
    hipLaunchKernelGGL((k_inbatch_bwd<KP>), dim3(g.tiles, g.splits, 2), dim3(IB_THREADS), 0, st, a);
    if (g.splits > 1) {
      const int64_t n = 2 * (int64_t)a.B * (KP / 4) + a.B;
      hipLaunchKernelGGL((k_inbatch_bwd_merge<KP>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
    }
  });
  return check_launch("k_inbatch_bwd");
}

// ---- the bank's launches: the batch's kernels on the longer list of ranges, the bank's between them ----

IbBankArgs ib_bank_args(const float *Su, int ld_u, const float *au, const float *Sc, int ld_c, const float *ac, const float *ac2, int B,
                        int kp, const float *corr, const int32_t *key, const fmx_item_bank_t *bank, float inv_b, void *lse) {
  const IbBankGeom q = ib_bank_geom(bank->capacity);
  IbBankArgs b;
  memset(&b, 0, sizeof(b));
  b.a = ib_args(Su, ld_u, au, Sc, ld_c, ac, ac2, B, kp, corr, key, inv_b, ib_bank_lse(B, bank->capacity, kp, lse));
  b.splits = b.a.splits;
  b.a.splits += q.splits_q;
  b.bS = bank->S;
  b.ba = bank->a;
  b.bcorr = bank->corr;
  b.bkey = bank->key;
  b.state = bank->state;
  b.M = bank->capacity;
  b.per_q = q.per_q;
  return b;
}

int ib_bank_forward_launch(IbBankArgs b, int kp, float *loss, float *score_out, float *bank_score_out, hipStream_t st) {
  const IbGeom g = ib_geom(b.a.B);
  b.a.loss = loss;
  b.a.score_out = score_out;
  b.bank_score_out = bank_score_out;
  const dim3 grid(g.tiles, g.splits), grid_q(g.tiles, ib_bank_geom(b.M).splits_q);
  with_kp(kp, [&](auto KP) {
    hipLaunchKernelGGL((k_inbatch_scan<KP, false>), grid, dim3(IB_THREADS), 0, st, b.a);
    hipLaunchKernelGGL((k_inbatch_bank_scan<KP, false>), grid_q, dim3(IB_THREADS), 0, st, b);
    hipLaunchKernelGGL((k_inbatch_scan<KP, true>), grid, dim3(IB_THREADS), 0, st, b.a);
    hipLaunchKernelGGL((k_inbatch_bank_scan<KP, true>), grid_q, dim3(IB_THREADS), 0, st, b);
    hipLaunchKernelGGL((k_inbatch_lse<KP>), dim3((b.a.B + 255) / 256), dim3(256), 0, st, b.a);
  });
  return check_launch("k_inbatch_scan / k_inbatch_bank_scan / k_inbatch_lse");
}

int ib_bank_backward_launch(IbBankArgs b, int kp, float *gSu, float *gSc, float *gac, hipStream_t st) {
  const IbGeom g = ib_geom(b.a.B);
  b.a.gSu = gSu;
  b.a.gSc = gSc;
  b.a.gac = gac;
  with_kp(kp, [&](auto KP) {
    hipLaunchKernelGGL((k_inbatch_bwd<KP>), dim3(g.tiles, g.splits, 2), dim3(IB_THREADS), 0, st, b.a);
    hipLaunchKernelGGL((k_inbatch_bank_bwd<KP>), dim3(g.tiles, ib_bank_geom(b.M).splits_q), dim3(IB_THREADS), 0, st, b);
    const int64_t n = 2 * (int64_t)b.a.B * (KP / 4) + b.a.B;
    hipLaunchKernelGGL((k_inbatch_bank_bwd_merge<KP>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, b);
  });
  return check_launch("k_inbatch_bwd / k_inbatch_bank_bwd");
}

int ib_bank_push_launch(const fmx_item_bank_t *bank, const float *Sc, int ld_c, const float *ac, const float *ac2, const float *corr,
                        const int32_t *key, int B, hipStream_t st) {
  IbPushArgs p;
  p.bS = bank->S;
  p.ba = bank->a;
  p.bcorr = bank->corr;
  p.bkey = bank->key;
  p.state = bank->state;
  p.Sc = Sc;
  p.ac = ac;
  p.ac2 = ac2;
  p.corr = corr;
  p.key = key;
  p.M = bank->capacity;
  p.kp = bank->kp;
  p.ld_c = ld_c;
  p.B = B;
  hipLaunchKernelGGL(k_inbatch_bank_push, dim3(1), dim3(IB_PUSH_THREADS), 0, st, p);
  return check_launch("k_inbatch_bank_push");
}

// what every bank call refuses; `pushes`: the call writes B slots
int check_bank(const fmx_item_bank_t *bank, int kp, const float *corr, const int32_t *key, int B, bool pushes, const char *who) {
  if (!bank) return fail(FMX_ERR_ARG, "%s: bank is null", who);
  if (!bank->S || !bank->a || !bank->state) return fail(FMX_ERR_ARG, "%s: bank->S, bank->a and bank->state are required", who);
  if (bank->capacity < 1) return fail(FMX_ERR_ARG, "%s: bank->capacity = %d must be >= 1", who, bank->capacity);
  if (bank->kp != kp) return fail(FMX_ERR_SHAPE, "%s: bank->kp = %d, the call's kp = %d", who, bank->kp, kp);
  if (!aligned16(bank->S)) return fail(FMX_ERR_ALIGN, "%s: bank->S must be 16-byte aligned", who);
  if ((corr == nullptr) != (bank->corr == nullptr))
    return fail(FMX_ERR_ARG, "%s: corr and bank->corr must both be given or both be null", who);
  if ((key == nullptr) != (bank->key == nullptr)) return fail(FMX_ERR_ARG, "%s: key and bank->key must both be given or both be null", who);
  if (bank->capacity > FMX_ITEM_BANK_MAX)
    return fail(FMX_ERR_UNSUPPORTED, "%s: bank->capacity = %d: at most %d slots are taken", who, bank->capacity, FMX_ITEM_BANK_MAX);
  if (pushes && B > bank->capacity)
    return fail(FMX_ERR_UNSUPPORTED, "%s: B = %d rows do not fit a bank of %d slots", who, B, bank->capacity);
  return FMX_OK;
}

int ib_occ_launch(const fmx_table_t *table, const int32_t *idx, const float *xv, const IbMask &mask, const float *gSu, const float *gSc,
                  const float *gac, const float *Sc, int ld_c, int B, float *occ, int ld_occ, hipStream_t st) {
  IbOccArgs a;
  a.rows = table->rows;
  a.foff = table->field_offsets;
  a.idx = idx;
  a.xv = xv;
  a.gSu = gSu;
  a.gSc = gSc;
  a.gac = gac;
  a.Sc = Sc;
  a.occ = occ;
  a.B = B;
  a.F = table->n_fields;
  a.stride = table->row_stride;
  a.ld_c = ld_c;
  a.ld_occ = ld_occ;
  a.mask = mask;
  const int64_t n = (int64_t)B * a.F * (table->kp / 4);
  with_kp(table->kp, [&](auto KP) { hipLaunchKernelGGL((k_inbatch_occ<KP>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a); });
  return check_launch("k_inbatch_occ");
}

// what the calls on the two [B, kp] arrays refuse
int check_sides(const float *Su, int ld_u, const float *au, const float *Sc, int ld_c, const float *ac, int B, int kp, const void *lse,
                int64_t lse_bytes, const char *who, int M = 0) {  // M: the capacity of a bank call's bank (its lse block is larger)
  if (!Su || !au || !Sc || !ac) return fail(FMX_ERR_ARG, "%s: Su, au, Sc and ac are required", who);
  if (B < 1) return fail(FMX_ERR_ARG, "%s: B = %d must be >= 1", who, B);
  if (!lpr_of(kp)) return fail(FMX_ERR_UNSUPPORTED, "%s: kp = %d must be 4, 8, 16, 32 or 64", who, kp);
  if (ld_u % 4 || ld_u < kp || ld_c % 4 || ld_c < kp)
    return fail(FMX_ERR_SHAPE, "%s: ld_u = %d and ld_c = %d must be multiples of 4 and >= kp = %d", who, ld_u, ld_c, kp);
  if (!aligned16(Su) || !aligned16(Sc)) return fail(FMX_ERR_ALIGN, "%s: Su and Sc must be 16-byte aligned", who);
  if (!lse) return fail(FMX_ERR_ARG, "%s: null workspace", who);
  if (!aligned16(lse)) return fail(FMX_ERR_ALIGN, "%s: workspace must be 16-byte aligned", who);
  const int64_t need = (int64_t)(M ? ib_bank_lse(B, M, kp, nullptr) : ib_lse(B, kp, nullptr)).bytes;
  if (lse_bytes < need)
    return fail(FMX_ERR_SHAPE, "%s: workspace of %lld bytes, %lld needed (%s)", who, (long long)lse_bytes, (long long)need,
                M ? "fmx_fm_inbatch_bank_lse_bytes" : "fmx_fm_inbatch_lse_bytes");
  return FMX_OK;
}

// ... and the calls on a table: the table, the batch and the item fields; fills the mask
int check_fields(const fmx_table_t *table, const int32_t *idx, int B, const int32_t *item_fields, int n_item_fields, IbMask *mask,
                 const char *who) {
  if (!table) return fail(FMX_ERR_ARG, "%s: table is null", who);
  if (!lpr_of(table->kp)) return fail(FMX_ERR_UNSUPPORTED, "%s: kp = %d must be 4, 8, 16, 32 or 64", who, table->kp);
  if (int rc = check_table(table)) return named(rc, who);
  if (!idx) return fail(FMX_ERR_ARG, "%s: idx is null", who);
  if (B < 1) return fail(FMX_ERR_ARG, "%s: B = %d must be >= 1", who, B);
  const int F = table->n_fields;
  if (n_item_fields < 1 || n_item_fields > F)
    return fail(FMX_ERR_ARG, "%s: n_item_fields = %d must lie in [1, %d]", who, n_item_fields, F);
  if (!item_fields) return fail(FMX_ERR_ARG, "%s: item_fields is null", who);
  if (mapped(table))
    return fail(FMX_ERR_UNSUPPORTED, "%s: tables whose fields are pieces of index columns (field_cols / field_base) are not taken", who);
  if (F > IB_MAX_FIELDS) return fail(FMX_ERR_UNSUPPORTED, "%s: %d fields: at most %d are taken", who, F, IB_MAX_FIELDS);
  memset(mask, 0, sizeof(*mask));
  for (int t = 0; t < n_item_fields; ++t) {
    const int f = item_fields[t];
    if (f < 0 || f >= F) return fail(FMX_ERR_ARG, "%s: item field %d is outside [0, %d)", who, f, F);
    if (mask->item(f)) return fail(FMX_ERR_ARG, "%s: item field %d is repeated", who, f);
    mask->w[f >> 5] |= 1u << (f & 31);
  }
  return FMX_OK;
}

// the step's workspace: [ the step workspace (carve) | LIST_BIAS_SCRATCH | pad to 256 | the in-batch area ]
struct IbWorkspace {
  Workspace w;
  int32_t *idx_u, *idx_c;
  float *xv_u, *xv_c, *Su, *Sc, *au, *sfirst, *sbi, *loss, *gSu, *gSc, *gac, *occ;
  void *lse;
  size_t bytes;
};
inline IbWorkspace ib_carve(const fmx_table_t *t, int B, void *base, int M = 0) {  // M: a bank step's capacity (its lse block)
  IbWorkspace r;
  r.w = carve(t, B, base);
  char *p = static_cast<char *>(base) + align_up(r.w.bytes + LIST_BIAS_SCRATCH, 256);
  auto take = [&](size_t n) {
    void *q = p;
    p += align_up(n, 256);
    return q;
  };
  const size_t BF = (size_t)B * t->n_fields * 4, Bk = (size_t)B * t->kp * 4, B1 = (size_t)B * 4;
  r.idx_u = static_cast<int32_t *>(take(BF));
  r.idx_c = static_cast<int32_t *>(take(BF));
  r.xv_u = static_cast<float *>(take(BF));
  r.xv_c = static_cast<float *>(take(BF));
  r.Su = static_cast<float *>(take(Bk));
  r.Sc = static_cast<float *>(take(Bk));
  r.au = static_cast<float *>(take(B1));
  r.sfirst = static_cast<float *>(take(B1));
  r.sbi = static_cast<float *>(take(B1));
  r.loss = static_cast<float *>(take(B1));
  r.gSu = static_cast<float *>(take(Bk));
  r.gSc = static_cast<float *>(take(Bk));
  r.gac = static_cast<float *>(take(B1));
  r.occ = static_cast<float *>(take(BF * t->kp));
  r.lse = take((M ? ib_bank_lse(B, M, t->kp, nullptr) : ib_lse(B, t->kp, nullptr)).bytes);
  r.bytes = (size_t)(p - static_cast<char *>(base));
  return r;
}

int check_step(const fmx_table_t *table, const fmx_hyper_t *hyper, int rule, const int32_t *idx, int B, const int32_t *item_fields,
               int n_item_fields, const void *workspace, int64_t workspace_bytes, const fmx_fwd_out_t *fwd, int64_t n_steps, IbMask *mask,
               const char *who, int M = 0) {
  if (!table) return fail(FMX_ERR_ARG, "%s: table is null", who);
  if (!hyper) return fail(FMX_ERR_ARG, "%s: hyper is null", who);
  if (int rc = check_fields(table, idx, B, item_fields, n_item_fields, mask, who)) return rc;
  if (int rc = check_workspace(table, B, workspace, workspace_bytes, who)) return rc;
  const int64_t need = (int64_t)ib_carve(table, B, nullptr, M).bytes;
  if (workspace_bytes < need)
    return fail(FMX_ERR_SHAPE, "%s: workspace of %lld bytes, %lld needed (%s)", who, (long long)workspace_bytes, (long long)need,
                M ? "fmx_fm_inbatch_bank_workspace_bytes" : "fmx_fm_inbatch_workspace_bytes");
  if (int rc = check_rule(table, rule)) return named(rc, who);
  if (int rc = check_adam(hyper, rule, n_steps)) return named(rc, who);
  if (int rc = check_sort_geometry(table, B)) return named(rc, who);
  if (fwd && fwd->loss && !aligned16(fwd->loss)) return fail(FMX_ERR_ALIGN, "%s: fwd->loss must be 16-byte aligned", who);
  return FMX_OK;
}

// one step; the arguments have been checked.  `hs`: the step's hyper-parameters (the stream: hyper_at_step); bank: null, or the
// item bank of fmx_fm_inbatch_bank_step: further negatives of the loss, and the step's own items pushed behind the update
int step_launch(const fmx_table_t *table, const fmx_hyper_t *hs, int rule, const int32_t *idx, const float *xv, const IbMask &mask,
                const float *corr, const int32_t *key, const fmx_item_bank_t *bank, int B, float inv_b, void *workspace,
                const fmx_fwd_out_t *fwd, float *loss_out, hipStream_t st) {
  const IbWorkspace b = ib_carve(table, B, workspace, bank ? bank->capacity : 0);
  const fmx_table_t tu = list_update_table(table, workspace, b.w.bytes);
  const int F = table->n_fields, kp = table->kp;
  int32_t *error = fwd ? fwd->error : nullptr;
  float *loss = (fwd && fwd->loss) ? fwd->loss : b.loss;
  const int64_t n = (int64_t)B * F;
  hipLaunchKernelGGL(k_inbatch_mask, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, idx, xv, n, F, mask, b.idx_u, b.xv_u, b.idx_c,
                     b.xv_c);
  if (int rc = check_launch("k_inbatch_mask")) return rc;
  if (int rc = sort_impl(table, idx, B, b.w.sorted, b.w.runs, error, st)) return rc;
  fmx_fwd_out_t ou, oc;
  memset(&ou, 0, sizeof(ou));
  memset(&oc, 0, sizeof(oc));
  ou.S = b.Su;
  ou.logit = b.au;
  ou.error = error;
  oc.S = b.Sc;
  oc.sfirst = b.sfirst;
  oc.sbi = b.sbi;
  oc.error = error;
  if (int rc = forward_impl(table, hs, b.idx_u, b.xv_u, nullptr, B, FMX_LOSS_NONE, 1.f, &ou, st)) return rc;
  if (int rc = forward_impl(table, hs, b.idx_c, b.xv_c, nullptr, B, FMX_LOSS_NONE, 1.f, &oc, st)) return rc;
  if (bank) {
    const IbBankArgs a = ib_bank_args(b.Su, kp, b.au, b.Sc, kp, b.sfirst, b.sbi, B, kp, corr, key, bank, inv_b, b.lse);
    if (int rc = ib_bank_forward_launch(a, kp, loss, nullptr, nullptr, st)) return rc;
    if (int rc = ib_bank_backward_launch(a, kp, b.gSu, b.gSc, b.gac, st)) return rc;
  } else {
    const IbArgs a = ib_args(b.Su, kp, b.au, b.Sc, kp, b.sfirst, b.sbi, B, kp, corr, key, inv_b, ib_lse(B, kp, b.lse));  // a_c = sfirst + sbi, added in the scan
    if (int rc = ib_forward_launch(a, kp, loss, nullptr, st)) return rc;
    if (int rc = ib_backward_launch(a, kp, b.gSu, b.gSc, b.gac, st)) return rc;
  }
  if (int rc = ib_occ_launch(table, idx, xv, mask, b.gSu, b.gSc, b.gac, b.Sc, kp, B, b.occ, F * kp, st)) return rc;
  if (int rc = update_occ_impl(&tu, hs, rule, b.w, b.xv_c, b.gac, b.occ, F * kp, B, loss, inv_b, loss_out, st)) return rc;
  return bank ? ib_bank_push_launch(bank, b.Sc, kp, b.sfirst, b.sbi, corr, key, B, st) : FMX_OK;  // (the update leaves S_c, sfirst, sbi alone)
}

// the stream's loop, shared by the plain and the bank entry
int stream_launch(const fmx_table_t *table, const fmx_hyper_t *hyper, int rule, const int32_t *idx_pool, const IbMask &mask,
                  const float *corr_pool, const int32_t *key_pool, const fmx_item_bank_t *bank, int n_pool, int B, float inv_b, int n_steps,
                  void *workspace, const fmx_fwd_out_t *fwd, float *loss_out, hipStream_t st) {
  for (int s = 0; s < n_steps; ++s) {
    const size_t p = (size_t)(s % n_pool);
    const fmx_hyper_t hs = hyper_at_step(hyper, rule, s);
    if (int rc = step_launch(table, &hs, rule, idx_pool + p * B * table->n_fields, nullptr, mask, corr_pool ? corr_pool + p * B : nullptr,
                             key_pool ? key_pool + p * B : nullptr, bank, B, inv_b, workspace, fwd, loss_out ? loss_out + s : nullptr, st))
      return rc;
  }
  return FMX_OK;
}

}  // namespace

extern "C" {

int32_t fmx_fm_inbatch_splits(int32_t B, int32_t kp) {
  if (B < 1) return fail(FMX_ERR_ARG, "fmx_fm_inbatch_splits: B = %d must be >= 1", B);
  if (!lpr_of(kp)) return fail(FMX_ERR_UNSUPPORTED, "fmx_fm_inbatch_splits: kp = %d must be 4, 8, 16, 32 or 64", kp);
  return ib_geom(B).splits;
}

int64_t fmx_fm_inbatch_lse_bytes(int32_t B, int32_t kp) {
  if (B < 1) return fail(FMX_ERR_ARG, "fmx_fm_inbatch_lse_bytes: B = %d must be >= 1", B);
  if (!lpr_of(kp)) return fail(FMX_ERR_UNSUPPORTED, "fmx_fm_inbatch_lse_bytes: kp = %d must be 4, 8, 16, 32 or 64", kp);
  return (int64_t)ib_lse(B, kp, nullptr).bytes;
}

int fmx_fm_inbatch_forward(const float *Su, int32_t ld_u, const float *au, const float *Sc, int32_t ld_c, const float *ac, int32_t B,
                           int32_t kp, const float *corr, const int32_t *key, float inv_b, void *lse, int64_t lse_bytes, float *loss,
                           float *score_out, fmx_stream_t stream) {
  const char *who = "fmx_fm_inbatch_forward";
  if (int rc = check_sides(Su, ld_u, au, Sc, ld_c, ac, B, kp, lse, lse_bytes, who)) return rc;
  if (!loss) return fail(FMX_ERR_ARG, "%s: loss is null", who);
  const IbArgs a = ib_args(Su, ld_u, au, Sc, ld_c, ac, nullptr, B, kp, corr, key, inv_b, ib_lse(B, kp, lse));
  return ib_forward_launch(a, kp, loss, score_out, static_cast<hipStream_t>(stream));
}

int fmx_fm_inbatch_backward(const float *Su, int32_t ld_u, const float *au, const float *Sc, int32_t ld_c, const float *ac, int32_t B,
                            int32_t kp, const float *corr, const int32_t *key, float inv_b, void *lse, int64_t lse_bytes, float *gSu,
                            float *gSc, float *gac, fmx_stream_t stream) {
  const char *who = "fmx_fm_inbatch_backward";
  if (int rc = check_sides(Su, ld_u, au, Sc, ld_c, ac, B, kp, lse, lse_bytes, who)) return rc;
  if (!gSu || !gSc || !gac) return fail(FMX_ERR_ARG, "%s: gSu, gSc and gac are required", who);
  if (!aligned16(gSu) || !aligned16(gSc)) return fail(FMX_ERR_ALIGN, "%s: gSu and gSc must be 16-byte aligned", who);
  const IbArgs a = ib_args(Su, ld_u, au, Sc, ld_c, ac, nullptr, B, kp, corr, key, inv_b, ib_lse(B, kp, lse));
  return ib_backward_launch(a, kp, gSu, gSc, gac, static_cast<hipStream_t>(stream));
}

int fmx_fm_inbatch_occ_grad(const fmx_table_t *table, const int32_t *idx, const float *xv, const int32_t *item_fields,
                            int32_t n_item_fields, const float *gSu, const float *gSc, const float *gac, const float *Sc, int32_t ld_c,
                            int32_t B, float *occ_grad, int32_t ld_occ, fmx_stream_t stream) {
  const char *who = "fmx_fm_inbatch_occ_grad";
  IbMask mask;
  if (int rc = check_fields(table, idx, B, item_fields, n_item_fields, &mask, who)) return rc;
  if (!gSu || !gSc || !gac || !Sc || !occ_grad) return fail(FMX_ERR_ARG, "%s: gSu, gSc, gac, Sc and occ_grad are required", who);
  if (ld_c % 4 || ld_c < table->kp) return fail(FMX_ERR_SHAPE, "%s: ld_c = %d must be a multiple of 4 and >= kp = %d", who, ld_c, table->kp);
  if (ld_occ % 4 || (int64_t)ld_occ < (int64_t)table->n_fields * table->kp)
    return fail(FMX_ERR_SHAPE, "%s: ld_occ = %d must be a multiple of 4 and >= n_fields * kp = %d", who, ld_occ, table->n_fields * table->kp);
  if (!aligned16(gSu) || !aligned16(gSc) || !aligned16(Sc) || !aligned16(occ_grad))
    return fail(FMX_ERR_ALIGN, "%s: gSu, gSc, Sc and occ_grad must be 16-byte aligned", who);
  return ib_occ_launch(table, idx, xv, mask, gSu, gSc, gac, Sc, ld_c, B, occ_grad, ld_occ, static_cast<hipStream_t>(stream));
}

int64_t fmx_fm_inbatch_workspace_bytes(const fmx_table_t *table, int32_t B, int32_t n_item_fields) {
  const char *who = "fmx_fm_inbatch_workspace_bytes";
  if (!table) return fail(FMX_ERR_ARG, "%s: table is null", who);
  if (int rc = check_table(table)) return named(rc, who);
  if (B < 1) return fail(FMX_ERR_ARG, "%s: B = %d must be >= 1", who, B);
  if (n_item_fields < 1 || n_item_fields > table->n_fields)
    return fail(FMX_ERR_ARG, "%s: n_item_fields = %d must lie in [1, %d]", who, n_item_fields, table->n_fields);
  return (int64_t)ib_carve(table, B, nullptr).bytes;
}

int fmx_fm_inbatch_step(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const int32_t *idx, const float *xv,
                        const int32_t *item_fields, int32_t n_item_fields, const float *corr, const int32_t *key, int32_t B, float inv_b,
                        void *workspace, int64_t workspace_bytes, const fmx_fwd_out_t *fwd, float *loss_out, fmx_stream_t stream) {
  const char *who = "fmx_fm_inbatch_step";
  IbMask mask;
  if (int rc = check_step(table, hyper, rule, idx, B, item_fields, n_item_fields, workspace, workspace_bytes, fwd, 1, &mask, who)) return rc;
  const fmx_hyper_t hs = hyper_for(hyper, rule);
  return step_launch(table, &hs, rule, idx, xv, mask, corr, key, nullptr, B, inv_b, workspace, fwd, loss_out, static_cast<hipStream_t>(stream));
}

int fmx_fm_inbatch_stream(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const int32_t *idx_pool,
                          const int32_t *item_fields, int32_t n_item_fields, const float *corr_pool, const int32_t *key_pool,
                          int32_t n_pool, int32_t B, float inv_b, int32_t n_steps, void *workspace, int64_t workspace_bytes,
                          const fmx_fwd_out_t *fwd, float *loss_out, fmx_stream_t stream) {
  const char *who = "fmx_fm_inbatch_stream";
  IbMask mask;
  if (int rc = check_step(table, hyper, rule, idx_pool, B, item_fields, n_item_fields, workspace, workspace_bytes, fwd,
                          n_steps > 0 ? n_steps : 0, &mask, who))
    return rc;
  if (n_pool < 1) return fail(FMX_ERR_ARG, "%s: n_pool = %d must be >= 1", who, n_pool);
  if (n_steps < 0) return fail(FMX_ERR_ARG, "%s: n_steps = %d must be >= 0", who, n_steps);
  return stream_launch(table, hyper, rule, idx_pool, mask, corr_pool, key_pool, nullptr, n_pool, B, inv_b, n_steps, workspace, fwd, loss_out,
                       static_cast<hipStream_t>(stream));
}

// ---- the cross-batch item bank ----

int32_t fmx_fm_inbatch_bank_splits(int32_t M, int32_t kp) {
  const char *who = "fmx_fm_inbatch_bank_splits";
  if (M < 1) return fail(FMX_ERR_ARG, "%s: M = %d must be >= 1", who, M);
  if (M > FMX_ITEM_BANK_MAX) return fail(FMX_ERR_UNSUPPORTED, "%s: M = %d: at most %d slots are taken", who, M, FMX_ITEM_BANK_MAX);
  if (!lpr_of(kp)) return fail(FMX_ERR_UNSUPPORTED, "%s: kp = %d must be 4, 8, 16, 32 or 64", who, kp);
  return ib_bank_geom(M).splits_q;
}

int64_t fmx_fm_inbatch_bank_lse_bytes(int32_t B, int32_t M, int32_t kp) {
  const char *who = "fmx_fm_inbatch_bank_lse_bytes";
  if (B < 1) return fail(FMX_ERR_ARG, "%s: B = %d must be >= 1", who, B);
  if (M < 1) return fail(FMX_ERR_ARG, "%s: M = %d must be >= 1", who, M);
  if (M > FMX_ITEM_BANK_MAX) return fail(FMX_ERR_UNSUPPORTED, "%s: M = %d: at most %d slots are taken", who, M, FMX_ITEM_BANK_MAX);
  if (!lpr_of(kp)) return fail(FMX_ERR_UNSUPPORTED, "%s: kp = %d must be 4, 8, 16, 32 or 64", who, kp);
  return (int64_t)ib_bank_lse(B, M, kp, nullptr).bytes;
}

int fmx_fm_inbatch_bank_forward(const float *Su, int32_t ld_u, const float *au, const float *Sc, int32_t ld_c, const float *ac,
                                int32_t B, int32_t kp, const float *corr, const int32_t *key, const fmx_item_bank_t *bank, float inv_b,
                                void *lse, int64_t lse_bytes, float *loss, float *score_out, float *bank_score_out,
                                fmx_stream_t stream) {
  const char *who = "fmx_fm_inbatch_bank_forward";
  if (int rc = check_bank(bank, kp, corr, key, B, false, who)) return rc;
  if (int rc = check_sides(Su, ld_u, au, Sc, ld_c, ac, B, kp, lse, lse_bytes, who, bank->capacity)) return rc;
  if (!loss) return fail(FMX_ERR_ARG, "%s: loss is null", who);
  const IbBankArgs a = ib_bank_args(Su, ld_u, au, Sc, ld_c, ac, nullptr, B, kp, corr, key, bank, inv_b, lse);
  return ib_bank_forward_launch(a, kp, loss, score_out, bank_score_out, static_cast<hipStream_t>(stream));
}

int fmx_fm_inbatch_bank_backward(const float *Su, int32_t ld_u, const float *au, const float *Sc, int32_t ld_c, const float *ac,
                                 int32_t B, int32_t kp, const float *corr, const int32_t *key, const fmx_item_bank_t *bank,
                                 float inv_b, void *lse, int64_t lse_bytes, float *gSu, float *gSc, float *gac, fmx_stream_t stream) {
  const char *who = "fmx_fm_inbatch_bank_backward";
  if (int rc = check_bank(bank, kp, corr, key, B, false, who)) return rc;
  if (int rc = check_sides(Su, ld_u, au, Sc, ld_c, ac, B, kp, lse, lse_bytes, who, bank->capacity)) return rc;
  if (!gSu || !gSc || !gac) return fail(FMX_ERR_ARG, "%s: gSu, gSc and gac are required", who);
  if (!aligned16(gSu) || !aligned16(gSc)) return fail(FMX_ERR_ALIGN, "%s: gSu and gSc must be 16-byte aligned", who);
  const IbBankArgs a = ib_bank_args(Su, ld_u, au, Sc, ld_c, ac, nullptr, B, kp, corr, key, bank, inv_b, lse);
  return ib_bank_backward_launch(a, kp, gSu, gSc, gac, static_cast<hipStream_t>(stream));
}

int fmx_fm_inbatch_bank_push(const fmx_item_bank_t *bank, const float *Sc, int32_t ld_c, const float *ac, const float *ac2,
                             const float *corr, const int32_t *key, int32_t B, fmx_stream_t stream) {
  const char *who = "fmx_fm_inbatch_bank_push";
  if (!bank) return fail(FMX_ERR_ARG, "%s: bank is null", who);
  if (!lpr_of(bank->kp)) return fail(FMX_ERR_UNSUPPORTED, "%s: bank->kp = %d must be 4, 8, 16, 32 or 64", who, bank->kp);
  if (B < 1) return fail(FMX_ERR_ARG, "%s: B = %d must be >= 1", who, B);
  if (int rc = check_bank(bank, bank->kp, corr, key, B, true, who)) return rc;
  if (!Sc || !ac) return fail(FMX_ERR_ARG, "%s: Sc and ac are required", who);
  if (ld_c % 4 || ld_c < bank->kp) return fail(FMX_ERR_SHAPE, "%s: ld_c = %d must be a multiple of 4 and >= kp = %d", who, ld_c, bank->kp);
  if (!aligned16(Sc)) return fail(FMX_ERR_ALIGN, "%s: Sc must be 16-byte aligned", who);
  return ib_bank_push_launch(bank, Sc, ld_c, ac, ac2, corr, key, B, static_cast<hipStream_t>(stream));
}

int64_t fmx_fm_inbatch_bank_workspace_bytes(const fmx_table_t *table, int32_t B, int32_t M, int32_t n_item_fields) {
  const char *who = "fmx_fm_inbatch_bank_workspace_bytes";
  if (!table) return fail(FMX_ERR_ARG, "%s: table is null", who);
  if (int rc = check_table(table)) return named(rc, who);
  if (B < 1) return fail(FMX_ERR_ARG, "%s: B = %d must be >= 1", who, B);
  if (M < 1) return fail(FMX_ERR_ARG, "%s: M = %d must be >= 1", who, M);
  if (M > FMX_ITEM_BANK_MAX) return fail(FMX_ERR_UNSUPPORTED, "%s: M = %d: at most %d slots are taken", who, M, FMX_ITEM_BANK_MAX);
  if (n_item_fields < 1 || n_item_fields > table->n_fields)
    return fail(FMX_ERR_ARG, "%s: n_item_fields = %d must lie in [1, %d]", who, n_item_fields, table->n_fields);
  return (int64_t)ib_carve(table, B, nullptr, M).bytes;
}

int fmx_fm_inbatch_bank_step(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const int32_t *idx, const float *xv,
                             const int32_t *item_fields, int32_t n_item_fields, const float *corr, const int32_t *key,
                             const fmx_item_bank_t *bank, int32_t B, float inv_b, void *workspace, int64_t workspace_bytes,
                             const fmx_fwd_out_t *fwd, float *loss_out, fmx_stream_t stream) {
  const char *who = "fmx_fm_inbatch_bank_step";
  IbMask mask;
  if (!table) return fail(FMX_ERR_ARG, "%s: table is null", who);
  if (int rc = check_bank(bank, table->kp, corr, key, B, true, who)) return rc;
  if (int rc = check_step(table, hyper, rule, idx, B, item_fields, n_item_fields, workspace, workspace_bytes, fwd, 1, &mask, who, bank->capacity))
    return rc;
  const fmx_hyper_t hs = hyper_for(hyper, rule);
  return step_launch(table, &hs, rule, idx, xv, mask, corr, key, bank, B, inv_b, workspace, fwd, loss_out, static_cast<hipStream_t>(stream));
}

int fmx_fm_inbatch_bank_stream(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const int32_t *idx_pool,
                               const int32_t *item_fields, int32_t n_item_fields, const float *corr_pool, const int32_t *key_pool,
                               const fmx_item_bank_t *bank, int32_t n_pool, int32_t B, float inv_b, int32_t n_steps, void *workspace,
                               int64_t workspace_bytes, const fmx_fwd_out_t *fwd, float *loss_out, fmx_stream_t stream) {
  const char *who = "fmx_fm_inbatch_bank_stream";
  IbMask mask;
  if (!table) return fail(FMX_ERR_ARG, "%s: table is null", who);
  if (int rc = check_bank(bank, table->kp, corr_pool, key_pool, B, true, who)) return rc;
  if (int rc = check_step(table, hyper, rule, idx_pool, B, item_fields, n_item_fields, workspace, workspace_bytes, fwd,
                          n_steps > 0 ? n_steps : 0, &mask, who, bank->capacity))
    return rc;
  if (n_pool < 1) return fail(FMX_ERR_ARG, "%s: n_pool = %d must be >= 1", who, n_pool);
  if (n_steps < 0) return fail(FMX_ERR_ARG, "%s: n_steps = %d must be >= 0", who, n_steps);
  return stream_launch(table, hyper, rule, idx_pool, mask, corr_pool, key_pool, bank, n_pool, B, inv_b, n_steps, workspace, fwd, loss_out,
                       static_cast<hipStream_t>(stream));
}

}  // extern "C"
