// fmx_inbatch_bank.inc -- the device code of the cross-batch item bank (fmx_fm_inbatch_bank_*, include/fmx.h), included by
// fmx_inbatch.hip inside its namespace: the bank's slots as further negatives of every row of an in-batch step.
//
// The batch's kernels run UNCHANGED on longer lists of ranges: the lse block of a bank call lays the bank's partial results behind
// the batch's ([splits + splits_q, B] for pm / ps / pn, [splits + splits_q, B, kp] for the gSu partial sums), and the batch's
// kernels are launched with IbArgs.splits = splits + splits_q and their own grid of `splits` ranges: k_inbatch_scan<KP, true> then
// takes m_i over the ranges of both kinds, k_inbatch_lse merges both kinds in order, and k_inbatch_bwd always writes partial sums.
// What is new, in k_inbatch_scan's layout (one wave per workgroup, thread t of tile T holding context row 64 T + t in its registers,
// the bank's rows as wave-uniform operands R at a time, no LDS, no scratch):
//   k_inbatch_bank_scan<KP, false>  grid (tiles, splits_q): the maximum of c_iq over the range's eligible slots -> pm [splits + y, B]
//   k_inbatch_bank_scan<KP, true>   the same grid: m_i = max over all pm, then s = n of the range's slots -> ps, pn [splits + y, B]
//   k_inbatch_bank_bwd<KP>          the same grid: the context role over the bank, gSu's partial sums -> pgu [splits + y, B, kp]
//   k_inbatch_bank_bwd_merge<KP>    gSu = the batch's partial sums then the bank's, in order; gSc, gac = the batch's
//   k_inbatch_bank_push             one workgroup: the batch's items to the slots (head + j) mod M, then the state
// A range is clipped to count: a slot >= count is not read (it may hold anything).

struct IbBankArgs {
  IbArgs a;  // a.splits = splits + splits_q: what the batch's kernels are given in a bank call
  const float *bS, *ba, *bcorr;
  const int32_t *bkey;
  const int32_t *state;
  float *bank_score_out;
  int M, per_q, splits;  // splits: the batch's ranges, the offset of the bank's partial results
};

// the valid slots of this workgroup's range: [q0, q1), empty when count <= q0
__device__ __forceinline__ int ib_bank_range(const IbBankArgs &b, int *q0) {
  const int count = min(b.M, max(b.state[1], 0));
  *q0 = blockIdx.y * b.per_q;
  return min(count, *q0 + b.per_q);
}

template <int KP, bool SUM>
__global__ __launch_bounds__(IB_THREADS) void k_inbatch_bank_scan(IbBankArgs b) {
  const IbArgs &a = b.a;
  const int i = blockIdx.x * IB_THREADS + (int)threadIdx.x;
  const bool valid = i < a.B;
  const int ir = valid ? i : a.B - 1;
  const float *__restrict__ bS = b.bS;
  const float *__restrict__ ba = b.ba;
  const float *__restrict__ bcorr = b.bcorr;
  const int32_t *__restrict__ bkey = b.bkey;
  const float4 *row = reinterpret_cast<const float4 *>(a.Su + (size_t)ir * a.ld_u);
  float4 v[KP / 4];
#pragma unroll
  for (int q = 0; q < KP / 4; ++q) v[q] = row[q];
  const float aui = a.au[ir];
  const bool keyed = bkey != nullptr;
  const int ki = keyed ? a.key[ir] : 0;
  int q0;
  const int q1 = ib_bank_range(b, &q0);
  float mi = 0.f;
  if constexpr (SUM) {
    mi = a.pm[ir];
    for (int p = 1; p < a.splits; ++p) mi = fmaxf(mi, a.pm[(size_t)p * a.B + ir]);
  }
  float mx = -INFINITY, s = 0.f;
  constexpr int R = ib_r<KP>();
  for (int jb = q0; jb < q1; jb += R) {
    float sc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int j = min(jb + r, q1 - 1);
      sc[r] = ib_score<KP>(reinterpret_cast<const float4 *>(bS + (size_t)j * KP), v, aui + ba[j]);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int j = jb + r;
      if (R > 1 && j >= q1) break;
      const float c = bcorr ? sc[r] - bcorr[j] : sc[r];
      const bool el = ib_eligible(i, -1, keyed, ki, keyed ? bkey[j] : 0);  // (a slot is never row i's own column)
      if constexpr (SUM) {
        const float e = expf(c - mi);
        if (el) s += e;
      } else {
        if (el) mx = fmaxf(mx, c);
        if (b.bank_score_out && valid) b.bank_score_out[(size_t)i * b.M + j] = sc[r];
      }
    }
  }
  if (!valid) return;
  const size_t o = (size_t)(b.splits + blockIdx.y) * a.B + i;
  if constexpr (SUM) {
    a.ps[o] = s;
    a.pn[o] = s;  // every bank item is a negative
  } else {
    a.pm[o] = mx;
  }
}

// the context role of the backward over the bank: gSu[i] += g_iq bank.S[q], g_iq = (exp(c_iq - m_i) / s_i) inv_b for eligible q
template <int KP>
__global__ __launch_bounds__(IB_THREADS) void k_inbatch_bank_bwd(IbBankArgs b) {
  const IbArgs &a = b.a;
  const int t = blockIdx.x * IB_THREADS + (int)threadIdx.x;
  const bool valid = t < a.B;
  const int tr = valid ? t : a.B - 1;
  const float *__restrict__ bS = b.bS;
  const float *__restrict__ ba = b.ba;
  const float *__restrict__ bcorr = b.bcorr;
  const int32_t *__restrict__ bkey = b.bkey;
  const float4 *row = reinterpret_cast<const float4 *>(a.Su + (size_t)tr * a.ld_u);
  float4 v[KP / 4], acc[KP / 4];
#pragma unroll
  for (int q = 0; q < KP / 4; ++q) {
    v[q] = row[q];
    acc[q] = splat(0.f);
  }
  const bool keyed = bkey != nullptr;
  const int kt = keyed ? a.key[tr] : 0;
  const float at = a.au[tr], mt = a.m[tr], st = a.s[tr];
  int q0;
  const int q1 = ib_bank_range(b, &q0);
  constexpr int R = ib_r<KP>();
  for (int ob = q0; ob < q1; ob += R) {
    float sc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int o = min(ob + r, q1 - 1);
      sc[r] = ib_score<KP>(reinterpret_cast<const float4 *>(bS + (size_t)o * KP), v, at + ba[o]);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int o = ob + r;
      if (R > 1 && o >= q1) break;
      const float c = bcorr ? sc[r] - bcorr[o] : sc[r];
      const bool el = ib_eligible(t, -1, keyed, kt, keyed ? bkey[o] : 0);
      const float gn = (expf(c - mt) / st) * a.inv_b;
      const float g = el ? gn : 0.f;
      const float4 *un = reinterpret_cast<const float4 *>(bS + (size_t)o * KP);
#pragma unroll
      for (int q = 0; q < KP / 4; ++q) {
        const float4 u4 = un[q];
        acc[q].x = fmaf(g, u4.x, acc[q].x);
        acc[q].y = fmaf(g, u4.y, acc[q].y);
        acc[q].z = fmaf(g, u4.z, acc[q].z);
        acc[q].w = fmaf(g, u4.w, acc[q].w);
      }
    }
  }
  if (!valid) return;
  float4 *dst = reinterpret_cast<float4 *>(a.pgu + ((size_t)(b.splits + blockIdx.y) * a.B + t) * KP);
#pragma unroll
  for (int q = 0; q < KP / 4; ++q) dst[q] = acc[q];
}

// k_inbatch_bwd_merge's threads; gSu over a.splits = splits + splits_q ranges, gSc and gac over the batch's `splits`
template <int KP>
__global__ __launch_bounds__(256) void k_inbatch_bank_bwd_merge(IbBankArgs b) {
  const IbArgs &a = b.a;
  constexpr int LPR = KP / 4;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x, nv = (int64_t)a.B * LPR;
  if (t < 2 * nv) {
    const bool item = t >= nv;
    const int64_t e = item ? t - nv : t;
    const float4 *p = reinterpret_cast<const float4 *>(item ? a.pgc : a.pgu) + e;
    const int ns = item ? b.splits : a.splits;
    float4 acc = p[0];
    for (int s = 1; s < ns; ++s) acc = acc + p[(size_t)s * nv];
    reinterpret_cast<float4 *>(item ? a.gSc : a.gSu)[e] = acc;
  } else if (t < 2 * nv + a.B) {
    const int64_t j = t - 2 * nv;
    float acc = a.pgac[j];
    for (int s = 1; s < b.splits; ++s) acc += a.pgac[(size_t)s * a.B + j];
    a.gac[j] = acc;
  }
}

constexpr int IB_PUSH_THREADS = 1024;

struct IbPushArgs {
  float *bS, *ba, *bcorr;
  int32_t *bkey, *state;
  const float *Sc, *ac, *ac2, *corr;
  const int32_t *key;
  int M, kp, ld_c, B;
};

// One workgroup.  Every thread reads the head, the barrier orders those reads before thread 0's write of the new state, and a slot
// is written by one thread (B <= M: the B slots are distinct).
__global__ __launch_bounds__(IB_PUSH_THREADS) void k_inbatch_bank_push(IbPushArgs p) {
  int head = p.state[0], count = p.state[1];
  head = (uint32_t)head < (uint32_t)p.M ? head : 0;
  count = min(p.M, max(count, 0));
  __syncthreads();
  if (threadIdx.x == 0) {
    p.state[0] = (int)(((int64_t)head + p.B) % p.M);
    p.state[1] = min(p.M, count + p.B);
  }
  const int lpr = p.kp / 4;
  for (int e = (int)threadIdx.x; e < p.B * lpr; e += IB_PUSH_THREADS) {
    const int j = e / lpr, q = e - j * lpr;
    const int slot = (int)(((int64_t)head + j) % p.M);
    reinterpret_cast<float4 *>(p.bS + (size_t)slot * p.kp)[q] = reinterpret_cast<const float4 *>(p.Sc + (size_t)j * p.ld_c)[q];
  }
  for (int j = (int)threadIdx.x; j < p.B; j += IB_PUSH_THREADS) {
    const int slot = (int)(((int64_t)head + j) % p.M);
    p.ba[slot] = ib_ac(p.ac, p.ac2, j);
    if (p.bcorr) p.bcorr[slot] = p.corr[j];
    if (p.bkey) p.bkey[slot] = p.key[j];
  }
}
