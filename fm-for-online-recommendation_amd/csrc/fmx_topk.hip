// fmx_topk.hip -- exact top-K over an FM table's candidates (fmx_fm_topk, include/fmx.h): the inner-product scan of
// U context sums against N candidate sums with a per-user running K-th-best threshold, and the merge of the candidate splits.
//
// A selection slot (one user of a workgroup) is an LDS buffer of `cap` 64-bit keys plus a count and a threshold key.  A key
// packs (score, position) so that the unsigned integer order IS the result order (score descending, position ascending):
//     key = ord(score) << 32 | (0xFFFFFFFF - position),   ord: the float bits made monotone, -0 taken as +0
// key 0 is no candidate (ord(-inf) = 0x007FFFFF > 0).  A pair whose key beats the slot's threshold (the K-th best key held,
// 0 while fewer than K are held) is appended; a slot that could overflow in the next chunk is sorted (bitonic, descending) and
// cut to its K best, which raises the threshold.  The set kept is the exact top K of what the slot has seen, whatever the
// order of the appends, so the result is independent of scheduling.
//
// fmx_mlp_topk (the DeepFM / NFM classes) feeds the same slots from a scan that runs the whole network on every pair, and
// fmx_afm_topk from one that computes the attentional FM's cross pairs.  The rank calls (fmx_*_rank) are the same three scans
// with the slots replaced by counters (fmx_rank.inc, which also holds ScanSink: what a scan does with a score, stated once for
// the FM and the network scan).  The host side of all six entry points is at the end of this file: a plan per family, a driver
// per call.
#include "fmx_host.h"

namespace {

constexpr int TK_THREADS = 256;       // a workgroup; also the candidates per chunk (one per thread)
constexpr int TK_MAX_UT = 16;         // users per workgroup of the scan
constexpr int TK_MAX_K = 256;
constexpr int TK_MAX_SPLITS = 128;    // candidate splits per user tile
constexpr int TK_SPLIT_MIN = 2048;    // fewest candidates per split
constexpr int TK_TILE_BUDGET = 1024;  // workgroups the scan aims for (user tiles x splits); 256 CUs, two resident each, twice over

struct TopkGeom {
  int ut, cap, tiles, splits, per;
};

// K <= 128: 16 users x 512 keys; K <= 256: 8 users x 1024 keys.  Both 64 KiB of LDS (two workgroups per CU).  A slot is
// compacted when it holds more than cap - 256 keys (a chunk may add 256) and then holds K, so a compaction drops >= 128 keys.
// The merge's single slot has the same capacity.
constexpr int topk_cap(int K) { return K <= 128 ? 512 : 1024; }
inline TopkGeom topk_geom(int U, int N, int K) {
  TopkGeom g;
  g.ut = K <= 128 ? 16 : 8;
  g.cap = topk_cap(K);
  g.tiles = (U + g.ut - 1) / g.ut;
  const int sn = std::min(TK_MAX_SPLITS, (N + TK_SPLIT_MIN - 1) / TK_SPLIT_MIN);
  const int s = std::max(1, std::min(sn, TK_TILE_BUDGET / g.tiles));
  const int per0 = (N + s - 1) / s;
  g.per = (per0 + TK_THREADS - 1) / TK_THREADS * TK_THREADS;
  g.splits = (N + g.per - 1) / g.per;
  return g;
}

// The workspace holds a partial result per (user, split): uint64 [U, splits, K] lists for fmx_fm_topk, int32 [U, splits, T + 1]
// counts for fmx_fm_rank.  U * splits is bounded by a formula that is monotone in U and N (the splits of the geometry are not):
// splits <= ceil(N / TK_SPLIT_MIN) and U * splits <= U + TK_TILE_BUDGET * TK_MAX_UT.
inline int64_t fm_scan_parts(int U, int N) {
  const int64_t sn = std::min<int64_t>(TK_MAX_SPLITS, (N + TK_SPLIT_MIN - 1) / TK_SPLIT_MIN);
  return std::min<int64_t>((int64_t)U * sn, (int64_t)U + (int64_t)TK_TILE_BUDGET * TK_MAX_UT);
}

struct TopkArgs {
  const float *Su, *au, *Sc, *ac;
  const int32_t *excl_off, *excl_pos;
  uint64_t *parts;
  int32_t *top_pos;
  float *top_score;
  int ld_u, ld_c, U, N, K, ut, cap, splits, per;
};

__device__ __forceinline__ uint64_t make_key(float s, int c) {
  uint32_t b = __float_as_uint(s);
  b = b == 0x80000000u ? 0u : b;
  const uint32_t o = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return ((uint64_t)o << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)c);
}
__device__ __forceinline__ float key_score(uint64_t k) {
  const uint32_t o = (uint32_t)(k >> 32);
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}
__device__ __forceinline__ int key_pos(uint64_t k) { return (int)(0xFFFFFFFFu - (uint32_t)k); }

// The FM score of a pair (include/fmx.h, fmx_fm_topk), stated once for the scan and for fmx_fm_mine_negatives:
//   score(u, c) = (au[u] + ac[c]) + dot,   dot = fma(Su[kp-1], Sc[kp-1], ... fma(Su[1], Sc[1], Su[0] * Sc[0]))
// su, au[u]: the user's row and its a_u (wave-uniform in both callers: scalar loads), v: the candidate's row in the lane's registers.
template <int KP>
__device__ __forceinline__ float fm_score(const float4 *su, const float *au, int u, const float4 (&v)[KP / 4], float acv) {
  float acc = su[0].x * v[0].x;
  acc = fmaf(su[0].y, v[0].y, acc);
  acc = fmaf(su[0].z, v[0].z, acc);
  acc = fmaf(su[0].w, v[0].w, acc);
#pragma unroll
  for (int q = 1; q < KP / 4; ++q) {
    const float4 sq = su[q];
    acc = fmaf(sq.x, v[q].x, acc);
    acc = fmaf(sq.y, v[q].y, acc);
    acc = fmaf(sq.z, v[q].z, acc);
    acc = fmaf(sq.w, v[q].w, acc);
  }
  return (au[u] + acv) + acc;
}

struct Slots {  // LDS: keys [n][cap], count [n], threshold [n]
  uint64_t *buf;
  uint64_t *thr;
  int *cnt;
};

// Sort the keys of every slot j < n holding more than `limit` (bitonic, descending, all such slots in one pass: the barriers
// are paid once, not per slot) and keep each one's K best; a slot left with K keys takes the K-th as its threshold.  Entered
// by the whole workgroup after a barrier (every thread reads the same counts); leaves through one.
__device__ void compact(const Slots &s, int n, int cap, int K, int limit) {
  int P = 2;
  bool any = false;
  for (int j = 0; j < n; ++j) {
    const int c = s.cnt[j];
    if (c > limit) {
      any = true;
      while (P < c) P <<= 1;
    }
  }
  if (!any) {  // still a barrier: the next chunk's appends must not change a count another thread has yet to read here
    __syncthreads();
    return;
  }
  int lp = 1;
  while ((1 << lp) < P) ++lp;
  const int half = P >> 1;
  for (int i = threadIdx.x; i < n * P; i += blockDim.x) {
    const int j = i >> lp, e = i & (P - 1);
    if (s.cnt[j] > limit && e >= s.cnt[j]) s.buf[(size_t)j * cap + e] = 0;
  }
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1)
    for (int jj = k >> 1; jj > 0; jj >>= 1) {
      for (int i = threadIdx.x; i < n * half; i += blockDim.x) {
        const int j = i >> (lp - 1), q = i & (half - 1);
        if (s.cnt[j] <= limit) continue;
        uint64_t *b = s.buf + (size_t)j * cap;
        const int lo = ((q & ~(jj - 1)) << 1) | (q & (jj - 1)), hi = lo + jj;  // jj a power of two: no integer division
        const uint64_t x = b[lo], y = b[hi];
        if ((lo & k) == 0 ? x < y : x > y) {
          b[lo] = y;
          b[hi] = x;
        }
      }
      __syncthreads();
    }
  if ((int)threadIdx.x < n && s.cnt[threadIdx.x] > limit) {
    const int j = threadIdx.x, m = s.cnt[j] < K ? s.cnt[j] : K;
    s.cnt[j] = m;
    if (m == K) s.thr[j] = s.buf[(size_t)j * cap + K - 1];
  }
  __syncthreads();
}

// append this lane's key to slot j when `keep`: one LDS atomic per wave
__device__ __forceinline__ void append(const Slots &s, int j, int cap, bool keep, uint64_t key) {
  const uint64_t m = __ballot(keep);
  if (m == 0) return;
  const int lane = threadIdx.x & (WAVE - 1);
  int base = 0;
  if (lane == 0) base = atomicAdd(&s.cnt[j], (int)__popcll(m));
  base = __shfl(base, 0);
  if (keep) s.buf[(size_t)j * cap + base + (int)__popcll(m & ((1ull << lane) - 1))] = key;
}

__device__ __forceinline__ bool excluded(const int32_t *off, const int32_t *pos, int u, int c) {
  int lo = off[u];
  const int end = off[u + 1];
  int hi = end;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (pos[mid] < c) lo = mid + 1;
    else hi = mid;
  }
  return lo < end && pos[lo] == c;
}

// write K results of a sorted slot: partial keys (more splits to merge) or the final rows
__device__ void emit(const Slots &s, int j, int cap, int K, uint64_t *part, int32_t *top_pos, float *top_score) {
  const uint64_t *b = s.buf + (size_t)j * cap;
  const int n = s.cnt[j];
  for (int i = threadIdx.x; i < K; i += blockDim.x) {
    const uint64_t key = i < n ? b[i] : 0;
    if (part) {
      part[i] = key;
    } else {
      top_pos[i] = key ? key_pos(key) : -1;
      top_score[i] = key ? key_score(key) : -INFINITY;
    }
  }
}

__device__ void init_slots(Slots &s, uint64_t *lds, int n, int cap) {
  s.buf = lds;
  s.thr = lds + (size_t)n * cap;
  s.cnt = reinterpret_cast<int *>(s.thr + n);
  if (threadIdx.x < n) {
    s.thr[threadIdx.x] = 0;
    s.cnt[threadIdx.x] = 0;
  }
  __syncthreads();
}

}  // namespace

#include "fmx_rank.inc"
#include "fmx_mine.inc"

namespace {

// grid (user tiles, splits).  Thread t scores candidate c0 + t against every user of the tile; the user's S_u and a_u are
// wave-uniform (scalar loads), the candidate's S_c row sits in the thread's registers for the whole chunk.
// The score is fm_score above.
// MODE (fmx_rank.inc): the top-K selection (Args = TopkArgs), or one of the rank call's two phases (Args = FmRankArgs; ut = 1
// and grid (U, T) for SCAN_KEYS).
template <int KP, int MODE = SCAN_TOPK, class Args = TopkArgs>
__global__ __launch_bounds__(TK_THREADS) void k_topk_scan(Args a) {
  extern __shared__ uint64_t tk_lds[];
  ScanSink<MODE, TK_MAX_UT, TK_THREADS> sink;
  const int u0 = blockIdx.x * a.ut, nu = min(a.ut, a.U - u0);
  if (!sink.open(a, tk_lds, u0, nu)) return;
  const int c_begin = sink.c_begin, c_end = sink.c_end;
  const float *__restrict__ Su = a.Su;
  const float *__restrict__ au = a.au;
  for (int c0 = c_begin; c0 < c_end; c0 += TK_THREADS) {
    const int c = c0 + (int)threadIdx.x;
    const bool valid = c < c_end;
    const int cr = valid ? c : c_begin;
    const float4 *row = reinterpret_cast<const float4 *>(a.Sc + (size_t)cr * a.ld_c);
    float4 v[KP / 4];
#pragma unroll
    for (int q = 0; q < KP / 4; ++q) v[q] = row[q];
    const float acv = a.ac[cr];
    // R users at a time (their S_u as wave-uniform values, 32 scalar registers): R independent product chains and R threshold
    // reads in flight instead of one round trip after the other
    constexpr int R = KP >= 32 ? 1 : 32 / KP;
    for (int j0 = 0; j0 < nu; j0 += R) {
      float score[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int u = u0 + min(j0 + r, nu - 1);
        const float4 *su = reinterpret_cast<const float4 *>(Su + (size_t)u * a.ld_u);
        score[r] = fm_score<KP>(su, au, u, v, acv);
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int j = j0 + r;
        if (R > 1 && j >= nu) break;
        sink.take(a, j, c, valid, score[r]);
      }
    }
    if constexpr (MODE == SCAN_TOPK) __syncthreads();  // every append of the chunk, before the counts are read
    sink.cut(a, c0);
  }
  if constexpr (MODE == SCAN_COUNT) __syncthreads();
  sink.close(a);
}

// one workgroup per user: the union of the user's `splits` sorted partial lists, read depth-major (the best of every list,
// then the second best, ...).  Lists are sorted and the threshold only rises, so once a whole round keeps nothing no later
// round can keep anything.
__global__ __launch_bounds__(TK_THREADS) void k_topk_merge(TopkArgs a) {
  extern __shared__ uint64_t tk_lds[];
  Slots s;
  init_slots(s, tk_lds, 1, a.cap);
  const int u = blockIdx.x, L = a.splits * a.K;
  const uint64_t *part = a.parts + (size_t)u * L;
  for (int i0 = 0; i0 < L; i0 += TK_THREADS) {
    const int i = i0 + (int)threadIdx.x;
    uint64_t key = 0;
    if (i < L) {
      const int d = i / a.splits, l = i - d * a.splits;
      key = part[(size_t)l * a.K + d];
    }
    const bool keep = key > s.thr[0];
    append(s, 0, a.cap, keep, key);
    if (!__syncthreads_or(keep)) break;
    compact(s, 1, a.cap, a.K, i0 == 0 ? a.K : a.cap - TK_THREADS);
  }
  compact(s, 1, a.cap, a.K, -1);
  emit(s, 0, a.cap, a.K, nullptr, a.top_pos + (size_t)u * a.K, a.top_score + (size_t)u * a.K);
}

// ---------------------------------------------------------------------------------------------------------------------
// fmx_mlp_topk: the same selection over the scores of the DeepFM / NFM network on the pair's bi-interaction vector
// ---------------------------------------------------------------------------------------------------------------------
// bi(u + c) = bi_u + bi_c + S_u (.) S_c, so a pair's network input is built in LDS from the two sides' rows, and the U x N
// forwards of the network run as GEMMs on chunks of 64 pairs (one user, 64 consecutive candidates): [64 x in] . W_l^T on
// v_mfma_f32_16x16x4_f32 (exact f32 products, accumulated in k order: the same bits as the fmaf chain the header states).
// Workgroup = one user x one candidate split, four waves: wave (wr, wc) of a WR x WC grid owns the row tiles wr * RPW ..
// + RPW - 1 (RPW = 4 / WR) and the column tiles wc, wc + WC, ... of every layer.  The weights go from L2 straight into the
// multiplying wave's registers (a pre-packed copy in the workspace, one 16-byte load per lane and four k-steps), the
// activations stay in LDS in the MFMA's operand order (one ds_read_b128 per lane and four k-steps).  Each pair's scores
// then go through the slot / compact / merge of fmx_fm_topk.

constexpr int TM_ROWS = 64;                 // pairs per chunk: four MFMA row tiles
constexpr int TM_MAX_H = 256, TM_MAX_L = 8;
constexpr int TM_TILE_BUDGET = 2048;        // workgroups the scan aims for: 256 CUs, two resident each, four times over
constexpr int TM_MAX_SPLITS = 1024;
constexpr int TM_SPLIT_WORK = 1 << 22;      // FLOPs a split holds at least (the network's cost sets the fewest candidates)
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct MlpShape {
  int k, H, L, K0, Hp, NT;  // K0 = k and Hp = H rounded up to 16; NT = Hp / 16 column tiles
};
inline MlpShape mlp_shape(const fmx_mlp_t *m) {
  MlpShape s;
  s.k = m->k;
  s.H = m->hidden;
  s.L = m->n_layers;
  s.K0 = (s.k + 15) / 16 * 16;
  s.Hp = (s.H + 15) / 16 * 16;
  s.NT = s.Hp / 16;
  return s;
}
struct MlpPackArgs {
  const float *params;
  float *packed;
  long long src_w[TM_MAX_L], src_b[TM_MAX_L], dst_w[TM_MAX_L], dst_b[TM_MAX_L];
  long long total;
  int k, H, L, K0, Hp, NT;
};

// Per layer l, where W_l [H, in_l] and b_l sit in mlp->params (src_*) and in the packed copy (dst_*): NT * (in / 16) blocks of
// 64 lanes x 4 floats (lane 16 kq + m, element s: W[16 ct + m][16 g + 4 s + kq], zero outside [H, in)), then the Hp biases
// (zero past H).  Returns the packed copy's floats; p may be null.
inline int64_t mlp_packed_floats(const MlpShape &s, MlpPackArgs *p) {
  int64_t src = 0, dst = 0;
  for (int l = 0; l < s.L; ++l) {
    const int64_t in = l == 0 ? s.k : s.H, inp = l == 0 ? s.K0 : s.Hp;
    if (p) {
      p->src_w[l] = src;
      p->src_b[l] = src + s.H * in;
      p->dst_w[l] = dst;
      p->dst_b[l] = dst + s.NT * inp * 16;
    }
    src += s.H * in + s.H;
    dst += s.NT * inp * 16 + s.Hp;
  }
  return dst;
}


struct MlpTopkGeom {
  int cap, splits, per;
};
inline int64_t tm_split_min(const MlpShape &s) {
  const int64_t flops = 2LL * s.Hp * (s.K0 + (int64_t)(s.L - 1) * s.Hp);
  const int64_t m = (TM_SPLIT_WORK / flops + TM_ROWS - 1) / TM_ROWS * TM_ROWS;
  return std::min<int64_t>(8192, std::max<int64_t>(TM_ROWS, m));
}
inline int64_t tm_max_splits(const MlpShape &s, int N) {
  const int64_t sm = tm_split_min(s);
  return std::min<int64_t>(TM_MAX_SPLITS, (N + sm - 1) / sm);
}
// one user per workgroup; splits = ceil(budget / U) within [1, tm_max_splits]; a slot holds K + one chunk, a power of two
inline MlpTopkGeom mlp_topk_geom(const MlpShape &s, int U, int N, int K) {
  MlpTopkGeom g;
  g.cap = 128;
  while (g.cap < K + TM_ROWS) g.cap <<= 1;
  const int64_t sp = std::max<int64_t>(1, std::min<int64_t>(tm_max_splits(s, N), (TM_TILE_BUDGET + U - 1) / U));
  const int64_t per0 = (N + sp - 1) / sp;
  g.per = (int)((per0 + TM_ROWS - 1) / TM_ROWS * TM_ROWS);
  g.splits = (N + g.per - 1) / g.per;
  return g;
}
// the workspace: the packed weights, then a partial result per (user, split); U * splits <= U * ceil(budget / U) < U + budget
inline int64_t mlp_scan_parts(const MlpShape &s, int U, int N) {
  return std::min<int64_t>((int64_t)U * tm_max_splits(s, N), (int64_t)U + TM_TILE_BUDGET);
}

// f(WC, NCT) as integral constants: the wave grid of the network scan for NT column tiles of 16.  WC wave columns (and 4 / WC
// wave rows); a wave owns NCT = ceil(NT / WC) column tiles of every layer.
template <class Fn>
decltype(auto) with_wave_grid(int NT, Fn &&f) {
  using std::integral_constant;
  if (NT <= 1) return f(integral_constant<int, 1>{}, integral_constant<int, 1>{});
  if (NT == 2) return f(integral_constant<int, 2>{}, integral_constant<int, 1>{});
  if (NT == 3) return f(integral_constant<int, 2>{}, integral_constant<int, 2>{});
  if (NT == 4) return f(integral_constant<int, 4>{}, integral_constant<int, 1>{});
  if (NT <= 8) return f(integral_constant<int, 4>{}, integral_constant<int, 2>{});
  if (NT <= 12) return f(integral_constant<int, 4>{}, integral_constant<int, 3>{});
  return f(integral_constant<int, 4>{}, integral_constant<int, 4>{});
}

// one thread per packed float
__global__ __launch_bounds__(256) void k_mlp_topk_pack(MlpPackArgs a) {
  const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
  if (o >= a.total) return;
  int l = 0;
  while (l + 1 < a.L && o >= a.dst_w[l + 1]) ++l;
  const int in = l == 0 ? a.k : a.H, inp = l == 0 ? a.K0 : a.Hp;
  float v = 0.f;
  if (o < a.dst_b[l]) {
    const long long e = o - a.dst_w[l];
    const int blk = (int)(e >> 8), lane = (int)(e >> 2) & 63, s = (int)e & 3;
    const int ct = blk / (inp / 16), g = blk - ct * (inp / 16);
    const int n = 16 * ct + (lane & 15), i = 16 * g + 4 * s + (lane >> 4);
    if (n < a.H && i < in) v = a.params[a.src_w[l] + (long long)n * in + i];
  } else {
    const int j = (int)(o - a.dst_b[l]);
    if (j < a.H) v = a.params[a.src_b[l] + j];
  }
  a.packed[o] = v;
}

struct MlpTopkArgs {
  const float *Su, *Bu, *au, *Sc, *Bc, *ac;
  const int32_t *excl_off, *excl_pos;
  const float *packed;
  long long woff[TM_MAX_L], boff[TM_MAX_L];
  uint64_t *parts;
  int32_t *top_pos;
  float *top_score;
  int ld_u, ld_c, U, N, K, kp, k, H, L, K0, Hp, fm_term, cap, splits, per;
};
struct MlpRankArgs : MlpTopkArgs {
  RankIo r;
};

// activation (row r < 64, column d) of a chunk with G groups of 16 columns: [row tile][G][lane 16 (d % 4) + r % 16][(d / 4) % 4]
__device__ __forceinline__ int xidx(int r, int d, int G) {
  return ((((r >> 4) * G + (d >> 4)) * 64 + (d & 3) * 16 + (r & 15)) << 2) + ((d >> 2) & 3);
}

// grid (U, splits).  Per chunk of 64 candidates: x0 into LDS, the L layers (MFMA, then relu into the same buffer between two
// barriers), then wave 0 scores row r = candidate c0 + r and appends it to the user's slot.
// MODE (fmx_rank.inc): the top-K selection (Args = MlpTopkArgs), or one of the rank call's two phases (Args = MlpRankArgs;
// grid (U, T) for SCAN_KEYS).  MFMA rows are independent: a pair's score does not depend on the chunk it is computed in.
template <int WC, int NCT, int MODE = SCAN_TOPK, class Args = MlpTopkArgs>
__global__ __launch_bounds__(256) void k_mlp_topk_scan(Args a) {
  extern __shared__ __attribute__((aligned(16))) float tm_lds[];
  constexpr int RPW = WC;  // row tiles per wave (4 row tiles over 4 / WC wave rows)
  const int NT = a.Hp / 16;
  const int wmax = a.K0 > a.Hp ? a.K0 : a.Hp;
  float *X = tm_lds;
  ScanSink<MODE, 1, TM_ROWS> sink;
  if (!sink.open(a, reinterpret_cast<uint64_t *>(X + (size_t)TM_ROWS * wmax), blockIdx.x, 1)) return;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, wr = w / WC, wc = w % WC;
  const int m = lane & 15, kq = lane >> 4;
  const int u = blockIdx.x;
  const float *__restrict__ Su = a.Su + (size_t)u * a.ld_u;
  const float *__restrict__ Bu = a.Bu + (size_t)u * a.ld_u;
  const float au = a.au[u];
  const int c_begin = sink.c_begin, c_end = sink.c_end;
  const int G0 = a.K0 / 16, Gh = a.Hp / 16;
  for (int c0 = c_begin; c0 < c_end; c0 += TM_ROWS) {
    // x0[r][d] = fma(Su[d], Sc[d], Bu[d] + Bc[d]) for d < k, 0 on the pad columns (rows past the split repeat its last one)
    for (int e = t; e < TM_ROWS * a.K0; e += 256) {
      const int r = e / a.K0, d = e - r * a.K0;
      const size_t c = (size_t)min(c0 + r, c_end - 1);
      float v = 0.f;
      if (d < a.k) v = fmaf(Su[d], a.Sc[c * a.ld_c + d], Bu[d] + a.Bc[c * a.ld_c + d]);
      X[xidx(r, d, G0)] = v;
    }
    __syncthreads();
    for (int l = 0; l < a.L; ++l) {
      const int G = l == 0 ? G0 : Gh;
      const f32x4 *Wp = reinterpret_cast<const f32x4 *>(a.packed + a.woff[l]) + lane;
      const float *bp = a.packed + a.boff[l];
      f32x4 acc[RPW][NCT], bcur[NCT], bnxt[NCT];
#pragma unroll
      for (int j = 0; j < NCT; ++j) {
        const int ct = wc + WC * j;
        const float b = ct < NT ? bp[16 * ct + m] : 0.f;
#pragma unroll
        for (int i = 0; i < RPW; ++i) acc[i][j] = f32x4{b, b, b, b};
        bcur[j] = ct < NT ? Wp[(size_t)ct * G * 64] : f32x4{0.f, 0.f, 0.f, 0.f};
      }
      for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int j = 0; j < NCT; ++j) {
          const int ct = wc + WC * j;
          bnxt[j] = (ct < NT && g + 1 < G) ? Wp[((size_t)ct * G + g + 1) * 64] : bcur[j];
        }
        f32x4 av[RPW];
#pragma unroll
        for (int i = 0; i < RPW; ++i) av[i] = reinterpret_cast<const f32x4 *>(X)[((wr * RPW + i) * G + g) * 64 + lane];
#pragma unroll
        for (int st = 0; st < 4; ++st)
#pragma unroll
          for (int j = 0; j < NCT; ++j) {
            if (wc + WC * j >= NT) continue;
#pragma unroll
            for (int i = 0; i < RPW; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i][st], bcur[j][st], acc[i][j], 0, 0, 0);
          }
#pragma unroll
        for (int j = 0; j < NCT; ++j) bcur[j] = bnxt[j];
      }
      __syncthreads();  // every wave has read this layer's input
      // lane (m, kq), register q holds row 4 kq + q, column m of the tile; relu keeps a NaN (as torch.relu does)
#pragma unroll
      for (int j = 0; j < NCT; ++j) {
        const int ct = wc + WC * j;
        if (ct >= NT) continue;
#pragma unroll
        for (int i = 0; i < RPW; ++i)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float v = acc[i][j][q];
            X[xidx(16 * (wr * RPW + i) + 4 * kq + q, 16 * ct + m, Gh)] = v < 0.f ? 0.f : v;
          }
      }
      __syncthreads();
    }
    if (t < TM_ROWS) {
      const int c = c0 + t;
      const bool valid = c < c_end;
      const size_t cr = (size_t)(valid ? c : c_begin);
      float sum = X[xidx(t, 0, Gh)];
      for (int j = 1; j < a.H; ++j) sum = sum + X[xidx(t, j, Gh)];
      float base = au + a.ac[cr];
      if (a.fm_term) {
        const float *sc = a.Sc + cr * a.ld_c;
        float dot = Su[0] * sc[0];
        for (int d = 1; d < a.kp; ++d) dot = fmaf(Su[d], sc[d], dot);
        base = base + dot;
      }
      sink.take(a, 0, c, valid, base + sum);
    }
    // the row sums have been read: the next chunk may overwrite the activations.  In every mode this is also the barrier the
    // sink's cut and close are entered after.
    __syncthreads();
    sink.cut(a, c0);
  }
  sink.close(a);
}
// ---------------------------------------------------------------------------------------------------------------------
// fmx_afm_topk: the same selection over the exact AFM logit of the combined sample
// ---------------------------------------------------------------------------------------------------------------------
// The context side (stats_u) and the item side (stats_c) carry their own pairs' softmax statistics (fmx_afm_side); what is
// left per (u, c) is the n_ctx x n_item cross pairs.  Workgroup = one user x one candidate split; thread = one candidate of
// a chunk of 256.  The user's embeddings and the attention parameters (a copy padded to kp in the workspace) are the same for
// every lane: the compiler reads them with scalar loads and they enter the FMAs as scalar operands, so the VALU does nothing
// but the pair arithmetic (n_ctx n_item (kp (t + 2) + 2 t) FMA-class operations per pair and one exp per cross pair).

constexpr int AT_SPLIT_WORK = 1 << 22;   // FLOPs a split holds at least
constexpr int AT_TILE_BUDGET = 2048;     // workgroups the scan aims for: 256 CUs, eight resident each
constexpr int AT_MAX_SPLITS = 1024;

struct AfmTopkArgs {
  const float *Eu, *su, *Ec, *sc;
  const float *packed;  // [ W (t x kp) | b (t) | h (t) | p (kp) ], zero-padded columns
  const int32_t *excl_off, *excl_pos;
  uint64_t *parts;
  int32_t *top_pos;
  float *top_score;
  int U, N, K, t, n_ctx, n_item, cap, splits, per;
};
struct AfmRankArgs : AfmTopkArgs {
  RankIo r;
};

inline int64_t at_pair_flops(int n_ctx, int n_item, int t, int kp) {
  return (int64_t)n_ctx * n_item * (2LL * t * kp + 4LL * t + 2LL * kp);
}
inline int64_t at_split_min(int n_ctx, int n_item, int t, int kp) {
  const int64_t m = (AT_SPLIT_WORK / at_pair_flops(n_ctx, n_item, t, kp) + TK_THREADS - 1) / TK_THREADS * TK_THREADS;
  return std::min<int64_t>(8192, std::max<int64_t>(TK_THREADS, m));
}
inline int64_t at_max_splits(int64_t split_min, int N) { return std::min<int64_t>(AT_MAX_SPLITS, (N + split_min - 1) / split_min); }
inline int at_kp(int k) { return k <= 4 ? 4 : k <= 8 ? 8 : k <= 16 ? 16 : k <= 32 ? 32 : 64; }
inline int64_t at_packed_bytes(int t) { return (int64_t)align_up((size_t)(t * 64 + 2 * t + 64) * 4, 256); }
// the workspace: the padded parameter copy (sized for kp = 64), then a partial result per (user, split); U * splits < U + budget.
// The split minimum is taken at the smallest kp that holds k, by the workspace size and by the call alike.
inline int64_t afm_scan_parts(const fmx_afm_t *afm, int n_ctx, int n_item, int U, int N) {
  const int64_t sm = at_split_min(n_ctx, n_item, afm->t, at_kp(afm->k));
  return std::min<int64_t>((int64_t)U * at_max_splits(sm, N), (int64_t)U + AT_TILE_BUDGET);
}

// one thread per float of the padded copy
__global__ __launch_bounds__(256) void k_afm_topk_pack(const float *params, int k, int t, int kp, float *packed) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  const int nW = t * kp;
  if (o >= nW + 2 * t + kp) return;
  float v;
  if (o < nW) {
    const int u = o / kp, d = o - u * kp;
    v = d < k ? params[u * k + d] : 0.f;
  } else if (o < nW + 2 * t) {
    v = params[t * k + (o - nW)];
  } else {
    const int d = o - nW - 2 * t;
    v = d < k ? params[t * k + 2 * t + d] : 0.f;
  }
  packed[o] = v;
}

// grid (U, splits).  The score (include/fmx.h, fmx_afm_topk): the cross pairs j-major (item field j ascending, then context
// field i ascending), each as k_afm's pair_terms, folded into a running (max, Z, R) by online rescaling, then the two sides.
// MODE (fmx_rank.inc): the top-K selection (Args = AfmTopkArgs), or one of the rank call's two phases (Args = AfmRankArgs; grid
// (U, T) for SCAN_KEYS).
// This scan spells its three modes out itself instead of going through ScanSink: with the sink its instantiations at kp = 16
// measured 0.3 - 1.2 % slower than this text on the same score loop (profiles/scan_seam_ab.txt, section B).
template <int KP, int MODE = SCAN_TOPK, class Args = AfmTopkArgs>
__global__ __launch_bounds__(TK_THREADS) void k_afm_topk_scan(Args a) {
  extern __shared__ uint64_t tk_lds[];
  Slots s;
  RankLds rk;
  int target = -1;
  if constexpr (MODE == SCAN_TOPK) init_slots(s, tk_lds, 1, a.cap);
  if constexpr (MODE == SCAN_COUNT) {
    __shared__ RankShared<1> sh;
    init_rank(rk, sh, a.r.tkeys + (size_t)blockIdx.x * a.r.T, 1, a.r.T);
  }
  if constexpr (MODE == SCAN_KEYS) {
    target = keys_target(a.r, blockIdx.x, blockIdx.y, a.N);
    if (target < 0) return;
  }
  const int u = blockIdx.x, t = a.t;
  const float *__restrict__ W = a.packed;
  const float *__restrict__ bW = W + t * KP;
  const float *__restrict__ h = bW + t;
  const float *__restrict__ p = h + t;
  const float *__restrict__ Eu = a.Eu + (size_t)u * a.n_ctx * KP;
  const float4 stu = reinterpret_cast<const float4 *>(a.su)[u];  // (lin_u, m_u, Z_u, R_u)
  const int c_begin = MODE == SCAN_KEYS ? target / TK_THREADS * TK_THREADS : blockIdx.y * a.per;
  const int c_end = min(a.N, c_begin + (MODE == SCAN_KEYS ? TK_THREADS : a.per));
  for (int c0 = c_begin; c0 < c_end; c0 += TK_THREADS) {
    const int c = c0 + (int)threadIdx.x;
    const bool valid = c < c_end;
    const size_t cr = (size_t)(valid ? c : c_begin);
    float mx = -INFINITY, Zx = 0.f, Rx = 0.f;
    for (int j = 0; j < a.n_item; ++j) {
      const float4 *row = reinterpret_cast<const float4 *>(a.Ec + (cr * a.n_item + j) * KP);
      float ec[KP];
#pragma unroll
      for (int q4 = 0; q4 < KP / 4; ++q4) {
        const float4 v = row[q4];
        ec[4 * q4] = v.x;
        ec[4 * q4 + 1] = v.y;
        ec[4 * q4 + 2] = v.z;
        ec[4 * q4 + 3] = v.w;
      }
      for (int i = 0; i < a.n_ctx; ++i) {
        const float *eu = Eu + i * KP;
        float q[KP];
#pragma unroll
        for (int d = 0; d < KP; ++d) q[d] = eu[d] * ec[d];
        float r = 0.f;
#pragma unroll
        for (int d = 0; d < KP; ++d) r = fmaf(p[d], q[d], r);
        float sx = 0.f;
        for (int v = 0; v < t; ++v) {
          float z = bW[v];
#pragma unroll
          for (int d = 0; d < KP; ++d) z = fmaf(W[v * KP + d], q[d], z);
          sx = fmaf(h[v], fmaxf(z, 0.f), sx);
        }
        // online rescaling: a new maximum scales the running sums by e^(old - new) and enters with weight 1
        const bool up = sx > mx;
        const float e = expf(up ? mx - sx : sx - mx);
        Zx = up ? fmaf(Zx, e, 1.f) : Zx + e;
        Rx = up ? fmaf(Rx, e, r) : fmaf(e, r, Rx);
        mx = up ? sx : mx;
      }
    }
    const float4 stc = reinterpret_cast<const float4 *>(a.sc)[cr];
    const float M = fmaxf(fmaxf(stu.y, stc.y), mx);
    const float eu_ = expf(stu.y - M), ec_ = expf(stc.y - M), ex = expf(mx - M);
    const float Z = fmaf(Zx, ex, fmaf(stc.z, ec_, stu.z * eu_));
    const float R = fmaf(Rx, ex, fmaf(stc.w, ec_, stu.w * eu_));
    const float score = (stu.x + stc.x) + R / Z;
    const uint64_t key = make_key(score, c);
    if constexpr (MODE == SCAN_TOPK) {
      bool keep = valid && score == score && key > s.thr[0];
      if (keep && a.excl_off) keep = !excluded(a.excl_off, a.excl_pos, u, c);
      append(s, 0, a.cap, keep, key);
      __syncthreads();
      compact(s, 1, a.cap, a.K, c0 == c_begin ? a.K : a.cap - TK_THREADS);
    } else if constexpr (MODE == SCAN_COUNT) {
      count_pair(rk, 0, a.r.T, valid, score, key, a.excl_off, a.excl_pos, u, c);
    } else if (valid && c == target) {
      a.r.tkeys[(size_t)u * a.r.T + blockIdx.y] = target_key(score, c, a.excl_off, a.excl_pos, u);
    }
  }
  if constexpr (MODE == SCAN_COUNT) {
    __syncthreads();
    emit_counts(rk, a.r, u, 1, a.splits, blockIdx.y);
  }
  if constexpr (MODE == SCAN_TOPK) {
    compact(s, 1, a.cap, a.K, -1);
    if (a.splits > 1)
      emit(s, 0, a.cap, a.K, a.parts + ((size_t)u * a.splits + blockIdx.y) * a.K, nullptr, nullptr);
    else
      emit(s, 0, a.cap, a.K, nullptr, a.top_pos + (size_t)u * a.K, a.top_score + (size_t)u * a.K);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side of the six entry points (fmx_{fm,mlp,afm}_{topk,rank}; include/fmx.h)
// ---------------------------------------------------------------------------------------------------------------------
// Two axes, each stated once.  A family's plan (FmScan, MlpScan, AfmScan) holds what both of its calls need: the checks, the
// bound on U * splits, the pack launch and the workspace prefix it fills, the geometry, the base argument struct and the
// dispatch to the scan's instantiation.  A call's end (TopkEnd, RankEnd) holds what it asks of any family: its size checks, its
// outputs and what a partial result weighs.  scan_topk / scan_rank drive any plan.
constexpr size_t slots_lds(int n, int cap) { return (size_t)n * cap * 8 + (size_t)n * 8 + (size_t)n * 4; }

// A launch of one of the slot kernels (256 threads).  A launch with dynamic LDS holds 64 KiB of keys or of activations plus
// a slot, above the default dynamic LDS limit, so such a kernel's limit is raised to 80 KiB on its first launch.
template <auto Kernel, class Args>
int launch_slots(const char *name, dim3 grid, size_t lds, hipStream_t st, const Args &a) {
  if (lds != 0) {
    static const bool raised = [] {
      (void)hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
      return true;
    }();
    (void)raised;
  }
  hipLaunchKernelGGL(Kernel, grid, dim3(TK_THREADS), lds, st, a);
  return check_launch(name);
}

// The merge of either scan's partial lists uint64 [U, splits, K] into the final rows; nothing to do for one split.  It reads
// the partial keys, K, the slot capacity, the splits and the outputs only.
int merge_topk(uint64_t *parts, int32_t *top_pos, float *top_score, int32_t U, int32_t K, int splits, hipStream_t st) {
  if (splits == 1) return FMX_OK;
  TopkArgs m{};
  m.parts = parts;
  m.top_pos = top_pos;
  m.top_score = top_score;
  m.U = U;
  m.K = K;
  m.cap = topk_cap(K);
  m.splits = splits;
  return launch_slots<k_topk_merge>("k_topk_merge", dim3(U), slots_lds(1, m.cap), st, m);
}

// ---- the two calls ------------------------------------------------------------------------------------------------------
// scan_K: the K of the family's geometry and arguments.  out_a / out_b: the call's two required outputs.  part_bytes: the
// workspace behind the family's prefix, given the family's bound on U * splits.  ws_args: how the family's *_workspace_bytes
// call begins ("", "mlp, ", "afm, n_ctx, n_item, ").
struct TopkEnd {
  int32_t K;
  int32_t *top_pos;
  float *top_score;
  int scan_K() const { return K; }
  const void *out_a() const { return top_pos; }
  const void *out_b() const { return top_score; }
  int check_sizes(const char *fn, int32_t U, int32_t N) const {
    if (U < 1 || N < 1) return fail(FMX_ERR_ARG, "%s: U=%d and N=%d must be >= 1", fn, U, N);
    if (K < 1) return fail(FMX_ERR_ARG, "%s: K=%d must be >= 1", fn, K);
    if (K > TK_MAX_K) return fail(FMX_ERR_UNSUPPORTED, "%s: K=%d, the kernels cover K <= %d", fn, K, TK_MAX_K);
    return FMX_OK;
  }
  int check_flag(const char *) const { return FMX_OK; }
  int64_t part_bytes(int64_t parts, int32_t) const { return parts * K * 8; }
  int check_ws(const char *fn, int64_t ws_bytes, int64_t need, const char *ws_args, int32_t U, int32_t N) const {
    if (ws_bytes < need)
      return fail(FMX_ERR_SHAPE, "%s: workspace of %lld bytes, %s_workspace_bytes(%s%d, %d, %d) = %lld", fn, (long long)ws_bytes, fn,
                  ws_args, U, N, K, (long long)need);
    return FMX_OK;
  }
};

struct RankEnd {
  const int32_t *targets;
  int32_t T, filtered;
  int32_t *rank_out;
  float *score_out;
  int32_t *n_cand_out;
  int scan_K() const { return 1; }
  const void *out_a() const { return targets; }
  const void *out_b() const { return rank_out; }
  int check_sizes(const char *fn, int32_t U, int32_t N) const {
    if (U < 1 || N < 1) return fail(FMX_ERR_ARG, "%s: U=%d and N=%d must be >= 1", fn, U, N);
    if (T < 1) return fail(FMX_ERR_ARG, "%s: T=%d must be >= 1", fn, T);
    if (T > RK_MAX_T) return fail(FMX_ERR_UNSUPPORTED, "%s: T=%d, one call covers T <= %d targets per user", fn, T, RK_MAX_T);
    return FMX_OK;
  }
  int check_flag(const char *fn) const {
    if (filtered != 0 && filtered != 1) return fail(FMX_ERR_ARG, "%s: filtered=%d must be 0 or 1", fn, filtered);
    return FMX_OK;
  }
  int64_t part_bytes(int64_t parts, int32_t U) const { return rank_ws_bytes(parts, U, T); }
  int check_ws(const char *fn, int64_t ws_bytes, int64_t need, const char *, int32_t, int32_t) const {
    if (ws_bytes < need)
      return fail(FMX_ERR_SHAPE, "%s: workspace of %lld bytes, %s_workspace_bytes = %lld", fn, (long long)ws_bytes, fn, (long long)need);
    return FMX_OK;
  }
};

// ---- the three families ---------------------------------------------------------------------------------------------------
struct ScanIn {  // what every family's call is given
  const char *fn;
  int32_t U, N, kp;
  const int32_t *excl_off, *excl_pos;
  void *ws;
  int64_t ws_bytes;
};

// The checks of the FM and network calls on their two sides, in this order.  A kp outside 4/8/16/32/64 returns bad_kp
// (include/fmx.h: FMX_ERR_SHAPE from the FM calls, FMX_ERR_UNSUPPORTED from the network's).
template <class Plan, class End>
int check_pair(const Plan &p, const End &e, int bad_kp, int64_t need, const char *ws_args) {
  const char *fn = p.fn;
  if (!p.Su || !p.au || !p.Sc || !p.ac || !p.ws || !e.out_a() || !e.out_b()) return fail(FMX_ERR_ARG, "%s: null argument", fn);
  if ((p.excl_off == nullptr) != (p.excl_pos == nullptr)) return fail(FMX_ERR_ARG, "%s: excl_offsets and excl_pos go together", fn);
  if (int rc = e.check_sizes(fn, p.U, p.N)) return rc;
  if (int rc = e.check_flag(fn)) return rc;
  if (!lpr_of(p.kp)) return fail(bad_kp, "%s: kp=%d must be 4/8/16/32/64", fn, p.kp);
  if (p.ld_u < p.kp || p.ld_c < p.kp || p.ld_u % 4 || p.ld_c % 4)
    return fail(FMX_ERR_SHAPE, "%s: ld_u=%d and ld_c=%d must be multiples of 4 and >= kp=%d", fn, p.ld_u, p.ld_c, p.kp);
  if (!aligned16(p.Su) || !aligned16(p.Sc) || !aligned16(p.ws))
    return fail(FMX_ERR_ALIGN, "%s: Su, Sc and the workspace must be 16-byte aligned", fn);
  return e.check_ws(fn, p.ws_bytes, need, ws_args, p.U, p.N);
}

struct FmScan : ScanIn {
  using Args = TopkArgs;
  using RankArgs = FmRankArgs;
  static constexpr const char *names[3] = {"k_topk_scan", "k_topk_scan (rank count)", "k_topk_scan (rank keys)"};
  const float *Su;
  int32_t ld_u;
  const float *au, *Sc;
  int32_t ld_c;
  const float *ac;
  TopkGeom g{};

  template <class End>
  static int64_t workspace_bytes(const char *fn, const End &e, int32_t U, int32_t N) {
    if (int rc = e.check_sizes(fn, U, N)) return rc;
    return e.part_bytes(fm_scan_parts(U, N), U);
  }
  template <class End>
  int check(const End &e) {
    return check_pair(*this, e, FMX_ERR_SHAPE, e.part_bytes(fm_scan_parts(U, N), U), "");
  }
  int64_t prefix() const { return 0; }
  int prepare(int K, hipStream_t) {
    g = topk_geom(U, N, K);
    return FMX_OK;
  }
  Args args(int K) const {
    return Args{Su, au, Sc, ac, excl_off, excl_pos, nullptr, nullptr, nullptr, ld_u, ld_c, U, N, K, g.ut, g.cap, g.splits, g.per};
  }
  int splits() const { return g.splits; }
  dim3 grid() const { return dim3(g.tiles, g.splits); }
  template <int MODE, class A>
  int launch(dim3 grid, A a, hipStream_t st) const {
    if (MODE == SCAN_KEYS) a.ut = 1;  // grid (U, T): one user per workgroup
    const size_t lds = MODE == SCAN_TOPK ? slots_lds(g.ut, g.cap) : 0;  // the counters are static LDS
    return with_kp(kp, [&](auto KP) { return launch_slots<k_topk_scan<KP, MODE, A>>(names[MODE], grid, lds, st, a); });
  }
};

int check_network(const char *fn, const fmx_mlp_t *mlp) {
  if (mlp->n_layers < 1 || mlp->n_layers > TM_MAX_L || mlp->hidden < 1 || mlp->hidden > TM_MAX_H || mlp->k < 1 || mlp->k > 64)
    return fail(FMX_ERR_UNSUPPORTED, "%s: needs 1 <= layers <= %d, 1 <= hidden <= %d, 1 <= k <= 64 (got %d, %d, %d)", fn, TM_MAX_L,
                TM_MAX_H, mlp->n_layers, mlp->hidden, mlp->k);
  return FMX_OK;
}

struct MlpScan : ScanIn {
  using Args = MlpTopkArgs;
  using RankArgs = MlpRankArgs;
  static constexpr const char *names[3] = {"k_mlp_topk_scan", "k_mlp_topk_scan (rank count)", "k_mlp_topk_scan (rank keys)"};
  const fmx_mlp_t *mlp;
  int32_t fm_term;
  const float *Su, *Bu;
  int32_t ld_u;
  const float *au, *Sc, *Bc;
  int32_t ld_c;
  const float *ac;
  MlpShape sh{};
  MlpTopkGeom g{};
  MlpPackArgs pk{};

  template <class End>
  static int64_t workspace_bytes(const char *fn, const fmx_mlp_t *mlp, const End &e, int32_t U, int32_t N) {
    if (!mlp) return fail(FMX_ERR_ARG, "%s: null mlp", fn);
    if (int rc = e.check_sizes(fn, U, N)) return rc;
    if (int rc = check_network(fn, mlp)) return rc;
    const MlpShape s = mlp_shape(mlp);
    return mlp_packed_floats(s, nullptr) * 4 + e.part_bytes(mlp_scan_parts(s, U, N), U);
  }
  template <class End>
  int check(const End &e) {
    if (!mlp || !mlp->params || !Bu || !Bc) return fail(FMX_ERR_ARG, "%s: null argument", fn);
    if (fm_term != 0 && fm_term != 1) return fail(FMX_ERR_ARG, "%s: fm_term=%d must be 0 or 1", fn, fm_term);
    if (int rc = check_network(fn, mlp)) return rc;
    if (mlp->k > kp) return fail(FMX_ERR_UNSUPPORTED, "%s: k=%d exceeds kp=%d", fn, mlp->k, kp);
    sh = mlp_shape(mlp);
    if (int rc = check_pair(*this, e, FMX_ERR_UNSUPPORTED, prefix() + e.part_bytes(mlp_scan_parts(sh, U, N), U), "mlp, ")) return rc;
    if (!aligned16(Bu) || !aligned16(Bc)) return fail(FMX_ERR_ALIGN, "%s: Bu and Bc must be 16-byte aligned", fn);
    return FMX_OK;
  }
  int64_t prefix() const { return mlp_packed_floats(sh, nullptr) * 4; }  // the packed weights
  int prepare(int K, hipStream_t st) {
    g = mlp_topk_geom(sh, U, N, K);
    pk = MlpPackArgs{mlp->params, static_cast<float *>(ws), {}, {}, {}, {}, 0, sh.k, sh.H, sh.L, sh.K0, sh.Hp, sh.NT};
    pk.total = mlp_packed_floats(sh, &pk);
    hipLaunchKernelGGL(k_mlp_topk_pack, dim3((unsigned)((pk.total + 255) / 256)), dim3(256), 0, st, pk);
    return check_launch("k_mlp_topk_pack");
  }
  Args args(int K) const {
    Args a{Su, Bu, au, Sc, Bc, ac, excl_off, excl_pos, pk.packed, {}, {}, nullptr, nullptr, nullptr,
           ld_u, ld_c, U, N, K, kp, sh.k, sh.H, sh.L, sh.K0, sh.Hp, fm_term, g.cap, g.splits, g.per};
    std::copy(pk.dst_w, pk.dst_w + sh.L, a.woff);
    std::copy(pk.dst_b, pk.dst_b + sh.L, a.boff);
    return a;
  }
  int splits() const { return g.splits; }
  dim3 grid() const { return dim3(U, g.splits); }
  template <int MODE, class A>
  int launch(dim3 grid, const A &a, hipStream_t st) const {
    // the activations, and the selection's slot behind them; the counters are static LDS
    const size_t lds = (size_t)TM_ROWS * std::max(sh.K0, sh.Hp) * 4 + (MODE == SCAN_TOPK ? slots_lds(1, g.cap) : 0);
    return with_wave_grid(sh.NT, [&](auto WC, auto NCT) {
      return launch_slots<k_mlp_topk_scan<WC, NCT, MODE, A>>(names[MODE], grid, lds, st, a);
    });
  }
};

struct AfmScan : ScanIn {
  using Args = AfmTopkArgs;
  using RankArgs = AfmRankArgs;
  static constexpr const char *names[3] = {"k_afm_topk_scan", "k_afm_topk_scan (rank count)", "k_afm_topk_scan (rank keys)"};
  const fmx_afm_t *afm;
  const float *Eu, *stats_u;
  int32_t n_ctx;
  const float *Ec, *stats_c;
  int32_t n_item;
  int per = 0, n_splits = 0, cap = 0;

  static int check_shape(const char *fn, const fmx_afm_t *afm, int32_t n_ctx, int32_t n_item) {
    if (afm->t < 1 || afm->t > 64 || afm->k < 1 || afm->k > 64)
      return fail(FMX_ERR_UNSUPPORTED, "%s: needs 1 <= t <= 64 and 1 <= k <= 64 (got t=%d, k=%d)", fn, afm->t, afm->k);
    if (n_ctx < 1 || n_item < 1) return fail(FMX_ERR_SHAPE, "%s: n_ctx=%d and n_item=%d must be >= 1", fn, n_ctx, n_item);
    if (n_ctx + n_item > 64) return fail(FMX_ERR_UNSUPPORTED, "%s: n_ctx + n_item = %d, the AFM takes at most 64 fields", fn, n_ctx + n_item);
    return FMX_OK;
  }
  template <class End>
  static int64_t workspace_bytes(const char *fn, const fmx_afm_t *afm, int32_t n_ctx, int32_t n_item, const End &e, int32_t U, int32_t N) {
    if (!afm) return fail(FMX_ERR_ARG, "%s: null afm", fn);
    if (int rc = e.check_sizes(fn, U, N)) return rc;
    if (int rc = check_shape(fn, afm, n_ctx, n_item)) return rc;
    return at_packed_bytes(afm->t) + e.part_bytes(afm_scan_parts(afm, n_ctx, n_item, U, N), U);
  }
  template <class End>
  int check(const End &e) {
    const int64_t need = workspace_bytes(fn, afm, n_ctx, n_item, e, U, N);  // the shape checks come first
    if (need < 0) return (int)need;
    if (!afm->params || !Eu || !stats_u || !Ec || !stats_c || !ws || !e.out_a() || !e.out_b()) return fail(FMX_ERR_ARG, "%s: null argument", fn);
    if ((excl_off == nullptr) != (excl_pos == nullptr)) return fail(FMX_ERR_ARG, "%s: excl_offsets and excl_pos go together", fn);
    if (!lpr_of(kp) || kp < afm->k) return fail(FMX_ERR_SHAPE, "%s: kp=%d must be 4/8/16/32/64 and >= k=%d", fn, kp, afm->k);
    if (!aligned16(Eu) || !aligned16(stats_u) || !aligned16(Ec) || !aligned16(stats_c) || !aligned16(ws))
      return fail(FMX_ERR_ALIGN, "%s: Eu, stats_u, Ec, stats_c and the workspace must be 16-byte aligned", fn);
    if (int rc = e.check_flag(fn)) return rc;
    char ws_args[48];
    snprintf(ws_args, sizeof ws_args, "afm, %d, %d, ", n_ctx, n_item);
    return e.check_ws(fn, ws_bytes, need, ws_args, U, N);
  }
  int64_t prefix() const { return at_packed_bytes(afm->t); }  // the padded parameter copy
  // one user per workgroup, splits = ceil(budget / U) within [1, max splits], a split a multiple of the chunk
  int prepare(int K, hipStream_t st) {
    const int64_t sm = at_split_min(n_ctx, n_item, afm->t, at_kp(afm->k));
    const int64_t sp = std::max<int64_t>(1, std::min<int64_t>(at_max_splits(sm, N), (AT_TILE_BUDGET + U - 1) / U));
    const int64_t per0 = (N + sp - 1) / sp;
    per = (int)((per0 + TK_THREADS - 1) / TK_THREADS * TK_THREADS);
    n_splits = (N + per - 1) / per;
    cap = topk_cap(K);
    const int packed_n = afm->t * kp + 2 * afm->t + kp;
    hipLaunchKernelGGL(k_afm_topk_pack, dim3((packed_n + 255) / 256), dim3(256), 0, st, afm->params, afm->k, afm->t, kp,
                       static_cast<float *>(ws));
    return check_launch("k_afm_topk_pack");
  }
  Args args(int K) const {
    return Args{Eu, stats_u, Ec, stats_c, static_cast<const float *>(ws), excl_off, excl_pos, nullptr, nullptr, nullptr,
                U, N, K, afm->t, n_ctx, n_item, cap, n_splits, per};
  }
  int splits() const { return n_splits; }
  dim3 grid() const { return dim3(U, n_splits); }
  template <int MODE, class A>
  int launch(dim3 grid, const A &a, hipStream_t st) const {
    const size_t lds = MODE == SCAN_TOPK ? slots_lds(1, cap) : 0;
    return with_kp(kp, [&](auto KP) { return launch_slots<k_afm_topk_scan<KP, MODE, A>>(names[MODE], grid, lds, st, a); });
  }
};

// ---- the two drivers ------------------------------------------------------------------------------------------------------
// the scan into partial lists behind the family's prefix (or, with one split, into the final rows), then the merge
template <class Plan>
int scan_topk(Plan p, const TopkEnd &e, fmx_stream_t stream) {
  if (int rc = p.check(e)) return rc;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (int rc = p.prepare(e.K, st)) return rc;
  typename Plan::Args a = p.args(e.K);
  a.parts = reinterpret_cast<uint64_t *>(static_cast<char *>(p.ws) + p.prefix());
  a.top_pos = e.top_pos;
  a.top_score = e.top_score;
  if (int rc = p.template launch<SCAN_TOPK>(p.grid(), a, st)) return rc;
  return merge_topk(a.parts, e.top_pos, e.top_score, p.U, e.K, p.splits(), st);
}

// the targets' keys on grid (U, T), the counting scan on the family's grid, then the finishing launch; the keys and the partial
// counts lie behind the family's prefix
template <class Plan>
int scan_rank(Plan p, const RankEnd &e, fmx_stream_t stream) {
  if (int rc = p.check(e)) return rc;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (int rc = p.prepare(1, st)) return rc;
  char *base = static_cast<char *>(p.ws) + p.prefix();
  const typename Plan::RankArgs a{p.args(1), RankIo{e.targets, reinterpret_cast<uint64_t *>(base),
                                                    reinterpret_cast<int32_t *>(base + rank_keys_bytes(p.U, e.T)), e.T}};
  if (int rc = p.template launch<SCAN_KEYS>(dim3(p.U, e.T), a, st)) return rc;
  if (int rc = p.template launch<SCAN_COUNT>(p.grid(), a, st)) return rc;
  return finish_rank(a.r, p.excl_off, p.excl_pos, p.U, p.N, p.splits(), e.filtered, e.rank_out, e.score_out, e.n_cand_out, st);
}

}  // namespace

extern "C" {

int64_t fmx_fm_topk_workspace_bytes(int32_t U, int32_t N, int32_t K) {
  return FmScan::workspace_bytes("fmx_fm_topk", TopkEnd{K, nullptr, nullptr}, U, N);
}
int64_t fmx_fm_rank_workspace_bytes(int32_t U, int32_t N, int32_t T) {
  return FmScan::workspace_bytes("fmx_fm_rank", RankEnd{nullptr, T, 0, nullptr, nullptr, nullptr}, U, N);
}
int64_t fmx_mlp_topk_workspace_bytes(const fmx_mlp_t *mlp, int32_t U, int32_t N, int32_t K) {
  return MlpScan::workspace_bytes("fmx_mlp_topk", mlp, TopkEnd{K, nullptr, nullptr}, U, N);
}
int64_t fmx_mlp_rank_workspace_bytes(const fmx_mlp_t *mlp, int32_t U, int32_t N, int32_t T) {
  return MlpScan::workspace_bytes("fmx_mlp_rank", mlp, RankEnd{nullptr, T, 0, nullptr, nullptr, nullptr}, U, N);
}
int64_t fmx_afm_topk_workspace_bytes(const fmx_afm_t *afm, int32_t n_ctx, int32_t n_item, int32_t U, int32_t N, int32_t K) {
  return AfmScan::workspace_bytes("fmx_afm_topk", afm, n_ctx, n_item, TopkEnd{K, nullptr, nullptr}, U, N);
}
int64_t fmx_afm_rank_workspace_bytes(const fmx_afm_t *afm, int32_t n_ctx, int32_t n_item, int32_t U, int32_t N, int32_t T) {
  return AfmScan::workspace_bytes("fmx_afm_rank", afm, n_ctx, n_item, RankEnd{nullptr, T, 0, nullptr, nullptr, nullptr}, U, N);
}

int fmx_fm_topk(const float *Su, int32_t ld_u, const float *au, int32_t U, const float *Sc, int32_t ld_c, const float *ac, int32_t N,
                int32_t kp, const int32_t *excl_offsets, const int32_t *excl_pos, int32_t K, void *workspace, int64_t workspace_bytes,
                int32_t *top_pos, float *top_score, fmx_stream_t stream) {
  return scan_topk(FmScan{{"fmx_fm_topk", U, N, kp, excl_offsets, excl_pos, workspace, workspace_bytes}, Su, ld_u, au, Sc, ld_c, ac},
                   TopkEnd{K, top_pos, top_score}, stream);
}

int fmx_fm_rank(const float *Su, int32_t ld_u, const float *au, int32_t U, const float *Sc, int32_t ld_c, const float *ac, int32_t N,
                int32_t kp, const int32_t *excl_offsets, const int32_t *excl_pos, const int32_t *targets, int32_t T, int32_t filtered,
                void *workspace, int64_t workspace_bytes, int32_t *rank_out, float *score_out, int32_t *n_cand_out,
                fmx_stream_t stream) {
  return scan_rank(FmScan{{"fmx_fm_rank", U, N, kp, excl_offsets, excl_pos, workspace, workspace_bytes}, Su, ld_u, au, Sc, ld_c, ac},
                   RankEnd{targets, T, filtered, rank_out, score_out, n_cand_out}, stream);
}

int fmx_mlp_topk(const fmx_mlp_t *mlp, int32_t fm_term, const float *Su, const float *Bu, int32_t ld_u, const float *au, int32_t U,
                 const float *Sc, const float *Bc, int32_t ld_c, const float *ac, int32_t N, int32_t kp, const int32_t *excl_offsets,
                 const int32_t *excl_pos, int32_t K, void *workspace, int64_t workspace_bytes, int32_t *top_pos, float *top_score,
                 fmx_stream_t stream) {
  return scan_topk(MlpScan{{"fmx_mlp_topk", U, N, kp, excl_offsets, excl_pos, workspace, workspace_bytes},
                           mlp, fm_term, Su, Bu, ld_u, au, Sc, Bc, ld_c, ac},
                   TopkEnd{K, top_pos, top_score}, stream);
}

int fmx_mlp_rank(const fmx_mlp_t *mlp, int32_t fm_term, const float *Su, const float *Bu, int32_t ld_u, const float *au, int32_t U,
                 const float *Sc, const float *Bc, int32_t ld_c, const float *ac, int32_t N, int32_t kp, const int32_t *excl_offsets,
                 const int32_t *excl_pos, const int32_t *targets, int32_t T, int32_t filtered, void *workspace, int64_t workspace_bytes,
                 int32_t *rank_out, float *score_out, int32_t *n_cand_out, fmx_stream_t stream) {
  return scan_rank(MlpScan{{"fmx_mlp_rank", U, N, kp, excl_offsets, excl_pos, workspace, workspace_bytes},
                           mlp, fm_term, Su, Bu, ld_u, au, Sc, Bc, ld_c, ac},
                   RankEnd{targets, T, filtered, rank_out, score_out, n_cand_out}, stream);
}

int fmx_afm_topk(const fmx_afm_t *afm, const float *Eu, const float *stats_u, int32_t n_ctx, int32_t U, const float *Ec,
                 const float *stats_c, int32_t n_item, int32_t N, int32_t kp, const int32_t *excl_offsets, const int32_t *excl_pos,
                 int32_t K, void *workspace, int64_t workspace_bytes, int32_t *top_pos, float *top_score, fmx_stream_t stream) {
  return scan_topk(AfmScan{{"fmx_afm_topk", U, N, kp, excl_offsets, excl_pos, workspace, workspace_bytes},
                           afm, Eu, stats_u, n_ctx, Ec, stats_c, n_item},
                   TopkEnd{K, top_pos, top_score}, stream);
}

int fmx_afm_rank(const fmx_afm_t *afm, const float *Eu, const float *stats_u, int32_t n_ctx, int32_t U, const float *Ec,
                 const float *stats_c, int32_t n_item, int32_t N, int32_t kp, const int32_t *excl_offsets, const int32_t *excl_pos,
                 const int32_t *targets, int32_t T, int32_t filtered, void *workspace, int64_t workspace_bytes, int32_t *rank_out,
                 float *score_out, int32_t *n_cand_out, fmx_stream_t stream) {
  return scan_rank(AfmScan{{"fmx_afm_rank", U, N, kp, excl_offsets, excl_pos, workspace, workspace_bytes},
                           afm, Eu, stats_u, n_ctx, Ec, stats_c, n_item},
                   RankEnd{targets, T, filtered, rank_out, score_out, n_cand_out}, stream);
}

}  // extern "C"
