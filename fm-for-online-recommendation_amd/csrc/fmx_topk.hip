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
#include "fmx_common.h"

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
inline TopkGeom topk_geom(int U, int N, int K) {
  TopkGeom g;
  g.ut = K <= 128 ? 16 : 8;
  g.cap = K <= 128 ? 512 : 1024;
  g.tiles = (U + g.ut - 1) / g.ut;
  const int sn = std::min(TK_MAX_SPLITS, (N + TK_SPLIT_MIN - 1) / TK_SPLIT_MIN);
  const int s = std::max(1, std::min(sn, TK_TILE_BUDGET / g.tiles));
  const int per0 = (N + s - 1) / s;
  g.per = (per0 + TK_THREADS - 1) / TK_THREADS * TK_THREADS;
  g.splits = (N + g.per - 1) / g.per;
  return g;
}

// Partial lists in the workspace: uint64 [U, splits, K].  Bounded by a formula that is monotone in U, N and K (the splits
// of the geometry are not): splits <= ceil(N / TK_SPLIT_MIN) and U * splits <= U + TK_TILE_BUDGET * TK_MAX_UT.
inline int64_t topk_ws_bytes(int U, int N, int K) {
  const int64_t sn = std::min<int64_t>(TK_MAX_SPLITS, (N + TK_SPLIT_MIN - 1) / TK_SPLIT_MIN);
  const int64_t parts = std::min<int64_t>((int64_t)U * sn, (int64_t)U + (int64_t)TK_TILE_BUDGET * TK_MAX_UT);
  return parts * K * 8;
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

// grid (user tiles, splits).  Thread t scores candidate c0 + t against every user of the tile; the user's S_u and a_u are
// wave-uniform (scalar loads), the candidate's S_c row sits in the thread's registers for the whole chunk.
//   score(u, c) = (au[u] + ac[c]) + dot,   dot = fma(Su[kp-1], Sc[kp-1], ... fma(Su[1], Sc[1], Su[0] * Sc[0]))
template <int KP>
__global__ __launch_bounds__(TK_THREADS) void k_topk_scan(TopkArgs a) {
  extern __shared__ uint64_t tk_lds[];
  Slots s;
  const int u0 = blockIdx.x * a.ut, nu = min(a.ut, a.U - u0);
  init_slots(s, tk_lds, nu, a.cap);
  const int c_begin = blockIdx.y * a.per, c_end = min(a.N, c_begin + a.per);
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
        score[r] = (au[u] + acv) + acc;
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int j = j0 + r;
        if (R > 1 && j >= nu) break;
        const uint64_t key = make_key(score[r], c);
        bool keep = valid && score[r] == score[r] && key > s.thr[j];
        if (keep && a.excl_off) keep = !excluded(a.excl_off, a.excl_pos, u0 + j, c);
        append(s, j, a.cap, keep, key);
      }
    }
    __syncthreads();
    // after the first chunk every slot is cut to K at once (the thresholds start rising); later only slots that could overflow
    compact(s, nu, a.cap, a.K, c0 == c_begin ? a.K : a.cap - TK_THREADS);
  }
  compact(s, nu, a.cap, a.K, -1);
  for (int j = 0; j < nu; ++j) {
    const int u = u0 + j;
    if (a.splits > 1)
      emit(s, j, a.cap, a.K, a.parts + ((size_t)u * a.splits + blockIdx.y) * a.K, nullptr, nullptr);
    else
      emit(s, j, a.cap, a.K, nullptr, a.top_pos + (size_t)u * a.K, a.top_score + (size_t)u * a.K);
  }
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

size_t slots_lds(int n, int cap) { return (size_t)n * cap * 8 + (size_t)n * 8 + (size_t)n * 4; }

template <int KP>
int launch_topk(const TopkArgs &a, const TopkGeom &g, hipStream_t st) {
  static const bool raised = [] {  // 64 KiB of keys + the counts and thresholds: above the default dynamic LDS limit
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_topk_scan<KP>), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_topk_merge), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
    return true;
  }();
  (void)raised;
  hipLaunchKernelGGL(k_topk_scan<KP>, dim3(g.tiles, g.splits), dim3(TK_THREADS), slots_lds(g.ut, g.cap), st, a);
  if (int rc = check_launch("k_topk_scan")) return rc;
  if (g.splits == 1) return FMX_OK;
  hipLaunchKernelGGL(k_topk_merge, dim3(a.U), dim3(TK_THREADS), slots_lds(1, g.cap), st, a);
  return check_launch("k_topk_merge");
}

int check_topk_sizes(int32_t U, int32_t N, int32_t K) {
  if (U < 1 || N < 1) return fail(FMX_ERR_ARG, "fmx_fm_topk: U=%d and N=%d must be >= 1", U, N);
  if (K < 1) return fail(FMX_ERR_ARG, "fmx_fm_topk: K=%d must be >= 1", K);
  if (K > TK_MAX_K) return fail(FMX_ERR_UNSUPPORTED, "fmx_fm_topk: K=%d, the kernels cover K <= %d", K, TK_MAX_K);
  return FMX_OK;
}

}  // namespace

extern "C" {

int64_t fmx_fm_topk_workspace_bytes(int32_t U, int32_t N, int32_t K) {
  if (int rc = check_topk_sizes(U, N, K)) return rc;
  return topk_ws_bytes(U, N, K);
}

int fmx_fm_topk(const float *Su, int32_t ld_u, const float *au, int32_t U, const float *Sc, int32_t ld_c, const float *ac, int32_t N,
                int32_t kp, const int32_t *excl_offsets, const int32_t *excl_pos, int32_t K, void *workspace, int64_t workspace_bytes,
                int32_t *top_pos, float *top_score, fmx_stream_t stream) {
  if (!Su || !au || !Sc || !ac || !workspace || !top_pos || !top_score) return fail(FMX_ERR_ARG, "fmx_fm_topk: null argument");
  if ((excl_offsets == nullptr) != (excl_pos == nullptr))
    return fail(FMX_ERR_ARG, "fmx_fm_topk: excl_offsets and excl_pos go together");
  if (int rc = check_topk_sizes(U, N, K)) return rc;
  if (kp != 4 && kp != 8 && kp != 16 && kp != 32 && kp != 64) return fail(FMX_ERR_SHAPE, "fmx_fm_topk: kp=%d must be 4/8/16/32/64", kp);
  if (ld_u < kp || ld_c < kp || ld_u % 4 || ld_c % 4)
    return fail(FMX_ERR_SHAPE, "fmx_fm_topk: ld_u=%d and ld_c=%d must be multiples of 4 and >= kp=%d", ld_u, ld_c, kp);
  if (!aligned16(Su) || !aligned16(Sc) || !aligned16(workspace))
    return fail(FMX_ERR_ALIGN, "fmx_fm_topk: Su, Sc and the workspace must be 16-byte aligned");
  const int64_t need = topk_ws_bytes(U, N, K);
  if (workspace_bytes < need)
    return fail(FMX_ERR_SHAPE, "fmx_fm_topk: workspace of %lld bytes, fmx_fm_topk_workspace_bytes(%d, %d, %d) = %lld",
                (long long)workspace_bytes, U, N, K, (long long)need);
  const TopkGeom g = topk_geom(U, N, K);
  TopkArgs a;
  a.Su = Su;
  a.au = au;
  a.Sc = Sc;
  a.ac = ac;
  a.excl_off = excl_offsets;
  a.excl_pos = excl_pos;
  a.parts = static_cast<uint64_t *>(workspace);
  a.top_pos = top_pos;
  a.top_score = top_score;
  a.ld_u = ld_u;
  a.ld_c = ld_c;
  a.U = U;
  a.N = N;
  a.K = K;
  a.ut = g.ut;
  a.cap = g.cap;
  a.splits = g.splits;
  a.per = g.per;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  switch (kp) {
    case 4: return launch_topk<4>(a, g, st);
    case 8: return launch_topk<8>(a, g, st);
    case 16: return launch_topk<16>(a, g, st);
    case 32: return launch_topk<32>(a, g, st);
    default: return launch_topk<64>(a, g, st);
  }
}

}  // extern "C"
