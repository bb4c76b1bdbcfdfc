// fmx_rank.inc -- exact ranks of held-out targets (fmx_fm_rank, fmx_mlp_rank, fmx_afm_rank; include/fmx.h): the device
// side that the three scans of fmx_topk.hip share.  Included by fmx_topk.hip ahead of its scans, which are templates on what
// they do with a score (SCAN_TOPK / SCAN_COUNT / SCAN_KEYS below): the score is the scan's own loop, instantiated again, the
// order is make_key's, the exclusion test is excluded().  What a scan does with a score in each of the three is stated once,
// in ScanSink below (the AFM scan, which measured slower through it, spells it out itself); the entry points are at the end of
// fmx_topk.hip.
//
// Two phases per family.  Phase 1 (SCAN_KEYS) scores the U x T target pairs and writes their keys (0: no eligible target) to
// the workspace.  Phase 2 (SCAN_COUNT) is the family's scan with the selection slots replaced by counters: for every user of the tile the T
// target keys sit in LDS (wave-uniform reads), a lane whose key beats a target key counts for it, counts are added per wave
// (one ballot and one LDS atomic per target that some lane beats), and the split's counters go to the workspace as partial
// sums int32 [U, splits, T + 1] (column T: the split's non-excluded NaN scores).  k_rank_finish folds the splits, applies
// `filtered` and writes the outputs.  Everything summed is an integer: the result does not depend on the order.

namespace {

constexpr int RK_MAX_T = 16;

// keys uint64 [U, T], then the partial counts int32 [parts, T + 1]
inline int64_t rank_keys_bytes(int U, int T) { return (int64_t)align_up((size_t)U * T * 8, 16); }
inline int64_t rank_ws_bytes(int64_t parts, int U, int T) { return rank_keys_bytes(U, T) + parts * (T + 1) * 4; }

struct RankIo {  // what the three families' rank kernels add to their top-K arguments
  const int32_t *targets;  // [U, T]
  uint64_t *tkeys;         // [U, T]
  int32_t *cnt;            // [U, splits, T + 1]
  int T;
};
struct FmRankArgs : TopkArgs {  // MlpRankArgs and AfmRankArgs follow their families' arguments in fmx_topk.hip
  RankIo r;
};

// What a scan does with its scores.  SCAN_TOPK: the selection slots.  SCAN_COUNT: phase 2.  SCAN_KEYS: phase 1 -- grid
// (U, T), workgroup (u, t) runs the scan's loop over the one chunk of consecutive candidates that holds targets[u, t], and the
// lane that holds the target writes its key.  The loop that computes the score is the same source in all three.
enum { SCAN_TOPK = 0, SCAN_COUNT = 1, SCAN_KEYS = 2 };

// SCAN_KEYS: target (u, t) when it lies in [0, N), else -1 after writing key 0 (the workgroup has nothing to scan)
__device__ __forceinline__ int keys_target(const RankIo &io, int u, int t, int N) {
  const int p = io.targets[(size_t)u * io.T + t];
  if (p >= 0 && p < N) return p;
  if (threadIdx.x == 0) io.tkeys[(size_t)u * io.T + t] = 0;
  return -1;
}

// the key of target p of user u with score `score`: 0 unless p is eligible (the caller has checked 0 <= p < N)
__device__ __forceinline__ uint64_t target_key(float score, int p, const int32_t *excl_off, const int32_t *excl_pos, int u) {
  if (!(score == score)) return 0;
  if (excl_off && excluded(excl_off, excl_pos, u, p)) return 0;
  return make_key(score, p);
}

struct RankLds {  // of n users: target keys [n][T], the smallest non-zero one [n] (all ones: none), counters [n][T + 1]
  uint64_t *tkey, *kmin;
  int *cnt;
};
template <int NU>
struct RankShared {
  uint64_t tkey[NU * RK_MAX_T], kmin[NU];
  int cnt[NU * (RK_MAX_T + 1)];
};

// tkeys: the keys of the tile's first user (the tile's users are consecutive rows).  Leaves through a barrier.
template <int NU>
__device__ void init_rank(RankLds &r, RankShared<NU> &sh, const uint64_t *tkeys, int n, int T) {
  r.tkey = sh.tkey;
  r.kmin = sh.kmin;
  r.cnt = sh.cnt;
  for (int i = threadIdx.x; i < n * T; i += blockDim.x) r.tkey[i] = tkeys[i];
  for (int i = threadIdx.x; i < n * (T + 1); i += blockDim.x) r.cnt[i] = 0;
  __syncthreads();
  if ((int)threadIdx.x < n) {
    uint64_t m = ~0ull;
    for (int t = 0; t < T; ++t) {
      const uint64_t k = r.tkey[threadIdx.x * T + t];
      if (k != 0 && k < m) m = k;
    }
    r.kmin[threadIdx.x] = m;
  }
  __syncthreads();
}

// This lane's pair (user u = slot j, candidate c) against the user's targets.  Like the top-K scan, the exclusion list is
// searched only by a lane that would count: one whose key beats some target key, or whose score is NaN (n_cand).  Called by
// whole waves.
__device__ __forceinline__ void count_pair(const RankLds &r, int j, int T, bool valid, float score, uint64_t key,
                                           const int32_t *excl_off, const int32_t *excl_pos, int u, int c) {
  bool nan = valid && !(score == score);
  bool cand = valid && score == score && key > r.kmin[j];
  if ((cand || nan) && excl_off) {
    const bool ex = excluded(excl_off, excl_pos, u, c);
    cand = cand && !ex;
    nan = nan && !ex;
  }
  const int lane = threadIdx.x & (WAVE - 1);
  int *cnt = r.cnt + j * (T + 1);
  const uint64_t mn = __ballot(nan);
  if (mn != 0 && lane == 0) atomicAdd(&cnt[T], (int)__popcll(mn));
  if (__ballot(cand) == 0) return;
  const uint64_t *tk = r.tkey + j * T;
  for (int t = 0; t < T; ++t) {
    const uint64_t k = tk[t];
    if (k == 0) continue;
    const uint64_t m = __ballot(cand && key > k);
    if (m != 0 && lane == 0) atomicAdd(&cnt[t], (int)__popcll(m));
  }
}

// the split's counters of the tile's n users (first user u0) to the workspace; entered after a barrier
__device__ void emit_counts(const RankLds &r, const RankIo &io, int u0, int n, int splits, int split) {
  const int W = io.T + 1;
  for (int i = threadIdx.x; i < n * W; i += blockDim.x) {
    const int j = i / W, t = i - j * W;
    io.cnt[((size_t)(u0 + j) * splits + split) * W + t] = r.cnt[i];
  }
}

// What a scan does with its scores, for the users u0 .. u0 + nu - 1 of a workgroup (nu <= NU; CHUNK: the candidates the scan
// scores between two cuts).  The scan keeps its score loop and its barriers; the MODE is spelled out here only.
//   open:  the mode's LDS state and the workgroup's candidates [c_begin, c_end); false when a SCAN_KEYS workgroup has no target
//   take:  the pair (slot j, candidate c) with its score; called by whole waves
//   cut:   after a chunk, SCAN_TOPK: the slots that could overflow go back to their K best.  Entered after a barrier.
//   close: the workgroup's results to the workspace or the final rows.  SCAN_COUNT: entered after a barrier.
template <int MODE, int NU, int CHUNK>
struct ScanSink {
  Slots s;
  RankLds rk;
  int target, u0, nu, c_begin, c_end;

  template <class Args, class User>
  __device__ __forceinline__ bool open(const Args &a, uint64_t *slot_lds, User first_user, int users) {
    u0 = (int)first_user;
    nu = users;
    target = -1;
    if constexpr (MODE == SCAN_TOPK) init_slots(s, slot_lds, nu, a.cap);
    if constexpr (MODE == SCAN_COUNT) {
      __shared__ RankShared<NU> sh;
      init_rank(rk, sh, a.r.tkeys + (size_t)first_user * a.r.T, nu, a.r.T);
    }
    if constexpr (MODE == SCAN_KEYS) {
      target = keys_target(a.r, u0, blockIdx.y, a.N);
      if (target < 0) return false;
    }
    c_begin = MODE == SCAN_KEYS ? target / CHUNK * CHUNK : blockIdx.y * a.per;
    c_end = min(a.N, c_begin + (MODE == SCAN_KEYS ? CHUNK : a.per));
    return true;
  }

  template <class Args>
  __device__ __forceinline__ void take(const Args &a, int j, int c, bool valid, float score) {
    const uint64_t key = make_key(score, c);
    if constexpr (MODE == SCAN_TOPK) {
      bool keep = valid && score == score && key > s.thr[j];
      if (keep && a.excl_off) keep = !excluded(a.excl_off, a.excl_pos, u0 + j, c);
      append(s, j, a.cap, keep, key);
    } else if constexpr (MODE == SCAN_COUNT) {
      count_pair(rk, j, a.r.T, valid, score, key, a.excl_off, a.excl_pos, u0 + j, c);
    } else if (valid && c == target) {  // (one user per workgroup: j = 0)
      a.r.tkeys[(size_t)u0 * a.r.T + blockIdx.y] = target_key(score, c, a.excl_off, a.excl_pos, u0);
    }
  }

  // after the first chunk every slot is cut to K at once (the thresholds start rising); later only slots that could overflow
  template <class Args>
  __device__ __forceinline__ void cut(const Args &a, int c0) {
    if constexpr (MODE == SCAN_TOPK) compact(s, nu, a.cap, a.K, c0 == c_begin ? a.K : a.cap - CHUNK);
  }

  template <class Args>
  __device__ __forceinline__ void close(const Args &a) {
    if constexpr (MODE == SCAN_COUNT) emit_counts(rk, a.r, u0, nu, a.splits, blockIdx.y);
    if constexpr (MODE == SCAN_TOPK) {
      compact(s, nu, a.cap, a.K, -1);
      for (int j = 0; j < nu; ++j) {
        const int u = u0 + j;
        if (a.splits > 1)
          emit(s, j, a.cap, a.K, a.parts + ((size_t)u * a.splits + blockIdx.y) * a.K, nullptr, nullptr);
        else
          emit(s, j, a.cap, a.K, nullptr, a.top_pos + (size_t)u * a.K, a.top_score + (size_t)u * a.K);
      }
    }
  }
};

// ---- the finishing launch: one workgroup per user ----------------------------------------------------------------------
struct RankFinishArgs {
  const uint64_t *tkeys;
  const int32_t *cnt;
  const int32_t *excl_off, *excl_pos;
  int32_t *rank_out;
  float *score_out;
  int32_t *n_cand_out;
  int N, T, splits, filtered;
};
constexpr int RK_FINISH_THREADS = 256;

// The user's T + 1 columns of partial counts are summed over the splits by stripes of threads (a user has up to 1024 splits:
// one lane walking them alone took 39 us of a 0.25 ms call), the user's distinct exclusions inside [0, N) are counted by all
// threads, both into LDS integers.  Then thread t < T: the target's count; under `filtered`, less the user's other distinct
// targets with a greater key (each was counted once as a candidate, however often it is listed).  n_cand = N - the exclusions
// - the non-excluded NaN scores.
__global__ __launch_bounds__(RK_FINISH_THREADS) void k_rank_finish(RankFinishArgs f) {
  __shared__ int tot[RK_MAX_T + 1];
  __shared__ int gone;
  const int u = blockIdx.x, tid = threadIdx.x, T = f.T, W = T + 1;
  const uint64_t *tk = f.tkeys + (size_t)u * T;
  const int32_t *cnt = f.cnt + (size_t)u * f.splits * W;
  if (tid < W) tot[tid] = 0;
  if (tid == 0) gone = 0;
  __syncthreads();
  const int col = tid % W, stripe = tid / W, stripes = RK_FINISH_THREADS / W;
  if (stripe < stripes) {
    int sum = 0;
    for (int s = stripe; s < f.splits; s += stripes) sum += cnt[(size_t)s * W + col];
    if (sum != 0) atomicAdd(&tot[col], sum);
  }
  if (f.n_cand_out && f.excl_off) {
    const int b = f.excl_off[u], e = f.excl_off[u + 1];
    int mine = 0;
    for (int i = b + tid; i < e; i += RK_FINISH_THREADS) {
      const int p = f.excl_pos[i];
      mine += (p >= 0 && p < f.N && (i == b || f.excl_pos[i - 1] != p)) ? 1 : 0;
    }
    if (mine != 0) atomicAdd(&gone, mine);
  }
  __syncthreads();
  if (tid < T) {
    const uint64_t key = tk[tid];
    int rank = -1;
    if (key != 0) {
      rank = tot[tid];
      if (f.filtered)
        for (int t2 = 0; t2 < T; ++t2) {
          const uint64_t k2 = tk[t2];
          if (k2 <= key) continue;
          bool first = true;
          for (int t3 = 0; t3 < t2; ++t3) first = first && tk[t3] != k2;
          rank -= first ? 1 : 0;
        }
    }
    f.rank_out[(size_t)u * T + tid] = rank;
    if (f.score_out) f.score_out[(size_t)u * T + tid] = key != 0 ? key_score(key) : -INFINITY;
  }
  if (f.n_cand_out && tid == 0) f.n_cand_out[u] = f.N - gone - tot[T];
}

int finish_rank(const RankIo &io, const int32_t *excl_off, const int32_t *excl_pos, int32_t U, int32_t N, int splits, int32_t filtered,
                int32_t *rank_out, float *score_out, int32_t *n_cand_out, hipStream_t st) {
  const RankFinishArgs f{io.tkeys, io.cnt, excl_off, excl_pos, rank_out, score_out, n_cand_out, N, io.T, splits, filtered};
  hipLaunchKernelGGL(k_rank_finish, dim3(U), dim3(RK_FINISH_THREADS), 0, st, f);
  return check_launch("k_rank_finish");
}

}  // namespace
