// fmx_mine.inc -- hard negatives for pairwise (BPR) training (fmx_fm_mine_negatives; include/fmx.h): per user, n_draw candidate
// positions drawn with Philox4x32-10, scored with fmx_fm_topk's score (fm_score, fmx_topk.hip), and the n_neg best eligible
// ones kept in make_key's order.  Included by fmx_topk.hip after fmx_rank.inc: the key, the score and excluded() are that
// file's, not restated.  Behind it, on the same draw layout and the same excluded(): popularity-sampled negatives from an alias
// table (fmx_alias_sample_negatives, k_alias_sample), which score nothing.
//
// A wavefront owns a user (four per workgroup, no LDS, no barrier, no atomics).  S_u, a_u, own_pos[u] and the user's
// exclusion bounds are wave-uniform (scalar loads).  Lane l takes draws l, l + 64, ...: at most MN_SLOTS = 16 per lane at
// n_draw = 1024, whose keys stay in registers (the loop over them is unrolled: constant register indices, no scratch).  A draw
// that is not eligible holds key 0, which is no candidate.  Selection: n_neg rounds of (the lane's greatest key, the wave's
// greatest by __shfl_xor, every lane clears the keys equal to it -- a position drawn twice has one key, so this is the
// de-duplication -- lane 0 stores).  Every loop is bounded by n_draw, n_neg or the exclusion list's length.
//
// The row gather: each lane loads its own candidate's row (KP / 4 16-byte loads at addresses no neighbour shares).

namespace {

constexpr int MN_MAX_DRAW = 1024, MN_MAX_NEG = 16;
constexpr int MN_WAVES = 4;                     // users per workgroup
constexpr int MN_SLOTS = MN_MAX_DRAW / WAVE;    // draws per lane

struct MineArgs {
  const float *Su, *au, *Sc, *ac;
  const int32_t *excl_off, *excl_pos, *own_pos;
  int32_t *neg_pos;
  float *neg_score;
  uint32_t key0, key1, off0, off1, u_base;
  int ld_u, ld_c, U, N, n_draw, n_neg;
};

// word `w` of Philox4x32-10 (Salmon et al. 2011) of counter (c0, c1, c2, c3) under key (k0, k1)
__device__ __forceinline__ uint32_t philox_word(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, int w) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = __umulhi(M0, c0), l0 = M0 * c0, h1 = __umulhi(M1, c2), l1 = M1 * c2;
    c0 = h1 ^ c1 ^ k0;
    c1 = l1;
    c2 = h0 ^ c3 ^ k1;
    c3 = l0;
    k0 += W0;
    k1 += W1;
  }
  return w == 0 ? c0 : w == 1 ? c1 : w == 2 ? c2 : c3;
}

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
  for (int m = 1; m < WAVE; m <<= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m);
    const uint64_t o = ((uint64_t)hi << 32) | lo;
    v = o > v ? o : v;
  }
  return v;
}

template <int KP>
__global__ __launch_bounds__(MN_WAVES *WAVE) void k_fm_mine(MineArgs a) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int u = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * MN_WAVES + (threadIdx.x >> 6)));
  if (u >= a.U) return;
  const float4 *su = reinterpret_cast<const float4 *>(a.Su + (size_t)u * a.ld_u);
  const int own = a.own_pos ? a.own_pos[u] : -1;
  const uint32_t uid = a.u_base + (uint32_t)u;
  uint64_t keys[MN_SLOTS];
#pragma unroll
  for (int i = 0; i < MN_SLOTS; ++i) {
    keys[i] = 0;
    if (i * WAVE < a.n_draw) {  // wave-uniform
      const int j = i * WAVE + lane;
      const uint32_t word = philox_word(a.key0, a.key1, a.off0, a.off1, uid, (uint32_t)(j >> 2), j & 3);
      const int c = (int)__umulhi(word, (uint32_t)a.N);  // (word * N) >> 32 < N
      const float4 *row = reinterpret_cast<const float4 *>(a.Sc + (size_t)c * a.ld_c);
      float4 v[KP / 4];
#pragma unroll
      for (int q = 0; q < KP / 4; ++q) v[q] = row[q];
      const float score = fm_score<KP>(su, a.au, u, v, a.ac[c]);
      bool ok = j < a.n_draw && score == score && c != own;
      if (ok && a.excl_off) ok = !excluded(a.excl_off, a.excl_pos, u, c);
      keys[i] = ok ? make_key(score, c) : 0;
    }
  }
  int32_t *out_pos = a.neg_pos + (size_t)u * a.n_neg;
  float *out_score = a.neg_score + (size_t)u * a.n_neg;
  for (int r = 0; r < a.n_neg; ++r) {
    uint64_t best = keys[0];
#pragma unroll
    for (int i = 1; i < MN_SLOTS; ++i) best = keys[i] > best ? keys[i] : best;
    best = wave_max_u64(best);
#pragma unroll
    for (int i = 0; i < MN_SLOTS; ++i) keys[i] = keys[i] == best ? 0 : keys[i];
    if (lane == 0) {
      out_pos[r] = best ? key_pos(best) : -1;
      out_score[r] = best ? key_score(best) : -INFINITY;
    }
  }
}

// ---- popularity-sampled negatives: fmx_alias_sample_negatives (include/fmx.h) ----
// Walker's alias method over a table built on the host (fmx.pairwise.alias_table).  A wavefront owns a row, as above; in round r
// lane l evaluates draw t = 64 r + l: words 2 (t & 1) and 2 (t & 1) + 1 of the Philox block (t >> 1) | 0x80000000 (the high bit:
// no block of k_fm_mine under the same seed and offset), a cell p < N, then p or alias[p].  A ballot and the count of the eligible
// lanes below put the eligible draws in draw order behind the `kept` of the rounds before.  No LDS, no atomics; at most
// ceil(n_try / 64) <= 16 rounds and excluded()'s search: nothing waits on anything.
struct AliasArgs {
  const uint32_t *thresh;
  const int32_t *alias;
  const float *logq;
  const int32_t *excl_off, *excl_pos, *own_pos;
  int32_t *neg_pos;
  float *neg_logq;
  uint32_t key0, key1, off0, off1, u_base;
  int U, N, n_neg, n_try;
};

__global__ __launch_bounds__(MN_WAVES *WAVE) void k_alias_sample(AliasArgs a) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int u = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * MN_WAVES + (threadIdx.x >> 6)));
  if (u >= a.U) return;
  const int own = a.own_pos ? a.own_pos[u] : -1;
  const uint32_t uid = a.u_base + (uint32_t)u;
  int32_t *out_pos = a.neg_pos + (size_t)u * a.n_neg;
  float *out_logq = a.neg_logq ? a.neg_logq + (size_t)u * a.n_neg : nullptr;
  const int rounds = (a.n_try + WAVE - 1) / WAVE;
  int kept = 0;  // wave-uniform: the eligible draws of the rounds so far
  for (int r = 0; r < rounds && kept < a.n_neg; ++r) {
    const int t = r * WAVE + lane;
    const uint32_t c3 = 0x80000000u + (uint32_t)(t >> 1);
    // (one block: the rounds of the second word are the first's, and the compiler keeps one copy)
    const uint32_t wa = philox_word(a.key0, a.key1, a.off0, a.off1, uid, c3, 2 * (t & 1));
    const uint32_t wb = philox_word(a.key0, a.key1, a.off0, a.off1, uid, c3, 2 * (t & 1) + 1);
    const uint32_t p = __umulhi(wa, (uint32_t)a.N);  // (wa * N) >> 32 < N
    const uint32_t th = a.thresh[p];
    const int al = a.alias[p];
    const int c = (wb >> 8) < th ? (int)p : al;
    bool ok = t < a.n_try && (uint32_t)c < (uint32_t)a.N && c != own;  // (a corrupt alias entry: dropped, never an address)
    if (ok && a.excl_off) ok = !excluded(a.excl_off, a.excl_pos, u, c);
    const uint64_t m = __ballot(ok);
    const int slot = kept + (int)__popcll(m & ((1ull << lane) - 1));
    if (ok && slot < a.n_neg) {
      out_pos[slot] = c;
      if (out_logq) out_logq[slot] = a.logq[c];
    }
    kept += (int)__popcll(m);
  }
  if (lane >= kept && lane < a.n_neg) {  // (n_neg <= MN_MAX_NEG < WAVE)
    out_pos[lane] = -1;
    if (out_logq) out_logq[lane] = -INFINITY;
  }
}

}  // namespace

extern "C" int fmx_alias_sample_negatives(const uint32_t *thresh, const int32_t *alias, const float *logq, int32_t N,
                                          const int32_t *excl_offsets, const int32_t *excl_pos, const int32_t *own_pos, int32_t U,
                                          int32_t n_neg, int32_t n_try, uint64_t seed, uint64_t offset, uint32_t u_base, int32_t *neg_pos,
                                          float *neg_logq, fmx_stream_t stream) {
  const char *fn = "fmx_alias_sample_negatives";
  if (!thresh || !alias || !neg_pos) return fail(FMX_ERR_ARG, "%s: null argument (thresh, alias, neg_pos)", fn);
  if (!logq && neg_logq) return fail(FMX_ERR_ARG, "%s: neg_logq without logq", fn);
  if ((excl_offsets == nullptr) != (excl_pos == nullptr)) return fail(FMX_ERR_ARG, "%s: excl_offsets and excl_pos go together", fn);
  if (U < 1 || N < 1) return fail(FMX_ERR_ARG, "%s: U=%d and N=%d must be >= 1", fn, U, N);
  if (n_try < 1 || n_neg < 1) return fail(FMX_ERR_ARG, "%s: n_try=%d and n_neg=%d must be >= 1", fn, n_try, n_neg);
  if (n_try > MN_MAX_DRAW || n_neg > MN_MAX_NEG)
    return fail(FMX_ERR_UNSUPPORTED, "%s: n_try=%d, n_neg=%d, the kernel covers n_try <= %d and n_neg <= %d", fn, n_try, n_neg,
                MN_MAX_DRAW, MN_MAX_NEG);
  if (n_neg > n_try) return fail(FMX_ERR_ARG, "%s: n_neg=%d exceeds n_try=%d", fn, n_neg, n_try);
  const AliasArgs a{thresh, alias, logq,
                    excl_offsets, excl_pos, own_pos,
                    neg_pos, neg_logq,
                    (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)offset, (uint32_t)(offset >> 32), u_base,
                    U, N, n_neg, n_try};
  hipLaunchKernelGGL(k_alias_sample, dim3((U + MN_WAVES - 1) / MN_WAVES), dim3(MN_WAVES * WAVE), 0, static_cast<hipStream_t>(stream), a);
  return check_launch("k_alias_sample");
}

extern "C" int fmx_fm_mine_negatives(const float *Su, int32_t ld_u, const float *au, int32_t U, const float *Sc, int32_t ld_c,
                                     const float *ac, int32_t N, int32_t kp, const int32_t *excl_offsets, const int32_t *excl_pos,
                                     const int32_t *own_pos, int32_t n_draw, int32_t n_neg, uint64_t seed, uint64_t offset,
                                     uint32_t u_base, int32_t *neg_pos, float *neg_score, fmx_stream_t stream) {
  const char *fn = "fmx_fm_mine_negatives";
  if (!Su || !au || !Sc || !ac || !neg_pos || !neg_score) return fail(FMX_ERR_ARG, "%s: null argument", fn);
  if ((excl_offsets == nullptr) != (excl_pos == nullptr)) return fail(FMX_ERR_ARG, "%s: excl_offsets and excl_pos go together", fn);
  if (U < 1 || N < 1) return fail(FMX_ERR_ARG, "%s: U=%d and N=%d must be >= 1", fn, U, N);
  if (n_draw < 1 || n_neg < 1) return fail(FMX_ERR_ARG, "%s: n_draw=%d and n_neg=%d must be >= 1", fn, n_draw, n_neg);
  if (n_draw > MN_MAX_DRAW || n_neg > MN_MAX_NEG)
    return fail(FMX_ERR_UNSUPPORTED, "%s: n_draw=%d, n_neg=%d, the kernel covers n_draw <= %d and n_neg <= %d", fn, n_draw, n_neg,
                MN_MAX_DRAW, MN_MAX_NEG);
  if (n_neg > n_draw) return fail(FMX_ERR_ARG, "%s: n_neg=%d exceeds n_draw=%d", fn, n_neg, n_draw);
  if (!lpr_of(kp)) return fail(FMX_ERR_UNSUPPORTED, "%s: kp=%d must be 4/8/16/32/64", fn, kp);
  if (ld_u % 4 || ld_c % 4) return fail(FMX_ERR_ALIGN, "%s: ld_u=%d and ld_c=%d must be multiples of 4", fn, ld_u, ld_c);
  if (ld_u < kp || ld_c < kp) return fail(FMX_ERR_SHAPE, "%s: ld_u=%d and ld_c=%d must be >= kp=%d", fn, ld_u, ld_c, kp);
  if (!aligned16(Su) || !aligned16(Sc)) return fail(FMX_ERR_ALIGN, "%s: Su and Sc must be 16-byte aligned", fn);
  const MineArgs a{Su, au, Sc, ac,
                   excl_offsets, excl_pos, own_pos,
                   neg_pos, neg_score,
                   (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)offset, (uint32_t)(offset >> 32), u_base,
                   ld_u, ld_c, U, N, n_draw, n_neg};
  const dim3 grid((U + MN_WAVES - 1) / MN_WAVES);
  return with_kp(kp, [&](auto KP) {
    hipLaunchKernelGGL(k_fm_mine<KP>, grid, dim3(MN_WAVES * WAVE), 0, static_cast<hipStream_t>(stream), a);
    return check_launch("k_fm_mine");
  });
}
