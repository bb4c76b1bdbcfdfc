// fmx_kernels.hip -- gfx950 (MI355X, CDNA4) kernels for the FM / DeepFM / NFM online hot path and their C ABI.
//
// Three kernels make one mini-batch step (DESIGN.md has the data layout and the byte accounting):
//
//   k_sort_occ    one workgroup per field: the batch's (local index, sample) pairs are packed into 32-bit
//                 composites and bitonic-sorted (registers + wave shuffles, LDS only for the cross-wave stages).
//                 Equal rows become adjacent runs ordered by sample, so the duplicate-row reduction the reference
//                 gets from embedding_dense_backward (reference fm_adam.py:67) is deterministic.  Independent of
//                 the weights.
//   k_fm_forward  one 64-lane wavefront per sample, LPR lanes per gathered row (16-byte loads, one request per
//                 64-byte row), every index / row load of the sample issued before the first use, butterfly
//                 shuffles for the field sums (reference fm_adam.py:35-53), fused loss / dlogit epilogue
//                 (fm_adam.py:61,66 / :76,80).
//   k_fm_update   (fmx_update.hip, with k_fm_fixup) one wavefront per tile of 64 sorted occurrences: ONE fused read-modify-write of
//                 every touched row under the chosen rule (reference loss.backward() + optimizer.step(), fm_adam.py:67-68 / :81-82).
//
// This unit holds the sort, the forward (whole and split over field owners), the loops over a device-resident pool, the owner step
// and the C ABI of the batched calls; the shared host-side checks (fmx_host.h) are defined here.  The stream walkers (one
// wavefront or workgroup per stream) are in fmx_online.hip.
//
// Everything is HBM / cache-line bound integer+fp32 work; there is no GEMM here and no MFMA.

#include <cmath>

#include "fmx_host.h"

// ------------------------------------------------------------------------------------------------------------
// host-side error plumbing (shared by the translation units: fmx_common.h)
// ------------------------------------------------------------------------------------------------------------
namespace fmxd {

thread_local char g_err[512] = "";

int fail(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

int check_launch(const char *what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(FMX_ERR_LAUNCH, "%s: %s", what, hipGetErrorString(e));
  return FMX_OK;
}

}  // namespace fmxd

namespace {

#include "fmx_sort.inc"

// ------------------------------------------------------------------------------------------------------------
// k_fm_forward
// ------------------------------------------------------------------------------------------------------------
struct FwdArgs {
  const float *rows;
  const int64_t *foff;
  const float *bias;
  const int32_t *idx;
  const float *xv;
  const float *y;
  fmx_fwd_out_t out;
  fmx_hyper_t h;
  int32_t B, F, kp, stride, zoff, loss_kind;
  int32_t ldS, ld1;  // floats between consecutive samples in out.S and in out.dz / out.loss (kp and 1 when dense)
  float inv_b;
  // fields as pieces of index columns (fmx_table_t.field_cols / field_base; both null on ordinary tables): Fc = columns of idx
  const int32_t *fcols, *fbase;
  int32_t Fc;
  union {            // one word, so that the struct -- and with it every k_fm_forward's kernarg loads -- keeps its size
    float margin;    // PAIR (fmx_pair.inc): the pair loss's margin; nothing else reads it
    int32_t list_g;  // LIST (fmx_list.inc): rows per list (the positive, then its negatives); nothing else reads it
  };
};

#ifdef FMX_STAMPS  // diagnostic build (tools/forward_stamps.sh): s_memrealtime (100 MHz) of every wave of the LAST k_fm_forward launch
__device__ unsigned long long g_fwd_stamps[8192 * 6];  // one record per sample; lane i stamps sample first_ + i, for i < count_
#define FMX_FSTAMP_AT(slot_, dep_, first_, count_)                                                                  \
  do {                                                                                                              \
    unsigned long long t_;                                                                                          \
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) : "v"(dep_) : "memory");                      \
    if (lane < (count_) && (first_) + lane < 8192) g_fwd_stamps[(size_t)((first_) + lane) * 6 + (slot_)] = t_;       \
  } while (0)
#else
#define FMX_FSTAMP_AT(slot_, dep_, first_, count_) do {} while (0)
#endif
#define FMX_FSTAMP(slot_, dep_) FMX_FSTAMP_AT(slot_, dep_, b, (int)exists)  // the wave's own sample

__device__ __forceinline__ float first_lane_f(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

// The part of the forward pass behind the row gather: field sums (butterfly over the lane groups), bi-interaction, logit,
// loss and dlogit, stores.  s / ss / fo: this lane's partial sums of e, e*e and of the first-order terms over ITS fields;
// bias: the bias weight (resolved while the rows were in flight).
// The loss epilogue (bce_loss_dz: two expf, a log1pf, an IEEE divide, ~100 VALU instructions) is a pure function of one sample's
// (z, y).  Evaluated by every wave on its lane 0 it takes the issue slots of a whole wave for one useful lane of 64, four waves per
// SIMD at once; instead the waves of a workgroup leave (fo, sbi, y) in LDS and, behind ONE barrier, the workgroup's first wave
// evaluates all of them, sample i on lane i: the same function of the same operands -- the same bits -- for a quarter of the
// instruction issue at four waves per workgroup.  Without a loss (the DeepFM loop) every wave stores its own three words.
// PAIR (fmx_fm_pair_forward, fmx_pair.inc; at least two waves per workgroup, B even): samples 2i and 2i + 1 are the positive and the
// negative of pair i and sit on neighbouring lanes of that first wave; each takes its partner's logit from lane ^ 1 and both
// evaluate the pair loss of the same difference -- the positive stores (loss_i, dz_i), the negative (0, -dz_i).  No label is read.
// LIST (fmx_fm_list_forward, fmx_list.inc; G = a.list_g rows per list, G * max(1, 4 / G) waves per workgroup -- up to 16, hence
// sh[3][16] and k_fm_forward_list's own launch bound -- and B a multiple of G): a workgroup holds whole lists, lane i of the first
// wave is position i % G of list i / G, and every lane evaluates its list's softmax cross-entropy from the list's G logits
// (list_loss_dz, fmx_common.h) -- the positive stores (loss_i, dz_0), a negative (0, dz_j).  No label and no loss_kind is read.
// LISTQ (fmx_fm_list_forward_q; with LIST): y is the row's correction corr[b] (a.y, carried through sh[2] as a label is) and the
// softmax is taken over c = z - y; the stored logit stays z.
template <int LPR, bool PAIR = false, bool LIST = false, bool LISTQ = false>
__device__ __forceinline__ void forward_finish(const FwdArgs &a, int b, const bool exists, const int lane, float4 s, float4 ss, float fo,
                                               bool bad, float y, const float bias) {
  const int q = lane % LPR;
  const int kp = LPR * 4;
  if (bad && a.out.error) *a.out.error = 1;  // (a wave that repeats the last sample repeats its verdict)

  fm_field_sums<LPR>(s, ss, fo, lane);
  float sbi;
  const float4 bi = fm_bi_dpp<LPR>(s, ss, sbi);
  // fo: lanes with q != 0 hold the sum of zeros; take the q == 0 value
  fo = first_lane_f(fo);
  FMX_FSTAMP(3, sbi);

  if (exists && lane < LPR) {
    if (a.out.S) *reinterpret_cast<float4 *>(a.out.S + (size_t)b * a.ldS + 4 * q) = s;
    if (a.out.bi) *reinterpret_cast<float4 *>(a.out.bi + (size_t)b * kp + 4 * q) = bi;
  }
  int n = exists ? 1 : 0;  // lanes 0 .. n - 1 finish samples b .. b + n - 1
  if ((PAIR || LIST || a.loss_kind != FMX_LOSS_NONE) && blockDim.x > WAVE) {  // (uniform over the launch)
    __shared__ float sh[3][LIST ? 16 : 4];
    const int w = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    if (lane == 0) {
      sh[0][w] = fo;
      sh[1][w] = sbi;
      sh[2][w] = y;
    }
    __syncthreads();
    if (w != 0) return;
    b = blockIdx.x * wpb;  // (this wave's own sample: it exists)
    n = min(wpb, a.B - b);
    const int l = lane < n ? lane : 0;
    fo = sh[0][l];
    sbi = sh[1][l];
    y = sh[2][l];
  }
  if (lane < n) {
    const int bl = b + lane;
    const float z = fo + sbi + bias;
    if (a.out.sfirst) a.out.sfirst[bl] = fo;
    if (a.out.sbi) a.out.sbi[bl] = sbi;
    if (a.out.logit) a.out.logit[bl] = z;
    if constexpr (PAIR) {
      const float zo = xor_lane_f<1>(z, lane);  // the partner's logit (n is even: the partner's lane is active)
      const bool pos = (lane & 1) == 0;
      float loss, dz;
      pair_loss_dz(pos ? z - zo : zo - z, a.margin, a.inv_b, loss, dz);  // both lanes: the same operands, the same bits
      if (a.out.loss) a.out.loss[(size_t)bl * a.ld1] = pos ? loss : 0.f;
      if (a.out.dz) a.out.dz[(size_t)bl * a.ld1] = pos ? dz : -dz;
    } else if constexpr (LIST) {
      float loss, dz;  // (n is a multiple of G: every lane of the list is active)
      if constexpr (LISTQ) list_loss_dz(z - y, lane, a.list_g, a.inv_b, loss, dz);
      else list_loss_dz(z, lane, a.list_g, a.inv_b, loss, dz);
      if (a.out.loss) a.out.loss[(size_t)bl * a.ld1] = lane % a.list_g == 0 ? loss : 0.f;
      if (a.out.dz) a.out.dz[(size_t)bl * a.ld1] = dz;
    } else if (a.loss_kind != FMX_LOSS_NONE) {
      float loss, dz;
      bce_loss_dz(a.loss_kind, z, y, a.inv_b, loss, dz);
      FMX_FSTAMP_AT(4, dz, b, n);
      if (a.out.loss) a.out.loss[(size_t)bl * a.ld1] = loss;
      if (a.out.dz) a.out.dz[(size_t)bl * a.ld1] = dz;
    }
    FMX_FSTAMP_AT(5, z, b, n);
  }
}

// 64-bit lane exchange (two ds_bpermute)
__device__ __forceinline__ int64_t shfl64(int64_t v, int src) {
  const int lo = __shfl((int)(uint32_t)v, src), hi = __shfl((int)(v >> 32), src);
  return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}
constexpr int64_t ROW_ABSENT = int64_t(1) << 62;  // set in a resolved row: the index lies outside the field (row = the field's first)

// NPASS > 0: the field loop is fully unrolled (F <= NPASS * SLOTS) and every load of the sample is issued before the first
// use.  NPASS == 0: generic.
// The sample's fields are resolved ONE PER LANE first: lane l of a window of WAVE consecutive fields loads field l's offsets,
// index and value and forms the table row, so the first round trip is one load per window of each (offsets, index, value)
// however many passes the sample takes; the passes then take their rows from the window by lane exchanges.  The rows, the
// order of the additions and so every result are those of k_fm_forward_part at one block, which loads per pass.
// MAPPED (tables whose fields are pieces of index columns; the generic field loop only): field f reads column fcols[f], holds
// the indices [fbase[f], fbase[f] + rows) of it, and an index outside belongs to another piece: no contribution, no error.
// HAS_X: xv is not null (without values every x is 1 and nothing is loaded for it).
// exists (wave-uniform): false for a wave behind the batch's last sample, which repeats that sample for the workgroup's barrier and
// stores nothing.
template <int LPR, int LAYOUT, int NPASS, bool MAPPED, bool HAS_X, bool PAIR = false, bool LIST = false, bool LISTQ = false>
__device__ __forceinline__ void forward_sample(const FwdArgs &a, const int b, const bool exists, const int lane) {
  constexpr int SLOTS = WAVE / LPR;
  constexpr int NP = NPASS > 0 ? NPASS : 1;
  constexpr int NW = NPASS > 0 ? (NP * SLOTS + WAVE - 1) / WAVE : 1;  // windows of WAVE fields
  const int slot = lane / LPR, q = lane % LPR;
  const int kp = LPR * 4;
  FMX_FSTAMP(0, lane);

  float4 s = splat(0.f), ss = splat(0.f);
  float fo = 0.f;
  bool bad = false;
  // the label and the bias are only needed by the epilogue, but a load issued there is one more dependent round trip
  // at the end of every wave: request them now, with the indices (every lane the same address: one request each)
  const float y_early = (LISTQ || (!PAIR && !LIST && a.loss_kind != FMX_LOSS_NONE)) ? a.y[b] : 0.f;  // (LISTQ: the row's correction)
  const float bias0_early = a.bias[0];
  const float bias1_early = LAYOUT == FMX_LAYOUT_WEIGHTS ? 0.f : a.bias[1];
  __builtin_amdgcn_sched_barrier(0);  // (left to itself the scheduler sinks the bias load behind the first waits of the gather:
                                      //  in-order vmcnt then makes the row requests wait for it -- one more round trip)
  float bias = 0.f;
  const int n_outer = NPASS > 0 ? 1 : (a.F + SLOTS - 1) / SLOTS;
  for (int it = 0; it < n_outer; ++it) {
    // Branch-free: a lane beyond the last field reads field F - 1's index and offsets, an index beyond the field's
    // vocabulary reads the field's first row, and the results are dropped by selects.  With `if (live) { loads; arithmetic on
    // them }` the compiler put an s_waitcnt vmcnt(0) at the end of every region: one dependent round trip per region.
    int fl[NW];
    bool wlive[NW];
    int64_t lo[NW], hi[NW];
    uint32_t li[NW];
    float xl[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const int f = (NPASS > 0 ? w * WAVE : it * SLOTS) + lane;
      wlive[w] = f < a.F;
      fl[w] = wlive[w] ? f : a.F - 1;
    }
#pragma unroll
    for (int w = 0; w < NW; ++w) {  // the offsets do not depend on the sample: first
      lo[w] = a.foff[fl[w]];
      hi[w] = a.foff[fl[w] + 1];
    }
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      size_t o = (size_t)b * a.F + fl[w];
      uint32_t fb = 0u;
      if (MAPPED) {
        o = (size_t)b * a.Fc + (a.fcols ? a.fcols[fl[w]] : fl[w]);
        fb = a.fbase ? (uint32_t)a.fbase[fl[w]] : 0u;
      }
      li[w] = (uint32_t)a.idx[o] - fb;  // (wraps to a huge value below the piece)
      xl[w] = HAS_X ? a.xv[o] : 1.f;
    }
    int64_t row[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const bool okw = wlive[w] && li[w] < (uint32_t)(hi[w] - lo[w]);
      row[w] = lo[w] + (okw ? li[w] : 0u);
      if (!okw) row[w] |= ROW_ABSENT;
      bad = bad || (!MAPPED && wlive[w] && !okw);
    }
    FMX_FSTAMP(1, (uint32_t)row[0]);
    // both layouts keep [ V | w ] at the head of the row: the forward never touches the FTRL (z, n) half
    float x[NP];
    float4 r0[NP];
    float rw[NP];
    bool ok[NP], live[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int f = NPASS > 0 ? p * SLOTS + slot : slot;  // relative to the first field of the window set
      const int w = NPASS > 0 ? (p * SLOTS) / WAVE : 0;
      live[p] = (NPASS > 0 ? f : it * SLOTS + f) < a.F;
      const int64_t r = shfl64(row[w], f % WAVE);
      x[p] = HAS_X ? __shfl(xl[w], f % WAVE) : 1.f;
      ok[p] = live[p] && !(r & ROW_ABSENT);
      const float *rp = a.rows + (size_t)(r & ~ROW_ABSENT) * a.stride;
      r0[p] = *reinterpret_cast<const float4 *>(rp + 4 * q);
      rw[p] = rp[kp];  // (every lane of the group: the same address, one request)
    }
    __builtin_amdgcn_sched_barrier(0);  // ... and every row request before the first sum
    // the bias weight while the rows are in flight (its loads came back with the window's)
    if (it == 0) {
      bias = bias_weight<LAYOUT>(bias0_early, bias1_early, a.h);
      asm volatile("" ::"v"(bias));  // (otherwise the compiler sinks it into lane 0's epilogue, behind the butterfly)
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const float4 e = x[p] * r0[p];
      const float f1 = ok[p] ? rw[p] * x[p] : 0.f;
      if (ok[p]) {  // selects
        s = s + e;
        ss = ss + e * e;
        fo += f1;
      }
      if (exists && live[p] && a.out.first && q == 0) a.out.first[(size_t)b * a.F + (it * NP + p) * SLOTS + slot] = f1;
    }
    FMX_FSTAMP(2, s.x + ss.x + fo);  // (every row of the pass set arrived and added)
  }
  forward_finish<LPR, PAIR, LIST, LISTQ>(a, b, exists, lane, s, ss, fo, bad, y_early, bias);
}

template <int LPR, int LAYOUT, int NPASS, bool MAPPED = false, bool PAIR = false>
__global__ __launch_bounds__(256) void k_fm_forward(FwdArgs a) {
  __builtin_amdgcn_s_setprio(3);  // ahead of the side-stream sort's waves at the CU's instruction arbiter
  int b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const bool exists = b < a.B;  // wave-uniform
  if (!exists) b = a.B - 1;     // (forward_finish has a workgroup barrier: the wave goes along and stores nothing)
  if (a.xv) forward_sample<LPR, LAYOUT, NPASS, MAPPED, true, PAIR>(a, b, exists, threadIdx.x & 63);
  else forward_sample<LPR, LAYOUT, NPASS, MAPPED, false, PAIR>(a, b, exists, threadIdx.x & 63);
}

// The LIST mode of k_fm_forward: the same body with forward_finish<LIST>'s epilogue, a kernel of its own because a workgroup of up
// to 16 waves needs its own launch bound (128 VGPRs per wave at 1024 threads) while k_fm_forward's instantiations keep theirs.  (The
// six lines are repeated, not shared through a device function: routed through one, the pointwise instantiations of k_fm_forward
// came out with another register assignment, and their code is to stay what it was -- tools/isa_diff.py.)
template <int LPR, int LAYOUT, int NPASS>
__global__ __launch_bounds__(64 * LIST_MAX_G) void k_fm_forward_list(FwdArgs a) {
  __builtin_amdgcn_s_setprio(3);
  int b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const bool exists = b < a.B;  // wave-uniform
  if (!exists) b = a.B - 1;     // (the barrier again; B_lists G need not be a multiple of the workgroup's waves when they exceed G)
  if (a.xv) forward_sample<LPR, LAYOUT, NPASS, false, true, false, true>(a, b, exists, threadIdx.x & 63);
  else forward_sample<LPR, LAYOUT, NPASS, false, false, false, true>(a, b, exists, threadIdx.x & 63);
}

// ... and its log-Q corrected form (fmx_fm_list_forward_q): forward_finish<LIST, LISTQ>, a.y = corr.  A kernel of its own name, so
// that k_fm_forward_list's instantiations keep theirs (tools/isa_diff.py matches kernels by name).
template <int LPR, int LAYOUT, int NPASS>
__global__ __launch_bounds__(64 * LIST_MAX_G) void k_fm_forward_listq(FwdArgs a) {
  __builtin_amdgcn_s_setprio(3);
  int b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const bool exists = b < a.B;  // wave-uniform
  if (!exists) b = a.B - 1;
  if (a.xv) forward_sample<LPR, LAYOUT, NPASS, false, true, false, true, true>(a, b, exists, threadIdx.x & 63);
  else forward_sample<LPR, LAYOUT, NPASS, false, false, false, true, true>(a, b, exists, threadIdx.x & 63);
}

// ------------------------------------------------------------------------------------------------------------
// k_fm_forward_part / k_fm_forward_finish: the forward pass split over FIELD OWNERS (model-parallel multi-GPU mode)
// ------------------------------------------------------------------------------------------------------------
// k_fm_forward sums a sample's rows in a fixed tree: lane group `slot` (of SLOTS = 64 / LPR) adds the fields
// slot, SLOTS + slot, 2 SLOTS + slot, ... in order, then a butterfly over the lane groups (slot ^ 1, ^ 2, ^ 4, ...).  The tree is
// cut into NB BLOCKS of SL = SLOTS / NB consecutive lane groups (NB a power of two); an owner holds one or more blocks -- the
// fields at their positions, as a table of its own: local field (lb NP + p) SL + s is position p SLOTS + (first block + lb) SL + s
// of the whole tree -- and k_fm_forward_part evaluates exactly those sub-trees for EVERY sample of the global batch: NB samples
// per wave, SL lane groups each, the butterfly levels below SL -- one record (S_part[kp], ss_part[kp], fo_part) per sample
// and block.  The records of a sample meet on the rank that holds its label (an all-to-all), where k_fm_forward_finish adds
// them in the order of the remaining butterfly levels, ((b0 + b1) + (b2 + b3)) + ..., and runs k_fm_forward's epilogue.
// The result is bit-identical to k_fm_forward on one GPU whose table has the same fields at the same positions.
struct PartArgs {
  const float *rows;
  const int64_t *foff;   // the owner's LOCAL table (blockIdx.y = local block lb): fields [lb NP SL, (lb + 1) NP SL) are the block's
  const int32_t *fcols, *fbase;  // fmx_table_t.field_cols / field_base, or null
  const int32_t *idx;    // [B, Fc], B = global batch
  const float *xv;       // [B, Fc] or null
  float *rec;            // [B / group][n_blocks][group, 2 kp + 4]: S | ss | fo, 0, 0, 0 -- the records of the `group` samples one rank
                         // holds the labels of lie together, block after block: one contiguous message per destination
  int32_t *error;
  int32_t B, F, Fc, stride, sl_log2, group;  // F: fields of the table (all blocks)
};

template <int LPR, int NPASS>
__global__ __launch_bounds__(256) void k_fm_forward_part(PartArgs a) {
  constexpr int SLOTS = WAVE / LPR;
  constexpr int kp = LPR * 4, REC = 2 * kp + 4;
  const int lane = threadIdx.x & 63;
  const int slot = lane / LPR, q = lane % LPR;
  const int SL = 1 << a.sl_log2;
  const int slot_l = slot & (SL - 1);
  const int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int b = wave * (SLOTS >> a.sl_log2) + (slot >> a.sl_log2);
  const bool valid = b < a.B;
  const int f0 = (int)blockIdx.y * NPASS * SL;  // first field of this block
  const bool pieces = a.fcols || a.fbase;
  // branch-free gather, as in forward_sample: every offset and index load, then every row load, then the sums by selects
  uint32_t li[NPASS], vocab[NPASS];
  float x[NPASS], xl[NPASS];
  int64_t lo[NPASS], hi[NPASS];
  bool live[NPASS], ok[NPASS];
  int fc[NPASS];
  const float *xsrc = a.xv ? a.xv : reinterpret_cast<const float *>(a.idx);
  const bool has_x = a.xv != nullptr;
  const int bc = valid ? b : 0;
#pragma unroll
  for (int p = 0; p < NPASS; ++p) {
    const int f = f0 + p * SL + slot_l;
    live[p] = valid && f < a.F;
    fc[p] = f < a.F ? f : a.F - 1;
  }
  int colp[NPASS];
  uint32_t fb[NPASS];
#pragma unroll
  for (int p = 0; p < NPASS; ++p) {
    lo[p] = a.foff[fc[p]];
    hi[p] = a.foff[fc[p] + 1];
    colp[p] = a.fcols ? a.fcols[fc[p]] : fc[p];
    fb[p] = a.fbase ? (uint32_t)a.fbase[fc[p]] : 0u;
  }
#pragma unroll
  for (int p = 0; p < NPASS; ++p) {
    const size_t o = (size_t)bc * a.Fc + colp[p];
    li[p] = (uint32_t)a.idx[o] - fb[p];  // (wraps to a huge value below the piece)
    xl[p] = xsrc[o];
  }
#pragma unroll
  for (int p = 0; p < NPASS; ++p) {
    x[p] = has_x ? xl[p] : 1.f;
    vocab[p] = (uint32_t)(hi[p] - lo[p]);
  }
  float4 r0[NPASS];
  float rw[NPASS];
#pragma unroll
  for (int p = 0; p < NPASS; ++p) {
    ok[p] = live[p] && li[p] < vocab[p];
    const float *rp = a.rows + (size_t)(lo[p] + (ok[p] ? li[p] : 0u)) * a.stride;
    r0[p] = *reinterpret_cast<const float4 *>(rp + 4 * q);
    rw[p] = rp[kp];
  }
  __builtin_amdgcn_sched_barrier(0);
  float4 s = splat(0.f), ss = splat(0.f);
  float fo = 0.f;
  bool bad = false;
#pragma unroll
  for (int p = 0; p < NPASS; ++p) {
    const float4 e = x[p] * r0[p];
    if (ok[p]) {  // selects
      s = s + e;
      ss = ss + e * e;
      fo += rw[p] * x[p];
    }
    bad = bad || (!pieces && live[p] && !ok[p]);
  }
  if (bad && a.error) *a.error = 1;
  fm_field_sums<LPR>(s, ss, fo, lane, SL);  // the butterfly levels inside the block's lane groups (wave-uniform conditions)
  if (valid && slot_l == 0) {
    const int dst = b / a.group;
    float *r = a.rec + (((size_t)dst * gridDim.y + blockIdx.y) * a.group + (b - dst * a.group)) * REC;
    *reinterpret_cast<float4 *>(r + 4 * q) = s;
    *reinterpret_cast<float4 *>(r + kp + 4 * q) = ss;
    if (q == 0) *reinterpret_cast<float4 *>(r + 2 * kp) = float4{fo, 0.f, 0.f, 0.f};
  }
}

struct FinishArgs {
  const float *parts;    // [G][B, 2 kp + 4]: block r holds rank r's records of THIS rank's B samples
  int64_t rank_stride;   // floats between the blocks
  const float *bias;
  const float *y;
  fmx_fwd_out_t out;
  fmx_hyper_t h;
  int32_t B, loss_kind, ldS, ld1;
  float inv_b;
};

template <int LPR, int LAYOUT, int G>
__global__ __launch_bounds__(256) void k_fm_forward_finish(FinishArgs a) {
  constexpr int SLOTS = WAVE / LPR;
  constexpr int kp = LPR * 4, REC = 2 * kp + 4;
  const int lane = threadIdx.x & 63;
  const int slot = lane / LPR, q = lane % LPR;
  const int b = (blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * SLOTS + slot;
  const bool valid = b < a.B;
  const float y_early = (valid && a.loss_kind != FMX_LOSS_NONE) ? a.y[b] : 0.f;
  const float bias0 = a.bias[0];
  const float bias1 = LAYOUT == FMX_LAYOUT_WEIGHTS ? 0.f : a.bias[1];
  float4 s[G], ss[G];
  float fo[G];
#pragma unroll
  for (int r = 0; r < G; ++r) {
    s[r] = ss[r] = splat(0.f);
    fo[r] = 0.f;
    if (valid) {
      const float *p = a.parts + (size_t)r * a.rank_stride + (size_t)b * REC;
      s[r] = *reinterpret_cast<const float4 *>(p + 4 * q);
      ss[r] = *reinterpret_cast<const float4 *>(p + kp + 4 * q);
      if (q == 0) fo[r] = p[2 * kp];
    }
  }
  // the butterfly levels ABOVE the owners' lane groups: rank pairs, then pairs of pairs, ...
#pragma unroll
  for (int st = 1; st < G; st <<= 1) {
#pragma unroll
    for (int r = 0; r < G; r += 2 * st) {
      s[r] = s[r] + s[r + st];
      ss[r] = ss[r] + ss[r + st];
      fo[r] += fo[r + st];
    }
  }
  float sbi;
  const float4 bi = fm_bi<LPR>(s[0], ss[0], sbi);
  if (!valid) return;
  if (a.out.S) *reinterpret_cast<float4 *>(a.out.S + (size_t)b * a.ldS + 4 * q) = s[0];
  if (a.out.bi) *reinterpret_cast<float4 *>(a.out.bi + (size_t)b * kp + 4 * q) = bi;
  if (q == 0) {
    const float z = fo[0] + sbi + bias_weight<LAYOUT>(bias0, bias1, a.h);
    if (a.out.sfirst) a.out.sfirst[b] = fo[0];
    if (a.out.sbi) a.out.sbi[b] = sbi;
    if (a.out.logit) a.out.logit[b] = z;
    if (a.loss_kind != FMX_LOSS_NONE) {
      float loss, dz;
      bce_loss_dz(a.loss_kind, z, y_early, a.inv_b, loss, dz);
      if (a.out.loss) a.out.loss[(size_t)b * a.ld1] = loss;
      if (a.out.dz) a.out.dz[(size_t)b * a.ld1] = dz;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------
// k_stream_read: HBM-read ceiling probe
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_stream_read(const float4 *buf, int64_t n16, float *sink) {
  float acc = 0.f;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += stride) {
    const float4 v = buf[i];
    acc += (v.x + v.y) + (v.z + v.w);
  }
  if (acc == 123456.789f) *sink = acc;  // keeps the loads live; practically never true
}

// k_gather_read: random-row read ceiling probe -- n rows of 64 or 128 bytes at pseudo-random (hashed) positions of a buffer,
// 16 bytes per lane, LPR lanes per row: the access pattern of the forward gather with nothing else around it
template <int LPR>
__global__ __launch_bounds__(256) void k_gather_read(const float4 *buf, uint64_t n_rows, int64_t n, uint32_t seed, float *sink) {
  const int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / LPR;
  const int q = threadIdx.x % LPR;
  if (g >= n) return;
  uint64_t h = ((uint64_t)g + seed) * 0x9E3779B97F4A7C15ull;
  h ^= h >> 29;
  h *= 0xBF58476D1CE4E5B9ull;
  h ^= h >> 32;
  const float4 v = buf[(h % n_rows) * LPR + q];
  if ((v.x + v.y) + (v.z + v.w) == 123456.789f) *sink = v.x;  // keeps the load live; practically never true
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------
// the shared host-side checks (declared in fmx_host.h) and the tuning switches
// ------------------------------------------------------------------------------------------------------------
namespace fmxd {

int refuse_adaptive(int rule, const char *who) {
  return fail(FMX_ERR_UNSUPPORTED, "%s: %s is not supported here (fmx_fm_update / fmx_fm_step / fmx_fm_stream / fmx_fm_online_run take it)",
              who, rule_name(rule));
}

int check_table(const fmx_table_t *t) {
  if (!t) return fail(FMX_ERR_ARG, "table is null");
  if (!t->rows || !t->field_offsets || !t->bias) return fail(FMX_ERR_ARG, "table has a null pointer");
  if (t->n_fields < 1 || t->n_rows < 1 || t->k < 1) return fail(FMX_ERR_ARG, "table sizes must be positive");
  if (!lpr_of(t->kp) || t->k > t->kp) return fail(FMX_ERR_SHAPE, "kp=%d must be 4/8/16/32/64 and >= k=%d", t->kp, t->k);
  if (t->layout != FMX_LAYOUT_WEIGHTS && t->layout != FMX_LAYOUT_FTRL && t->layout != FMX_LAYOUT_MOMENTS)
    return fail(FMX_ERR_ARG, "unknown layout %d", t->layout);
  int need = t->kp + 4;
  if (t->layout != FMX_LAYOUT_WEIGHTS) {  // FTRL and MOMENTS: [ head | pad | kp | kp ] from z_offset
    if (t->z_offset % 4 || t->z_offset < t->kp + 4)
      return fail(FMX_ERR_SHAPE, "z_offset=%d must be a multiple of 4 and >= kp + 4 = %d", t->z_offset, t->kp + 4);
    need = t->z_offset + 2 * t->kp;
  }
  if (t->row_stride % 4 || t->row_stride < need)
    return fail(FMX_ERR_SHAPE, "row_stride=%d must be a multiple of 4 and >= %d", t->row_stride, need);
  if (!aligned16(t->rows)) return fail(FMX_ERR_ALIGN, "table rows must be 16-byte aligned");
  if (t->max_field_rows < 1 || t->max_field_rows > t->n_rows) return fail(FMX_ERR_SHAPE, "max_field_rows out of range");
  if (t->n_sort_fields < 0 || (t->n_sort_fields > 0 && (t->n_sort_fields < t->n_fields || !t->sort_offsets || !t->sort_cols ||
                                                        t->max_sort_field_rows < 1 || t->max_sort_field_rows > t->max_field_rows)))
    return fail(FMX_ERR_SHAPE, "sort fields: n_sort_fields >= n_fields with sort_offsets, sort_cols and max_sort_field_rows, or 0");
  if (t->n_cols < 0 || (t->field_cols && t->n_cols < 1)) return fail(FMX_ERR_SHAPE, "field_cols needs n_cols >= 1");
  return FMX_OK;
}

int check_rule(const fmx_table_t *t, int rule) {
  if (rule == FMX_RULE_FTRL) {
    if (t->layout != FMX_LAYOUT_FTRL) return fail(FMX_ERR_ARG, "FMX_RULE_FTRL needs FMX_LAYOUT_FTRL");
  } else if (rule == FMX_RULE_SIGNADAM || rule == FMX_RULE_SGD) {
    if (t->layout != FMX_LAYOUT_WEIGHTS) return fail(FMX_ERR_ARG, "rule %d needs FMX_LAYOUT_WEIGHTS", rule);
  } else if (adaptive_rule(rule)) {
    if (t->layout != FMX_LAYOUT_MOMENTS) return fail(FMX_ERR_ARG, "%s needs FMX_LAYOUT_MOMENTS", rule_name(rule));
  } else {
    return fail(FMX_ERR_ARG, "unknown rule %d", rule);
  }
  return FMX_OK;
}

int check_adam(const fmx_hyper_t *h, int rule, int64_t n_steps) {
  if (rule != FMX_RULE_ADAM || !h) return FMX_OK;
  if (!(h->beta1 >= 0.f && h->beta1 < 1.f && h->beta2 >= 0.f && h->beta2 < 1.f))
    return fail(FMX_ERR_ARG, "FMX_RULE_ADAM: beta1 = %g and beta2 = %g must lie in [0, 1)", h->beta1, h->beta2);
  if (h->step < 0 || (int64_t)h->step + n_steps > INT32_MAX)
    return fail(FMX_ERR_ARG, "FMX_RULE_ADAM: step = %d must be >= 0 and step + steps of the call <= 2^31 - 1", h->step);
  return FMX_OK;
}

int check_sort_geometry(const fmx_table_t *t, int B) {
  if (B < 1) return fail(FMX_ERR_ARG, "B must be >= 1");
  const int Bp = fmx_sorted_width(B);
  if (Bp > MAX_SORT_WIDTH)
    return fail(FMX_ERR_UNSUPPORTED, "batch %d exceeds the LDS sort width %d", B, MAX_SORT_WIDTH);
  const int bbits = fmx_sorted_bbits(B);
  if ((uint64_t)(max_sort_rows(t) - 1) >= (uint64_t)(SENT >> bbits))
    return fail(FMX_ERR_UNSUPPORTED, "largest sort field (%lld rows) and batch %d do not fit a 32-bit (index, sample) composite: "
                "split the large fields (fmx_table_t.sort_offsets)", (long long)max_sort_rows(t), B);
  return FMX_OK;
}

int check_workspace(const fmx_table_t *t, int B, const void *workspace, int64_t workspace_bytes, const char *who) {
  if (!workspace) return fail(FMX_ERR_ARG, "%s: null workspace", who);
  if (!aligned16(workspace)) return fail(FMX_ERR_ALIGN, "%s: workspace must be 16-byte aligned", who);
  const int64_t need = (int64_t)carve(t, B, nullptr).bytes;
  if (workspace_bytes < need)
    return fail(FMX_ERR_SHAPE, "%s: workspace of %lld bytes, %lld needed for B = %d and %d sort fields (fmx_workspace_bytes)", who,
                (long long)workspace_bytes, (long long)need, B, n_sort_fields(t));
  return FMX_OK;
}

int named(int rc, const char *who) {
  if (rc != FMX_OK && !strstr(g_err, who)) {
    char msg[sizeof(g_err)];
    snprintf(msg, sizeof(msg), "%s", g_err);
    snprintf(g_err, sizeof(g_err), "%s: %s", who, msg);
  }
  return rc;
}

int check_pair_args(const fmx_table_t *table, const fmx_hyper_t *hyper, const int32_t *idx, int64_t n_pairs, const char *count_name,
                    float margin, const char *who) {
  if (!table) return fail(FMX_ERR_ARG, "%s: table is null", who);
  if (int rc = check_table(table)) return named(rc, who);
  if (!hyper) return fail(FMX_ERR_ARG, "%s: hyper is null", who);
  if (!idx) return fail(FMX_ERR_ARG, "%s: idx is null", who);
  if (n_pairs < 1) return fail(FMX_ERR_ARG, "%s: %s = %lld must be >= 1", who, count_name, (long long)n_pairs);
  if (!(margin >= 0.f) || !std::isfinite(margin)) return fail(FMX_ERR_ARG, "%s: margin = %g must be finite and >= 0", who, (double)margin);
  if (mapped(table))
    return fail(FMX_ERR_UNSUPPORTED, "%s: tables whose fields are pieces of index columns (field_cols / field_base) are not taken", who);
  return FMX_OK;
}

int check_list_args(const fmx_table_t *table, const fmx_hyper_t *hyper, const int32_t *idx, int32_t B_lists, int32_t G, int32_t *rows,
                    const char *who) {
  if (int rc = check_pair_args(table, hyper, idx, B_lists, "B_lists", 0.f, who)) return rc;
  if (G < 2) return fail(FMX_ERR_ARG, "%s: G = %d: a list is a positive and at least one negative (G >= 2)", who, G);
  if (G > LIST_MAX_G) return fail(FMX_ERR_UNSUPPORTED, "%s: G = %d: at most %d rows per list (one workgroup holds a list's waves)", who, G, LIST_MAX_G);
  if ((int64_t)B_lists * G > INT32_MAX) return fail(FMX_ERR_ARG, "%s: B_lists = %d, G = %d: B_lists * G rows exceed int32", who, B_lists, G);
  *rows = B_lists * G;
  return FMX_OK;
}

Tune &tune() {
  static Tune t = [] {
    Tune x;
    if (const char *e = getenv("FMX_WPB_FWD")) x.wpb_fwd = atoi(e);
    if (const char *e = getenv("FMX_WPB_UPD")) x.wpb_upd = atoi(e);
    if (const char *e = getenv("FMX_SORT_E")) x.sort_e = atoi(e);
    if (const char *e = getenv("FMX_SORT_AHEAD")) x.sort_ahead = atoi(e);
    if (const char *e = getenv("FMX_SORT_RESIDENT")) x.sort_resident = atoi(e);
    if (const char *e = getenv("FMX_ONLINE_PERSISTENT")) x.online_persistent = atoi(e);
    if (const char *e = getenv("FMX_INLINE_FIXUP")) x.inline_fixup = atoi(e);
    if (const char *e = getenv("FMX_SORT_CHUNKED")) x.sort_chunked = atoi(e);
    if (const char *e = getenv("FMX_UPD_ORDER")) x.upd_order = atoi(e);
    if (const char *e = getenv("FMX_MLP_CHAIN")) x.mlp_chain = atoi(e);
    auto ok = [](int v) { return v == 1 || v == 2 || v == 4; };
    if (!ok(x.wpb_fwd)) x.wpb_fwd = 4;
    if (!ok(x.wpb_upd)) x.wpb_upd = 2;
    return x;
  }();
  return t;
}
}  // namespace fmxd
namespace {

// ---- a library-owned side stream per device: the occurrence sort does not depend on the weights, so it runs beside
//      the forward pass (fmx_fm_step) or one batch ahead (fmx_fm_stream).  Created on first use, never destroyed. ----
struct Side {
  hipStream_t stream = nullptr;  // the sort runs here
  hipStream_t main = nullptr;    // stands in for the caller's stream when that is the legacy default stream, which
                                 // cannot be captured into a hipGraph
  hipEvent_t fork = nullptr, sorted[2] = {nullptr, nullptr}, consumed[2] = {nullptr, nullptr};
  hipEvent_t user_fork = nullptr, user_join = nullptr;
};

Side *side_for_current_device() {
  static std::mutex mu;
  static Side sides[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
  std::lock_guard<std::mutex> lock(mu);
  Side &sd = sides[dev];
  if (!sd.stream) {
    // the sort is background work: lowest stream priority for it, highest for the stand-in main stream
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    if (hipStreamCreateWithPriority(&sd.stream, hipStreamNonBlocking, lo) != hipSuccess) return nullptr;
    if (hipStreamCreateWithPriority(&sd.main, hipStreamNonBlocking, hi) != hipSuccess) return nullptr;
    bool ok = hipEventCreateWithFlags(&sd.fork, hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(&sd.user_fork, hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(&sd.user_join, hipEventDisableTiming) == hipSuccess;
    for (int i = 0; i < 2 && ok; ++i) {
      ok = hipEventCreateWithFlags(&sd.sorted[i], hipEventDisableTiming) == hipSuccess &&
           hipEventCreateWithFlags(&sd.consumed[i], hipEventDisableTiming) == hipSuccess;
    }
    if (!ok) return nullptr;
  }
  return &sd;
}

// ---- per device, beside Side: the sort fields' row counts of the tables k_fm_update has seen, as its dispatch orders.  The
//      offsets are device memory, so a table's first update pays one blocking copy of them (update_order, fmx_host.h) ----
struct UpdOrders {
  struct Entry {
    const int64_t *offs = nullptr;  // the key: the offsets pointer the update uses, the sort fields, n_rows, the largest sort field
    int F = 0;
    int64_t n_rows = 0, max_rows = 0;
    bool known = false;                   // false: the copy failed -- index order, and no second attempt
    uint8_t order[2][UPD_ORDER_MAX];      // ascending, descending
  };
  static constexpr int N = 8;  // tables per device; the oldest entry is replaced
  Entry e[N];
  int next = 0;
};

}  // namespace
namespace fmxd {

// order_words = the table's sort fields in ascending (mode 1) or descending (mode 2) row count, from the per-device cache
static bool cached_order(const fmx_table_t *table, int mode, bool may_fill, uint32_t *order_words) {
  memset(order_words, 0, UPD_ORDER_MAX);
  const int F = n_sort_fields(table);
  if ((mode != 1 && mode != 2) || F < 1 || F > UPD_ORDER_MAX) return false;
  static std::mutex mu;
  static UpdOrders per_device[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return false;
  const int64_t *offs = sort_offsets(table);
  std::lock_guard<std::mutex> lock(mu);
  UpdOrders &c = per_device[dev];
  UpdOrders::Entry *hit = nullptr;
  for (UpdOrders::Entry &x : c.e)
    if (x.offs == offs && x.F == F && x.n_rows == table->n_rows && x.max_rows == max_sort_rows(table)) hit = &x;
  if (!hit) {
    if (!may_fill) return false;
    hit = &c.e[c.next];
    c.next = (c.next + 1) % UpdOrders::N;
    hit->offs = offs;
    hit->F = F;
    hit->n_rows = table->n_rows;
    hit->max_rows = max_sort_rows(table);
    int64_t off[UPD_ORDER_MAX + 1], rows[UPD_ORDER_MAX];
    // (another thread may be capturing a stream of its own: the copy is no part of that capture, and must not end it)
    hipStreamCaptureMode cm = hipStreamCaptureModeRelaxed;
    const bool swapped = hipThreadExchangeStreamCaptureMode(&cm) == hipSuccess;
    hit->known = hipMemcpy(off, offs, sizeof(int64_t) * (size_t)(F + 1), hipMemcpyDeviceToHost) == hipSuccess;
    if (swapped) (void)hipThreadExchangeStreamCaptureMode(&cm);
    if (!hit->known) (void)hipGetLastError();  // not this launch's error: index order for this table
    for (int f = 0; f < F && hit->known; ++f) rows[f] = off[f + 1] - off[f];
    if (hit->known) hit->known = upd_order_of(rows, F, 1, hit->order[0]) == F && upd_order_of(rows, F, 2, hit->order[1]) == F;
  }
  if (!hit->known) return false;
  memcpy(order_words, hit->order[mode - 1], (size_t)F);  // byte i of the words: slot i's field (little-endian, as the kernel reads it)
  return true;
}

bool update_order(const fmx_table_t *table, bool may_fill, uint32_t *order_words) {
  return cached_order(table, tune().upd_order, may_fill, order_words);
}

bool sort_walk_order(const fmx_table_t *table, uint32_t *order_words) { return cached_order(table, 2, false, order_words); }

}  // namespace fmxd
namespace {

constexpr int OVERLAP_MIN_BATCH = 512;  // below this the extra event traffic costs more than the sort

// PAIR (fmx_fm_pair_forward): at least two waves per workgroup -- the batch is even and so is every workgroup's first sample, so
// a pair never straddles workgroups
template <int LPR, int NPASS, bool MAPPED = false, bool PAIR = false>
void launch_forward_np(const FwdArgs &a, int layout, hipStream_t st) {
  const int wpb = PAIR && tune().wpb_fwd < 2 ? 2 : tune().wpb_fwd;
  const dim3 grid((a.B + wpb - 1) / wpb), block(64 * wpb);
  // the forward reads [ V | w ] and the bias weight: a MOMENTS table is read as a WEIGHTS one (bias[0] is the weight)
  if (layout == FMX_LAYOUT_FTRL) hipLaunchKernelGGL((k_fm_forward<LPR, FMX_LAYOUT_FTRL, NPASS, MAPPED, PAIR>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((k_fm_forward<LPR, FMX_LAYOUT_WEIGHTS, NPASS, MAPPED, PAIR>), grid, block, 0, st, a);
}

template <int LPR, bool PAIR = false>
void launch_forward(const FwdArgs &a, int layout, hipStream_t st) {
  const int slots = WAVE / LPR;
  const int np = (a.F + slots - 1) / slots;
  if constexpr (!PAIR) {  // (the pair forward refuses such tables on the host)
    if (a.fcols || a.fbase) {  // fields are pieces of index columns: the generic field loop (the additions and their order are the same)
      launch_forward_np<LPR, 0, true>(a, layout, st);
      return;
    }
  }
  if (!with_one_of<1, 2, 3, 4>(np, [&](auto NP) { launch_forward_np<LPR, NP, false, PAIR>(a, layout, st); }))
    launch_forward_np<LPR, 0, false, PAIR>(a, layout, st);
}

// LIST (fmx_fm_list_forward): G * max(1, 4 / G) waves per workgroup -- 4, 3, 4 at G = 2, 3, 4, then G -- so a workgroup holds whole
// lists and no list straddles two; B_lists * G need not be a multiple of that (the waves past the last row go along to the barrier)
// (Q: k_fm_forward_listq, the corrected form, a.y = corr)
template <int LPR, bool Q = false>
void launch_forward_list(const FwdArgs &a, int layout, hipStream_t st) {
  const int G = a.list_g, wpb = G * (4 / G > 1 ? 4 / G : 1);
  const dim3 grid((a.B + wpb - 1) / wpb), block(64 * wpb);
  const int slots = WAVE / LPR, np = (a.F + slots - 1) / slots;
  auto launch = [&](auto NP) {
    if constexpr (Q) {
      if (layout == FMX_LAYOUT_FTRL) hipLaunchKernelGGL((k_fm_forward_listq<LPR, FMX_LAYOUT_FTRL, NP>), grid, block, 0, st, a);
      else hipLaunchKernelGGL((k_fm_forward_listq<LPR, FMX_LAYOUT_WEIGHTS, NP>), grid, block, 0, st, a);
    } else {
      if (layout == FMX_LAYOUT_FTRL) hipLaunchKernelGGL((k_fm_forward_list<LPR, FMX_LAYOUT_FTRL, NP>), grid, block, 0, st, a);
      else hipLaunchKernelGGL((k_fm_forward_list<LPR, FMX_LAYOUT_WEIGHTS, NP>), grid, block, 0, st, a);
    }
  };
  if (!with_one_of<1, 2, 3, 4>(np, launch)) launch(std::integral_constant<int, 0>{});
}

// threads and LDS bytes of a k_sort_occ workgroup at E composites per thread; sets a.small_bits
template <int E>
uint32_t sort_occ_shape(SortArgs &a, int &threads) {
  threads = a.Bp / E;
  uint32_t lds = (uint32_t)(a.Bp * sizeof(uint32_t));
  // fields of at most 511 rows take one counting pass inside the same launch (fmx_sort.inc, radix_field): on the Criteo list 24
  // of the 39 fields -- the launch's length is still the network's (the 15 larger fields), its chip time is not
  if (a.Bp <= RADIX_SMALL_WIDTH && threads >= 64) {
    a.small_bits = RADIX_SMALL_BITS;
    const uint32_t need = (uint32_t)radix_small_lds_bytes(a.Bp, threads);
    if (need > lds) lds = need;
  }
  return lds;
}

template <int E>
void launch_sort(SortArgs a, hipStream_t st) {
  int threads;
  const uint32_t lds = sort_occ_shape<E>(a, threads);
  const int grid = a.n_batches >= 8 ? 8 * a.F * ((a.n_batches + 7) / 8) : a.F * a.n_batches;
  hipLaunchKernelGGL((k_sort_occ<E>), dim3(grid), dim3(threads), lds, st, a);
}

// The resident-capped form (k_sort_occ_resident): min(units, cap) workgroups, rounded up to a multiple of 8 (every XCD serves
// its own batches).  *launched = false, and nothing issued, on a device whose workgroups cannot be kept one to a CU: the caller
// then issues the uncapped grid.
template <int E>
int launch_sort_resident(SortArgs a, int cap, const fmx_table_t *table, hipStream_t st, bool *launched) {
  *launched = false;
  int dev = 0, lds_cu = 0, lds_wg = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&lds_cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev) != hipSuccess ||
      hipDeviceGetAttribute(&lds_wg, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) {
    (void)hipGetLastError();
    return FMX_OK;
  }
  int threads;
  uint32_t lds = sort_occ_shape<E>(a, threads);
  // ONE workgroup per CU: two of 1,024 threads fill all 8 wave slots of every SIMD and close the CU to the step's kernels, which
  // is what this form is there to prevent.  Nothing in a launch says "one per CU"; a request for more than half of the CU's LDS
  // does (the unit itself needs Bp words and the counters, 41 KB at Bp = 4,096 -- three would fit).  The step's kernels use
  // next to no LDS and are not held up by it.
  const uint32_t one_per_cu = (uint32_t)align_up((size_t)lds_cu / 2 + 1, 256);
  if (one_per_cu > lds) lds = one_per_cu;
  if (lds > (uint32_t)lds_wg) return FMX_OK;
  if (int rc = raise_lds_limit<k_sort_occ_resident<E>>(lds_wg, "k_sort_occ_resident")) return rc;
  ResidentSortArgs ra;
  ra.s = a;
  const int units = a.n_batches * a.F;
  ra.n_wg = ((units < cap ? units : cap) + 7) / 8 * 8;
  ra.ordered = sort_walk_order(table, ra.order) ? 1 : 0;
  hipLaunchKernelGGL((k_sort_occ_resident<E>), dim3(ra.n_wg), dim3(threads), lds, st, ra);
  *launched = true;
  return FMX_OK;
}

// tune().sort_resident as a number of workgroups for the current device.  The default is one workgroup on HALF of the CUs (128 on
// the MI355X), between two bounds: the update's waves must still fit in one round -- (CUs - R) x 12 + R x 8 >= 2,497 at B = 4,096
// on the Criteo list: R <= 143 -- and the launch must end well inside the group it runs beside (16 steps, 310 us).  Measured in the
// steady loop ("r7"): R = 32 / 64 / 96 / 128 sort for 333 / 180 / 121 / 96 us and give 22.15 / 19.27 / 19.29 /
// 19.19 us per step against 19.60 uncapped.
int sort_resident_cap() {
  const int v = tune().sort_resident;
  if (v >= 0) return v;
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return cus / 2;
}

int prepare_sort(int B) {
  if ((size_t)fmx_sorted_width(B) * 4 <= 64 * 1024) return FMX_OK;
  static std::mutex mu;
  static bool raised = false;
  std::lock_guard<std::mutex> lock(mu);
  if (!raised) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_sort_occ<8>), hipFuncAttributeMaxDynamicSharedMemorySize, MAX_SORT_WIDTH * 4);
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_sort_occ<16>), hipFuncAttributeMaxDynamicSharedMemorySize, MAX_SORT_WIDTH * 4);
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_sort_occ<32>), hipFuncAttributeMaxDynamicSharedMemorySize, MAX_SORT_WIDTH * 4);
    if (e != hipSuccess) return fail(FMX_ERR_LAUNCH, "hipFuncSetAttribute: %s", hipGetErrorString(e));
    raised = true;
  }
  return FMX_OK;
}

int prepare_merge(int Bp) {
  if ((size_t)(Bp + Bp / 32) * 4 <= 64 * 1024) return FMX_OK;
  static std::mutex mu;
  static bool raised = false;
  std::lock_guard<std::mutex> lock(mu);
  if (!raised) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_sort_merge), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (MAX_SORT_WIDTH + MAX_SORT_WIDTH / 32) * 4);
    if (e != hipSuccess) return fail(FMX_ERR_LAUNCH, "hipFuncSetAttribute: %s", hipGetErrorString(e));
    raised = true;
  }
  return FMX_OK;
}

}  // namespace

int fmxd::sort_impl(const fmx_table_t *table, const int32_t *idx, int32_t B, uint32_t *sorted, uint32_t *runs, int32_t *error,
                    hipStream_t st, const SortBatch *mb) {
  SortArgs a;
  a.n_pool = mb ? mb->n_pool : 1;
  a.pool_first = mb ? mb->first : 0;
  a.n_batches = mb ? mb->n_batches : 1;
  a.pool_stride = mb ? mb->pool_stride : 0;
  a.sorted_stride = mb ? mb->sorted_stride : 0;
  a.idx = idx;
  a.foff = table->field_offsets;
  a.soff = sort_offsets(table);
  a.cols = sort_cols(table);
  a.sorted = sorted;
  a.error = error;
  a.B = B;
  a.F = n_sort_fields(table);
  a.Fi = n_cols(table);
  a.small_bits = 0;
  a.fcols = table->field_cols;
  a.fbase = table->field_base;
  a.Bp = fmx_sorted_width(B);
  a.bbits = fmx_sorted_bbits(B);
  // the chunked form wins on LATENCY (one or two batches per launch: the prefetched global sorts of the multi-GPU modes, a
  // single step); a launch of many batches fills the chip either way and the rank merge then costs more work than the
  // bitonic stages it replaces (8 batches of 16,384: 294 vs 118 us)
  if (a.Bp >= (tune().sort_chunked > 1 ? 2 * SORT_CHUNK : SORT_CHUNKED_MIN_WIDTH) && tune().sort_chunked && runs &&
      (a.n_batches <= 2 || tune().sort_chunked > 1)) {
    // chunk sort + rank merge, spread over the chip (k_sort_chunk / k_sort_merge)
    if (int rc = prepare_merge(a.Bp)) return rc;
    ChunkArgs c;
    c.s = a;
    c.runs = runs;
    c.runs_stride = (int64_t)align_up((size_t)a.F * a.Bp * 4, 256) / 4;
    c.C = a.Bp / SORT_CHUNK;
    const int units1 = a.n_batches * c.C, grid1 = 8 * a.F * ((units1 + 7) / 8);
    hipLaunchKernelGGL(k_sort_chunk, dim3(grid1), dim3(SORT_CHUNK_THREADS), 0, st, c);
    const int units2 = a.n_batches * a.F, grid2 = 8 * c.C * ((units2 + 7) / 8);
    hipLaunchKernelGGL(k_sort_merge, dim3(grid2), dim3(SORT_CHUNK_THREADS), (uint32_t)((a.Bp + a.Bp / 32) * sizeof(uint32_t)), st, c);
    return check_launch("k_sort_chunk / k_sort_merge");
  }
  if (int rc = prepare_sort(B)) return rc;
  // E elements per thread, Bp / E threads (a multiple of 64, at most 1024)
  int E = a.Bp <= 64 ? 1 : a.Bp <= 128 ? 2 : a.Bp <= 4096 ? 4 : a.Bp <= 8192 ? 8 : a.Bp <= 16384 ? 16 : 32;
  const int want = tune().sort_e;
  if (want > E && want <= 32 && (want & (want - 1)) == 0 && a.Bp / want >= 64) E = want;
  // (not at 32 composites per thread -- lists wider than 16,384: a unit's own 128 KB of LDS keep its workgroups one to a CU as
  // it is, and the walking loop around the widest network does not fit the registers)
  if (mb && mb->resident > 0 && E <= 16) {
    bool launched = false;
    int rc = FMX_OK;
    with_one_of<1, 2, 4, 8, 16>(E, [&](auto E_) { rc = launch_sort_resident<E_>(a, mb->resident, table, st, &launched); });
    if (rc != FMX_OK) return rc;
    if (launched) return check_launch("k_sort_occ_resident");
  }
  if (!with_one_of<1, 2, 4, 8, 16>(E, [&](auto E_) { launch_sort<E_>(a, st); })) launch_sort<32>(a, st);
  return check_launch("k_sort_occ");
}

namespace {

// sorts steps [first_step, first_step + n) of a pool of n_pool batches (step s takes batch s mod n_pool) with one launch, into
// n consecutive sorted buffers of the workspace from `sorted` on; resident > 0: the resident-capped form (SortBatch)
int sort_pool(const fmx_table_t *table, const int32_t *idx_pool, int n_pool, int B, int first_step, int n, const Workspace &w,
              uint32_t *sorted, int32_t *error, hipStream_t st, int resident = 0) {
  SortBatch mb;
  mb.n_pool = n_pool;
  mb.first = first_step % n_pool;
  mb.n_batches = n;
  mb.pool_stride = (int64_t)B * (int64_t)n_cols(table);
  mb.sorted_stride = (int64_t)w.sorted_stride;
  mb.resident = resident;
  return sort_impl(table, idx_pool, B, sorted, w.runs, error, st, &mb);
}

// A loop called on the legacy default stream (handle 0: it cannot be captured and is slow to enqueue on) runs on the side's
// stand-in main stream instead, after the caller's work; the caller's stream waits for it when the guard goes.  `st` is the
// stream to issue on.  No detour without a side (sd == nullptr) or on any other stream.
struct Detour {
  Side *sd;
  hipStream_t user, st;
  Detour(Side *side, hipStream_t stream) : sd(stream == nullptr ? side : nullptr), user(stream), st(stream) {
    if (!sd) return;
    (void)hipEventRecord(sd->user_fork, user);
    st = sd->main;
    (void)hipStreamWaitEvent(st, sd->user_fork, 0);
  }
  ~Detour() {
    if (!sd) return;
    (void)hipEventRecord(sd->user_join, st);
    (void)hipStreamWaitEvent(user, sd->user_join, 0);
  }
  Detour(const Detour &) = delete;
  Detour &operator=(const Detour &) = delete;
};

// The online loop over a device-resident pool (fmx_fm_stream, fmx_deepfm_stream): step s takes batch s mod n_pool and runs
// before_update(s, idx, y, st), then update(s, sorted, st) with the batch's sorted occurrence list; either returns a status.
// The occurrence sort does not depend on the weights: groups of `ahead` batches are sorted by ONE launch on the side stream
// while the previous group runs forward / update / fixup on `stream`.  Ring of 2 * ahead sorted buffers; per group one sort
// launch and four event operations, so the host issues ~3.6 runtime calls per step instead of 8 (at ~4 us each the per-batch
// version was host-bound).  Below OVERLAP_MIN_BATCH every group is sorted on `stream` in front of its steps.
template <class BeforeUpdate, class Update>
int pool_loop(const fmx_table_t *table, const int32_t *idx_pool, const float *y_pool, int n_pool, int B, int n_steps,
              const Workspace &w, int32_t *error, hipStream_t stream, BeforeUpdate &&before_update, Update &&update) {
  Side *sd = (B >= OVERLAP_MIN_BATCH && n_steps > 0) ? side_for_current_device() : nullptr;
  const Detour detour(sd, stream);
  const hipStream_t st = detour.st;
  const size_t F = (size_t)n_cols(table);
  int ahead = tune().sort_ahead;
  if (ahead < 1) ahead = 1;
  if (ahead > SORT_AHEAD_MAX) ahead = SORT_AHEAD_MAX;
  // the first group holds up to 4 batches, the others `ahead` (8): one launch sorts four batches in about the time of one (one
  // workgroup per field and batch: 18.4 against 17.1 us, tools/micro/sort_bench.hip), so the first update waits no longer than
  // behind a one-batch group, and a short call issues three sort launches and their events instead of five while the device
  // is still waiting for the host.  Group g uses half (g & 1) of the ring of 2 * ahead sorted buffers.
  auto group_size = [&](int g, int first_step) {
    int n = g == 0 ? 4 : ahead;
    if (n > ahead) n = ahead;
    if (n > n_steps - first_step) n = n_steps - first_step;
    return n;
  };
  // The side stream's launches from the call's THIRD group on run beside a whole group of `ahead` steps and their lists are
  // needed a group later: they take the resident-capped form, which leaves the step's kernels their wave slots (fmx_sort.inc,
  // k_sort_occ_resident).  The first group's length is what the first update waits for, and the second group is sorted beside
  // the first's four steps and needed right behind them (capped as well, a 20-step call took 21.7 - 22.0 us per step instead
  // of 20.7 - 21.1): one workgroup per unit for both, as ever.
  const int resident = sd ? sort_resident_cap() : 0;
  auto sort_group = [&](int g, int first_step, int n, hipStream_t where) -> int {  // steps [first_step, first_step + n)
    return sort_pool(table, idx_pool, n_pool, B, first_step, n, w, w.sorted + (size_t)(g & 1) * ahead * w.sorted_stride, error, where,
                     sd && g >= 2 ? resident : 0);
  };
  int rc = FMX_OK;
  if (sd) {
    (void)hipEventRecord(sd->fork, st);
    (void)hipStreamWaitEvent(sd->stream, sd->fork, 0);
    rc = sort_group(0, 0, group_size(0, 0), sd->stream);
    (void)hipEventRecord(sd->sorted[0], sd->stream);
  }
  int first_step = 0;
  for (int g = 0; first_step < n_steps && rc == FMX_OK; ++g) {
    const int n = group_size(g, first_step);
    const int next_first = first_step + n;
    if (!sd) rc = sort_group(g, first_step, n, st);
    for (int i = 0; i < n && rc == FMX_OK; ++i) {
      const int s = first_step + i, j = s % n_pool;
      rc = before_update(s, idx_pool + (size_t)j * B * F, y_pool ? y_pool + (size_t)j * B : nullptr, st);  // (no labels: the pair loss)
      if (sd && i == 0) (void)hipStreamWaitEvent(st, sd->sorted[g & 1], 0);
      if (rc == FMX_OK) rc = update(s, w.sorted + ((size_t)(g & 1) * ahead + i) * w.sorted_stride, st);
      // the next group is sorted while this one runs; its launch is issued BEHIND the group's first step, so that at the start
      // of a call -- the device idle, every launch waiting for the host -- the first forward and update are not held up by it
      if (sd && i == 0 && next_first < n_steps && rc == FMX_OK) {
        if (g >= 1) (void)hipStreamWaitEvent(sd->stream, sd->consumed[(g + 1) & 1], 0);  // group g-1 is done with that half
        rc = sort_group(g + 1, next_first, group_size(g + 1, next_first), sd->stream);
        (void)hipEventRecord(sd->sorted[(g + 1) & 1], sd->stream);
      }
    }
    if (sd) (void)hipEventRecord(sd->consumed[g & 1], st);
    first_step = next_first;
  }
  return rc;
}

FwdArgs fill_fwd(const fmx_table_t *table, const fmx_hyper_t *hyper, const int32_t *idx, const float *xv, const float *y,
                 int32_t B, int32_t loss_kind, float inv_b, const fmx_fwd_out_t *out) {
  FwdArgs a;
  a.ldS = out->sample_ld > 0 ? out->sample_ld : table->kp;
  a.ld1 = out->sample_ld > 0 ? out->sample_ld : 1;
  a.rows = table->rows;
  a.foff = table->field_offsets;
  a.bias = table->bias;
  a.idx = idx;
  a.xv = xv;
  a.y = y;
  a.out = *out;
  a.h = kernel_hyper(hyper, -1);
  a.B = B;
  a.F = table->n_fields;
  a.Fc = n_cols(table);
  a.fcols = table->field_cols;
  a.fbase = table->field_base;
  a.kp = table->kp;
  a.stride = table->row_stride;
  a.zoff = table->z_offset;
  a.loss_kind = loss_kind;
  a.inv_b = inv_b;
  a.margin = 0.f;  // (the list forward puts its G in the same word)
  return a;
}

}  // namespace

int fmxd::forward_impl(const fmx_table_t *table, const fmx_hyper_t *hyper, const int32_t *idx, const float *xv, const float *y,
                       int32_t B, int32_t loss_kind, float inv_b, const fmx_fwd_out_t *out, hipStream_t st) {
  const FwdArgs a = fill_fwd(table, hyper, idx, xv, y, B, loss_kind, inv_b, out);
  with_lpr(table->kp, [&](auto LPR) { launch_forward<LPR>(a, table->layout, st); });
  return check_launch("k_fm_forward");
}

namespace {

template <int LPR>
int launch_forward_part(const PartArgs &a, int np, int n_local_blocks, hipStream_t st) {
  const int per_wave = (WAVE / LPR) >> a.sl_log2, waves = (a.B + per_wave - 1) / per_wave;
  const dim3 grid((waves + 3) / 4, n_local_blocks), block(256);
  if (!with_one_of<1, 2, 3, 4>(np, [&](auto NP) { hipLaunchKernelGGL((k_fm_forward_part<LPR, NP>), grid, block, 0, st, a); }))
    return fail(FMX_ERR_UNSUPPORTED, "fmx_fm_forward_partial: more than 4 fields per lane group");
  return check_launch("k_fm_forward_part");
}

template <int LPR, int LAYOUT>
int launch_forward_finish_g(const FinishArgs &a, int G, hipStream_t st) {
  const int waves = (a.B + (WAVE / LPR) - 1) / (WAVE / LPR);
  const dim3 grid((waves + 3) / 4), block(256);
  if (!with_one_of<1, 2, 4, 8, 16>(G, [&](auto G_) { hipLaunchKernelGGL((k_fm_forward_finish<LPR, LAYOUT, G_>), grid, block, 0, st, a); }))
    return fail(FMX_ERR_ARG, "fmx_fm_forward_finish: n_owners must be 1, 2, 4, 8 or 16");
  return check_launch("k_fm_forward_finish");
}

template <int LPR>
int launch_forward_finish(const FinishArgs &a, int layout, int G, hipStream_t st) {
  if (G > WAVE / LPR) return fail(FMX_ERR_ARG, "fmx_fm_forward_finish: more owners than lane groups");
  return layout == FMX_LAYOUT_FTRL ? launch_forward_finish_g<LPR, FMX_LAYOUT_FTRL>(a, G, st)      // MOMENTS: as WEIGHTS (bias[0])
                                   : launch_forward_finish_g<LPR, FMX_LAYOUT_WEIGHTS>(a, G, st);
}

// the tree cut into n_blocks blocks, the table holding n_local_blocks of them: fields [lb NP SL, (lb + 1) NP SL) are block lb's
int part_impl(const fmx_table_t *table, const int32_t *idx, const float *xv, int32_t B, int32_t n_blocks, int32_t n_local_blocks,
              int32_t group, float *parts_out, int32_t *error, hipStream_t st) {
  if (group <= 0) group = B;
  if (B % group) return fail(FMX_ERR_SHAPE, "fmx_fm_forward_partial: B = %d is not a multiple of group = %d", B, group);
  const int lpr = lpr_of(table->kp), slots = WAVE / lpr;
  if (n_blocks < 1 || n_blocks > slots || (n_blocks & (n_blocks - 1))) return fail(FMX_ERR_ARG, "n_blocks must be a power of two <= %d", slots);
  if (n_local_blocks < 1 || n_local_blocks > n_blocks) return fail(FMX_ERR_ARG, "n_local_blocks must be in [1, n_blocks]");
  const int sl = slots / n_blocks;
  if (n_local_blocks > 1 && table->n_fields % (n_local_blocks * sl))  // (one block: a ragged last pass is fine)
    return fail(FMX_ERR_SHAPE, "a table of %d blocks of %d lane groups holds a multiple of %d fields (empty fields fill the holes), not %d",
                n_local_blocks, sl, n_local_blocks * sl, table->n_fields);
  int sl_log2 = 0;
  while ((1 << sl_log2) < sl) ++sl_log2;
  PartArgs a;
  a.rows = table->rows;
  a.foff = table->field_offsets;
  a.fcols = table->field_cols;
  a.fbase = table->field_base;
  a.idx = idx;
  a.xv = xv;
  a.rec = parts_out;
  a.error = error;
  a.B = B;
  a.F = table->n_fields;
  a.Fc = n_cols(table);
  a.stride = table->row_stride;
  a.sl_log2 = sl_log2;
  a.group = group;
  const int np = (table->n_fields + n_local_blocks * sl - 1) / (n_local_blocks * sl);
  return with_lpr(table->kp, [&](auto LPR) { return launch_forward_part<LPR>(a, np, n_local_blocks, st); });
}

int check_forward_args(const fmx_table_t *table, const fmx_hyper_t *hyper, const int32_t *idx, const float *y, int32_t B,
                       int32_t loss_kind, const fmx_fwd_out_t *out) {
  if (int rc = check_table(table)) return rc;
  if (!hyper || !idx || !out) return fail(FMX_ERR_ARG, "fmx_fm_forward: null argument");
  if (B < 1) return fail(FMX_ERR_ARG, "B must be >= 1");
  if (loss_kind < FMX_LOSS_NONE || loss_kind > FMX_LOSS_BCE_SIGMOID) return fail(FMX_ERR_ARG, "unknown loss %d", loss_kind);
  if (loss_kind != FMX_LOSS_NONE && !y) return fail(FMX_ERR_ARG, "a loss needs labels y");
  if ((out->S && !aligned16(out->S)) || (out->bi && !aligned16(out->bi)))
    return fail(FMX_ERR_ALIGN, "S and bi must be 16-byte aligned");
  if (out->sample_ld != 0 && (out->sample_ld < table->kp || out->sample_ld % 4))
    return fail(FMX_ERR_SHAPE, "sample_ld=%d must be 0 or a multiple of 4 that is >= kp", out->sample_ld);
  return FMX_OK;
}

int check_step_args(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, int32_t loss_kind, int32_t B,
                    const void *workspace, const fmx_fwd_out_t *fwd) {
  if (int rc = check_table(table)) return rc;
  if (int rc = check_rule(table, rule)) return rc;
  if (int rc = check_sort_geometry(table, B)) return rc;
  if (!hyper || !workspace) return fail(FMX_ERR_ARG, "null hyper / workspace");
  if (int rc = check_adam(hyper, rule, 1)) return rc;
  if (!aligned16(workspace)) return fail(FMX_ERR_ALIGN, "workspace must be 16-byte aligned");
  if (!fwd || !fwd->S || !fwd->dz || !fwd->loss) return fail(FMX_ERR_ARG, "fwd->S, fwd->loss, fwd->dz are required");
  if (!aligned16(fwd->S) || !aligned16(fwd->dz) || !aligned16(fwd->loss))
    return fail(FMX_ERR_ALIGN, "fwd->S, fwd->dz and fwd->loss must be 16-byte aligned");
  if (loss_kind != FMX_LOSS_BCE_LOGITS && loss_kind != FMX_LOSS_BCE_SIGMOID) return fail(FMX_ERR_ARG, "a step needs a loss");
  return FMX_OK;
}

// ---- the step and the stream of the pure FM, once for its objectives (pointwise, pair, list).  The arguments have been
//      checked; forward(idx, xv, y, st) launches the objective's forward into fwd; `tu` is the table as the update sees it
//      (the list form's: list_update_table).  `rows`: the full-width rows of a step ----
// One stream: sort -> forward -> update.  (Until r3 the sort ran on the side stream beside the forward pass; a dependency that
// crosses streams costs 5 - 6 us on the device and four more runtime calls on the host, as much as the overlap of a 7 us forward
// with an 18 us sort saves -- and a caller of single steps is host-bound: FMAdam.update_embedding 65 - 73 against 90 - 112 us
// per batch, tools/class_surface_profile.py.  Loops over many batches: stream_run, where a sort launch covers 16 of them.)
template <class Forward>
int step_run(const fmx_table_t *table, const fmx_table_t *tu, const fmx_hyper_t *hyper, int32_t rule, const int32_t *idx, const float *xv,
             const float *y, int32_t rows, float inv_b, const Workspace &w, const fmx_fwd_out_t *fwd, float *loss_out, hipStream_t st,
             Forward &&forward) {
  if (int rc = sort_impl(table, idx, rows, w.sorted, w.runs, fwd->error, st)) return rc;
  if (int rc = forward(idx, xv, y, st)) return rc;
  return update_impl(tu, hyper, rule, w, w.sorted, xv, fwd->S, fwd->dz, fwd->dz, nullptr, rows, fwd->loss, inv_b, loss_out, st, nullptr,
                     fwd->sample_ld, fwd->error);
}

// n_steps of them over a pool of n_pool batches (pool_loop: the sorts of a group of steps in one launch, ahead of them)
template <class Forward>
int stream_run(const fmx_table_t *table, const fmx_table_t *tu, const fmx_hyper_t *hyper, int32_t rule, const int32_t *idx_pool,
               const float *y_pool, int32_t n_pool, int32_t rows, float inv_b, int32_t n_steps, const Workspace &w, const fmx_fwd_out_t *fwd,
               float *loss_out, hipStream_t st, Forward &&forward) {
  auto before_update = [&](int, const int32_t *idx, const float *y, hipStream_t s_) { return forward(idx, nullptr, y, s_); };
  auto update = [&](int s, const uint32_t *sorted, hipStream_t s_) {
    const fmx_hyper_t hs = hyper_at_step(hyper, rule, s);
    return update_impl(tu, &hs, rule, w, sorted, nullptr, fwd->S, fwd->dz, fwd->dz, nullptr, rows, fwd->loss, inv_b,
                       loss_out ? loss_out + s : nullptr, s_, nullptr, fwd->sample_ld, fwd->error);
  };
  return pool_loop(table, idx_pool, y_pool, n_pool, rows, n_steps, w, fwd->error, st, before_update, update);
}

// the pointwise objective's forward, as step_run and stream_run call it (the pair's and the list's: pair_forward, list_forward)
inline auto point_forward(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t B, int32_t loss_kind, float inv_b,
                          const fmx_fwd_out_t *fwd) {
  return [=](const int32_t *idx, const float *xv, const float *y, hipStream_t st) {
    return forward_impl(table, hyper, idx, xv, y, B, loss_kind, inv_b, fwd, st);
  };
}

// what the pair and list streams refuse of their pool and step count
int check_pool_steps(int32_t n_pool, int32_t n_steps, const char *who) {
  if (n_pool < 1) return fail(FMX_ERR_ARG, "%s: n_pool = %d must be >= 1", who, n_pool);
  if (n_steps < 0) return fail(FMX_ERR_ARG, "%s: n_steps = %d must be >= 0", who, n_steps);
  return FMX_OK;
}

#include "fmx_pair.inc"
#include "fmx_list.inc"

}  // namespace

// ------------------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------------------
extern "C" {

int fmx_version(void) { return FMX_VERSION; }

int fmx_set_option(const char *name, int value) {
  if (!name) return fail(FMX_ERR_ARG, "fmx_set_option: null name");
  Tune &t = tune();
  int *slot = nullptr;
  if (!strcmp(name, "inline_fixup")) slot = &t.inline_fixup;
  else if (!strcmp(name, "sort_ahead")) slot = &t.sort_ahead;
  else if (!strcmp(name, "sort_resident")) slot = &t.sort_resident;
  else if (!strcmp(name, "online_persistent")) slot = &t.online_persistent;
  else if (!strcmp(name, "afm_online_persistent")) slot = &t.afm_online_persistent;
  else if (!strcmp(name, "afm_pair_online_persistent")) slot = &t.afm_pair_online_persistent;
  else if (!strcmp(name, "sort_chunked")) slot = &t.sort_chunked;
  else if (!strcmp(name, "upd_order")) slot = &t.upd_order;
  else if (!strcmp(name, "mlp_chain")) slot = &t.mlp_chain;
  else return fail(FMX_ERR_ARG, "fmx_set_option: unknown option '%s'", name);
  const int old = *slot;
  *slot = slot == &t.sort_resident && value < 0 ? -1 : value;
  return old;
}

const char *fmx_last_error_string(void) { return g_err; }

int fmx_update_order(const int64_t *rows, int32_t n, int32_t mode, uint8_t *order) {
  if (!rows || !order) return fail(FMX_ERR_ARG, "fmx_update_order: null argument");
  if (n < 1) return fail(FMX_ERR_ARG, "fmx_update_order: n = %d must be >= 1", (int)n);
  if (mode < 0 || mode > 2) return fail(FMX_ERR_ARG, "fmx_update_order: mode = %d is none of 0, 1, 2", (int)mode);
  return upd_order_of(rows, n, mode, order);
}

int fmx_sorted_width(int B) {
  int w = 64;
  while (w < B && w < (1 << 30)) w <<= 1;
  return w;
}

int fmx_sorted_bbits(int B) {
  int w = fmx_sorted_width(B), bits = 0;
  while ((1 << bits) < w) ++bits;
  return bits;
}

int64_t fmx_workspace_bytes(const fmx_table_t *table, int32_t B) {
  if (check_table(table) != FMX_OK) return FMX_ERR_ARG;
  if (B < 1) return fail(FMX_ERR_ARG, "B must be >= 1");
  return (int64_t)carve(table, B, nullptr).bytes;
}

int fmx_fm_forward(const fmx_table_t *table, const fmx_hyper_t *hyper, const int32_t *idx, const float *xv,
                   const float *y, int32_t B, int32_t loss_kind, float inv_b, const fmx_fwd_out_t *out,
                   fmx_stream_t stream) {
  if (int rc = check_forward_args(table, hyper, idx, y, B, loss_kind, out)) return rc;
  return forward_impl(table, hyper, idx, xv, y, B, loss_kind, inv_b, out, static_cast<hipStream_t>(stream));
}

int fmx_fm_forward_partial(const fmx_table_t *table, const int32_t *idx, const float *xv, int32_t B, int32_t n_blocks,
                           int32_t n_local_blocks, int32_t group, float *parts_out, int32_t *error, fmx_stream_t stream) {
  if (int rc = check_table(table)) return rc;
  if (!idx || !parts_out) return fail(FMX_ERR_ARG, "fmx_fm_forward_partial: null argument");
  if (B < 1) return fail(FMX_ERR_ARG, "B must be >= 1");
  if (!aligned16(parts_out)) return fail(FMX_ERR_ALIGN, "parts_out must be 16-byte aligned");
  return part_impl(table, idx, xv, B, n_blocks, n_local_blocks, group, parts_out, error, static_cast<hipStream_t>(stream));
}

int fmx_fm_forward_finish(const fmx_hyper_t *hyper, const float *bias, int32_t layout, int32_t kp, const float *parts,
                          int64_t owner_stride, int32_t n_owners, const float *y, int32_t B, int32_t loss_kind, float inv_b,
                          const fmx_fwd_out_t *out, fmx_stream_t stream) {
  if (!hyper || !bias || !parts || !out) return fail(FMX_ERR_ARG, "fmx_fm_forward_finish: null argument");
  if (layout != FMX_LAYOUT_WEIGHTS && layout != FMX_LAYOUT_FTRL && layout != FMX_LAYOUT_MOMENTS)
    return fail(FMX_ERR_ARG, "unknown layout %d", layout);
  if (!lpr_of(kp)) return fail(FMX_ERR_SHAPE, "kp=%d must be 4/8/16/32/64", kp);
  if (B < 1) return fail(FMX_ERR_ARG, "B must be >= 1");
  if (loss_kind < FMX_LOSS_NONE || loss_kind > FMX_LOSS_BCE_SIGMOID) return fail(FMX_ERR_ARG, "unknown loss %d", loss_kind);
  if (loss_kind != FMX_LOSS_NONE && !y) return fail(FMX_ERR_ARG, "a loss needs labels y");
  if (!aligned16(parts) || owner_stride % 4 || (out->S && !aligned16(out->S)) || (out->bi && !aligned16(out->bi)))
    return fail(FMX_ERR_ALIGN, "parts, S and bi must be 16-byte aligned, owner_stride a multiple of 4");
  if (out->sample_ld != 0 && (out->sample_ld < kp || out->sample_ld % 4))
    return fail(FMX_ERR_SHAPE, "sample_ld=%d must be 0 or a multiple of 4 that is >= kp", out->sample_ld);
  FinishArgs a;
  a.parts = parts;
  a.rank_stride = owner_stride;
  a.bias = bias;
  a.y = y;
  a.out = *out;
  a.h = kernel_hyper(hyper, -1);
  a.B = B;
  a.loss_kind = loss_kind;
  a.ldS = out->sample_ld > 0 ? out->sample_ld : kp;
  a.ld1 = out->sample_ld > 0 ? out->sample_ld : 1;
  a.inv_b = inv_b;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return with_lpr(kp, [&](auto LPR) { return launch_forward_finish<LPR>(a, layout, n_owners, st); });
}

int fmx_sort_occurrences(const fmx_table_t *table, const int32_t *idx, int32_t B, void *workspace, int64_t workspace_bytes, int32_t *error,
                         fmx_stream_t stream) {
  if (int rc = check_table(table)) return rc;
  if (!idx || !workspace) return fail(FMX_ERR_ARG, "fmx_sort_occurrences: null argument");
  if (!aligned16(workspace)) return fail(FMX_ERR_ALIGN, "workspace must be 16-byte aligned");
  if (int rc = check_sort_geometry(table, B)) return rc;
  if (int rc = check_workspace(table, B, workspace, workspace_bytes, "fmx_sort_occurrences")) return rc;
  const Workspace w = carve(table, B, workspace);
  return sort_impl(table, idx, B, w.sorted, w.runs, error, static_cast<hipStream_t>(stream));
}

int fmx_fm_update(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, void *workspace, int64_t workspace_bytes, const float *xv,
                  const float *S, const float *dz_first, const float *dz_bi, const float *gbi, int32_t B,
                  int32_t sample_ld, const float *loss_b, float inv_b, float *loss_out, fmx_stream_t stream) {
  if (int rc = check_table(table)) return rc;
  if (sample_ld != 0 && (sample_ld < table->kp || sample_ld % 4))
    return fail(FMX_ERR_SHAPE, "sample_ld=%d must be 0 or a multiple of 4 that is >= kp", sample_ld);
  if (int rc = check_rule(table, rule)) return rc;
  if (!hyper || !workspace || !S || !dz_first) return fail(FMX_ERR_ARG, "fmx_fm_update: null argument");
  if (int rc = check_adam(hyper, rule, 1)) return rc;
  if (!dz_bi && !gbi) return fail(FMX_ERR_ARG, "fmx_fm_update: one of dz_bi / gbi is required");
  if (int rc = check_sort_geometry(table, B)) return rc;
  if (!aligned16(workspace) || !aligned16(S) || (gbi && !aligned16(gbi)) ||
      (sample_ld == 0 && (!aligned16(dz_first) || (loss_b && !aligned16(loss_b)))))
    return fail(FMX_ERR_ALIGN, "workspace, S, gbi (and dense dz_first / loss_b) must be 16-byte aligned");
  if (int rc = check_workspace(table, B, workspace, workspace_bytes, "fmx_fm_update")) return rc;
  const Workspace w = carve(table, B, workspace);
  return update_impl(table, hyper, rule, w, w.sorted, xv, S, dz_first, dz_bi, gbi, B, loss_b, inv_b, loss_out,
                     static_cast<hipStream_t>(stream), nullptr, sample_ld);
}

int fmx_fm_update_occ(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, void *workspace, int64_t workspace_bytes,
                      const float *xv, const float *dz_first, const float *occ_grad, int32_t ld_occ, int32_t B, const float *loss_b,
                      float inv_b, float *loss_out, fmx_stream_t stream) {
  if (int rc = check_table(table)) return rc;
  if (mapped(table)) return fail(FMX_ERR_UNSUPPORTED, "fmx_fm_update_occ: tables whose fields are pieces of index columns are not supported");
  if (int rc = check_rule(table, rule)) return rc;
  if (!hyper || !workspace || !dz_first || !occ_grad) return fail(FMX_ERR_ARG, "fmx_fm_update_occ: null argument");
  if (int rc = check_adam(hyper, rule, 1)) return rc;
  if (int rc = check_sort_geometry(table, B)) return rc;
  if (ld_occ % 4 || (int64_t)ld_occ < (int64_t)table->n_fields * table->kp)
    return fail(FMX_ERR_SHAPE, "fmx_fm_update_occ: ld_occ=%d must be a multiple of 4 and >= n_fields * kp = %d", ld_occ,
                table->n_fields * table->kp);
  if (!aligned16(workspace) || !aligned16(occ_grad) || !aligned16(dz_first) || (loss_b && !aligned16(loss_b)))
    return fail(FMX_ERR_ALIGN, "fmx_fm_update_occ: workspace, occ_grad, dz_first and loss_b must be 16-byte aligned");
  if (int rc = check_workspace(table, B, workspace, workspace_bytes, "fmx_fm_update_occ")) return rc;
  const Workspace w = carve(table, B, workspace);
  return update_occ_impl(table, hyper, rule, w, xv, dz_first, occ_grad, ld_occ, B, loss_b, inv_b, loss_out,
                         static_cast<hipStream_t>(stream));
}

// NFM's input logit: the first-order sum plus the bias (reference nfm_adam.py:78-88), one fp32 add per sample as the trainer does it
__global__ void k_first_plus_bias(float *out, const float *sfirst, const float *bias, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) out[b] = sfirst[b] + bias[0];
}

// The mini-batch DeepFM loop over a device-resident pool (BASELINE configs[3]): per step the forward of the tables, the MLP
// section on bi (fmx_mlp_section: k_mlp_chain, k_mlp_wgrad_stream, k_mlp_reduce with the SGD of the MLP applied in it) and the
// table update with dL/dbi, all issued from here; the occurrence sorts run in groups on the side stream (pool_loop).
// Through the Python trainer the same step is bound by its host side (84 us of calls per step for 67 us of kernels).
// fmx_deepfm_stream (opt null: the network under SGD by lr_mlp, the tables under the weights / FTRL rules) and fmx_deepfm_stream_opt
// (the network under opt's rule, the tables under any rule; every check of the network in front of the first launch)
static int deepfm_stream_impl(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_mlp_t *mlp, int32_t loss_kind,
                              int32_t fm_term, const int32_t *idx_pool, const float *y_pool, int32_t n_pool, int32_t B, float inv_b,
                              int32_t n_steps, void *workspace, int64_t workspace_bytes, void *mlp_workspace, int64_t mlp_workspace_bytes,
                              const fmx_fwd_out_t *fwd, float *dz, float *gbi, float *grads, float lr_mlp, const fmx_mlp_opt_t *opt,
                              float *loss_out, fmx_stream_t stream, const char *who, float pair_margin = -1.f) {
  const bool pair = pair_margin >= 0.f;  // fmx_deepfm_pair_stream: B = 2 B_pairs rows, the pair loss under that margin, no labels
  if (!opt && adaptive_rule(rule)) return refuse_adaptive(rule, who);
  if (int rc = check_table(table)) return rc;
  if (int rc = check_rule(table, rule)) return rc;
  if (!hyper || !mlp || !workspace || !mlp_workspace || !fwd || !fwd->S || !fwd->bi || !fwd->logit || !dz || !gbi || !grads)
    return fail(FMX_ERR_ARG, "%s: null argument (fwd needs S, bi and logit)", who);
  if (fwd->sample_ld != 0) return fail(FMX_ERR_ARG, "%s: dense forward outputs only (sample_ld = 0)", who);
  // NFM: k_first_plus_bias reads bias[0], the bias weight of the weights and the moments layouts
  if (!fm_term && (!fwd->sfirst || (opt ? table->layout == FMX_LAYOUT_FTRL : table->layout != FMX_LAYOUT_WEIGHTS)))
    return fail(FMX_ERR_UNSUPPORTED, "%s: fm_term = 0 (NFM) needs fwd->sfirst and a table in the weights%s layout", who, opt ? " or the moments" : "");
  if (!idx_pool || (!pair && !y_pool) || n_pool < 1 || n_steps < 0 || B < 1) return fail(FMX_ERR_ARG, "%s: bad pool / step count", who);
  if (opt) {
    if (int rc = check_adam(hyper, rule, n_steps)) return rc;
    if (int rc = mlp_opt_check(mlp, B, mlp_workspace, mlp_workspace_bytes, grads, opt, n_steps, who)) return rc;
  }
  if (pair && !opt) {  // the pair stream is told the size of the network's workspace under either rule, and checks it
    const int64_t need = fmx_mlp_section_workspace_bytes(mlp, B);
    if (need < 0) return fail(FMX_ERR_UNSUPPORTED, "%s: needs 1 <= layers <= %d, k >= 1, hidden >= 1", who, MLP_BIG_MAX_L);
    if (mlp_workspace_bytes < need)
      return fail(FMX_ERR_SHAPE, "%s: the MLP workspace holds %lld bytes, fmx_mlp_section_workspace_bytes asks for %lld", who,
                  (long long)mlp_workspace_bytes, (long long)need);
  }
  if (mlp->k > table->kp) return fail(FMX_ERR_SHAPE, "%s: the MLP reads k=%d columns of a bi of kp=%d", who, mlp->k, table->kp);
  if (!aligned16(gbi) || !aligned16(dz)) return fail(FMX_ERR_ALIGN, "dz and gbi must be 16-byte aligned");
  if (int rc = check_sort_geometry(table, B)) return rc;
  if (int rc = check_workspace(table, B, workspace, workspace_bytes, who)) return rc;
  const Workspace w = carve(table, B, workspace);
  MlpReduceArgs red;  // the section's last launch, set up by before_update, rides inside the table update's (k_fm_update_rider)
  auto before_update = [&](int s, const int32_t *idx, const float *y, hipStream_t st) -> int {
    int rc = forward_impl(table, hyper, idx, nullptr, nullptr, B, FMX_LOSS_NONE, inv_b, fwd, st);
    if (rc == FMX_OK && !fm_term) {  // NFM: the network's input logit is first-order + bias; the FM logit's buffer holds it
      hipLaunchKernelGGL(k_first_plus_bias, dim3((B + 255) / 256), dim3(256), 0, st, fwd->logit, fwd->sfirst, table->bias, B);
      rc = check_launch("fmx_deepfm_stream (k_first_plus_bias)");
    }
    if (rc == FMX_OK)
      rc = mlp_section_deferred_reduce(mlp, loss_kind, fwd->bi, table->kp, fwd->logit, y, B, inv_b, mlp_workspace, nullptr, dz, gbi, table->kp,
                                       grads, opt ? 0.f : lr_mlp, loss_out ? loss_out + s : nullptr, st, &red, who, pair_margin);
    if (rc == FMX_OK && opt) mlp_reduce_set_opt(red, *opt, opt->step + s + 1);  // step s of the call is step t = opt->step + s + 1 of the network
    return rc;
  };
  auto update = [&](int s, const uint32_t *sorted, hipStream_t st) {
    const fmx_hyper_t hs = hyper_at_step(hyper, rule, s);  // ... and step t = hyper->step + s + 1 of the tables (as in stream_run)
    return update_impl(table, &hs, rule, w, sorted, nullptr, fwd->S, dz, fm_term ? dz : nullptr, gbi, B, nullptr, inv_b, nullptr, st, nullptr, 0,
                       fwd->error, &red);
  };
  return pool_loop(table, idx_pool, y_pool, n_pool, B, n_steps, w, fwd->error, static_cast<hipStream_t>(stream), before_update, update);
}

int fmx_deepfm_stream(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_mlp_t *mlp, int32_t loss_kind, int32_t fm_term,
                      const int32_t *idx_pool, const float *y_pool, int32_t n_pool, int32_t B, float inv_b, int32_t n_steps,
                      void *workspace, int64_t workspace_bytes, void *mlp_workspace, const fmx_fwd_out_t *fwd, float *dz, float *gbi,
                      float *grads, float lr_mlp, float *loss_out, fmx_stream_t stream) {
  return deepfm_stream_impl(table, hyper, rule, mlp, loss_kind, fm_term, idx_pool, y_pool, n_pool, B, inv_b, n_steps, workspace, workspace_bytes,
                            mlp_workspace, 0, fwd, dz, gbi, grads, lr_mlp, nullptr, loss_out, stream, "fmx_deepfm_stream");
}

int fmx_deepfm_stream_opt(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_mlp_t *mlp, int32_t loss_kind,
                          int32_t fm_term, const int32_t *idx_pool, const float *y_pool, int32_t n_pool, int32_t B, float inv_b,
                          int32_t n_steps, void *workspace, int64_t workspace_bytes, void *mlp_workspace, int64_t mlp_workspace_bytes,
                          const fmx_fwd_out_t *fwd, float *dz, float *gbi, float *grads, const fmx_mlp_opt_t *opt, float *loss_out,
                          fmx_stream_t stream) {
  if (!opt) return fail(FMX_ERR_ARG, "fmx_deepfm_stream_opt: opt is null");
  return deepfm_stream_impl(table, hyper, rule, mlp, loss_kind, fm_term, idx_pool, y_pool, n_pool, B, inv_b, n_steps, workspace, workspace_bytes,
                            mlp_workspace, mlp_workspace_bytes, fwd, dz, gbi, grads, 0.f, opt, loss_out, stream, "fmx_deepfm_stream_opt");
}

// the pair form of the two streams above: B_pairs pairs are 2 B_pairs rows of the pool (row 2 i the positive, row 2 i + 1 the
// negative), the table forward has no loss, the MLP section evaluates the pair loss (k_mlp_chain<true> / k_mlp_pair_loss), and
// sort, update and the riding reduction are the pointwise stream's on those rows.  The refusals of the fmx_fm_pair_* family come
// first, then deepfm_stream_impl's
int fmx_deepfm_pair_stream(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_mlp_t *mlp, int32_t fm_term,
                           const int32_t *idx_pool, int32_t n_pool, int32_t B_pairs, float margin, float inv_b, int32_t n_steps,
                           void *workspace, int64_t workspace_bytes, void *mlp_workspace, int64_t mlp_workspace_bytes,
                           const fmx_fwd_out_t *fwd, float *dz, float *gbi, float *grads, float lr_mlp, const fmx_mlp_opt_t *opt,
                           float *loss_out, fmx_stream_t stream) {
  const char *who = "fmx_deepfm_pair_stream";
  if (int rc = check_pair_args(table, hyper, idx_pool, B_pairs, "B_pairs", margin, who)) return rc;
  if (int rc = check_sort_geometry(table, pair_rows(B_pairs))) return rc;  // (as fmx_sort_occurrences reports it)
  if (int rc = check_pool_steps(n_pool, n_steps, who)) return rc;
  return named(deepfm_stream_impl(table, hyper, rule, mlp, FMX_LOSS_NONE, fm_term, idx_pool, nullptr, n_pool, 2 * B_pairs, inv_b, n_steps, workspace,
                                  workspace_bytes, mlp_workspace, mlp_workspace_bytes, fwd, dz, gbi, grads, opt ? 0.f : lr_mlp, opt,
                                  loss_out, stream, who, margin),
               who);
}

// The list form of fmx_deepfm_pair_stream: B_lists lists of G rows are B_lists G rows of the pool (row G i the positive of list i,
// then its G - 1 negatives), the table forward has no loss, the MLP section evaluates the list loss (fmx_mlp_list_section's body,
// mlp_list_section_deferred_reduce in fmx_mlp_list.inc: the separate-GEMM form with k_mlp_list_loss at the loss site, never
// k_mlp_chain), and sort and update are the pointwise stream's on those rows -- with the update on list_update_table's copy of
// the table, so that the bias rule runs on the LIST_BIAS_SCRATCH bytes behind the step workspace (fmx_list.inc's header says
// why; fmx_fm_list_step does the same).  The section's reduction RIDES in the table update's launch (k_fm_update_rider), as in
// the streams above.  corr_pool [n_pool, B_lists G] or null rides where the pointwise stream's labels ride (pool_loop's y_pool).
// A function of its own beside deepfm_stream_impl, whose inline checks of the network and opt are repeated here; the refusals of
// the fmx_fm_list_* family come first.
int fmx_deepfm_list_stream(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_mlp_t *mlp, int32_t fm_term,
                           const int32_t *idx_pool, int32_t n_pool, int32_t B_lists, int32_t G, const float *corr_pool, float inv_b,
                           int32_t n_steps, void *workspace, int64_t workspace_bytes, void *mlp_workspace, int64_t mlp_workspace_bytes,
                           const fmx_fwd_out_t *fwd, float *dz, float *gbi, float *grads, float lr_mlp, const fmx_mlp_opt_t *opt,
                           float *loss_out, fmx_stream_t stream) {
  const char *who = "fmx_deepfm_list_stream";
  int32_t B = 0;  // the rows of a step
  if (int rc = check_list_args(table, hyper, idx_pool, B_lists, G, &B, who)) return rc;
  if (int rc = check_sort_geometry(table, B)) return named(rc, who);
  if (int rc = check_pool_steps(n_pool, n_steps, who)) return rc;
  if (!opt && adaptive_rule(rule)) return refuse_adaptive(rule, who);
  if (int rc = check_rule(table, rule)) return named(rc, who);
  if (!mlp || !workspace || !mlp_workspace || !fwd || !fwd->S || !fwd->bi || !fwd->logit || !dz || !gbi || !grads)
    return fail(FMX_ERR_ARG, "%s: null argument (fwd needs S, bi and logit)", who);
  if (fwd->sample_ld != 0) return fail(FMX_ERR_ARG, "%s: dense forward outputs only (sample_ld = 0)", who);
  // NFM: k_first_plus_bias reads bias[0], the bias weight of the weights and the moments layouts
  if (!fm_term && (!fwd->sfirst || (opt ? table->layout == FMX_LAYOUT_FTRL : table->layout != FMX_LAYOUT_WEIGHTS)))
    return fail(FMX_ERR_UNSUPPORTED, "%s: fm_term = 0 (NFM) needs fwd->sfirst and a table in the weights%s layout", who, opt ? " or the moments" : "");
  if (opt) {
    if (int rc = check_adam(hyper, rule, n_steps)) return named(rc, who);
    if (int rc = mlp_opt_check(mlp, B, mlp_workspace, mlp_workspace_bytes, grads, opt, n_steps, who)) return rc;
  } else {  // the size of the network's workspace is checked under either rule
    const int64_t need = fmx_mlp_section_workspace_bytes(mlp, B);
    if (need < 0) return fail(FMX_ERR_UNSUPPORTED, "%s: needs 1 <= layers <= %d, k >= 1, hidden >= 1", who, MLP_BIG_MAX_L);
    if (mlp_workspace_bytes < need)
      return fail(FMX_ERR_SHAPE, "%s: the MLP workspace holds %lld bytes, fmx_mlp_section_workspace_bytes asks for %lld", who,
                  (long long)mlp_workspace_bytes, (long long)need);
  }
  if (mlp->k > table->kp) return fail(FMX_ERR_SHAPE, "%s: the MLP reads k=%d columns of a bi of kp=%d", who, mlp->k, table->kp);
  if (!aligned16(gbi) || !aligned16(dz)) return fail(FMX_ERR_ALIGN, "%s: dz and gbi must be 16-byte aligned", who);
  if (int rc = check_workspace(table, B, workspace, workspace_bytes, who)) return rc;
  const Workspace w = carve(table, B, workspace);
  // the step workspace and LIST_BIAS_SCRATCH bytes behind it (fmx_fm_list_workspace_bytes), as fmx_list.inc checks it
  if (workspace_bytes < (int64_t)w.bytes + LIST_BIAS_SCRATCH)
    return fail(FMX_ERR_SHAPE, "%s: workspace of %lld bytes, %lld needed: the step's and %lld bytes behind it (fmx_fm_list_workspace_bytes)", who,
                (long long)workspace_bytes, (long long)((int64_t)w.bytes + LIST_BIAS_SCRATCH), (long long)LIST_BIAS_SCRATCH);
  const fmx_table_t tu = list_update_table(table, workspace, w.bytes);
  MlpReduceArgs red;  // the section's last launch, set up by before_update, rides inside the table update's (k_fm_update_rider)
  auto before_update = [&](int s, const int32_t *idx, const float *corr, hipStream_t st) -> int {
    int rc = forward_impl(table, hyper, idx, nullptr, nullptr, B, FMX_LOSS_NONE, inv_b, fwd, st);
    if (rc == FMX_OK && !fm_term) {  // NFM: the network's input logit is first-order + bias; the FM logit's buffer holds it
      hipLaunchKernelGGL(k_first_plus_bias, dim3((B + 255) / 256), dim3(256), 0, st, fwd->logit, fwd->sfirst, table->bias, B);
      rc = check_launch("fmx_deepfm_list_stream (k_first_plus_bias)");
    }
    if (rc == FMX_OK)
      rc = mlp_list_section_deferred_reduce(mlp, fwd->bi, table->kp, fwd->logit, corr, B_lists, G, inv_b, mlp_workspace, mlp_workspace_bytes,
                                            nullptr, dz, gbi, table->kp, grads, opt ? 0.f : lr_mlp, loss_out ? loss_out + s : nullptr, st,
                                            &red, who);
    if (rc == FMX_OK && opt) mlp_reduce_set_opt(red, *opt, opt->step + s + 1);  // step s of the call is step t = opt->step + s + 1 of the network
    return rc;
  };
  auto update = [&](int s, const uint32_t *sorted, hipStream_t st) {
    const fmx_hyper_t hs = hyper_at_step(hyper, rule, s);  // ... and step t = hyper->step + s + 1 of the tables
    return update_impl(&tu, &hs, rule, w, sorted, nullptr, fwd->S, dz, fm_term ? dz : nullptr, gbi, B, nullptr, inv_b, nullptr, st, nullptr, 0,
                       fwd->error, &red);
  };
  return pool_loop(table, idx_pool, corr_pool, n_pool, B, n_steps, w, fwd->error, static_cast<hipStream_t>(stream), before_update, update);
}

// ---- the field-owner step with the library's own communicator (fmx_comm.hip) ----
static int owner_geometry(const Comm *c, const fmx_table_t *table, int32_t B, int32_t slot, int &GB, const char *who) {
  if (!c) return fail(FMX_ERR_ARG, "%s: null communicator", who);
  if (int rc = check_table(table)) return rc;
  if (B < 1) return fail(FMX_ERR_ARG, "%s: B must be >= 1", who);
  if (slot < 0 || slot >= FMX_COMM_SLOTS) return fail(FMX_ERR_ARG, "%s: slot %d outside [0, %d)", who, slot, FMX_COMM_SLOTS);
  if ((int64_t)B * c->world > MAX_SORT_WIDTH) return fail(FMX_ERR_UNSUPPORTED, "%s: %d ranks x %d samples exceed one exact step (%d)", who, c->world, B, MAX_SORT_WIDTH);
  GB = B * c->world;
  return check_sort_geometry(table, GB);
}

int fmx_owner_prefetch(fmx_comm_t *comm, const fmx_table_t *table, const int32_t *idx_local, int32_t B, int32_t slot, int32_t *idx_all,
                       void *workspace, int64_t workspace_bytes, int32_t *error, fmx_stream_t stream) {
  Comm *c = reinterpret_cast<Comm *>(comm);
  int GB = 0;
  if (int rc = owner_geometry(c, table, B, slot, GB, "fmx_owner_prefetch")) return rc;
  if (!idx_local || (!idx_all && !(c->world == 1 && !c->force))) return fail(FMX_ERR_ARG, "fmx_owner_prefetch: null argument");
  if (int rc = check_workspace(table, GB, workspace, workspace_bytes, "fmx_owner_prefetch")) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream), pf = c->pf_stream;
  // behind whatever wrote idx_local on the caller's stream, and behind the step that last used this slot's buffers
  (void)hipEventRecord(c->fork, st);
  (void)hipStreamWaitEvent(pf, c->fork, 0);
  if (c->used[slot]) (void)hipStreamWaitEvent(pf, c->free_[slot], 0);
  const size_t words = (size_t)B * n_cols(table);
  // one rank, nothing forced: no copy -- the lists are sorted from idx_local itself, which the caller then also hands to
  // fmx_owner_step as idx_all (and keeps unchanged until that step has run)
  const bool alone = c->world == 1 && !c->force;
  if (!alone)
    if (int rc = comm_all_gather(c, 1, idx_local, idx_all, words, pf)) return rc;
  const Workspace w = carve(table, GB, workspace);
  if (int rc = sort_impl(table, alone ? idx_local : idx_all, GB, w.sorted, w.runs, error, pf)) return rc;
  (void)hipEventRecord(c->ready[slot], pf);
  return FMX_OK;
}

int fmx_owner_step(fmx_comm_t *comm, const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, int32_t loss_kind,
                   const int32_t *idx_all, const float *y_local, int32_t B, int32_t slot, void *workspace, int64_t workspace_bytes,
                   const fmx_owner_bufs_t *bufs, float *loss_out, int32_t *error, fmx_stream_t stream) {
  Comm *c = reinterpret_cast<Comm *>(comm);
  int GB = 0;
  if (adaptive_rule(rule)) return refuse_adaptive(rule, "fmx_owner_step");
  if (int rc = owner_geometry(c, table, B, slot, GB, "fmx_owner_step")) return rc;
  if (int rc = check_rule(table, rule)) return rc;
  if (!hyper || !idx_all || !y_local || !bufs || !bufs->parts_send || !bufs->parts_recv || !bufs->rec_local || !bufs->rec_all)
    return fail(FMX_ERR_ARG, "fmx_owner_step: null argument");
  if (loss_kind != FMX_LOSS_BCE_LOGITS && loss_kind != FMX_LOSS_BCE_SIGMOID) return fail(FMX_ERR_ARG, "a step needs a loss");
  if (!aligned16(bufs->parts_send) || !aligned16(bufs->parts_recv) || !aligned16(bufs->rec_local) || !aligned16(bufs->rec_all))
    return fail(FMX_ERR_ALIGN, "fmx_owner_step: the record buffers must be 16-byte aligned");
  if (int rc = check_workspace(table, GB, workspace, workspace_bytes, "fmx_owner_step")) return rc;
  const bool alone = c->world == 1 && !c->force;
  if (alone ? false : (bufs->parts_recv == bufs->parts_send || bufs->rec_all == bufs->rec_local))
    return fail(FMX_ERR_ARG, "fmx_owner_step: with an exchange the receive buffers must be buffers of their own");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int kp = table->kp, rec_in = 2 * kp + 4, rec_out = kp + 4;
  const float inv_b = 1.0f / (float)GB;
  (void)hipStreamWaitEvent(st, c->ready[slot], 0);  // the slot's gather + sort
  // 1. every owned block's sub-tree for every sample of the global batch, destination-major
  if (int rc = part_impl(table, idx_all, nullptr, GB, c->n_blocks, c->block_count[c->rank], B, bufs->parts_send, error, st)) return rc;
  // 2. the records of this rank's samples from every block
  if (int rc = comm_exchange_blocks(c, bufs->parts_send, bufs->parts_recv, (size_t)B * rec_in, st)) return rc;
  // 3. the rest of the tree, bias, loss, dlogit -> one (S, dlogit, loss) record per local sample
  fmx_fwd_out_t out;
  memset(&out, 0, sizeof(out));
  out.S = bufs->rec_local;
  out.dz = bufs->rec_local + kp;
  out.loss = bufs->rec_local + kp + 1;
  out.sample_ld = rec_out;
  out.error = error;
  if (int rc = fmx_fm_forward_finish(hyper, table->bias, table->layout, kp, bufs->parts_recv, (int64_t)B * rec_in, c->n_blocks, y_local, B,
                                     loss_kind, inv_b, &out, stream))
    return rc;
  // 4. everybody's records
  if (int rc = comm_all_gather(c, 0, bufs->rec_local, bufs->rec_all, (size_t)B * rec_out, st)) return rc;
  // 5. the owned rows (and the replicated bias, identically everywhere)
  const Workspace w = carve(table, GB, workspace);
  const float *rec = bufs->rec_all;
  if (int rc = update_impl(table, hyper, rule, w, w.sorted, nullptr, rec, rec + kp, rec + kp, nullptr, GB, rec + kp + 1, inv_b, loss_out, st,
                           nullptr, rec_out, error))
    return rc;
  (void)hipEventRecord(c->free_[slot], st);
  c->used[slot] = true;
  return FMX_OK;
}

int fmx_fm_step(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, int32_t loss_kind,
                const int32_t *idx, const float *xv, const float *y, int32_t B, float inv_b, void *workspace, int64_t workspace_bytes,
                const fmx_fwd_out_t *fwd, float *loss_out, fmx_stream_t stream) {
  if (int rc = check_step_args(table, hyper, rule, loss_kind, B, workspace, fwd)) return rc;
  if (!idx || !y) return fail(FMX_ERR_ARG, "fmx_fm_step: idx and y are required");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (int rc = check_workspace(table, B, workspace, workspace_bytes, "fmx_fm_step")) return rc;
  return step_run(table, table, hyper, rule, idx, xv, y, B, inv_b, carve(table, B, workspace), fwd, loss_out, st,
                  point_forward(table, hyper, B, loss_kind, inv_b, fwd));
}

int fmx_fm_stream(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, int32_t loss_kind,
                  const int32_t *idx_pool, const float *y_pool, int32_t n_pool, int32_t B, float inv_b,
                  int32_t n_steps, void *workspace, int64_t workspace_bytes, const fmx_fwd_out_t *fwd, float *loss_out, float *kernel_ms,
                  fmx_stream_t stream) {
  if (int rc = check_step_args(table, hyper, rule, loss_kind, B, workspace, fwd)) return rc;
  if (!idx_pool || !y_pool || n_pool < 1 || n_steps < 0) return fail(FMX_ERR_ARG, "fmx_fm_stream: bad pool / step count");
  if (int rc = check_adam(hyper, rule, n_steps)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (int rc = check_workspace(table, B, workspace, workspace_bytes, "fmx_fm_stream")) return rc;
  const Workspace w = carve(table, B, workspace);
  if (!kernel_ms)  // production path
    return stream_run(table, table, hyper, rule, idx_pool, y_pool, n_pool, B, inv_b, n_steps, w, fwd, loss_out, st,
                      point_forward(table, hyper, B, loss_kind, inv_b, fwd));

  // measuring mode: everything on `stream`.  An event pair costs several microseconds of its own on this stack (slot 3
  // measures exactly that: two records with nothing between), so launches are timed in groups of up to 8 steps between
  // two events and the pair's own cost is subtracted: ONE sort launch for the group's batches (as in the production
  // loop), then the group's forwards back to back, then its updates back to back -- every launch on a DIFFERENT batch of
  // the pool (its own sorted list, its own S / dz / loss), so the rows come from HBM / MALL as they do in production
  // instead of from an L2 warmed by the previous launch of the same batch.  The forwards of a group all read the table
  // before the group's updates, so this pass is a measurement, not the online algorithm.
  const int REP = 8, n_ev = 5;
  const int n_groups = (n_steps + REP - 1) / REP;
  const size_t F = (size_t)n_cols(table);
  const size_t region = align_up((size_t)B * table->kp + 2 * (size_t)B, 64);  // floats: S | dz | loss of one batch
  float *tmp = nullptr;
  hipEvent_t *ev = nullptr;
  int rc = FMX_OK;
  {
    const Detour detour(st == nullptr ? side_for_current_device() : nullptr, st);  // off the legacy stream, as in pool_loop
    st = detour.st;
    if (n_groups > 0 && hipMalloc(&tmp, REP * region * sizeof(float)) != hipSuccess)
      return fail(FMX_ERR_LAUNCH, "hipMalloc (measuring mode)");
    ev = new hipEvent_t[(size_t)n_groups * n_ev];
    for (int i = 0; i < n_groups * n_ev; ++i) (void)hipEventCreate(&ev[i]);
    for (int g = 0; g < n_groups && rc == FMX_OK; ++g) {
      const int first = g * REP, n = (n_steps - first) < REP ? (n_steps - first) : REP;
      hipEvent_t *e = ev + (size_t)g * n_ev;
      (void)hipEventRecord(e[0], st);
      rc = sort_pool(table, idx_pool, n_pool, B, first, n, w, w.sorted, fwd->error, st);
      (void)hipEventRecord(e[1], st);
      for (int r = 0; r < n && rc == FMX_OK; ++r) {
        const int j = (first + r) % n_pool;
        fmx_fwd_out_t fr = *fwd;
        fr.S = tmp + (size_t)r * region;
        fr.dz = fr.S + (size_t)B * table->kp;
        fr.loss = fr.dz + B;
        fr.sample_ld = 0;
        rc = forward_impl(table, hyper, idx_pool + (size_t)j * B * F, nullptr, y_pool + (size_t)j * B, B, loss_kind, inv_b, &fr, st);
      }
      (void)hipEventRecord(e[2], st);
      for (int r = 0; r < n && rc == FMX_OK; ++r) {
        const float *S = tmp + (size_t)r * region, *dz = S + (size_t)B * table->kp;
        const fmx_hyper_t hs = hyper_at_step(hyper, rule, first + r);
        rc = update_impl(table, &hs, rule, w, w.sorted + (size_t)r * w.sorted_stride, nullptr, S, dz, dz, nullptr, B, dz + B, inv_b,
                         loss_out ? loss_out + first + r : nullptr, st, nullptr, 0, fwd->error);
      }
      (void)hipEventRecord(e[3], st);
      (void)hipEventRecord(e[4], st);
    }
    (void)hipStreamSynchronize(st);
  }
  for (int k = 0; k < 4; ++k) kernel_ms[k] = 0.f;
  if (rc == FMX_OK && n_groups > 0) {
    double t_sort = 0, t_fwd = 0, t_upd = 0, t_pair = 0;
    for (int g = 0; g < n_groups; ++g) {
      hipEvent_t *e = ev + (size_t)g * n_ev;
      float pair = 0.f, ms[3] = {0.f, 0.f, 0.f};
      (void)hipEventElapsedTime(&pair, e[3], e[4]);
      for (int k = 0; k < 3; ++k) (void)hipEventElapsedTime(&ms[k], e[k], e[k + 1]);
      t_pair += pair;
      t_sort += fmaxf(ms[0] - pair, 0.f);
      t_fwd += fmaxf(ms[1] - pair, 0.f);
      t_upd += fmaxf(ms[2] - pair, 0.f);
    }
    // returned as (average per launch) x n_steps, so that dividing by n_steps gives the per-launch averages
    kernel_ms[0] = (float)(t_sort / n_groups * n_steps);  // one launch per group of up to 8 batches, as in production
    kernel_ms[1] = (float)t_fwd;                           // n_steps forward launches in all
    kernel_ms[2] = (float)t_upd;
    kernel_ms[3] = (float)(t_pair / n_groups * n_steps);
  }
  for (int i = 0; i < n_groups * n_ev; ++i) (void)hipEventDestroy(ev[i]);
  delete[] ev;
  if (tmp) (void)hipFree(tmp);
  return rc;
}

// ---- the pairwise-ranking loss (fmx_pair.inc) ----
int fmx_fm_pair_forward(const fmx_table_t *table, const fmx_hyper_t *hyper, const int32_t *idx, const float *xv, int32_t B_pairs,
                        float margin, float inv_b, const fmx_fwd_out_t *out, fmx_stream_t stream) {
  return pair_forward_call(table, hyper, idx, xv, B_pairs, margin, inv_b, out, static_cast<hipStream_t>(stream));
}

int fmx_fm_pair_step(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const int32_t *idx, const float *xv,
                     int32_t B_pairs, float margin, float inv_b, void *workspace, int64_t workspace_bytes, const fmx_fwd_out_t *fwd,
                     float *loss_out, fmx_stream_t stream) {
  return pair_step_call(table, hyper, rule, idx, xv, B_pairs, margin, inv_b, workspace, workspace_bytes, fwd, loss_out,
                        static_cast<hipStream_t>(stream));
}

int fmx_fm_pair_stream(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const int32_t *idx_pool, int32_t n_pool,
                       int32_t B_pairs, float margin, float inv_b, int32_t n_steps, void *workspace, int64_t workspace_bytes,
                       const fmx_fwd_out_t *fwd, float *loss_out, fmx_stream_t stream) {
  return pair_stream_call(table, hyper, rule, idx_pool, n_pool, B_pairs, margin, inv_b, n_steps, workspace, workspace_bytes, fwd,
                          loss_out, static_cast<hipStream_t>(stream));
}

// ---- the listwise (sampled-softmax) loss (fmx_list.inc) ----
int64_t fmx_fm_list_workspace_bytes(const fmx_table_t *table, int32_t B_lists, int32_t G) {
  if (check_table(table) != FMX_OK) return FMX_ERR_ARG;
  if (B_lists < 1 || G < 2 || G > LIST_MAX_G || (int64_t)B_lists * G > INT32_MAX)
    return fail(FMX_ERR_ARG, "fmx_fm_list_workspace_bytes: B_lists >= 1, 2 <= G <= %d and B_lists * G within int32", LIST_MAX_G);
  return list_workspace_bytes(table, B_lists * G);
}

int fmx_fm_list_forward(const fmx_table_t *table, const fmx_hyper_t *hyper, const int32_t *idx, const float *xv, int32_t B_lists,
                        int32_t G, float inv_b, const fmx_fwd_out_t *out, fmx_stream_t stream) {
  return list_forward_call(table, hyper, idx, xv, nullptr, B_lists, G, inv_b, out, static_cast<hipStream_t>(stream), "fmx_fm_list_forward");
}

int fmx_fm_list_forward_q(const fmx_table_t *table, const fmx_hyper_t *hyper, const int32_t *idx, const float *xv, const float *corr,
                          int32_t B_lists, int32_t G, float inv_b, const fmx_fwd_out_t *out, fmx_stream_t stream) {
  if (!corr) return fail(FMX_ERR_ARG, "fmx_fm_list_forward_q: corr is null");
  return list_forward_call(table, hyper, idx, xv, corr, B_lists, G, inv_b, out, static_cast<hipStream_t>(stream), "fmx_fm_list_forward_q");
}

int fmx_fm_list_step(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const int32_t *idx, const float *xv,
                     int32_t B_lists, int32_t G, float inv_b, void *workspace, int64_t workspace_bytes, const fmx_fwd_out_t *fwd,
                     float *loss_out, fmx_stream_t stream) {
  return list_step_call(table, hyper, rule, idx, xv, nullptr, B_lists, G, inv_b, workspace, workspace_bytes, fwd, loss_out,
                        static_cast<hipStream_t>(stream), "fmx_fm_list_step");
}

int fmx_fm_list_step_q(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const int32_t *idx, const float *xv,
                       const float *corr, int32_t B_lists, int32_t G, float inv_b, void *workspace, int64_t workspace_bytes,
                       const fmx_fwd_out_t *fwd, float *loss_out, fmx_stream_t stream) {
  if (!corr) return fail(FMX_ERR_ARG, "fmx_fm_list_step_q: corr is null");
  return list_step_call(table, hyper, rule, idx, xv, corr, B_lists, G, inv_b, workspace, workspace_bytes, fwd, loss_out,
                        static_cast<hipStream_t>(stream), "fmx_fm_list_step_q");
}

int fmx_fm_list_stream(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const int32_t *idx_pool, int32_t n_pool,
                       int32_t B_lists, int32_t G, float inv_b, int32_t n_steps, void *workspace, int64_t workspace_bytes,
                       const fmx_fwd_out_t *fwd, float *loss_out, fmx_stream_t stream) {
  return list_stream_call(table, hyper, rule, idx_pool, nullptr, n_pool, B_lists, G, inv_b, n_steps, workspace, workspace_bytes, fwd,
                          loss_out, static_cast<hipStream_t>(stream), "fmx_fm_list_stream");
}

int fmx_fm_list_stream_q(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const int32_t *idx_pool, const float *corr_pool,
                         int32_t n_pool, int32_t B_lists, int32_t G, float inv_b, int32_t n_steps, void *workspace,
                         int64_t workspace_bytes, const fmx_fwd_out_t *fwd, float *loss_out, fmx_stream_t stream) {
  if (!corr_pool) return fail(FMX_ERR_ARG, "fmx_fm_list_stream_q: corr_pool is null");
  return list_stream_call(table, hyper, rule, idx_pool, corr_pool, n_pool, B_lists, G, inv_b, n_steps, workspace, workspace_bytes, fwd,
                          loss_out, static_cast<hipStream_t>(stream), "fmx_fm_list_stream_q");
}

int fmx_fm_list_online_run(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const int32_t *idx, const float *xv, int32_t N,
                           int32_t G, uint8_t *rank_out, float *logit_out, float *loss_out, int32_t *error, fmx_stream_t stream) {
  return list_online_call(table, hyper, rule, idx, xv, N, G, rank_out, logit_out, loss_out, error, static_cast<hipStream_t>(stream));
}

int fmx_gather_read(const void *buf, int64_t bytes, int32_t row_bytes, int64_t n_rows_read, uint32_t seed, float *sink, fmx_stream_t stream) {
  if (!buf || !sink || bytes < 128 || n_rows_read < 1) return fail(FMX_ERR_ARG, "fmx_gather_read: bad buffer / count");
  if (row_bytes != 64 && row_bytes != 128) return fail(FMX_ERR_ARG, "fmx_gather_read: rows of 64 or 128 bytes");
  if (!aligned16(buf)) return fail(FMX_ERR_ALIGN, "fmx_gather_read: buffer must be 16-byte aligned");
  const int lpr = row_bytes / 16;
  const uint64_t n_rows = (uint64_t)bytes / (uint64_t)row_bytes;
  const int64_t threads = n_rows_read * lpr;
  const dim3 grid((unsigned)((threads + 255) / 256)), block(256);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (lpr == 4) hipLaunchKernelGGL((k_gather_read<4>), grid, block, 0, st, static_cast<const float4 *>(buf), n_rows, n_rows_read, seed, sink);
  else hipLaunchKernelGGL((k_gather_read<8>), grid, block, 0, st, static_cast<const float4 *>(buf), n_rows, n_rows_read, seed, sink);
  return check_launch("k_gather_read");
}

#ifdef FMX_STAMPS
int fmx_debug_forward_stamps(unsigned long long *host_out) {  // [8192][6]; diagnostic build only (not in include/fmx.h)
  return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_fwd_stamps), sizeof(unsigned long long) * 8192 * 6) == hipSuccess ? FMX_OK : FMX_ERR_LAUNCH;
}
#endif

int fmx_stream_read(const void *buf, int64_t bytes, float *sink, fmx_stream_t stream) {
  if (!buf || !sink || bytes < 16 || bytes % 16) return fail(FMX_ERR_ARG, "fmx_stream_read: bad buffer");
  if (!aligned16(buf)) return fail(FMX_ERR_ALIGN, "fmx_stream_read: buffer must be 16-byte aligned");
  hipLaunchKernelGGL(k_stream_read, dim3(256 * 8), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const float4 *>(buf), bytes / 16, sink);
  return check_launch("k_stream_read");
}

}  // extern "C"
