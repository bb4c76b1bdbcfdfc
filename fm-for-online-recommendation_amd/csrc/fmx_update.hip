// fmx_update.hip -- the table update: k_fm_update (one wavefront per tile of 64 sorted occurrences, ONE fused read-modify-write per
// touched row; runs that cross tiles are handed over inside the launch), its forms from explicit per-occurrence gradients
// (k_fm_update_occ) and with the MLP's gradient reduction riding along (k_fm_update_rider), and k_fm_fixup for the launches without
// the hand-off.  The other units reach these through update_impl / update_occ_impl (fmx_host.h) alone.

#include "fmx_host.h"

namespace {

// Agent-scope relaxed atomic accesses compile to `global_store/load ... sc1` (write-through / L1-bypassing): the form
// the in-launch hand-off of partial records uses on BOTH sides (MI355X_MICROARCH.md, "Valid forms": every store and every
// load of the handed-off bytes sc1, the storing wave's s_waitcnt vmcnt(0) before its flag store).
__device__ __forceinline__ void st_sc1(float *p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// 16-byte store: one instruction per lane (`global_store_dwordx4 ... sc1`; scalar sc1 stores are one fabric write each).
typedef float v4f __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void st_sc1_4(float *p, float4 v) {
  const v4f x = {v.x, v.y, v.z, v.w};
  asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(x) : "memory");
}
__device__ __forceinline__ void store_part_sc1(float *rec, int q, int kp, float4 cV, float4 cA, float cw) {
  st_sc1_4(rec + 4 * q, cV);
  st_sc1_4(rec + kp + 4 * q, cA);
  if (q == 0) st_sc1(rec + 2 * kp, cw);
}

// ------------------------------------------------------------------------------------------------------------
// k_fm_update
// ------------------------------------------------------------------------------------------------------------
struct UpdArgs {
  float *rows;
  const int64_t *foff;
  float *bias;
  const uint32_t *sorted;
  float *parts;   // [F * tiles, 2 (lead, trail), REC] partial sums of runs that cross a tile boundary
  int32_t *meta;  // [F * tiles, 2] (lead_state, trail_state)
  const float *xv;
  const float *S;
  const float *dz_first;
  const float *dz_bi;
  const float *gbi;
  const float *loss_b;
  float *loss_out;
  int32_t *step_counter;  // null: loss_out[0]; else loss_out[*step_counter], then *step_counter += 1
  fmx_hyper_t h;
  int32_t B, F, Bp, bbits, kp, stride, zoff;
  int32_t ldS, ld1;  // floats between consecutive samples in S and in dz_first / dz_bi / loss_b (kp and 1 when dense)
  int32_t ldG;       // ... and in gbi (kp when dense)
  const int32_t *cols;  // sort field -> field, or null; fcols: field -> column of xv, or null; Fx: columns of xv
  const int32_t *fcols;
  int32_t Fx;
  float *red;        // [16][4] partial (sum dlogit, sum loss, launch sequence, -) of the batch slices (B > RED_SLICE)
  uint32_t seq;      // launch sequence number tagging the tile meta words (INL) and the slice partials of this launch
  int32_t *error;    // INL: set to 2 if a hand-off wait ran into its bound
  float inv_b;
  // the dispatch order of the tiles (update_body): slot i of the grid's tile waves works on sort field order[i], one byte each,
  // by value -- a wave reads its byte with one scalar load of its own kernel arguments, not from memory behind a pointer.
  // ordered == 0: index order (slot i = field i)
  int32_t ordered;
  uint32_t order[UPD_ORDER_MAX / 4];
};

// tile meta states
constexpr int LEAD_NONE = 0, LEAD_CLOSES = 1, LEAD_THROUGH = 2;

// The bias gradient (sum of dlogit over the batch) and the mean loss.  The batch is cut into slices of RED_SLICE samples, one
// workgroup each (the first workgroups of the launch): with the samples' (S, dlogit, loss) records gathered from G ranks the
// values lie 80 bytes apart, one 64-byte request each, and ONE workgroup walking 2 x 32,768 of them was the longest path of
// the launch by far (47-53 us of the update at 8 x 4,096 samples against 13 at 4,096).  One slice (B <= RED_SLICE): the sum
// and the update in place, as before.  Several: every slice's workgroup leaves (sum dlogit, sum loss, launch sequence) as ONE
// 16-byte write-through granule; the first workgroup polls the others' granules until they carry this launch's sequence number
// (data and tag in one granule: no ordering needed; they belong to workgroups dispatched right behind it, which wait on
// nothing), adds the partials in slice order and applies the update -- or, without the in-launch hand-off, k_fm_fixup's
// last workgroup does that.  The order of the additions depends on the batch size alone: every mode gives the same bits.
constexpr int RED_SLICE = 4096;
__host__ __device__ inline int red_slices(int B) { return (B + RED_SLICE - 1) / RED_SLICE; }

template <int LAYOUT, int RULE>
__device__ __forceinline__ void apply_bias_and_loss(const UpdArgs &a, float db, float ls) {
  constexpr bool MOM = LAYOUT == FMX_LAYOUT_MOMENTS;
  float b0 = a.bias[0], b1 = LAYOUT != FMX_LAYOUT_WEIGHTS ? a.bias[1] : 0.f, b2 = MOM ? a.bias[2] : 0.f;
  bias_step<LAYOUT, RULE>(b0, b1, b2, db, a.h);
  st4(a.bias, b0);
  if (LAYOUT == FMX_LAYOUT_FTRL || (MOM && RULE == FMX_RULE_ADAM)) st4(a.bias + 1, b1);
  if (MOM) st4(a.bias + 2, b2);
  if (a.loss_b && a.loss_out) {
    int i = 0;
    if (a.step_counter) {
      i = *a.step_counter;
      *a.step_counter = i + 1;
    }
    a.loss_out[i] = ls * a.inv_b;
  }
}

// the partials of all R slices added in slice order (thread 0 of the calling workgroup applies them)
template <int LAYOUT, int RULE>
__device__ void finish_bias_and_loss(const UpdArgs &a, int R, bool poll) {
  __shared__ float part[2 * 16];
  const int t = threadIdx.x;
  bool failed = false;
  if (t < R) {
    const v4f *src = reinterpret_cast<const v4f *>(a.red) + t;
    v4f g = {0.f, 0.f, 0.f, 0.f};
    if (poll) {
      for (int spin = 0;; ++spin) {
        asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=v"(g) : "v"(src) : "memory");
        if (__float_as_uint(g.z) == a.seq) break;
        if (spin >= (1 << 20)) {
          failed = true;
          break;
        }
        __builtin_amdgcn_s_sleep(1);
      }
    } else {
      g = *src;
    }
    part[2 * t] = g.x;
    part[2 * t + 1] = g.y;
  }
  if (failed && a.error) *a.error = 2;
  __syncthreads();
  if (t == 0) {
    float db = 0.f, ls = 0.f;
    for (int r = 0; r < R; ++r) {
      db += part[2 * r];
      ls += part[2 * r + 1];
    }
    apply_bias_and_loss<LAYOUT, RULE>(a, db, ls);
  }
}

template <int LAYOUT, int RULE, bool INL>
__device__ void bias_and_loss(const UpdArgs &a, int r) {
  __shared__ float sm[256];
  const int R = red_slices(a.B);
  const int first = r * RED_SLICE, n = (a.B - first) < RED_SLICE ? (a.B - first) : RED_SLICE;
  const float db = block_sum(a.dz_first + (size_t)first * a.ld1, n, a.ld1, sm);
  float ls = 0.f;
  if (a.loss_b && a.loss_out) ls = block_sum(a.loss_b + (size_t)first * a.ld1, n, a.ld1, sm);
  if (R == 1) {
    if (threadIdx.x == 0) apply_bias_and_loss<LAYOUT, RULE>(a, db, ls);
    return;
  }
  if (threadIdx.x == 0) st_sc1_4(a.red + 4 * r, float4{db, ls, __uint_as_float(a.seq), 0.f});
  if (INL && r == 0) finish_bias_and_loss<LAYOUT, RULE>(a, R, true);
}

// partial-sum record: [cV (kp) | cA (kp) | cw, pad3]
__device__ __forceinline__ void store_part(float *rec, int q, int kp, float4 cV, float4 cA, float cw) {
  *reinterpret_cast<float4 *>(rec + 4 * q) = cV;
  *reinterpret_cast<float4 *>(rec + kp + 4 * q) = cA;
  if (q == 0) rec[2 * kp] = cw;
}

// run sums carried per occurrence: cV = sum x G S (vector), cA = sum x^2 G (a scalar when G is one: pure FM), cw
template <bool VEC> struct CoefA;
template <> struct CoefA<true> {
  float4 v;
  __device__ __forceinline__ void zero() { v = splat(0.f); }
  __device__ __forceinline__ void add(const CoefA &o) { v = v + o.v; }
  __device__ __forceinline__ float4 vec() const { return v; }
  __device__ __forceinline__ CoefA up(int d) const { return {shfl_up4(v, d)}; }
};
template <> struct CoefA<false> {
  float v;
  __device__ __forceinline__ void zero() { v = 0.f; }
  __device__ __forceinline__ void add(const CoefA &o) { v += o.v; }
  __device__ __forceinline__ float4 vec() const { return splat(v); }
  __device__ __forceinline__ CoefA up(int d) const { return {__shfl_up(v, d)}; }
};

#ifdef FMX_STAMPS  // diagnostic build (tools/update_stamps.sh): s_memrealtime (100 MHz) of every tile wave of the LAST k_fm_update launch
__device__ unsigned long long g_upd_stamps[8192 * 6];
#define FMX_STAMP(slot_, dep_)                                                                                      \
  do {                                                                                                              \
    unsigned long long t_;                                                                                          \
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) : "v"(dep_) : "memory");                      \
    if (lane == 0 && gt < 8192) g_upd_stamps[(size_t)gt * 6 + (slot_)] = t_;                                         \
  } while (0)
#else
#define FMX_STAMP(slot_, dep_) do {} while (0)
#endif

// One wave per tile of 64 sorted occurrences of one field.  Lane group s (LPR lanes; lane q owns coordinates 4q..4q+3)
// walks EPG = 64 / SLOTS CONSECUTIVE occurrences sequentially, so duplicates inside a group are summed in registers;
// one segmented scan over the SLOTS groups (log2(SLOTS) steps of wave shuffles) carries the sums of runs that span
// groups.  At the tail of a run: the row update when the run began in this tile, a partial record otherwise.
// OCC (fmx_fm_update_occ): the occurrence's gradient is given explicitly -- cV adds E[b, field] (a.gbi, a.ldG floats per
// sample, kp per field; x already applied), cA = 0 -- instead of x (S_b - x V) G_b; everything else is the same code.
template <int LPR, int LAYOUT, int RULE, bool HAS_GBI, bool INL, bool OCC = false>
__device__ __forceinline__ void update_body(const UpdArgs &a, const int blk) {
  constexpr int SLOTS = WAVE / LPR;  // lane groups
  constexpr int EPG = LPR;           // consecutive occurrences per group
  constexpr int REC = 2 * LPR * 4 + 4;
  constexpr bool PREFETCH_ROWS = EPG <= 4;
  using CA = CoefA<HAS_GBI>;
  const int n_red = red_slices(a.B);
  if (blk < n_red) {  // the first blocks (dispatched first) own the bias and the loss reduction, one slice of the batch each
    bias_and_loss<LAYOUT, RULE, INL>(a, blk);
    return;
  }
  const int lane = threadIdx.x & 63;
  const int slot = lane / LPR, q = lane % LPR;
  const int kp = LPR * 4;
  const int tiles_per_field = a.Bp >> 6;
  // The wave's DISPATCH SLOT d chooses its work; the STORAGE index gt = f * tiles_per_field + t (parts, meta, flag words:
  // k_fm_fixup's and the records' addressing) follows from the work.  Slot i of the fields belongs to sort field order[i] (the
  // host's permutation: fields in ascending row count by default, update_order), tile t of a field stays tile t.  The small
  // fields' tiles -- chains of dependent round trips with almost no bytes -- then have their requests in ahead of the large
  // fields' burst of row lines, and the burst's own tail is shorter for it ("r6": the launch's last
  // large-field combiner 8.5 - 9.1 -> 8.1 - 8.4 us; descending order: +0.7 us per step).  Nothing else depends on the slot:
  // the order is invisible in every result, and a stale or missing one costs time only.
  const int d = (blk - n_red) * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform: scalar
  if (d >= a.F * tiles_per_field) return;
  const int tshift = a.bbits - 6;  // tiles_per_field = Bp / 64 = 1 << tshift
  int f = d >> tshift;
  const int t = d & (tiles_per_field - 1);
  if (a.ordered) {
    // The byte comes through the kernel-argument segment pointer (UpdArgs is the first argument of every kernel of this body),
    // NOT as a.order[...]: one variable index into `a` and the compiler gives up loading the arguments in one burst at the top
    // of the kernel -- it then fetches each one where it is used, 64 scalar loads with a wait each on the wave's critical path
    // (measured: +0.45 us per launch under every order).
    typedef const __attribute__((address_space(4))) uint32_t karg_u32;  // the constant address space: a scalar load
    karg_u32 *ka = (karg_u32 *)__builtin_amdgcn_kernarg_segment_ptr();
    f = (int)((ka[offsetof(UpdArgs, order) / 4 + (f >> 2)] >> ((f & 3) * 8)) & 0xFFu);
  }
  const int gt = f * tiles_per_field + t;
  const int base = t << 6;
  const uint32_t *sf = a.sorted + (size_t)f * a.Bp;
  const int bbits = a.bbits;
  const uint32_t bmask = (1u << bbits) - 1u;
  const int e0 = base + slot * EPG;
  FMX_STAMP(0, lane);

  uint32_t c[EPG];
  if constexpr (EPG % 4 == 0) {  // 16-byte loads (e0 is a multiple of EPG)
#pragma unroll
    for (int j = 0; j < EPG; j += 4) {
      const uint4 t = *reinterpret_cast<const uint4 *>(sf + e0 + j);
      c[j] = t.x;
      c[j + 1] = t.y;
      c[j + 2] = t.z;
      c[j + 3] = t.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < EPG; ++j) c[j] = sf[e0 + j];
  }
  const uint32_t kprev = (e0 == 0 ? SENT : sf[e0 - 1]) >> bbits;
  const uint32_t knext = (e0 + EPG < a.Bp ? sf[e0 + EPG] : SENT) >> bbits;
  const uint32_t tile_prevkey = (base == 0 ? SENT : sf[base - 1]) >> bbits;
  const size_t row0 = (size_t)a.foff[f];
  float *part = a.parts + (size_t)gt * 2 * REC;

  uint32_t k[EPG];
  bool val[EPG], tail[EPG];
#pragma unroll
  for (int j = 0; j < EPG; ++j) {
    k[j] = c[j] >> bbits;
    val[j] = c[j] != SENT;
  }
#pragma unroll
  for (int j = 0; j < EPG; ++j) tail[j] = val[j] && (k[j] != (j + 1 < EPG ? k[j + 1] : knext));
  FMX_STAMP(1, k[0] + knext + kprev + tile_prevkey);  // the sorted list has arrived

  // ---- issue the loads: rows of the runs that end here (HBM / MALL), then S of every occurrence (L2) ----
  // Branch-free: an occurrence that is not the tail of a run starting in this tile requests the field's FIRST row instead
  // (one address for all such lanes: one request per instruction) and never looks at the result.  With
  // `if (tail) row[j] = load_row(...)` the compiler closed every j's region with s_waitcnt vmcnt(0): the four row requests
  // of a lane group -- HBM / Infinity Cache round trips -- went out one after the other.
  RowRegs row[PREFETCH_ROWS ? EPG : 1];
  // INL: the row of the run that comes in from the previous tile (updated by THIS wave if the run ends here, by nobody
  // else in this launch) is requested with the other rows, instead of behind this wave's own stores
  RowRegs row_in;
  row_in.v = row_in.z = row_in.n = row_in.fo = splat(0.f);
  const bool run_comes_in = INL && base > 0 && val[0] && k[0] == tile_prevkey;  // meaningful in lane group 0
  auto request_rows = [&]() {
    if (PREFETCH_ROWS) {
#pragma unroll
      for (int j = 0; j < EPG; ++j) {
        const bool need = tail[j] && k[j] != tile_prevkey;
        row[j] = load_row<LAYOUT, RULE>(a.rows + (row0 + (need ? k[j] : 0u)) * (size_t)a.stride, q, kp, a.zoff);
      }
    }
    if (INL)  // (branch-free like the rows above; used by lane group 0 of a closing tile only)
      row_in = load_row<LAYOUT, RULE>(a.rows + (row0 + ((slot == 0 && run_comes_in) ? tile_prevkey : 0u)) * (size_t)a.stride, q, kp, a.zoff);
  };
  // A tile whose last run goes on into the next tile PUBLISHES its partial sums (below) for the tile that closes the run,
  // and the publication waits for everything this wave has in flight (s_waitcnt vmcnt(0) before the flag): such a tile
  // requests its rows only AFTER it has published -- its sums need S and dlogit (L2), not the rows (HBM / Infinity Cache).
  const bool tile_open_early = INL && __shfl((int)(val[EPG - 1] && k[EPG - 1] == knext), WAVE - 1) != 0;  // wave-uniform
  // Branch-free like the rows: a padding entry reads sample 0 and its contribution is dropped by a select.  (`if (val[j])
  // { loads; products }` closed every j's region with s_waitcnt vmcnt(0): four dependent L2 round trips per lane group.)
  float4 cV[EPG];
  CA cA[EPG];
  float cw[EPG];
  {
    const bool has_x = a.xv != nullptr;
    const float *xsrc = has_x ? a.xv : a.dz_first;  // something loadable
    const int fld = (has_x && a.cols) ? a.cols[f] : f;
    const int col = (has_x && a.fcols) ? a.fcols[fld] : fld;
    int efld = 0;  // OCC: the field whose slot of E this sort field's occurrences read
    if constexpr (OCC) efld = a.cols ? a.cols[f] : f;
    float4 S4[EPG], G4[EPG];
    float xl[EPG], dzf[EPG], dzbl[EPG];
    uint32_t bj[EPG];
#pragma unroll
    for (int j = 0; j < EPG; ++j) bj[j] = val[j] ? (c[j] & bmask) : 0u;
    // What the common callers do not need is not requested: feature values when there are none, and the bi-interaction's
    // coefficient when it is the first-order one (pure FM, DeepFM: dz_bi == dz_first; NFM: none).  Wave-uniform branches AHEAD
    // of the other requests: the wait the compiler puts at their joins covers nothing else.  (No measurable change of the
    // launch: the 2.5 us between the list's arrival and the arrival of S / dlogit / rows -- in-kernel stamps,
    // tools/update_stamps.sh -- are the ~110 K distinct row lines of a step at the chip's ~54 G random lines per second.)
    const bool sep_dzbi = a.dz_bi != nullptr && a.dz_bi != a.dz_first;
#pragma unroll
    for (int j = 0; j < EPG; ++j) {
      xl[j] = 1.f;
      dzbl[j] = 0.f;
    }
    if (has_x) {
#pragma unroll
      for (int j = 0; j < EPG; ++j) xl[j] = xsrc[(size_t)bj[j] * a.Fx + col];
    }
    if (sep_dzbi) {
#pragma unroll
      for (int j = 0; j < EPG; ++j) dzbl[j] = a.dz_bi[(size_t)bj[j] * a.ld1];
    }
#pragma unroll
    for (int j = 0; j < EPG; ++j) {
      const uint32_t b = bj[j];
      if constexpr (OCC) S4[j] = *reinterpret_cast<const float4 *>(a.gbi + (size_t)b * a.ldG + (size_t)efld * kp + 4 * q);
      else S4[j] = *reinterpret_cast<const float4 *>(a.S + (size_t)b * a.ldS + 4 * q);
      dzf[j] = a.dz_first[(size_t)b * a.ld1];
      if constexpr (HAS_GBI) G4[j] = *reinterpret_cast<const float4 *>(a.gbi + (size_t)b * a.ldG + 4 * q);
      else G4[j] = splat(0.f);
    }
    if (!tile_open_early) request_rows();
#pragma unroll
    for (int j = 0; j < EPG; ++j) {
      const float x = xl[j];
      const float dzb = a.dz_bi ? (sep_dzbi ? dzbl[j] : dzf[j]) : 0.f;
      const float w1 = x * dzf[j];
      float4 v;
      CA ca;
      if constexpr (OCC) {
        v = S4[j];
        ca.zero();
      } else if constexpr (HAS_GBI) {
        const float4 G = splat(dzb) + G4[j];
        const float4 xG = x * G;
        v = xG * S4[j];
        ca.v = x * xG;
      } else {
        const float xG = x * dzb;
        v = xG * S4[j];
        ca.v = x * xG;
      }
      cV[j] = splat(0.f);
      cA[j].zero();
      cw[j] = 0.f;
      if (val[j]) {  // selects
        cV[j] = v;
        cA[j] = ca;
        cw[j] = w1;
      }
    }
  }

  // ---- pass 1: the sum of the group's last run, and whether the group lies inside one longer run ----
  float4 tV = splat(0.f);
  CA tA;
  tA.zero();
  float tw = 0.f;
  bool uniform = true;
#pragma unroll
  for (int j = 0; j < EPG; ++j) {
    if (j > 0 && k[j] != k[j - 1]) {
      tV = splat(0.f);
      tA.zero();
      tw = 0.f;
      uniform = false;
    }
    tV = tV + cV[j];
    tA.add(cA[j]);
    tw += cw[j];
  }
  const bool lead_open = val[0] && k[0] == kprev;
  const bool trail_open = val[EPG - 1] && k[EPG - 1] == knext;
  bool pass = uniform && lead_open && trail_open;
  if (!trail_open) {
    tV = splat(0.f);
    tA.zero();
    tw = 0.f;
  }
  // ---- segmented scan over the groups: carry_out(s) = v(s) + (pass(s) ? carry_out(s-1) : 0) ----
#pragma unroll
  for (int off = 1; off < SLOTS; off <<= 1) {
    const float4 uV = shfl_up4(tV, off * LPR);
    const CA uA = tA.up(off * LPR);
    const float uw = __shfl_up(tw, off * LPR);
    const bool up = __shfl_up((int)pass, off * LPR) != 0;
    if (slot >= off) {
      if (pass) {
        tV = tV + uV;
        tA.add(uA);
        tw += uw;
      }
      pass = pass && up;
    }
  }
  // carry into this group = carry out of the previous one
  float4 accV = shfl_up4(tV, LPR);
  CA accA = tA.up(LPR);
  float accw = __shfl_up(tw, LPR);
  if (slot == 0 || !lead_open) {
    accV = splat(0.f);
    accA.zero();
    accw = 0.f;
  }

  // ---- the tile's hand-off state is known before any row is touched: does the run that came in end here (this tile
  //      CLOSES it), does the tile lie inside one run (THROUGH), does its last run go on (trail)?  The sum of that last
  //      run so far is the last group's carry-out.  With the in-launch hand-off (INL) the record and the flag word
  //      (launch sequence << 4 | lead_state << 2 | trail_state) are published NOW, before the row updates of pass 2, so
  //      that closing tiles further on never wait for this tile's FTRL arithmetic and store acknowledgements: records
  //      write-through, s_waitcnt vmcnt(0), then the flag as an agent-scope atomic; records and flags sc1 on both sides.
  bool closes_here = false;
#pragma unroll
  for (int j = 0; j < EPG; ++j) closes_here = closes_here || (tail[j] && k[j] == tile_prevkey);
  int lead_state = __ballot(closes_here) != 0ull ? LEAD_CLOSES : LEAD_NONE;
  int trail_state = 0;
  const bool tile_open = __shfl((int)trail_open, WAVE - 1) != 0;
  if (tile_open) {
    const bool through = __shfl((int)(k[EPG - 1] == tile_prevkey), WAVE - 1) != 0;
    if (through) lead_state = LEAD_THROUGH;  // the whole tile is one run, open at both ends
    else trail_state = 1;
    if (slot == SLOTS - 1) {
      if (INL) store_part_sc1(part + (through ? 0 : REC), q, kp, tV, tA.vec(), tw);
      else store_part(part + (through ? 0 : REC), q, kp, tV, tA.vec(), tw);
    }
  }
  if (INL) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    FMX_STAMP(2, lane);  // every load issued so far (S / dlogit, the rows unless the tile publishes first) has arrived
    if (lane == 0)
      __hip_atomic_store(a.meta + (size_t)gt * 2, (int32_t)((a.seq << 4) | ((uint32_t)lead_state << 2) | (uint32_t)trail_state),
                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else if (lane == 0) {
    a.meta[(size_t)gt * 2] = lead_state;
    a.meta[(size_t)gt * 2 + 1] = trail_state;
  }

  if (tile_open_early) request_rows();
  // ---- pass 2: walk the occurrences again; at the tail of a run apply the update or leave a partial ----
  float4 leadV = splat(0.f), leadA = splat(0.f);  // INL: this tile's part of the run that came in and ends here
  float leadw = 0.f;
  bool have_lead = false;
#pragma unroll
  for (int j = 0; j < EPG; ++j) {
    if (j > 0 && k[j] != k[j - 1]) {
      accV = splat(0.f);
      accA.zero();
      accw = 0.f;
    }
    accV = accV + cV[j];
    accA.add(cA[j]);
    accw += cw[j];
    if (tail[j]) {
      if (k[j] != tile_prevkey) {
        float *rp = a.rows + (row0 + k[j]) * (size_t)a.stride;
        const RowRegs r = PREFETCH_ROWS ? row[PREFETCH_ROWS ? j : 0] : load_row<LAYOUT, RULE>(rp, q, kp, a.zoff);
        update_row<LAYOUT, RULE>(rp, q, kp, a.zoff, r, accV, accA.vec(), accw, a.h);
      } else {
        // the run that came in from the previous tile ends here: its part inside this tile stays in registers for this
        // wave's combine below (INL), or goes to memory for k_fm_fixup
        if (INL) {
          leadV = accV;
          leadA = accA.vec();
          leadw = accw;
          have_lead = true;
        } else {
          store_part(part, q, kp, accV, accA.vec(), accw);
        }
      }
    }
  }
  FMX_STAMP(3, lane);  // pass 2 done: the row updates of the runs inside the tile are issued
  if (!INL) return;
  // ---- in-launch hand-off (INL): the CLOSING tile of a run sums the records of the tiles before it (they were
  //      dispatched earlier and wait on nothing) and applies the row update -- no second launch.
  //      No deadlock, whatever the dispatch order of the FIELDS: the tiles this wave waits for are tiles tj < t of ITS OWN
  //      field, and a field's tiles keep their relative order in the grid -- slot(f, tj) = position(f) * tiles_per_field + tj
  //      < slot(f, t).  Workgroups start in block-index order, so those waves are resident (or done) when this one runs, and
  //      they publish before they wait for anything: a tile publishes ahead of its own combine, and a combine never waits
  //      for a combine.  The bias / loss blocks poll only blocks behind them that wait on nothing. ----
  if (lead_state != LEAD_CLOSES) return;  // wave-uniform
  float *rp = a.rows + (row0 + tile_prevkey) * (size_t)a.stride;
  const RowRegs r = row_in;  // lanes < LPR: requested at the top (the row is final until this wave writes it)
  // this tile's own part of the run: from the registers of the lane group that closed it to every lane group's lane q
  const int src0 = __ffsll((long long)__ballot(have_lead)) - 1;  // first lane of that group (q == 0)
  const float4 ownV = shfl4(leadV, src0 + q), ownA = shfl4(leadA, src0 + q);
  const float ownw = __shfl(leadw, src0);
  // distance m to the head tile: tiles t-1, t-2, ... are THROUGH until the head (trail_state == 1)
  int m = 0;
  bool failed = false;
  for (int j0 = 1; j0 <= t && m == 0 && !failed; j0 += 64) {
    const int tj = t - j0 - lane;  // lane i looks at tile t - j0 - i
    int w = 0;
    bool ready = false;
    for (int spin = 0;; ++spin) {
      if (tj >= 0 && !ready) {
        w = __hip_atomic_load(a.meta + ((size_t)f * tiles_per_field + tj) * 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ready = ((uint32_t)w >> 4) == (a.seq & 0x0FFFFFFFu);
      }
      const bool is_through = tj >= 0 && ready && ((w >> 2) & 3) == LEAD_THROUGH;
      const unsigned long long stop = __ballot(!is_through);  // not published yet, or not THROUGH, or before the field
      if (stop == 0ull) break;                                // 64 THROUGH tiles: look further back
      const int pos = __ffsll((long long)stop) - 1;
      const bool resolved = __shfl((int)(ready || tj < 0), pos) != 0;
      if (resolved) {  // the chain ends at a published tile: it must be the head (its last run goes on)
        if (__shfl((int)(tj >= 0 && (w & 3) == 1), pos) != 0) m = j0 + pos;
        else failed = true;
        break;
      }
      if (spin >= (1 << 20)) {
        failed = true;
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
  }
  if (failed || m == 0 || m > t) {
    if (lane == 0 && a.error) *a.error = 2;
    return;
  }
  // the same record order and lane-group assignment as k_fm_fixup, so both modes give identical bits
  const size_t gh = (size_t)gt - m;
  float4 aV = splat(0.f), aA = splat(0.f);
  float aw = 0.f;
  for (int j = slot; j <= m; j += SLOTS) {
    if (j == m) {  // this tile's own record: the last one of its lane group, as in k_fm_fixup's order
      aV = aV + ownV;
      aA = aA + ownA;
      aw += ownw;
    } else {
      const float *rec = j == 0 ? a.parts + (gh * 2 + 1) * REC : a.parts + (gh + j) * 2 * REC;
      aV = aV + ld_sc1_4(rec + 4 * q);
      aA = aA + ld_sc1_4(rec + kp + 4 * q);
      aw += ld_sc1(rec + 2 * kp);
    }
  }
#pragma unroll
  for (int mm = LPR; mm < WAVE; mm <<= 1) {
    aV = aV + shfl_xor4(aV, mm);
    aA = aA + shfl_xor4(aA, mm);
    aw += __shfl_xor(aw, mm);
  }
  if (lane < LPR) update_row<LAYOUT, RULE>(rp, q, kp, a.zoff, r, aV, aA, aw, a.h);
  FMX_STAMP(4, lane);  // a closing tile: the crossing run's row is updated
}

template <int LPR, int LAYOUT, int RULE, bool HAS_GBI, bool INL>
__global__ __launch_bounds__(256) void k_fm_update(UpdArgs a) {
  __builtin_amdgcn_s_setprio(3);  // ahead of the side-stream sort's waves at the CU's instruction arbiter
  update_body<LPR, LAYOUT, RULE, HAS_GBI, INL>(a, blockIdx.x);
}

// The table update from explicit per-occurrence gradients (fmx_fm_update_occ; the AFM step's embedding gradient)
template <int LPR, int LAYOUT, int RULE, bool INL>
__global__ __launch_bounds__(256) void k_fm_update_occ(UpdArgs a) {
  __builtin_amdgcn_s_setprio(3);
  update_body<LPR, LAYOUT, RULE, false, INL, true>(a, blockIdx.x);
}

// The same launch with a RIDER: the workgroups behind the update's own carry the fixed-order reduction of the MLP's partial weight
// gradients (mlp_reduce_block: a few hundred latency-bound waves that the table update neither feeds nor needs -- both wait only for
// the launches in front).  fmx_deepfm_stream: one launch and 6 - 7 us less per step than k_mlp_reduce as a launch of its own in front
// of the update; on a second stream the same overlap lost to the cross-stream hand-off.  Identical results.
template <int LPR, int LAYOUT, int RULE, bool HAS_GBI>
__global__ __launch_bounds__(256) void k_fm_update_rider(UpdArgs a, MlpReduceArgs r, int n_update_blocks, int rider_blocks_per_layer) {
  __builtin_amdgcn_s_setprio(3);
  if ((int)blockIdx.x >= n_update_blocks) {
    const int rb = (int)blockIdx.x - n_update_blocks;
    mlp_reduce_block(r, rb / rider_blocks_per_layer, rb % rider_blocks_per_layer, rider_blocks_per_layer);
    return;
  }
  update_body<LPR, LAYOUT, RULE, HAS_GBI, true>(a, blockIdx.x);
}

// Runs that cross tile boundaries: the wave of the tile holding the run's head adds the partial sums in tile order
// (trail of the head tile, then the lead partial of every following tile up to the one where the run ends) and
// applies the row update.
template <int LPR, int LAYOUT, int RULE>
__global__ __launch_bounds__(256) void k_fm_fixup(UpdArgs a) {
  constexpr int SLOTS = WAVE / LPR;
  constexpr int REC = 2 * LPR * 4 + 4;
  const int lane = threadIdx.x & 63;
  const int slot = lane / LPR, q = lane % LPR;
  const int kp = LPR * 4;
  const int tiles_per_field = a.Bp >> 6;
  if (blockIdx.x == gridDim.x - 1 && red_slices(a.B) > 1) {  // (an extra workgroup: the slices' bias / loss partials, in slice order)
    finish_bias_and_loss<LAYOUT, RULE>(a, red_slices(a.B), false);
    return;
  }
  const int gt = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (gt >= a.F * tiles_per_field) return;
  const int f = gt / tiles_per_field;
  const int t = gt - f * tiles_per_field;
  // three dependent round trips instead of five: the head flag, the run's key (last entry of the tile) and the meta of
  // the following tiles are loaded together; the row is requested as soon as the key is known, before the partial
  // records are summed
  const int my_trail = a.meta[(size_t)gt * 2 + 1];
  const uint32_t key = a.sorted[(size_t)f * a.Bp + ((size_t)t << 6) + 63] >> a.bbits;
  const int tj0 = t + 1 + lane;
  const int st0 = tj0 < tiles_per_field ? a.meta[((size_t)f * tiles_per_field + tj0) * 2] : LEAD_NONE;
  if (my_trail != 1) return;  // wave-uniform
  float *rp = a.rows + ((size_t)a.foff[f] + key) * (size_t)a.stride;
  RowRegs r;
  if (lane < LPR) r = load_row<LAYOUT, RULE>(rp, q, kp, a.zoff);
  // m = number of following tiles that hold a piece of the run
  int m = 0;
  for (int j0 = 1; t + j0 < tiles_per_field; j0 += 64) {
    const int tj = t + j0 + lane;
    const int st = j0 == 1 ? st0 : (tj < tiles_per_field ? a.meta[((size_t)f * tiles_per_field + tj) * 2] : LEAD_NONE);
    const unsigned long long stop = __ballot(st != LEAD_THROUGH);
    if (stop != 0ull) {
      const int pos = __ffsll((long long)stop) - 1;
      const int st_pos = __shfl(st, pos);
      m = j0 + pos - (st_pos == LEAD_CLOSES ? 0 : 1);
      break;
    }
    m = j0 + 63;
  }
  if (t + m >= tiles_per_field) m = tiles_per_field - 1 - t;
  float4 aV = splat(0.f), aA = splat(0.f);
  float aw = 0.f;
  for (int j = slot; j <= m; j += SLOTS) {
    const float *rec = j == 0 ? a.parts + ((size_t)gt * 2 + 1) * REC : a.parts + (size_t)(gt + j) * 2 * REC;
    aV = aV + *reinterpret_cast<const float4 *>(rec + 4 * q);
    aA = aA + *reinterpret_cast<const float4 *>(rec + kp + 4 * q);
    aw += rec[2 * kp];
  }
#pragma unroll
  for (int mm = LPR; mm < WAVE; mm <<= 1) {
    aV = aV + shfl_xor4(aV, mm);
    aA = aA + shfl_xor4(aA, mm);
    aw += __shfl_xor(aw, mm);
  }
  if (lane < LPR) update_row<LAYOUT, RULE>(rp, q, kp, a.zoff, r, aV, aA, aw, a.h);
}

// The in-launch hand-offs tag their flag words with a per-launch sequence number passed as a kernel argument; a captured
// launch would replay a frozen number, so captures take the paths without hand-offs.
bool is_capturing(hipStream_t st) {
  if (!st) return false;  // the legacy default stream cannot be captured
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
}

template <int LPR, bool HAS_GBI, bool INL>
void launch_update(const UpdArgs &a, int rule, hipStream_t st) {
  const int tiles = a.F * (a.Bp >> 6);
  const int wpb = tune().wpb_upd;
  const dim3 grid((tiles + wpb - 1) / wpb + red_slices(a.B)), block(64 * wpb);
  with_rule(rule, [&](auto LAYOUT, auto RULE) { hipLaunchKernelGGL((k_fm_update<LPR, LAYOUT, RULE, HAS_GBI, INL>), grid, block, 0, st, a); });
}

template <int LPR>
void launch_update_rider(const UpdArgs &a, int rule, const MlpReduceArgs &r, hipStream_t st) {  // HAS_GBI, in-launch hand-off
  const int tiles = a.F * (a.Bp >> 6);
  const int wpb = tune().wpb_upd;
  const int n_upd = (tiles + wpb - 1) / wpb + red_slices(a.B), per = mlp_reduce_blocks_per_layer(r, 64 * wpb);
  const dim3 grid(n_upd + per * r.n_layers), block(64 * wpb);
  with_rule(rule, [&](auto LAYOUT, auto RULE) {  // (the MOMENTS rules: fmx_deepfm_stream_opt)
    hipLaunchKernelGGL((k_fm_update_rider<LPR, LAYOUT, RULE, true>), grid, block, 0, st, a, r, n_upd, per);
  });
}

template <int LPR>
void launch_fixup(const UpdArgs &a, int rule, hipStream_t st) {
  const int tiles = a.F * (a.Bp >> 6);
  const int wpb = tune().wpb_upd;
  const dim3 grid((tiles + wpb - 1) / wpb + (red_slices(a.B) > 1 ? 1 : 0)), block(64 * wpb);
  with_rule(rule, [&](auto LAYOUT, auto RULE) { hipLaunchKernelGGL((k_fm_fixup<LPR, LAYOUT, RULE>), grid, block, 0, st, a); });
}

template <int LPR>
void launch_update_pair(const UpdArgs &a, int rule, bool has_gbi, hipStream_t st) {
  if (tune().inline_fixup && !is_capturing(st)) {  // one launch: the closing tile of a crossing run sums the records itself
    if (has_gbi) launch_update<LPR, true, true>(a, rule, st);
    else launch_update<LPR, false, true>(a, rule, st);
    return;
  }
  if (has_gbi) launch_update<LPR, true, false>(a, rule, st);
  else launch_update<LPR, false, false>(a, rule, st);
  launch_fixup<LPR>(a, rule, st);
}

// the update from explicit per-occurrence gradients: the same grid, hand-off and fixup as launch_update_pair
template <int LPR>
void launch_update_occ_pair(const UpdArgs &a, int rule, hipStream_t st) {
  const int tiles = a.F * (a.Bp >> 6);
  const int wpb = tune().wpb_upd;
  const dim3 grid((tiles + wpb - 1) / wpb + red_slices(a.B)), block(64 * wpb);
  const bool inl = tune().inline_fixup && !is_capturing(st);
  with_rule(rule, [&](auto LAYOUT, auto RULE) {
    if (inl) hipLaunchKernelGGL((k_fm_update_occ<LPR, LAYOUT, RULE, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_fm_update_occ<LPR, LAYOUT, RULE, false>), grid, block, 0, st, a);
  });
  if (!inl) launch_fixup<LPR>(a, rule, st);
}

UpdArgs fill_upd(const fmx_table_t *table, const fmx_hyper_t *hyper, const Workspace &w, const uint32_t *sorted,
                 const float *xv, const float *S, const float *dz_first, const float *dz_bi, const float *gbi, int32_t B,
                 const float *loss_b, float inv_b, float *loss_out, int32_t *step_counter, int32_t sample_ld,
                 int32_t *err_flag, hipStream_t st) {
  UpdArgs a;
  // (a capturing stream: the order is used when the table is known already, never looked up -- the look-up is a blocking copy)
  a.ordered = update_order(table, !is_capturing(st), a.order) ? 1 : 0;
  a.ldS = sample_ld > 0 ? sample_ld : table->kp;
  a.ld1 = sample_ld > 0 ? sample_ld : 1;
  a.ldG = sample_ld > 0 ? sample_ld : table->kp;
  static std::atomic<uint32_t> launch_seq{1};
  a.seq = launch_seq.fetch_add(1) & 0x0FFFFFFFu;
  if (a.seq == 0) a.seq = launch_seq.fetch_add(1) & 0x0FFFFFFFu;  // 0 is what a zeroed workspace holds
  a.error = err_flag;
  a.rows = table->rows;
  a.foff = sort_offsets(table);  // the update walks the SORT fields' lists; a sort field's rows start at its own offset
  a.cols = sort_cols(table);
  a.Fx = n_cols(table);
  a.fcols = table->field_cols;
  a.bias = table->bias;
  a.sorted = sorted;
  a.parts = w.parts;
  a.meta = w.meta;
  a.red = reinterpret_cast<float *>(w.counter);
  a.xv = xv;
  a.S = S;
  a.dz_first = dz_first;
  a.dz_bi = dz_bi;
  a.gbi = gbi;
  a.loss_b = loss_b;
  a.loss_out = loss_out;
  a.step_counter = step_counter;
  a.h = kernel_hyper(hyper, -1);  // (ADAM's constants: update_impl)
  a.B = B;
  a.F = n_sort_fields(table);
  a.Bp = fmx_sorted_width(B);
  a.bbits = fmx_sorted_bbits(B);
  a.kp = table->kp;
  a.stride = table->row_stride;
  a.zoff = table->z_offset;
  a.inv_b = inv_b;
  return a;
}

}  // namespace

namespace fmxd {

int update_impl(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const Workspace &w,
                const uint32_t *sorted, const float *xv,
                const float *S, const float *dz_first, const float *dz_bi, const float *gbi, int32_t B,
                const float *loss_b, float inv_b, float *loss_out, hipStream_t st,
                int32_t *step_counter, int32_t sample_ld, int32_t *err_flag, const MlpReduceArgs *rider) {
  UpdArgs a = fill_upd(table, hyper, w, sorted, xv, S, dz_first, dz_bi, gbi, B, loss_b, inv_b, loss_out, step_counter,
                       sample_ld, err_flag, st);
  if (rule == FMX_RULE_ADAM)  // this launch is step t = hyper->step + 1: its constants in double, once (adam_consts)
    adam_consts(hyper->lr, hyper->beta1, hyper->beta2, hyper->step + 1, a.h.lr, a.h.beta1, a.h.beta2);
  if (rider) {
    if (gbi != nullptr && tune().inline_fixup && !is_capturing(st)) {  // the one-launch form of the update: the rider goes with it
      with_lpr(table->kp, [&](auto LPR) { launch_update_rider<LPR>(a, rule, *rider, st); });
      return check_launch("k_fm_update_rider");
    }
    mlp_launch_reduce(*rider, st);  // otherwise the reduction as a launch of its own, in front
  }
  with_lpr(table->kp, [&](auto LPR) { launch_update_pair<LPR>(a, rule, gbi != nullptr, st); });
  return check_launch("k_fm_update / k_fm_fixup");
}

// occ [B, ld_occ]: sample b's gradients of its fields' rows, field f's kp floats at b * ld_occ + f * kp (update_body's OCC)
int update_occ_impl(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const Workspace &w, const float *xv,
                    const float *dz_first, const float *occ, int32_t ld_occ, int32_t B, const float *loss_b, float inv_b,
                    float *loss_out, hipStream_t st) {
  UpdArgs a = fill_upd(table, hyper, w, w.sorted, xv, nullptr, dz_first, nullptr, occ, B, loss_b, inv_b, loss_out, nullptr, 0,
                       nullptr, st);
  a.ldG = ld_occ;
  if (rule == FMX_RULE_ADAM) adam_consts(hyper->lr, hyper->beta1, hyper->beta2, hyper->step + 1, a.h.lr, a.h.beta1, a.h.beta2);
  with_lpr(table->kp, [&](auto LPR) { launch_update_occ_pair<LPR>(a, rule, st); });
  return check_launch("k_fm_update_occ / k_fm_fixup");
}

}  // namespace fmxd

#ifdef FMX_STAMPS
extern "C" int fmx_debug_update_stamps(unsigned long long *host_out) {  // [8192][6]; diagnostic build only (not in include/fmx.h)
  return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_upd_stamps), sizeof(unsigned long long) * 8192 * 6) == hipSuccess ? FMX_OK : FMX_ERR_LAUNCH;
}
#endif
