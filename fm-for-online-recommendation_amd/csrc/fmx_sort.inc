// fmx_sort.inc -- the occurrence sort: for every (sort) field the batch's (local index, sample) pairs as 32-bit composites
// (index << bbits) | sample, ascending, padded with 0xFFFFFFFF.  Equal rows become adjacent runs ordered by sample, so the
// duplicate-row reduction the reference gets from embedding_dense_backward (fm_adam.py:67) is deterministic.  Independent of the
// weights.  Included inside the anonymous namespace of fmx_kernels.hip (and by tools/micro/sort_bench.hip).
//   k_sort_radix                  stable LSD counting sort on the index bits (batches up to 8,192): the default
//   k_sort_occ                    bitonic network, one workgroup per field (wider batches)
//   k_sort_chunk + k_sort_merge   bitonic chunks + rank merge, spread over the chip (wide batches, one or two per launch)

// ------------------------------------------------------------------------------------------------------------
// k_sort_occ
// ------------------------------------------------------------------------------------------------------------
struct SortArgs {
  // one launch may sort several batches of a pool: workgroup (f, j) sorts field f of batch (pool_first + j) % n_pool into
  // sorted + j * sorted_stride (n_batches == 1 and pool_stride == 0 for a single batch)
  int32_t n_pool, pool_first, n_batches;
  int64_t pool_stride, sorted_stride;  // in elements
  const int32_t *idx;
  const int64_t *foff;   // the fields' row offsets (range check of an index against its field)
  const int64_t *soff;   // the SORT fields' row offsets: a refinement of foff (fmx_table_t.sort_offsets), or foff itself
  const int32_t *cols;   // the field every sort field is a piece of, or null (sort field == field)
  const int32_t *fcols;  // the idx column of every FIELD, or null (field f reads column f): fmx_table_t.field_cols
  const int32_t *fbase;  // the column-local index of every field's first row, or null (0): fmx_table_t.field_base
  uint32_t *sorted;
  int32_t *error;
  int32_t B, F, Bp, bbits;  // F: number of SORT fields
  int32_t Fi;               // columns of idx
  int32_t small_bits;       // k_sort_occ: sort fields of at most this many index bits take ONE counting pass (radix_field) instead
                            // of the bitonic network; 0: none (the launch's LDS is then sized for the network alone)
};

// Bitonic network on N = Bp composites held E per thread in a blocked layout (element i = tid * E + r):
//   partner distance j <  E        in-thread compare-exchange
//   E <= j < 64 E                  partner in another lane of the wave: xor_lane<j / E>
//   j >= 64 E                      partner in another wave: through LDS
template <int E, int LJ>
__device__ __forceinline__ void bitonic_lane_stage(uint32_t (&v)[E], int i0, int lane, int k) {
  const bool lower = (lane & LJ) == 0;
  const bool up = (i0 & k) == 0;  // (i & k) is the same for all r because k > j >= E
  const bool take_min = lower == up;
#pragma unroll
  for (int r = 0; r < E; ++r) {
    const uint32_t o = xor_lane<LJ>(v[r], lane);
    const uint32_t lo = v[r] < o ? v[r] : o, hi = v[r] < o ? o : v[r];
    v[r] = take_min ? lo : hi;
  }
}

template <int E>
__device__ __forceinline__ void bitonic_local(uint32_t (&v)[E], int tid, int k, int jmax) {
  // stages j = jmax, jmax/2, ..., 1 of merge level k, all of which stay inside one wave
  const int i0 = tid * E;
  const int lane = tid & 63;
  if (jmax >= 32 * E) bitonic_lane_stage<E, 32>(v, i0, lane, k);
  if (jmax >= 16 * E) bitonic_lane_stage<E, 16>(v, i0, lane, k);
  if (jmax >= 8 * E) bitonic_lane_stage<E, 8>(v, i0, lane, k);
  if (jmax >= 4 * E) bitonic_lane_stage<E, 4>(v, i0, lane, k);
  if (jmax >= 2 * E) bitonic_lane_stage<E, 2>(v, i0, lane, k);
  if (jmax >= E) bitonic_lane_stage<E, 1>(v, i0, lane, k);
#pragma unroll
  for (int j = E / 2; j > 0; j >>= 1) {
    if (j <= jmax) {
#pragma unroll
      for (int r = 0; r < E; ++r) {
        if ((r & j) == 0) {
          const bool up = ((i0 + r) & k) == 0;
          const uint32_t x = v[r], y = v[r + j];
          if ((x > y) == up) { v[r] = y; v[r + j] = x; }
        }
      }
    }
  }
}

// composites of samples i0 .. i0 + E - 1 of field f: every index load is issued before the first is used (a branch per
// element -- range check, error flag -- made the compiler wait for each load in turn: E dependent HBM round trips)
// Sort field f is rows [soff[f], soff[f + 1]) of field col: an index outside that piece belongs to another piece of the
// field (padding here, no error); an index outside the FIELD raises the flag.
template <int E>
__device__ __forceinline__ void load_composites(const SortArgs &a, int f, int i0, uint32_t (&v)[E]) {
  const int fld = a.cols ? a.cols[f] : f;
  const int col = a.fcols ? a.fcols[fld] : fld;
  const int64_t f_lo = a.foff[fld];
  const uint32_t field_rows = (uint32_t)(a.foff[fld + 1] - f_lo);
  const bool pieces = a.fcols || a.fbase;  // a field is a piece of its column: an index outside it is not an error
  const uint32_t base = (uint32_t)(a.soff[f] - f_lo) + (a.fbase ? (uint32_t)a.fbase[fld] : 0u), piece_rows = (uint32_t)(a.soff[f + 1] - a.soff[f]);
  uint32_t li[E];
#pragma unroll
  for (int r = 0; r < E; ++r) {
    const int i = i0 + r;
    li[r] = (uint32_t)a.idx[(size_t)(i < a.B ? i : a.B - 1) * a.Fi + col];
  }
  bool bad = false;
#pragma unroll
  for (int r = 0; r < E; ++r) {
    const int i = i0 + r;
    const uint32_t lp = li[r] - base;  // wraps to a huge value below the piece
    const bool mine = i < a.B && lp < piece_rows;
    v[r] = mine ? ((lp << a.bbits) | (uint32_t)i) : SENT;
    bad = bad || (!pieces && i < a.B && li[r] >= field_rows);
  }
  if (bad && a.error) *a.error = 1;
}

// ------------------------------------------------------------------------------------------------------------
// k_sort_radix: the occurrence sort as a stable LSD counting sort on the index bits
// ------------------------------------------------------------------------------------------------------------
// The lists are the ones k_sort_occ produces (composites are unique, so any correct sort gives the same bits), but a field
// costs one or two counting passes instead of a bitonic network of 78 dependent stages on 16 waves of one CU.  Samples are
// already in order, so only the index needs sorting, and stably: position = (elements with a smaller digit) + (earlier
// elements with the same digit).
//   * the batch is cut into 64-sample chunks; wave w of the workgroup owns R consecutive chunks (R = Bp / threads);
//   * per chunk the lanes holding equal digits find each other with one ballot per digit bit (match-any), rank = earlier lanes
//     of the group; the group's first lane bumps the wave's OWN counter of that digit in LDS (u16 cnt[digit][wave]: no atomics,
//     the order is the program's); every lane keeps (count before the chunk + rank) = its rank inside the wave;
//   * a fixed-order scan over cnt in (digit-major, wave-minor) order turns the counters into bases: position = base + rank;
//   * an index of up to RADIX_D bits takes one pass straight to memory, wider ones ceil(bits / RADIX_D) passes, ping-pong in LDS.
// Integer work only: bit-exact by construction, no dependence on timing.
constexpr int RADIX_D = 11;            // digit bits per pass: 2^11 digits x 4 waves x 2 bytes = 16 KB of counters
#ifndef FMX_RADIX_THREADS
#define FMX_RADIX_THREADS 256          // (tools/micro/sort_bench.hip builds other widths)
#endif
constexpr int RADIX_THREADS = FMX_RADIX_THREADS;  // threads per workgroup (256 = 4 waves: one per SIMD)
constexpr int RADIX_MAX_WIDTH = 8192;  // widest batch this kernel takes (LDS: 2 x Bp words + Bp half-words + counters)
// k_sort_occ's small fields: at most RADIX_SMALL_BITS index bits (511 rows + the padding key) in ONE counting pass by the
// launch's own (wide) workgroup, batches up to RADIX_SMALL_WIDTH: 2^9 digits x 16 waves x 2 bytes = 16 KB of counters
constexpr int RADIX_SMALL_BITS = 9, RADIX_SMALL_WIDTH = 4096;
__host__ __device__ inline size_t radix_small_lds_bytes(int Bp, int nt) {
  return (size_t)Bp * 4 + 64 * 4 + (size_t)Bp * 2 + ((size_t)(1 << RADIX_SMALL_BITS) * (nt / 64)) * 2;
}

__host__ __device__ inline size_t radix_lds_bytes(int Bp, int nt) {
  const int nw = nt / 64;
  return (size_t)Bp * 4 * 2 + (size_t)Bp * 2 + ((size_t)(1 << RADIX_D) * nw) * 2 + 64 * 4;
}

// digit groups of a wave: mask of the lanes whose `dg` equals this lane's (d ballots)
__device__ __forceinline__ unsigned long long match_digits(uint32_t dg, int d) {
  unsigned long long m = ~0ull;
  for (int b = 0; b < d; ++b) {
    const bool bit = (dg >> b) & 1u;
    const unsigned long long bal = __ballot(bit);
    m &= bit ? bal : ~bal;
  }
  return m;
}

// One counting pass over `src` (LDS, Bp composites in the current order): dg = (composite >> shift) & mask.
//   to_lds: positions scattered into dst_lds; else into dst_glb, valid composites as they are, the padding as SENT.
// cnt: u16 [n_dig][nw]; lrank: u16 [Bp]; sc: 64 words of scan scratch.  Ends with a barrier.
__device__ __forceinline__ void radix_pass(const uint32_t *src, uint32_t *dst_lds, uint32_t *dst_glb, uint16_t *cnt, uint16_t *lrank,
                                           uint32_t *sc, int Bp, int shift, int d, uint32_t pad_from, uint32_t *starts) {
  const int tid = threadIdx.x, nt = blockDim.x, nw = nt >> 6, w = tid >> 6, lane = tid & 63;
  const int n_dig = 1 << d, R = Bp / nt;
  const uint32_t mask = (uint32_t)n_dig - 1u;
  for (int i = tid; i < (n_dig * nw + 1) / 2; i += nt) reinterpret_cast<uint32_t *>(cnt)[i] = 0u;
  __syncthreads();
  // ---- count: the wave walks its R chunks in sample order ----
  for (int r = 0; r < R; ++r) {
    const int p = (w * R + r) * 64 + lane;
    const uint32_t dg = (src[p] >> shift) & mask;
    const unsigned long long m = match_digits(dg, d);
    const unsigned long long below = m & ((1ull << lane) - 1ull);
    const int rank = __popcll(below), n = __popcll(m);
    const uint32_t old = cnt[dg * nw + w];
    lrank[p] = (uint16_t)(old + rank);
    if (rank == 0) cnt[dg * nw + w] = (uint16_t)(old + n);
  }
  __syncthreads();
  // ---- scan: thread t owns the consecutive digits [t kpt, (t + 1) kpt); counters -> exclusive bases, digit-major ----
  const int kpt = (n_dig + nt - 1) / nt;
  const int k0 = tid * kpt, k1 = (k0 + kpt < n_dig) ? k0 + kpt : n_dig;
  uint32_t tot = 0;
  for (int k = k0; k < k1; ++k)
    for (int ww = 0; ww < nw; ++ww) tot += cnt[k * nw + ww];
  uint32_t inc = tot;  // inclusive scan over the wave
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t u = __shfl_up(inc, o);
    if (lane >= o) inc += u;
  }
  if (lane == 63) sc[w] = inc;
  __syncthreads();
  uint32_t run = inc - tot;
  for (int ww = 0; ww < w; ++ww) run += sc[ww];
  for (int k = k0; k < k1; ++k) {
    if (starts) starts[k] = run;  // first position of digit k's run (one-pass fields: digit == local index)
    for (int ww = 0; ww < nw; ++ww) {
      const uint32_t c = cnt[k * nw + ww];
      cnt[k * nw + ww] = (uint16_t)run;
      run += c;
    }
  }
  __syncthreads();
  // ---- scatter ----
  for (int r = 0; r < R; ++r) {
    const int p = (w * R + r) * 64 + lane;
    const uint32_t c = src[p];
    const uint32_t dg = (c >> shift) & mask;
    const uint32_t pos = (uint32_t)cnt[dg * nw + w] + (uint32_t)lrank[p];
    if (dst_lds) dst_lds[pos] = c;
    else dst_glb[pos] = c >= pad_from ? SENT : c;
  }
  __syncthreads();
}

// One field by counting passes: idx / out already point at the batch, smem holds radix_lds_bytes(Bp, blockDim.x) -- or, ONE_PASS
// (the caller knows the field has at most RADIX_SMALL_BITS index bits), radix_small_lds_bytes: no second key buffer.
template <bool ONE_PASS>
__device__ __forceinline__ void radix_field(const SortArgs &a, int f, const int32_t *idx, uint32_t *out, uint32_t *rsm, uint32_t *st_out) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const int Bp = a.Bp, R = Bp / nt, w = tid >> 6, lane = tid & 63;
  uint32_t *keys = rsm, *alt = rsm + Bp, *sc = ONE_PASS ? alt : alt + Bp;
  uint16_t *lrank = reinterpret_cast<uint16_t *>(sc + 64);
  uint16_t *cnt = lrank + Bp;

  const int fld = a.cols ? a.cols[f] : f;
  const int col = a.fcols ? a.fcols[fld] : fld;
  const int64_t f_lo = a.foff[fld];
  const uint32_t field_rows = (uint32_t)(a.foff[fld + 1] - f_lo);
  const bool pieces = a.fcols || a.fbase;
  const uint32_t base = (uint32_t)(a.soff[f] - f_lo) + (a.fbase ? (uint32_t)a.fbase[fld] : 0u), piece_rows = (uint32_t)(a.soff[f + 1] - a.soff[f]);
  // keys 0 .. piece_rows - 1 are rows of the piece, key piece_rows is the padding (beyond the batch, another piece of the field,
  // an index outside the field): it sorts behind every row and leaves as SENT
  const int bits = piece_rows ? 32 - __clz((int)piece_rows) : 1;  // (an empty field: every key is the padding)
  const uint32_t pad_from = piece_rows << a.bbits;
  bool bad = false;
  for (int r0 = 0; r0 < R; r0 += 4) {  // four independent loads in flight per thread
    uint32_t li[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int r = r0 + u < R ? r0 + u : R - 1;
      const int i = (w * R + r) * 64 + lane;
      li[u] = (uint32_t)idx[(size_t)(i < a.B ? i : a.B - 1) * a.Fi + col];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (r0 + u < R) {
        const int i = (w * R + r0 + u) * 64 + lane;
        const uint32_t lp = li[u] - base;
        const bool mine = i < a.B && lp < piece_rows;
        keys[i] = ((mine ? lp : piece_rows) << a.bbits) | (uint32_t)i;
        bad = bad || (!pieces && i < a.B && li[u] >= field_rows);
      }
    }
  }
  if (bad && a.error) *a.error = 1;
  uint32_t *st = bits <= RADIX_D ? st_out : nullptr;
  // ceil(bits / RADIX_D) passes over digits of (nearly) equal width, lowest first; the last one writes the list
  const int n_pass = (bits + RADIX_D - 1) / RADIX_D;
  int shift = a.bbits, left = bits;
  uint32_t *src = keys, *dst = alt;
  for (int ps = 0; ps < n_pass; ++ps) {
    const int d = (left + (n_pass - ps) - 1) / (n_pass - ps);
    const bool last = ps + 1 == n_pass;
    radix_pass(src, last ? nullptr : dst, out, cnt, lrank, sc, Bp, shift, d, pad_from, last ? st : nullptr);
    shift += d;
    left -= d;
    uint32_t *t = src;
    src = dst;
    dst = t;
  }
}

// Device body of the occurrence sort of ONE field (the calling workgroup: nt threads, nt * E == Bp): the full bitonic
// network, stages with partner distance < 64 E in registers / DPP, the cross-wave stages through LDS (Bp words); 78
// dependent stages at Bp = 4096.  (Tried and removed: every wave sorting its 64 E composites in registers followed by
// binary-search merge rounds in LDS -- 36 stages + 4 rounds, but LDS-bandwidth bound: 31 us against 22.)
template <int E>
__device__ __forceinline__ void sort_field(const SortArgs &a, int f, uint32_t *sm) {
  const int tid = threadIdx.x, nt = blockDim.x;
  if (a.small_bits > 0) {  // (workgroup-uniform) a small field: one counting pass instead of the network's 78 dependent stages
    const uint32_t piece_rows = (uint32_t)(a.soff[f + 1] - a.soff[f]);
    const int bits = piece_rows ? 32 - __clz((int)piece_rows) : 1;
    if (bits <= a.small_bits) {
      radix_field<true>(a, f, a.idx, a.sorted + (size_t)f * a.Bp, sm, nullptr);
      return;
    }
  }
  uint32_t v[E];
  load_composites<E>(a, f, tid * E, v);
  const int wave_span = 64 * E;  // elements held by one wave
  uint32_t *dst = a.sorted + (size_t)f * a.Bp;
  const int half = a.Bp >> 1;
  for (int k = 2; k <= a.Bp; k <<= 1) {
    int j = k >> 1;
    if (j >= wave_span) {
      // cross-wave stages through LDS
#pragma unroll
      for (int r = 0; r < E; ++r) sm[tid * E + r] = v[r];
      __syncthreads();
      for (; j >= wave_span; j >>= 1) {
        for (int t = tid; t < half; t += nt) {
          const int i = 2 * t - (t & (j - 1));
          const int l = i + j;
          const uint32_t x = sm[i], y = sm[l];
          const bool up = (i & k) == 0;
          if ((x > y) == up) { sm[i] = y; sm[l] = x; }
        }
        __syncthreads();
      }
#pragma unroll
      for (int r = 0; r < E; ++r) v[r] = sm[tid * E + r];
      __syncthreads();
    }
    bitonic_local<E>(v, tid, k, j);
  }
#pragma unroll
  for (int r = 0; r < E; ++r) dst[(size_t)tid * E + r] = v[r];
}

// (unit, inner) of this block: units are spread round-robin over the 8 XCDs, the `n_inner` blocks of a unit share one
// (blocks b and b + 8 share an XCD and its L2; placement is for speed only)
__device__ __forceinline__ bool xcd_unit(int n_units, int n_inner, int &unit, int &inner) {
  const int b = blockIdx.x, x = b & 7, s = b >> 3;
  inner = s % n_inner;
  unit = (s / n_inner) * 8 + x;
  return unit < n_units;
}

// Grid (launches of 8 or more batches): 8 * F * ceil(n_batches / 8) workgroups; the F workgroups of one batch sit on ONE XCD: each of them reads one
// column of the batch's [B, Fi] index slab, i.e. 4 bytes of every 128-byte line, so a slab whose workgroups were dealt over
// all eight XCDs was fetched from HBM by every one of them (21 MB per 8 batches against 5 MB of indices).
template <int E>
__global__ __launch_bounds__(1024) void k_sort_occ(SortArgs a) {
  extern __shared__ uint32_t sm[];
  int j, f;  // batch slot of this launch, sort field
  if (a.n_batches >= 8) {
    if (!xcd_unit(a.n_batches, a.F, j, f)) return;
  } else {  // few batches: all their workgroups on one or a few XCDs would leave most of the chip idle (39 workgroups on 32 CUs)
    j = blockIdx.x / a.F;
    f = blockIdx.x - j * a.F;
  }
  if (j > 0 || a.pool_stride != 0) {
    a.idx += (size_t)((a.pool_first + j) % a.n_pool) * a.pool_stride;
    a.sorted += (size_t)j * a.sorted_stride;
  }
  sort_field<E>(a, f, sm);
}

// The same lists from a grid of `n_wg` workgroups (a multiple of 8, at most one per unit), each walking several units: the form
// of the online loop's side-stream group launches that run beside a whole group of steps (lists needed a group later).  It bounds how many CUs
// carry a sort workgroup while the step's own kernels run beside it: a 1,024-thread workgroup takes 4 of a SIMD's 8 wave slots
// and 160 of its 512 VGPRs, so a CU with one of them holds 8 waves of the FTRL update (144 VGPRs) instead of 12 and a CU with two
// holds none -- the uncapped grid (624 workgroups for 16 Criteo batches) took the update's one round of waves to two on the
// launches beside it.  The host requests more than half of a CU's LDS for the launch, so no CU ever holds two.
//   * workgroup b serves XCD x = b & 7 and that XCD's batches j = x, x + 8, ... (a batch's units stay on ONE XCD, as above);
//   * the XCD's units are dealt FIELD-major -- every batch of the first field, then the next field -- round-robin over its
//     n_wg / 8 workgroups, fields in the host's order (largest first where the row counts are known), so the bitonic fields
//     spread evenly and the counting-pass fields fill the tail;
//   * the assignment is static: no atomics, no flags, no workgroup waits for another.
// Which workgroup sorts a unit is invisible in the lists; a stale or missing order costs time only.
struct ResidentSortArgs {
  SortArgs s;
  int32_t n_wg;     // the grid
  int32_t ordered;  // 0: fields in index order
  uint32_t order[UPD_ORDER_MAX / 4];  // position i of the walk is sort field order[i], one byte each (as UpdArgs::order)
};

template <int E>
__global__ __launch_bounds__(1024) void k_sort_occ_resident(ResidentSortArgs ra) {
  extern __shared__ uint32_t sm[];
  const SortArgs &a = ra.s;
  const int x = blockIdx.x & 7, s = blockIdx.x >> 3, per_xcd = ra.n_wg >> 3;
  const int nb = x < a.n_batches ? (a.n_batches - x + 7) >> 3 : 0;  // this XCD's batches
  for (int u = s; u < nb * a.F; u += per_xcd) {
    const int pos = u / nb, j = x + 8 * (u - pos * nb);
    int f = pos;
    if (ra.ordered) {  // through the kernel-argument segment, not ra.order[...]: no variable index into a by-value argument (k_fm_update)
      typedef const __attribute__((address_space(4))) uint32_t karg_u32;
      karg_u32 *ka = (karg_u32 *)__builtin_amdgcn_kernarg_segment_ptr();
      f = (int)((ka[offsetof(ResidentSortArgs, order) / 4 + (pos >> 2)] >> ((pos & 3) * 8)) & 0xFFu);
      if (f >= a.F) f = pos;  // (the host sends a permutation of the fields; nothing outside the lists is written whatever it sends)
    }
    SortArgs ua = a;
    ua.idx += (size_t)((a.pool_first + j) % a.n_pool) * a.pool_stride;
    ua.sorted += (size_t)j * a.sorted_stride;
    sort_field<E>(ua, f, sm);
    __syncthreads();  // the next unit reuses the LDS
  }
}

// ------------------------------------------------------------------------------------------------------------
// k_sort_chunk + k_sort_merge: the occurrence sort for Bp >= 2 * SORT_CHUNK, spread over the chip
// ------------------------------------------------------------------------------------------------------------
// One workgroup per field keeps a 4,096-composite sort on ONE CU: 78 dependent bitonic stages, VALU-issue bound there
// (22 us per batch while 217 CUs idle).  Here a field's Bp composites are cut into chunks of SORT_CHUNK = 1,024:
//   k_sort_chunk  workgroup (field, chunk, batch): 256 threads x 4 composites, the bitonic network on 1,024 (55 stages,
//                 3 of them through LDS) -> `runs` [F, Bp], every chunk sorted;
//   k_sort_merge  workgroup (field, chunk, batch): the field's C sorted chunks in LDS (Bp words, 16-byte loads); every
//                 composite of chunk c finds its rank among the other chunks by binary search (stable: ties -- only the
//                 0xFFFFFFFF padding ties -- count for earlier chunks, not for later ones) and is stored at
//                 sorted[f][own index + sum of ranks].
// The result is the same array the one-workgroup sort produces (composites are unique, so any correct sort gives the
// same bits).  Block -> work mapping is XCD-aware (blocks b and b + 8 share an XCD and its L2): the F workgroups that
// read one chunk's [1024, F] slab of idx (each 128-byte line of it holds 32 of a sample's 39 indices and is read by
// the workgroups of 32 fields) sit on ONE XCD, so the slab is fetched from HBM once instead of once per XCD; likewise
// the C merge workgroups of a field read the same Bp words.  Placement is for speed only.
constexpr int SORT_CHUNK_E = 4, SORT_CHUNK_THREADS = SORT_CHUNK / SORT_CHUNK_E;  // (SORT_CHUNK: fmx_common.h)
// from this width on the chunked form is the faster one for ONE batch per launch (MI355X, Criteo vocabulary: 4,096: 17.5 vs
// 18.5 us; 8,192: 24 vs 36; 16,384: 60 vs 74; 32,768 x 6 fields: 58 us) -- launches of 8 batches: 29 vs 27, 71 vs 55, 294 vs 118
constexpr int SORT_CHUNKED_MIN_WIDTH = 8192;

struct ChunkArgs {
  SortArgs s;          // s.sorted: the final lists; runs: the chunk-sorted intermediate, same shape
  uint32_t *runs;
  int64_t runs_stride; // elements between the batches of one launch
  int32_t C;           // chunks per field = Bp / SORT_CHUNK
};

__global__ __launch_bounds__(SORT_CHUNK_THREADS) void k_sort_chunk(ChunkArgs a) {
  constexpr int E = SORT_CHUNK_E;
  __shared__ uint32_t sm[SORT_CHUNK];
  int unit, f;
  if (!xcd_unit(a.s.n_batches * a.C, a.s.F, unit, f)) return;
  const int j = unit / a.C, c = unit - j * a.C;
  const int32_t *idx = a.s.idx + (size_t)((a.s.pool_first + j) % a.s.n_pool) * a.s.pool_stride;
  uint32_t *dst = a.runs + (size_t)j * a.runs_stride + (size_t)f * a.s.Bp + (size_t)c * SORT_CHUNK;
  const int tid = threadIdx.x;
  uint32_t v[E];
  {
    SortArgs sa = a.s;
    sa.idx = idx;
    load_composites<E>(sa, f, c * SORT_CHUNK + tid * E, v);
  }
  constexpr int wave_span = 64 * E;
  for (int k = 2; k <= SORT_CHUNK; k <<= 1) {
    int jj = k >> 1;
    if (jj >= wave_span) {  // partner in another wave: through LDS
#pragma unroll
      for (int r = 0; r < E; ++r) sm[tid * E + r] = v[r];
      __syncthreads();
      for (; jj >= wave_span; jj >>= 1) {
        for (int t = tid; t < SORT_CHUNK / 2; t += SORT_CHUNK_THREADS) {
          const int i = 2 * t - (t & (jj - 1));
          const int l = i + jj;
          const uint32_t x = sm[i], y = sm[l];
          const bool up = (i & k) == 0;
          if ((x > y) == up) { sm[i] = y; sm[l] = x; }
        }
        __syncthreads();
      }
#pragma unroll
      for (int r = 0; r < E; ++r) v[r] = sm[tid * E + r];
      __syncthreads();
    }
    bitonic_local<E>(v, tid, k, jj);
  }
  *reinterpret_cast<uint4 *>(dst + tid * E) = uint4{v[0], v[1], v[2], v[3]};
}

__global__ __launch_bounds__(SORT_CHUNK_THREADS) void k_sort_merge(ChunkArgs a) {
  constexpr int E = SORT_CHUNK_E;
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];  // the field's C sorted chunks: Bp words
  int unit, c;
  if (!xcd_unit(a.s.n_batches * a.s.F, a.C, unit, c)) return;
  const int j = unit / a.s.F, f = unit - j * a.s.F;
  const uint32_t *src = a.runs + (size_t)j * a.runs_stride + (size_t)f * a.s.Bp;
  uint32_t *dst = a.s.sorted + (size_t)j * a.s.sorted_stride + (size_t)f * a.s.Bp;
  const int tid = threadIdx.x;
  // LDS image: element i of the field at word i + (i >> 5).  A binary search reads the odd multiples of 1024 / 2^d at
  // depth d; unpadded, all of them fall into one or two of the 32 banks (up to 32-way conflicts, 8x the time over the 11
  // steps: 13 us per launch); one pad word per 32 spreads every depth over the banks (at most 2-way).
  auto at = [](int i) { return i + (i >> 5); };
  {
    uint4 t[8];  // up to Bp = 8 * 1024: every global load in flight before the first LDS store
    const int n_it = a.s.Bp / (SORT_CHUNK_THREADS * 4);
    for (int it0 = 0; it0 < n_it; it0 += 8) {
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (it0 + u < n_it) t[u] = *reinterpret_cast<const uint4 *>(src + (it0 + u) * SORT_CHUNK_THREADS * 4 + tid * 4);
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (it0 + u < n_it) {
          const int i = (it0 + u) * SORT_CHUNK_THREADS * 4 + tid * 4;  // i .. i + 3 share i >> 5
          uint32_t *d4 = smem + at(i);
          d4[0] = t[u].x; d4[1] = t[u].y; d4[2] = t[u].z; d4[3] = t[u].w;
        }
    }
  }
  __syncthreads();
  uint32_t v[E];
  int pos[E];
#pragma unroll
  for (int r = 0; r < E; ++r) {
    v[r] = smem[at(c * SORT_CHUNK + tid * E + r)];
    pos[r] = tid * E + r;
  }
  for (int o = 0; o < a.C; ++o) {
    if (o == c) continue;  // workgroup-uniform
    const uint32_t *run = smem + at(o * SORT_CHUNK);  // SORT_CHUNK is a multiple of 32: run[at(m)] is element m of the run
    const bool before = o < c;  // ties: an equal composite of an earlier chunk goes first (stable)
    // number of the run's composites that go before v[r] (ties: an equal composite of an EARLIER chunk goes first; only
    // the 0xFFFFFFFF padding ties): fixed-step binary searches without branches -- a short-circuit in the comparison
    // compiled to a branch and a wait per LDS read, 132 dependent reads per thread -- the E searches of a thread
    // interleaved, so each step has E reads in flight
    int cnt[E];
#pragma unroll
    for (int r = 0; r < E; ++r) cnt[r] = 0;
#pragma unroll
    for (int step = SORT_CHUNK / 2; step >= 1; step >>= 1) {
#pragma unroll
      for (int r = 0; r < E; ++r) {
        const uint32_t m = run[at(cnt[r] + step - 1)];
        const int goes_before = (int)(m < v[r]) | ((int)before & (int)(m == v[r]));
        cnt[r] += goes_before ? step : 0;
      }
    }
#pragma unroll
    for (int r = 0; r < E; ++r) {  // cnt <= SORT_CHUNK - 1 here: one more comparison for the last element
      const uint32_t m = run[at(cnt[r])];
      cnt[r] += (int)(m < v[r]) | ((int)before & (int)(m == v[r]));
      pos[r] += cnt[r];
    }
  }
#pragma unroll
  for (int r = 0; r < E; ++r) dst[pos[r]] = v[r];
}

// Grid: as k_sort_occ (F workgroups per batch; launches of 8 or more batches keep a batch's workgroups on one XCD).
// starts: null, or u32 [n_batches][F][starts_ld]: for every sort field of at most RADIX_D index bits the first list position of
// each local index (entries [0, rows]; [rows] = number of valid occurrences) -- the run table of the small-vocabulary fields.
__global__ __launch_bounds__(RADIX_THREADS) void k_sort_radix(SortArgs a, uint32_t *starts, int32_t starts_ld) {
  extern __shared__ __attribute__((aligned(16))) uint32_t rsm[];
  int j, f;
  if (a.n_batches >= 8) {
    if (!xcd_unit(a.n_batches, a.F, j, f)) return;
  } else {
    j = blockIdx.x / a.F;
    f = blockIdx.x - j * a.F;
  }
  const int32_t *idx = a.idx;
  uint32_t *out = a.sorted + (size_t)f * a.Bp;
  if (j > 0 || a.pool_stride != 0) {
    idx += (size_t)((a.pool_first + j) % a.n_pool) * a.pool_stride;
    out += (size_t)j * a.sorted_stride;
  }
  radix_field<false>(a, f, idx, out, rsm, starts ? starts + ((size_t)j * a.F + f) * starts_ld : nullptr);
}
