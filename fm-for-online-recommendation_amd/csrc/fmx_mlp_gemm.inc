// fmx_mlp_gemm.inc -- the relu MLP on top of the bi-interaction vector at mini-batch sizes (BASELINE configs[3]: 3 x 256,
// B = 4096): forward, loss, backward as fp32 MFMA GEMMs.  Included by fmx_kernels.hip inside its anonymous namespace.
//
// Reference: deepfm_adam.py:38-44,79-89 (the network: x_l = relu(W_l x_{l-1} + b_l), logit contribution sum_j x_L[j]),
// deepfm_adam.py:106-119 / nfm_adam.py:105-118 (fit = forward, loss, backward); the reference runs it as nn.Linear + autograd.
//
// One kernel, three operand layouts:
//   forward   H_l   [B, N]  = relu(H_{l-1} [B, K] . W_l^T + b_l)          A K-contiguous, B = W_l [N, K] K-contiguous
//   dgrad     dH_{l-1} [B, K'] = (dH_l [B, N] . W_l [N, K']) * (H_{l-1} > 0)   A K-contiguous, B N-contiguous
//   wgrad     dW_l  [N, K'] = dH_l^T [N, B] . H_{l-1} [B, K']              A M-contiguous, B N-contiguous, split over B
// The bias gradients (column sums of dH_l over the same batch splits) are written next to each split's partial dW_l by
// extra workgroups of the wgrad launch, so one fixed-order reduction finishes both.
// v_mfma_f32_32x32x2_f32: exact f32 products, f32 accumulation in k order -- the same arithmetic as a scalar fmaf chain,
// so results differ from rocBLAS only by summation order (MI355X peak 157 TFLOP/s; these GEMMs are 0.03-0.5 GFLOP each and
// mostly launch/latency bound: a 64 x 64 tile per workgroup gives 256 workgroups at B = 4096, N = 256).
// Block tile 64 x 64 x 128, four waves (2 x 2) of one 32 x 32 accumulator each, operands staged k-major in LDS
// (As[k][m], Bs[k][n]: the MFMA's one-float-per-lane operands are then conflict-free ds_read_b32), global loads of the
// next tile in flight during the MFMAs of the current one, two LDS buffers (139 KB of the CU's 160 KB), one barrier per
// tile.  Measured at 3 x 256, B = 4096 (tools/mlp_section_times.py): 124 us for the section's 10 launches, of which
// ~40 us are launch floor (3.5 us per dependent launch), ~40 us MFMA time (80 TFLOP/s inside the k loops), ~27 us the
// epilogues and ~15 us exposed fetch/stage: with K = 256 a workgroup's pipeline fill and drain cost as much as its MFMAs.

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int G_BM = 64, G_BN = 64, G_BK = 128;  // G_BK: the k depth of the forward / dgrad tiles
constexpr int G_BK_WGRAD = 32;                   // the wgrad's: 35 KB of LDS and 90 VGPRs, so up to four workgroups (16 waves) share a CU -- a CU's
                                                 // load ceiling rises with its wave count (tools/micro/cu_bandwidth.hip); k depth 64: 26.6 us, 32: 23.1 us
// LDS row length: 68 floats where rows are written as 16-byte pieces, 65 where a k-contiguous operand is written transposed
constexpr int g_row(int transposed) { return transposed ? 65 : 68; }
constexpr size_t g_lds_bytes(int bk) { return 2 * (size_t)bk * (68 + 68) * 4; }
constexpr size_t G_LDS_BYTES = g_lds_bytes(G_BK);
enum { EPI_NONE = 0, EPI_BIAS_RELU = 1, EPI_MASK = 2 };

struct GemmArgs {
  const float *A;
  const float *Bm;
  float *C;
  const float *bias;  // EPI_BIAS_RELU: [N]
  const float *mask;  // EPI_MASK: [M, ldmask]; the product is kept where mask > 0
  const float *rowadd;  // EPI_MASK: null, or [M] added to every element of row m before the mask (Hedge: the layer's own
                        // output gradient joins the gradient arriving from the layer above)
  int M, N, K;
  int lda, ldb, ldc, ldmask;
  int k_chunk;               // K range per blockIdx.z (split-K); partial z goes to C + z * c_split_stride
  long long c_split_stride;
  int zero_cols_to;          // columns [N, zero_cols_to) of C are written as zeros (padding of gbi)
  unsigned a_bytes, b_bytes; // extents of A and Bm in memory (buffer descriptors of the 16-byte load path)
  int vec;                   // 16-byte global loads allowed (alignment, leading dimensions and extents checked on the host)
  unsigned long long *stamps = nullptr;  // debug (FMX_MLP_CHAIN=3, k_mlp_wgrad): 8 s_memrealtime stamps per workgroup, else null
};

// 4 consecutive elements along the contiguous axis of an operand, zero-filled outside [0, n_valid).
// VEC (every extent along a contiguous axis, every leading dimension and every base pointer a multiple of 4 floats, checked
// on the host): a group of 4 is entirely inside or entirely outside, so the load is ONE 16-byte buffer load whose offset is
// pushed out of the descriptor's range when the group is outside -- the hardware returns zeros, and the fetch has no
// branches and no waits (a conditional global load compiles to a branch per load, the element-wise form below to one per
// element).
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
template <bool VEC>
__device__ __forceinline__ float4 g_load4(const float *base, __amdgpu_buffer_rsrc_t rsrc, size_t elem_off, int n_valid) {
  if constexpr (VEC) {
    const unsigned off = n_valid >= 4 ? (unsigned)(elem_off * 4) : 0xFFFFFFF0u;
    const u32x4 r = __builtin_amdgcn_raw_buffer_load_b128(rsrc, off, 0, 0);
    return {__uint_as_float(r.x), __uint_as_float(r.y), __uint_as_float(r.z), __uint_as_float(r.w)};
  } else {
    const float *p = base + elem_off;
    float4 v = {0.f, 0.f, 0.f, 0.f};
    if (n_valid > 0) v.x = p[0];
    if (n_valid > 1) v.y = p[1];
    if (n_valid > 2) v.z = p[2];
    if (n_valid > 3) v.w = p[3];
    return v;
  }
}

template <int AT, int BT, int EPI, bool VEC, int BK>
__device__ __forceinline__ void gemm_body(const GemmArgs &a, const int bx, const int by, const int bz) {
  constexpr int G_BK = BK;                                 // shadows the namespace-scope depth inside the body
  constexpr int G_NLD = G_BM * BK / 4 / 256;               // 16-byte loads per thread, operand and tile
  extern __shared__ float g_smem[];
  constexpr int SA = g_row(AT == 0), SB = g_row(BT == 1);
  float *const As = g_smem;                       // [2][G_BK][SA]
  float *const Bs = g_smem + 2 * G_BK * 68;       // [2][G_BK][SB]
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int wm = w >> 1, wn = w & 1;
  const int m0 = by * G_BM, n0 = bx * G_BN;
  const int k_begin = bz * a.k_chunk;
  const int k_end = min(a.K, k_begin + a.k_chunk);
  const int n_tiles = (k_end - k_begin + G_BK - 1) / G_BK;

  float4 ra[G_NLD], rb[G_NLD];
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.A), 0, VEC ? a.a_bytes : 0, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.Bm), 0, VEC ? a.b_bytes : 0, 0x00020000);
  auto fetch = [&](int kt) {
    const int kb = k_begin + kt * G_BK;
#pragma unroll
    for (int i = 0; i < G_NLD; ++i) {
      const int f = t + i * 256;
      if (AT == 0) {  // A[m * lda + k]: 32 threads cover the 128 k of one row
        const int m = f >> 5, k4 = (f & 31) * 4;
        const int gm = m0 + m, gk = kb + k4;
        ra[i] = g_load4<VEC>(a.A, rsA, (size_t)gm * a.lda + gk, gm < a.M ? k_end - gk : 0);
      } else {  // A[k * lda + m]: 16 threads cover 64 m of one k
        const int k = f >> 4, m4 = (f & 15) * 4;
        const int gk = kb + k, gm = m0 + m4;
        ra[i] = g_load4<VEC>(a.A, rsA, (size_t)gk * a.lda + gm, gk < k_end ? a.M - gm : 0);
      }
      if (BT == 1) {  // B[n * ldb + k]
        const int n = f >> 5, k4 = (f & 31) * 4;
        const int gn = n0 + n, gk = kb + k4;
        rb[i] = g_load4<VEC>(a.Bm, rsB, (size_t)gn * a.ldb + gk, gn < a.N ? k_end - gk : 0);
      } else {  // B[k * ldb + n], optionally with a virtual column of ones
        const int k = f >> 4, n4 = (f & 15) * 4;
        const int gk = kb + k, gn = n0 + n4;
        rb[i] = g_load4<VEC>(a.Bm, rsB, (size_t)gk * a.ldb + gn, gk < k_end ? a.N - gn : 0);
      }
    }
  };
  auto stage = [&](int buf, int kt) {
    float *const Ab = As + buf * G_BK * SA, *const Bb = Bs + buf * G_BK * SB;
#pragma unroll
    for (int i = 0; i < G_NLD; ++i) {
      const int f = t + i * 256;
      if (AT == 0) {
        const int m = f >> 5, k4 = (f & 31) * 4;
        Ab[k4 * SA + m] = ra[i].x;
        Ab[(k4 + 1) * SA + m] = ra[i].y;
        Ab[(k4 + 2) * SA + m] = ra[i].z;
        Ab[(k4 + 3) * SA + m] = ra[i].w;
      } else {
        const int k = f >> 4, m4 = (f & 15) * 4;
        *reinterpret_cast<float4 *>(Ab + k * SA + m4) = ra[i];
      }
      if (BT == 1) {
        const int n = f >> 5, k4 = (f & 31) * 4;
        Bb[k4 * SB + n] = rb[i].x;
        Bb[(k4 + 1) * SB + n] = rb[i].y;
        Bb[(k4 + 2) * SB + n] = rb[i].z;
        Bb[(k4 + 3) * SB + n] = rb[i].w;
      } else {
        const int k = f >> 4, n4 = (f & 15) * 4;
        *reinterpret_cast<float4 *>(Bb + k * SB + n4) = rb[i];
      }
    }
  };

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  unsigned long long *const stamps = a.stamps ? a.stamps + (size_t)blockIdx.x * 8 : nullptr;
  if (stamps && t == 0) {
    stamps[0] = __builtin_amdgcn_s_memrealtime();
    stamps[7] = __builtin_amdgcn_s_getreg(20 | (3 << 11));  // XCC_ID
  }
  if (n_tiles > 0) {
    fetch(0);
    stage(0, 0);
  }
  __syncthreads();
  if (stamps && t == 0) stamps[1] = __builtin_amdgcn_s_memrealtime();
  const int am = wm * 32 + (lane & 31), bn = wn * 32 + (lane & 31), kh = lane >> 5;
  for (int kt = 0; kt < n_tiles; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < n_tiles) fetch(kt + 1);
    const float *Ab = As + buf * G_BK * SA + am + kh * SA, *Bb = Bs + buf * G_BK * SB + bn + kh * SB;
    // 16 k per chunk: the 16 LDS reads of the next chunk are issued before the 8 MFMAs of the current one (a rolled
    // read -> wait -> MFMA loop exposes the LDS latency on every MFMA: 13 us instead of 5 for 4096 x 256 x 256).
    // Rows beyond the tile's k range hold zeros, so a short last tile (K = k = 16 in layer 1) just runs fewer chunks.
    const int k_here = min(G_BK, k_end - (k_begin + kt * G_BK));
    const int n_chunks = (k_here + 15) >> 4;
    float av[2][8], bv[2][8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      av[0][j] = Ab[(2 * j) * SA];
      bv[0][j] = Bb[(2 * j) * SB];
    }
    for (int c = 0; c < n_chunks; c += 2) {
      const float *A1 = Ab + (c + 1) * 16 * SA, *B1 = Bb + (c + 1) * 16 * SB;
      if (c + 1 < n_chunks) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          av[1][j] = A1[(2 * j) * SA];
          bv[1][j] = B1[(2 * j) * SB];
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[0][j], bv[0][j], acc, 0, 0, 0);
      if (c + 1 < n_chunks) {
        const float *A2 = Ab + (c + 2) * 16 * SA, *B2 = Bb + (c + 2) * 16 * SB;
        if (c + 2 < n_chunks) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            av[0][j] = A2[(2 * j) * SA];
            bv[0][j] = B2[(2 * j) * SB];
          }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[1][j], bv[1][j], acc, 0, 0, 0);
      }
    }
    if (kt + 1 < n_tiles) stage(buf ^ 1, kt + 1);
    __syncthreads();
    if (stamps && t == 0 && (kt == 0 || kt == 1 || kt == 3 || kt == n_tiles - 1))
      stamps[kt == 0 ? 2 : kt == 1 ? 3 : kt == 3 ? 4 : 5] = __builtin_amdgcn_s_memrealtime();
  }

  // C/D layout of the 32 x 32 accumulator: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
  float *C = a.C + (size_t)bz * a.c_split_stride;
  const int n = n0 + wn * 32 + (lane & 31);
  float bias_n = 0.f;
  if (EPI == EPI_BIAS_RELU && n < a.N) bias_n = a.bias[n];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    if (m >= a.M) continue;
    if (n < a.N) {
      float v = acc[r];
      if (EPI == EPI_BIAS_RELU) v = fmaxf(v + bias_n, 0.f);
      if (EPI == EPI_MASK) v = a.mask[(size_t)m * a.ldmask + n] > 0.f ? (a.rowadd ? v + a.rowadd[m] : v) : 0.f;
      C[(size_t)m * a.ldc + n] = v;
    } else if (n < a.zero_cols_to) {
      C[(size_t)m * a.ldc + n] = 0.f;
    }
  }
  if (stamps && t == 0) stamps[6] = __builtin_amdgcn_s_memrealtime();
}

template <int AT, int BT, int EPI, bool VEC>
__global__ __launch_bounds__(256) void k_mlp_gemm(GemmArgs a) {
  __builtin_amdgcn_s_setprio(3);  // ahead of a side-stream sort's waves (see k_fm_forward)
  gemm_body<AT, BT, EPI, VEC, G_BK>(a, blockIdx.x, blockIdx.y, blockIdx.z);
}

// every layer's weight-gradient product in ONE launch: blockIdx.z runs over the layers' batch splits back to back
struct WgradBatch {
  GemmArgs g[MLP_BIG_MAX_L];
  int z_end[MLP_BIG_MAX_L];  // exclusive prefix of the splits
  int n;
  int bias_col[MLP_BIG_MAX_L];  // column of the partial [M, ldc] that receives the split's column sums of dH_l (= in_l)
  int tx, ty;                   // the tile grid of the largest layer
  unsigned long long *stamps;   // debug, see GemmArgs
};

// column sums of dH_l [rows k_begin..k_end) -> partial z, column bias_col.  Block y covers 64 columns; the four waves take
// rows r = w (mod 4) with 16 loads in flight each, then the four partial sums are added in wave order (fixed order).
__device__ __forceinline__ void wgrad_bias_cols(const GemmArgs &a, int bias_col, int bz, int col_block) {
  __shared__ float part[4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int m = col_block * 64 + lane;
  const int k_begin = bz * a.k_chunk, k_end = min(a.K, k_begin + a.k_chunk);
  float s = 0.f;
  if (m < a.M) {
#pragma unroll 16
    for (int b = k_begin + w; b < k_end; b += 4) s += a.A[(size_t)b * a.lda + m];
  }
  part[w][lane] = s;
  __syncthreads();
  if (w == 0 && m < a.M)
    a.C[(size_t)bz * a.c_split_stride + (size_t)m * a.ldc + bias_col] = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
}

// The launch is ONE-dimensional and XCD-aware.  Workgroups go to the eight XCDs round-robin by their linear index, each
// XCD has its own L2, and the 16 tiles (+ bias blocks) of one (layer, batch split) read the same 256 rows of dH_l and
// H_{l-1}: dealt over the XCDs in grid order they missed L2 87 % of the time (TCC_HIT / TCC_MISS 0.11 M / 0.78 M per launch)
// and the launch moved its 84 MB of operand reads over the fabric, 23 us = 3.6 TB/s.  Here split z lives on XCD z % 8: index
// = 8 * (slot in the XCD) + XCD, slot = (z / 8) * wg_per_split + (tile or bias block).
__global__ __launch_bounds__(256) void k_mlp_wgrad(WgradBatch b) {
  __builtin_amdgcn_s_setprio(3);
  const int id = blockIdx.x, xcd = id & 7, slot = id >> 3;
  const int per = b.tx * b.ty + b.ty;
  const int z = (slot / per) * 8 + xcd, s = slot % per;
  if (z >= b.z_end[b.n - 1]) return;
  int l = 0;
  while (l + 1 < b.n && z >= b.z_end[l]) ++l;
  const GemmArgs &a = b.g[l];
  const int bz = z - (l == 0 ? 0 : b.z_end[l - 1]);
  if (s >= b.tx * b.ty) {  // the bias columns: blocks of 64 columns of dH_l
    if ((s - b.tx * b.ty) * 64 < a.M) wgrad_bias_cols(a, b.bias_col[l], bz, s - b.tx * b.ty);
    return;
  }
  const int bx = s % b.tx, by = s / b.tx;
  if (bx * G_BN >= a.N || by * G_BM >= a.M) return;  // the tile grid is the largest layer's
  GemmArgs g = a;
  g.stamps = b.stamps;
  if (a.vec) gemm_body<1, 0, EPI_NONE, true, G_BK_WGRAD>(g, bx, by, bz);
  else gemm_body<1, 0, EPI_NONE, false, G_BK_WGRAD>(g, bx, by, bz);
}

// ---- loss on (base + row sums of the last activation), dL/dlogit, and dH_L = dz * (H_L > 0).  One wave per sample. ----
struct MlpLossArgs {
  const float *H;     // [B, ldh] last activation
  float *dH;          // [B, ldh]
  const float *base;  // [B] the part of the logit that does not come from the MLP
  const float *y;
  float *out;         // [B] logit (may be null)
  float *dz;          // [B]
  float *loss_b;      // [B]
  int B, hidden, ldh, loss_kind;
  float inv_b;
  float margin;       // k_mlp_pair_loss only (appended: the offsets k_mlp_loss reads do not depend on it)
};

// the row sum of k_mlp_loss and k_mlp_pair_loss: strided per lane, then a fixed butterfly (every lane ends with the same bits)
__device__ __forceinline__ float mlp_row_sum(const float *h, int hidden, int lane) {
  float s = 0.f;
  for (int j = lane; j < hidden; j += 64) s += h[j];
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) s += __shfl_xor(s, m);
  return s;
}

// ---- the pair form (fmx_mlp_pair_section): B = 2 B_pairs rows, row 2 i the positive of pair i, row 2 i + 1 its negative; the
//      loss is pair_loss_dz of d_i = z[2 i] - z[2 i + 1].  ONE wave owns a PAIR: it takes both rows' sums as k_mlp_loss takes
//      one (the same loop, the same butterfly: z has k_mlp_loss's bits), so nothing crosses a wave -- no LDS, no barrier.
//      dz[2 i + 1] is dz[2 i] negated, loss_b[2 i + 1] = +0; no label is read. ----
__global__ __launch_bounds__(256) void k_mlp_pair_loss(MlpLossArgs a) {
  const int lane = threadIdx.x & 63;
  const int b = 2 * (blockIdx.x * 4 + (threadIdx.x >> 6));  // the pair's positive row
  if (b >= a.B) return;                                     // (a.B is even: both rows exist or neither)
  const float *h = a.H + (size_t)b * a.ldh;
  const float z0 = a.base[b] + mlp_row_sum(h, a.hidden, lane);
  const float z1 = a.base[b + 1] + mlp_row_sum(h + a.ldh, a.hidden, lane);
  float loss, dz;
  pair_loss_dz(z0 - z1, a.margin, a.inv_b, loss, dz);
  if (lane == 0) {
    if (a.out) {
      a.out[b] = z0;
      a.out[b + 1] = z1;
    }
    a.dz[b] = dz;
    a.dz[b + 1] = -dz;
    a.loss_b[b] = loss;
    a.loss_b[b + 1] = 0.f;
  }
  float *d = a.dH + (size_t)b * a.ldh;
  for (int j = lane; j < a.hidden; j += 64) {
    d[j] = h[j] > 0.f ? dz : 0.f;
    d[a.ldh + j] = h[a.ldh + j] > 0.f ? -dz : 0.f;
  }
}

__global__ __launch_bounds__(256) void k_mlp_loss(MlpLossArgs a) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= a.B) return;
  const float *h = a.H + (size_t)b * a.ldh;
  float s = 0.f;
  for (int j = lane; j < a.hidden; j += 64) s += h[j];  // fixed order: strided per lane, then a fixed butterfly
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) s += __shfl_xor(s, m);
  const float z = a.base[b] + s;
  float loss, dz;
  bce_loss_dz(a.loss_kind, z, a.y[b], a.inv_b, loss, dz);
  if (lane == 0) {
    if (a.out) a.out[b] = z;
    a.dz[b] = dz;
    a.loss_b[b] = loss;
  }
  float *d = a.dH + (size_t)b * a.ldh;
  for (int j = lane; j < a.hidden; j += 64) d[j] = h[j] > 0.f ? dz : 0.f;
}

// ---- forward only: logit = base + row sum of the last activation; optionally sigmoid(base + row sum) of EVERY layer
//      (what the ONN classes' forward() returns).  One wave per sample. ----
struct MlpOutArgs {
  const float *acts;  // [L][act_stride] activations, rows of `hidden`
  size_t act_stride;
  const float *base;
  float *logit;       // [B] or null
  float *layers;      // [L, B] or null
  int B, hidden, n_layers;
};

__global__ __launch_bounds__(256) void k_mlp_outputs(MlpOutArgs a) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= a.B) return;
  for (int l = a.layers ? 0 : a.n_layers - 1; l < a.n_layers; ++l) {
    const float *h = a.acts + (size_t)l * a.act_stride + (size_t)b * a.hidden;
    float s = 0.f;
    for (int j = lane; j < a.hidden; j += 64) s += h[j];
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) s += __shfl_xor(s, m);
    if (lane == 0) {
      const float z = a.base[b] + s;
      if (a.layers) a.layers[(size_t)l * a.B + b] = sigmoidf_(z);
      if (a.logit && l == a.n_layers - 1) a.logit[b] = z;
    }
  }
}

// ---- Hedge (reference deepfm_onn.py:109-154) at mini-batch sizes: per layer BCELoss(sigmoid(base + row sum of x_l), y),
//      its alpha-weighted output gradient (autograd's clamped form: (p - y) / max(p (1 - p), 1e-12) * p (1 - p)), and the
//      top layer's dH.  One wave per sample. ----
struct MlpHedgeLossArgs {
  const float *acts;  // [L][act_stride]
  size_t act_stride;
  float *dH_top;      // [B, hidden] gradient of the last activation
  const float *base, *y, *alpha;
  float *dzl;         // [L, B] alpha_l * d loss_l / d out_l[b]
  float *loss_lb;     // [L, B] per-sample losses
  int B, hidden, n_layers;
  float inv_b;
};

__global__ __launch_bounds__(256) void k_mlp_hedge_loss(MlpHedgeLossArgs a) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= a.B) return;
  const float yy = a.y[b], base = a.base[b];
  for (int l = 0; l < a.n_layers; ++l) {
    const float *h = a.acts + (size_t)l * a.act_stride + (size_t)b * a.hidden;
    float s = 0.f;
    for (int j = lane; j < a.hidden; j += 64) s += h[j];
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) s += __shfl_xor(s, m);
    const float p = sigmoidf_(base + s);
    const float lp = fmaxf(logf(p), -100.f), l1p = fmaxf(log1pf(-p), -100.f);
    const float pq = p * (1.f - p);
    const float g = a.alpha[l] * ((p - yy) / fmaxf(pq, 1e-12f)) * pq * a.inv_b;
    if (lane == 0) {
      a.loss_lb[(size_t)l * a.B + b] = -(yy * lp + (1.f - yy) * l1p);
      a.dzl[(size_t)l * a.B + b] = g;
    }
    if (l == a.n_layers - 1) {
      float *d = a.dH_top + (size_t)b * a.hidden;
      for (int j = lane; j < a.hidden; j += 64) d[j] = h[j] > 0.f ? g : 0.f;
    }
  }
}

// alpha_i <- max(alpha_i * b^loss_i, s / L), normalised (deepfm_onn.py:147-154); loss_i = mean over the batch, fixed order
struct MlpHedgeAlphaArgs {
  const float *loss_lb;
  float *alpha, *losses_out;
  int B, n_layers;
  float inv_b, hedge_b, hedge_s;
};

__global__ __launch_bounds__(256) void k_mlp_hedge_alpha(MlpHedgeAlphaArgs a) {
  __shared__ float sm[256];
  __shared__ float ls[MLP_BIG_MAX_L];
  for (int l = 0; l < a.n_layers; ++l) {
    const float s = block_sum(a.loss_lb + (size_t)l * a.B, a.B, 1, sm);
    if (threadIdx.x == 0) ls[l] = s * a.inv_b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float al[MLP_BIG_MAX_L], z = 0.f;
    for (int i = 0; i < a.n_layers; ++i) {
      al[i] = fmaxf(a.alpha[i] * powf(a.hedge_b, ls[i]), a.hedge_s / (float)a.n_layers);
      z += al[i];
    }
    for (int i = 0; i < a.n_layers; ++i) {
      a.alpha[i] = al[i] / z;
      if (a.losses_out) a.losses_out[i] = ls[i];
    }
  }
}

// ---- split-K partials -> flat gradients (W_l then b_l per layer, the layout of fmx_mlp_t.params), fixed order over the
//      splits; block (0, 0) also reduces the per-sample losses.  blockIdx.y = layer. ----
// (struct MlpReduceArgs and the reduction itself -- mlp_reduce_block -- live in fmx_common.h: k_fm_update_rider of fmx_update.hip
// carries the same blocks inside the table update's launch)
__global__ __launch_bounds__(256) void k_mlp_reduce(MlpReduceArgs a) { mlp_reduce_block(a, blockIdx.y, blockIdx.x, gridDim.x); }


// ------------------------------------------------------------------------------------------------------------
// k_mlp_chain: forward, loss and the dgrad chain of the whole network for a slab of 16 samples in ONE workgroup
// ------------------------------------------------------------------------------------------------------------
// Everything of the section except the weight gradients is row-local: H_l = relu(H_{l-1} W_l^T + b_l), the loss on the row
// sum of H_L, dH_{l-1} = (dH_l W_l) * (H_{l-1} > 0).  As ten launches (three forward GEMMs, the loss, three dgrad GEMMs, ...)
// the section is launch / fill / drain bound: 64 x 64 tiles at K = 256 spend as long filling and draining as multiplying
// (115 us for 21 us of MFMA work).  Here one workgroup of FOUR waves (one per SIMD) carries 16 samples through every layer
// and back (v_mfma_f32_16x16x4_f32; exact f32 products).
//
// Round 3: the weights go from L2 STRAIGHT INTO THE REGISTERS of the wave that multiplies them.  With 16 rows per workgroup no
// weight is used by more than one wave (wave w owns the output columns 64 w .. 64 w + 63), so the LDS ring of round 2 -- twelve
// loader waves, a 32 KB panel per 0.45 us through ds_write (~80 B/clk) and back through ds_read_b32, one 16-wave barrier per
// panel -- was overhead only: 8.3 us per 256 x 256 layer for 3.7 us of MFMA issue, 5.6 us of it the LDS traffic and the
// barriers alone.  Now a wave keeps CH_D chunks of 16 k (four 16-byte loads per lane each) in flight and there is no barrier
// inside a GEMM:
//   forward  (W_l is [n][k], k contiguous): lane (m, kq) of tile i loads W[n0 + 16 i + m][16 c + 4 kq .. + 3]: ONE load carries
//            the B operands of FOUR k-steps of one tile (the lane's k at step s is 16 c + 4 kq + s);
//   backward (W_l is [k][n], n contiguous): the wave's four tiles are the STRIDED column sets n = 64 w + 4 m + e, e = 0 .. 3, so
//            lane (m, kq) loads W[16 c + 4 kq + s][64 w + 4 m .. + 3]: one load carries the B operands of ONE k-step of all
//            FOUR tiles (whole 128-byte lines, no transposition), and the lane's four outputs of a row are 16 contiguous bytes.
// The activations stay in LDS "quad-major" [k / 4][16 rows][k % 4]: the A operands of a chunk (the lane's row, its four k) are
// one lane-linear ds_read_b128.  The relu masks of the dgrad chain are the sign bits of the forward outputs, which the SAME lane
// produced (16 bits per thread and layer, in LDS).  H_l and dH_l are also
// written to global memory for the weight-gradient launch (k_mlp_wgrad + k_mlp_reduce).  B / 16 workgroups of 256 threads,
// 41 KB of LDS, fixed summation orders (deterministic).
constexpr int CH_R = 16, CH_MAXH = 256, CH_MAXL = 8;
constexpr int CH_D = 6;  // chunks of 16 k a wave keeps in flight (even: the forward requests them in pairs = whole lines)
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct ChainArgs {
  const float *params;  // flat: per layer W_l [H, in_l] then b_l [H]
  const float *bi;      // [B, ld_bi], the first k columns
  const float *base, *y;
  float *acts, *dH;     // [L][act_stride]: H_l and dL/dH_l, rows of H floats
  size_t act_stride;
  float *logit_out;     // [B] or null
  float *dz_out, *loss_b;
  float *gbi_out;       // [B, ld_gbi]
  long long w_off[CH_MAXL], b_off[CH_MAXL];
  int B, k, H, L, ld_bi, ld_gbi, loss_kind;
  float inv_b;
  unsigned long long *stamps;  // debug (FMX_MLP_CHAIN=2): [workgroup][16] s_memrealtime after every phase, else null
  float margin;                // k_mlp_chain<true> only (appended: the offsets the pointwise kernel reads do not depend on it)
};

// LDS: two activation buffers [H / 4][16][4], the row-sum partials [4][16], dL/dlogit [16], the relu bits [L][256 threads]
inline size_t chain_lds_bytes(int H) { return ((size_t)2 * H * CH_R + 4 * CH_R + CH_R) * sizeof(float) + (size_t)CH_MAXL * 4 * CH_MAXH; }

// Is the network one the chain kernel takes?  (hidden = 256: 64 columns per wave; k = 16, 32, 48 or 64; 16-byte weight loads)
inline bool chain_eligible(const fmx_mlp_t *m) {
  return m->hidden == CH_MAXH && m->k % 16 == 0 && m->k >= 16 && m->k <= 64 && m->n_layers <= CH_MAXL && aligned16(m->params);
}

__device__ __forceinline__ f32x4 chain_ld16(__amdgpu_buffer_rsrc_t rs, unsigned voff, unsigned soff) {
  const u32x4 x = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, 0);
  return f32x4{__uint_as_float(x.x), __uint_as_float(x.y), __uint_as_float(x.z), __uint_as_float(x.w)};
}

// forward GEMM of the slab: acc[i] (tile i = the STRIDED columns 64 w + 4 m + i, m = 0 .. 15, as in the dgrad: a lane's four
// outputs of a row are then 16 contiguous bytes for the epilogue's stores) = in[16, K] . W^T, W [256][K] row-major (k
// contiguous), K = 16 NCH.  in: LDS quad-major.
// The B operand of the MFMA wants lane (m, kq) to hold W[row 64 w + 4 m + i][16 c + 4 kq .. + 3].  REQUESTED in that shape (lanes
// m = 0 .. 15 of a 16-lane group on sixteen different rows) a load moves 16 bytes per clock: the texture addresser takes a
// QUAD of lanes per clock and wants its 64 bytes contiguous (tools/micro/l2_shapes.hip: 38 GB/s per CU for that shape and for
// 8 rows x 128 bytes with the lanes of a quad on different rows, 77 with two lanes contiguous, 151 with four -- the same
// 16 rows x 64 bytes, lane L on row L / 4, piece L % 4 -- as for whole lines or 1 KB contiguous).  So the lanes request the
// chunk in THAT order and the registers are put in operand order by one lane permutation each (ds_bpermute_b32: lane
// 16 kq + m takes lane 4 m + kq; the LDS crossbar, no memory), one chunk ahead of the MFMAs that use them.  Measured per
// 256 x 256 layer: 9.4 us requested in operand shape, 10.0 us as whole lines with a DPP exchange of one lane bit (8 rows x 128
// bytes, a quad on four rows: no better), 6.3 us for the dgrad's requests (wrong results: the floor of this form).
template <int NCH>
__device__ __forceinline__ void chain_fwd(const float *W, const float *Ain, f32x4 (&acc)[4], int w, int lane) {
  constexpr int K = 16 * NCH;
  const int m = lane & 15, kq = lane >> 4;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(W), 0, CH_MAXH * K * 4, 0x00020000);
  unsigned voff[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) voff[i] = (unsigned)(((64 * w + 4 * (lane >> 2) + i) * K + 4 * (lane & 3)) * 4);
  const int from = (4 * m + kq) * 4;  // ds_bpermute: byte address of the source lane
  f32x4 b[NCH][4];
  // a chunk is 64 bytes of a row: the two chunks of a 128-byte line are requested back to back
#pragma unroll
  for (int c = 0; c < CH_D && c < NCH; c += 2) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      b[c][i] = chain_ld16(rs, voff[i] + 64 * c, 0);
      if (c + 1 < NCH) b[c + 1][i] = chain_ld16(rs, voff[i] + 64 * (c + 1), 0);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  const f32x4 *ap = reinterpret_cast<const f32x4 *>(Ain) + lane;
  f32x4 a_cur = ap[0];
  f32x4 t_cur[4];  // the current chunk in operand order
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) t_cur[i][j] = __int_as_float(__builtin_amdgcn_ds_bpermute(from, __float_as_int(b[0][i][j])));
  // The scheduling barriers keep the requests where they are written: left alone, the compiler sinks every load to just
  // before its first use (three or four in flight instead of 4 CH_D: the L2 latency exposed at every chunk).
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    f32x4 a_nxt = a_cur;
    if (c + 1 < NCH) a_nxt = ap[(c + 1) * 64];
    if ((c & 1) == 0 && c + CH_D < NCH) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        b[c + CH_D][i] = chain_ld16(rs, voff[i] + 64 * (c + CH_D), 0);
        if (c + CH_D + 1 < NCH) b[c + CH_D + 1][i] = chain_ld16(rs, voff[i] + 64 * (c + CH_D + 1), 0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    f32x4 t_nxt[4];  // the next chunk's permutation, among this chunk's MFMAs
#pragma unroll
    for (int i = 0; i < 4; ++i) t_nxt[i] = t_cur[i];
    if (c + 1 < NCH) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) t_nxt[i][j] = __int_as_float(__builtin_amdgcn_ds_bpermute(from, __float_as_int(b[c + 1][i][j])));
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur[s], t_cur[i][s], acc[i], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 4; ++i) t_cur[i] = t_nxt[i];
    a_cur = a_nxt;
  }
}

// dgrad GEMM of the slab: acc[e] (tile e = columns 64 w + 4 m + e, m = 0 .. 15) = in[16, K] . W, W [K][256] row-major, K = 16 NCH
template <int NCH>
__device__ __forceinline__ void chain_bwd(const float *W, const float *Ain, f32x4 (&acc)[4], int w, int lane) {
  constexpr int N = CH_MAXH;
  const int m = lane & 15, kq = lane >> 4;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(W), 0, 16 * NCH * N * 4, 0x00020000);
  const unsigned voff = (unsigned)(((4 * kq) * N + 64 * w + 4 * m) * 4);
  f32x4 b[NCH][4];  // [chunk][k-step s], the components are the tiles e
#pragma unroll
  for (int c = 0; c < CH_D && c < NCH; ++c) {
#pragma unroll
    for (int s = 0; s < 4; ++s) b[c][s] = chain_ld16(rs, voff + s * N * 4, c * 16 * N * 4);
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) acc[e] = f32x4{0.f, 0.f, 0.f, 0.f};
  const f32x4 *ap = reinterpret_cast<const f32x4 *>(Ain) + lane;
  f32x4 a_cur = ap[0];
  // The scheduling barriers keep the requests where they are written: left alone, the compiler sinks every load to just
  // before its first use (three or four in flight instead of 4 CH_D: the L2 latency exposed at every chunk).
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    f32x4 a_nxt = a_cur;
    if (c + 1 < NCH) a_nxt = ap[(c + 1) * 64];
    if (c + CH_D < NCH) {
#pragma unroll
      for (int s = 0; s < 4; ++s) b[c + CH_D][s] = chain_ld16(rs, voff + s * N * 4, (c + CH_D) * 16 * N * 4);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur[s], b[c][s][e], acc[e], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    a_cur = a_nxt;
  }
}

// the first layer's dgrad: dL/dbi[16, N] = dH_1[16, 256] . W_1, W_1 [256][N] row-major, N = 16 NT0 (= k <= 64).  Too few
// columns for four waves: the k range is split instead (wave w: k = 64 w .. 64 w + 63, natural 16-column tiles, 4-byte
// loads, all requested up front) and the four partial tiles are summed through LDS in wave order.
template <int NT0>
__device__ __forceinline__ void chain_bwd_first(const float *W, const float *Ain, float *part, int w, int lane) {
  constexpr int N = 16 * NT0;
  const int m = lane & 15, kq = lane >> 4;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(W), 0, CH_MAXH * N * 4, 0x00020000);
  const unsigned voff = (unsigned)(((64 * w + 4 * kq) * N + m) * 4);
  float b[4][4][NT0];
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int i = 0; i < NT0; ++i)
        b[c][s][i] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, voff + ((16 * c + s) * N + 16 * i) * 4, 0, 0));
  f32x4 acc[NT0];
#pragma unroll
  for (int i = 0; i < NT0; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  const f32x4 *ap = reinterpret_cast<const f32x4 *>(Ain) + lane;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const f32x4 a = ap[(4 * w + c) * 64];
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int i = 0; i < NT0; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b[c][s][i], acc[i], 0, 0, 0);
  }
#pragma unroll
  for (int i = 0; i < NT0; ++i) reinterpret_cast<f32x4 *>(part)[(w * 4 + i) * 64 + lane] = acc[i];
}

// PAIR (fmx_mlp_pair_section): the rows are pairs, row 2 i the positive and row 2 i + 1 the negative, and the loss site evaluates
// pair_loss_dz on z[2 i] - z[2 i + 1] instead of the BCE on a label.  A slab's first row and a.B are even, so a pair lies in one
// slab, on two neighbouring lanes of the t < CH_R threads, valid or not together.  PAIR = false: the pointwise section.
template <bool PAIR>
__global__ __launch_bounds__(256) void k_mlp_chain(ChainArgs a) {
  extern __shared__ __attribute__((aligned(16))) float ch_smem[];
  constexpr int H = CH_MAXH;
  float *A0 = ch_smem, *A1 = A0 + (size_t)H * CH_R;
  float *red = A1 + (size_t)H * CH_R;                 // [4][16] row-sum partials of the waves
  float *dzs = red + 4 * CH_R;                        // [16] dL/dlogit of the rows
  unsigned *msk = reinterpret_cast<unsigned *>(dzs + CH_R);  // [L][256]: per thread, bit 4 i + r = (H_l > 0) of its outputs
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int m = lane & 15, kq = lane >> 4;
  const int b0 = blockIdx.x * CH_R;
  int n_stamp = 0;
  auto stamp = [&]() {
    if (a.stamps && threadIdx.x == 0) a.stamps[(size_t)blockIdx.x * 16 + n_stamp] = __builtin_amdgcn_s_memrealtime();
    ++n_stamp;
  };
  stamp();
  // ---- the slab of bi, quad-major: element (row, k) at (k / 4) * 64 + row * 4 + k % 4 ----
  {
    const int r = t >> 4;
    for (int kk = t & 15; kk < a.k; kk += 16) A0[(kk >> 2) * 64 + r * 4 + (kk & 3)] = b0 + r < a.B ? a.bi[(size_t)(b0 + r) * a.ld_bi + kk] : 0.f;
  }
  __syncthreads();
  float *Ain = A0, *Aout = A1;
  f32x4 acc[4];
  float psum[4] = {0.f, 0.f, 0.f, 0.f};
  // ---- forward ----
  for (int l = 0; l < a.L; ++l) {
    const float *W = a.params + a.w_off[l], *bias = a.params + a.b_off[l];
    // the bias of this lane's columns 64 w + 4 m .. + 3, requested before the GEMM: behind it the load latency would be exposed
    const f32x4 bn4 = *reinterpret_cast<const f32x4 *>(bias + 64 * w + 4 * m);
    if (l > 0) chain_fwd<H / 16>(W, Ain, acc, w, lane);
    else if (a.k == 16) chain_fwd<1>(W, Ain, acc, w, lane);
    else if (a.k == 32) chain_fwd<2>(W, Ain, acc, w, lane);
    else if (a.k == 48) chain_fwd<3>(W, Ain, acc, w, lane);
    else chain_fwd<4>(W, Ain, acc, w, lane);
    float *act = a.acts + (size_t)l * a.act_stride;
    const bool last = l == a.L - 1;
    unsigned bits = 0;  // bit 4 i + r: (H_l > 0) at row 4 kq + r, column 64 w + 4 m + i -- the dgrad of layer l + 1 has the same lane there
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 4 * kq + r;
      f32x4 v;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        v[i] = fmaxf(acc[i][r] + bn4[i], 0.f);
        if (v[i] > 0.f) bits |= 1u << (4 * i + r);
        if (last) psum[r] += v[i];  // tiles in order
      }
      *reinterpret_cast<f32x4 *>(Aout + (16 * w + m) * 64 + row * 4) = v;
      if (b0 + row < a.B) __builtin_nontemporal_store(v, reinterpret_cast<f32x4 *>(act + (size_t)(b0 + row) * H + 64 * w + 4 * m));
    }
    msk[l * 256 + t] = bits;  // read back by this thread only
    __syncthreads();
    float *tmp = Ain;
    Ain = Aout;
    Aout = tmp;
    stamp();
  }
  // ---- loss on base + row sum of H_L: lanes of a row group (same kq), then the four waves, in a fixed order ----
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float s = psum[r];
    s += xor_lane_f<1>(s, lane);
    s += xor_lane_f<2>(s, lane);
    s += xor_lane_f<4>(s, lane);
    s += xor_lane_f<8>(s, lane);
    if (m == 0) red[w * CH_R + 4 * kq + r] = s;
  }
  __syncthreads();
  if (t < CH_R) {
    const int b = b0 + t;
    float dz = 0.f;
    if constexpr (PAIR) {
      const bool ok = b < a.B;
      const float s = ((red[t] + red[CH_R + t]) + red[2 * CH_R + t]) + red[3 * CH_R + t];
      const float z = (ok ? a.base[b] : 0.f) + s;
      const float zo = xor_lane_f<1>(z, lane);  // the partner's logit: taken by all sixteen lanes, in front of the branch on ok
      const bool pos = (t & 1) == 0;
      float loss, g;
      pair_loss_dz(pos ? z - zo : zo - z, a.margin, a.inv_b, loss, g);  // both lanes: the same operands, the same bits
      if (ok) {
        dz = pos ? g : -g;
        if (a.logit_out) a.logit_out[b] = z;
        a.dz_out[b] = dz;
        a.loss_b[b] = pos ? loss : 0.f;
      }
    } else if (b < a.B) {
      const float s = ((red[t] + red[CH_R + t]) + red[2 * CH_R + t]) + red[3 * CH_R + t];
      const float z = a.base[b] + s;
      float loss;
      bce_loss_dz(a.loss_kind, z, a.y[b], a.inv_b, loss, dz);
      if (a.logit_out) a.logit_out[b] = z;
      a.dz_out[b] = dz;
      a.loss_b[b] = loss;
    }
    dzs[t] = dz;
  }
  __syncthreads();
  {  // dH_L = dz * (H_L > 0): quad-major for the first dgrad, row-major in memory for the weight gradients
    float *dh = a.dH + (size_t)(a.L - 1) * a.act_stride;
#pragma unroll
    for (int it = 0; it < H * CH_R / 4 / 256; ++it) {
      const int idx4 = t + 256 * it, q = idx4 >> 4, row = idx4 & 15;
      const f32x4 h = reinterpret_cast<const f32x4 *>(Ain)[idx4];
      const float dz = dzs[row];
      const f32x4 v = {h[0] > 0.f ? dz : 0.f, h[1] > 0.f ? dz : 0.f, h[2] > 0.f ? dz : 0.f, h[3] > 0.f ? dz : 0.f};
      reinterpret_cast<f32x4 *>(Aout)[idx4] = v;
      if (b0 + row < a.B) __builtin_nontemporal_store(v, reinterpret_cast<f32x4 *>(dh + (size_t)(b0 + row) * H + 4 * q));
    }
  }
  __syncthreads();
  {
    float *tmp = Ain;
    Ain = Aout;
    Aout = tmp;
  }
  stamp();
  // ---- dgrad chain ----
  for (int l = a.L - 1; l >= 1; --l) {
    const float *W = a.params + a.w_off[l];
    const unsigned mb = msk[(l - 1) * 256 + t];  // (H_{l-1} > 0) of this lane's outputs, from the forward pass
    chain_bwd<H / 16>(W, Ain, acc, w, lane);
    float *dh = a.dH + (size_t)(l - 1) * a.act_stride;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 4 * kq + r;
      const bool ok = b0 + row < a.B;
      f32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = ok && ((mb >> (4 * e + r)) & 1u) ? acc[e][r] : 0.f;
      *reinterpret_cast<f32x4 *>(Aout + (16 * w + m) * 64 + row * 4) = v;
      if (ok) __builtin_nontemporal_store(v, reinterpret_cast<f32x4 *>(dh + (size_t)(b0 + row) * H + 64 * w + 4 * m));
    }
    __syncthreads();
    float *tmp = Ain;
    Ain = Aout;
    Aout = tmp;
    stamp();
  }
  {  // the first layer: dL/dbi = dH_1 . W_1
    const float *W = a.params + a.w_off[0];
    const int nt0 = a.k >> 4;
    if (nt0 == 1) chain_bwd_first<1>(W, Ain, Aout, w, lane);
    else if (nt0 == 2) chain_bwd_first<2>(W, Ain, Aout, w, lane);
    else if (nt0 == 3) chain_bwd_first<3>(W, Ain, Aout, w, lane);
    else chain_bwd_first<4>(W, Ain, Aout, w, lane);
    __syncthreads();
    for (int i = 0; i < nt0; ++i) {  // thread t: component r = t / 64 of lane t % 64's accumulator; the waves in order
      const int r = w, row = 4 * kq + r, n = 16 * i + m;
      const float s = ((Aout[((0 * 4 + i) * 64 + lane) * 4 + r] + Aout[((1 * 4 + i) * 64 + lane) * 4 + r]) + Aout[((2 * 4 + i) * 64 + lane) * 4 + r]) +
                      Aout[((3 * 4 + i) * 64 + lane) * 4 + r];
      if (b0 + row < a.B) a.gbi_out[(size_t)(b0 + row) * a.ld_gbi + n] = s;
    }
    for (int e = t; e < CH_R * (a.ld_gbi - a.k); e += 256) {  // the padding columns of gbi
      const int row = e / (a.ld_gbi - a.k), c = a.k + e % (a.ld_gbi - a.k);
      if (b0 + row < a.B) a.gbi_out[(size_t)(b0 + row) * a.ld_gbi + c] = 0.f;
    }
  }
  stamp();
}

// ------------------------------------------------------------------------------------------------------------
// k_mlp_wgrad_stream: every layer's dW_l | db_l with the operands streamed from L2 straight into registers
// ------------------------------------------------------------------------------------------------------------
// dW_l [H, in] = dH_l^T [H, B] . H_{l-1} [B, in]: the reduction runs over the BATCH, and both operands lie in memory with the
// batch as the row index and the other dimension contiguous -- the dgrad's situation on both sides (k_mlp_chain): with the
// 16 x 16 x 4 MFMA's tiles STRIDED (A-tile e = the rows n0 + 4 i + e of dW, B-tile e' = the columns k0 + 4 j + e') lane
// (m, kq) needs dH[b + kq][n0 + 4 m .. + 3] and H[b + kq][k0 + 4 m .. + 3]: ONE 16-byte load per operand and step of 4 batch
// rows feeds the 16 MFMAs of a 64 x 64 block (16 accumulators per wave), whole lines, a quad of lanes contiguous.  No LDS
// staging, no barrier in the loop: a wave keeps WS_D steps in flight.  A workgroup = one 64 x 64 block of one layer over one
// batch split; its four waves take a quarter of the split's rows each and add their blocks through LDS in wave order at the
// end (fixed order: deterministic); the bias gradient is the column sum of the A operand (four adds per step), written by
// the workgroups of block column 0.  Layers narrower than 64 columns (the first: in = k) use natural 16-column B tiles with
// 4-byte loads and, a quarter of the MFMAs per step, four times the splits: as few workgroups as long as the others they
// doubled up on 32 CUs and made those the last to finish (13.1 against 10.3 us, tools/mlp_wgrad_stamps.py).
// One-dimensional XCD-aware launch as k_mlp_wgrad: the blocks of one (layer, split) read the same rows.
// Replaces k_mlp_wgrad (64 x 64 x 32 tiles staged through LDS, one barrier per tile: 1.7 us per tile for 0.43 us of MFMA --
// each tile's loads waited for inside the tile, tools/mlp_wgrad_stamps.py; 23.1 us per launch whatever the L2 hit rate)
// wherever the 16-byte path applies; the old kernel stays as the fallback for odd shapes.
constexpr int WS_D = 8;  // steps of 4 batch rows (two 16-byte loads per lane) in flight per wave
struct WgradLayer {
  const float *dH;   // [B, lda]
  const float *Hp;   // [B, ldb]
  float *P;          // partials [n_split][M][ldp]: columns 0 .. N - 1 dW, column N db
  long long split_stride;
  int M, N, lda, ldb, ldp;
  int tiles_m, tiles_n;  // 64 x 64 blocks
  int rows_per_split;    // a multiple of 16
};
struct WgradStream {
  WgradLayer g[MLP_BIG_MAX_L];
  int z_end[MLP_BIG_MAX_L];  // exclusive prefix of the layers' splits
  int n, per;                // layers; workgroup slots per split (the largest layer's blocks)
  int B;
  unsigned long long *stamps;  // debug (FMX_MLP_CHAIN=3): 8 s_memrealtime stamps per workgroup, else null
};

// NB = 4: B-tiles strided over 64 columns (16-byte loads); NB = 1 .. 3: NB natural 16-column tiles (4-byte loads), N = 16 NB
template <int NB>
__device__ __forceinline__ void wgrad_stream_body(const WgradLayer &a, int bi, int bj, int bz, int B, int rps, float *lds, unsigned long long *stamps) {
  constexpr bool WIDE = NB == 4;
  const int t = threadIdx.x, lane = t & 63, m = lane & 15, kq = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);  // wave-uniform for the compiler too: the buffer descriptors below depend on it
  const int n0 = bi * 64, k0 = bj * 64;
  // this wave's rows: a quarter of the split
  const int q = rps >> 2;
  const int b_lo = bz * rps + w * q;
  int rows = min(B, bz * rps + rps) - b_lo;
  rows = rows < 0 ? 0 : rows > q ? q : rows;
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.dH) + (size_t)b_lo * a.lda, 0, rows * a.lda * 4, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.Hp) + (size_t)b_lo * a.ldb, 0, rows * a.ldb * 4, 0x00020000);
  const bool okA = n0 + 4 * m < a.M;
  unsigned offA = (unsigned)((kq * a.lda + n0 + 4 * m) * 4), offB;
  bool okB[NB];
  if (WIDE) {
    okB[0] = k0 + 4 * m < a.N;
    offB = (unsigned)((kq * a.ldb + k0 + 4 * m) * 4);
  } else {
#pragma unroll
    for (int j = 0; j < NB; ++j) okB[j] = 16 * j + m < a.N;
    offB = (unsigned)((kq * a.ldb + m) * 4);
  }
  const unsigned stepA = (unsigned)(4 * a.lda * 4), stepB = (unsigned)(4 * a.ldb * 4);
  f32x4 ra[WS_D];
  f32x4 rb[WS_D];  // WIDE: the four B-tiles' operands; else component j = tile j
  auto issue = [&](int u) {
    const u32x4 x = __builtin_amdgcn_raw_buffer_load_b128(rsA, okA ? offA : 0xFFFFFFF0u, 0, 0);
    ra[u] = f32x4{__uint_as_float(x.x), __uint_as_float(x.y), __uint_as_float(x.z), __uint_as_float(x.w)};
    if (WIDE) {
      const u32x4 y = __builtin_amdgcn_raw_buffer_load_b128(rsB, okB[0] ? offB : 0xFFFFFFF0u, 0, 0);
      rb[u] = f32x4{__uint_as_float(y.x), __uint_as_float(y.y), __uint_as_float(y.z), __uint_as_float(y.w)};
    } else {
      rb[u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < NB; ++j) rb[u][j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsB, okB[j] ? offB + 64 * j : 0xFFFFFFF0u, 0, 0));
    }
    offA += stepA;
    offB += stepB;
  };
  f32x4 acc[4][NB];
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int j = 0; j < NB; ++j) acc[e][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 bsum = {0.f, 0.f, 0.f, 0.f};
  if (stamps && t == 0) {
    stamps[0] = __builtin_amdgcn_s_memrealtime();
    stamps[7] = __builtin_amdgcn_s_getreg(20 | (3 << 11)) | (__builtin_amdgcn_s_getreg(4 | (31 << 11)) << 8);  // XCC_ID, HW_ID
  }
#pragma unroll
  for (int u = 0; u < WS_D; ++u) issue(u);
  __builtin_amdgcn_sched_barrier(0);
  const int n_steps = (q + 3) >> 2;
  for (int s0 = 0; s0 < n_steps; s0 += WS_D) {  // steps beyond the wave's rows load zeros (the descriptor ends with the rows)
#pragma unroll
    for (int u = 0; u < WS_D; ++u) {
      const f32x4 av = ra[u], bv = rb[u];
#pragma unroll
      for (int j = 0; j < NB; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], bv[j], acc[e][j], 0, 0, 0);
      {  // the bias sums belong to THIS step: instruction selection is free to place a plain add anywhere after its load, and
         // placed the adds of five later slots here, each with its own wait (vmcnt 14 -> 5: three steps in flight instead of eight)
        f32x4 av_here = av;
        asm volatile("" : "+v"(av_here));
        bsum += av_here;
      }
      issue(u);
      // the requests stay HERE: a scheduling barrier alone pins the machine scheduler, not the passes before it, which sank
      // the loads of five steps behind the MFMAs of the fifth (two or three steps in flight instead of eight)
      asm volatile("" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
    }
    if (stamps && t == 0 && s0 == 0) stamps[1] = __builtin_amdgcn_s_memrealtime();
  }
  if (stamps && t == 0) stamps[2] = __builtin_amdgcn_s_memrealtime();
  // ---- the four waves' blocks added in wave order through LDS, two A-tiles per round (32 KB: a launch that carries other
  //      workgroups beside these must not reserve 64 KB for each of them); in a round wave w sums tile w / 2, rows 2 (w % 2) .. + 1 ----
  f32x4 *const L4 = reinterpret_cast<f32x4 *>(lds);  // [wave][tile of the round][r][lane]
  float *const Lb = lds + 4 * 2 * 4 * 64 * 4;         // [wave][16 m][4 e]
  // bias: this lane's column sums over its rows; the four k-slots of a wave, then the waves, in a fixed order
  if (bj == 0) {
    f32x4 s = bsum;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float v = s[e];
      v += xor_lane_f<16>(v, lane);
      v += xor_lane_f<32>(v, lane);
      s[e] = v;
    }
    if (kq == 0) *reinterpret_cast<f32x4 *>(Lb + (w * 16 + m) * 4) = s;
  }
  float *const P = a.P + (size_t)bz * a.split_stride;
#pragma unroll
  for (int round = 0; round < 2; ++round) {
    if (round) __syncthreads();  // the first round's sums are read
#pragma unroll
    for (int ee = 0; ee < 2; ++ee) {
      const int e = 2 * round + ee;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < NB; ++j) v[j] = acc[e][j][r];
        L4[((w * 2 + ee) * 4 + r) * 64 + lane] = v;
      }
    }
    __syncthreads();
    if (stamps && t == 0 && round == 0) stamps[3] = __builtin_amdgcn_s_memrealtime();
    const int ee = w >> 1, e = 2 * round + ee;
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
      const int r = 2 * (w & 1) + rr;
      const f32x4 v = ((L4[((0 * 2 + ee) * 4 + r) * 64 + lane] + L4[((1 * 2 + ee) * 4 + r) * 64 + lane]) + L4[((2 * 2 + ee) * 4 + r) * 64 + lane]) +
                      L4[((3 * 2 + ee) * 4 + r) * 64 + lane];
      const int n = n0 + 4 * (4 * kq + r) + e;  // the accumulator's row 4 kq + r of A-tile e
      if (n >= a.M) continue;
      if (WIDE) {
        if (k0 + 4 * m < a.N) __builtin_nontemporal_store(v, reinterpret_cast<f32x4 *>(P + (size_t)n * a.ldp + k0 + 4 * m));
      } else {
#pragma unroll
        for (int j = 0; j < NB; ++j)
          if (16 * j + m < a.N) P[(size_t)n * a.ldp + 16 * j + m] = v[j];
      }
    }
  }
  if (bj == 0 && t < 64) {  // db: columns n0 + t
    const int mm = t >> 2, e = t & 3;
    const float v = ((Lb[(0 * 16 + mm) * 4 + e] + Lb[(1 * 16 + mm) * 4 + e]) + Lb[(2 * 16 + mm) * 4 + e]) + Lb[(3 * 16 + mm) * 4 + e];
    if (n0 + t < a.M) P[(size_t)(n0 + t) * a.ldp + a.N] = v;
  }
  if (stamps && t == 0) stamps[4] = __builtin_amdgcn_s_memrealtime();
}

constexpr size_t WS_LDS_BYTES = (size_t)4 * 2 * 4 * 64 * 16 + 4 * 16 * 4 * 4;  // two tiles of the four waves' blocks + their bias sums

__global__ __launch_bounds__(256) void k_mlp_wgrad_stream(WgradStream b) {
  extern __shared__ __attribute__((aligned(16))) float ws_smem[];
  __builtin_amdgcn_s_setprio(3);
  const int id = blockIdx.x, xcd = id & 7, slot = id >> 3;
  const int z = (slot / b.per) * 8 + xcd, s = slot % b.per;
  if (z >= b.z_end[b.n - 1]) return;
  int l = 0;
  while (l + 1 < b.n && z >= b.z_end[l]) ++l;
  const WgradLayer &a = b.g[l];
  if (s >= a.tiles_m * a.tiles_n) return;
  const int bz = z - (l == 0 ? 0 : b.z_end[l - 1]);
  const int bi = s / a.tiles_n, bj = s % a.tiles_n;
  unsigned long long *const st8 = b.stamps ? b.stamps + (size_t)blockIdx.x * 8 : nullptr;
  if (a.N >= 64) wgrad_stream_body<4>(a, bi, bj, bz, b.B, a.rows_per_split, ws_smem, st8);
  else if (a.N > 32) wgrad_stream_body<3>(a, bi, bj, bz, b.B, a.rows_per_split, ws_smem, st8);
  else if (a.N > 16) wgrad_stream_body<2>(a, bi, bj, bz, b.B, a.rows_per_split, ws_smem, st8);
  else wgrad_stream_body<1>(a, bi, bj, bz, b.B, a.rows_per_split, ws_smem, st8);
}

// ---- host side ----
struct MlpBigWs {
  float *acts;  // [L][B, hidden]
  float *dH;    // [L][B, hidden]: dL/dH_l, all kept so that the weight-gradient products run as one launch at the end
  float *loss_b;
  float *dzl, *loss_lb;  // Hedge: [L, B] each
  float *parts[MLP_BIG_MAX_L];
  int ldp[MLP_BIG_MAX_L];
  int n_split;
  size_t bytes;
};

MlpBigWs mlp_big_carve(const fmx_mlp_t *mlp, int B, void *base) {
  MlpBigWs w;
  const size_t H = (size_t)mlp->hidden, L = (size_t)mlp->n_layers;
  const size_t act = align_up((size_t)B * H * 4, 256);
  char *p = static_cast<char *>(base);
  size_t o = 0;
  w.acts = reinterpret_cast<float *>(p + o);
  o += L * act;
  w.dH = reinterpret_cast<float *>(p + o);
  o += L * act;
  w.loss_b = reinterpret_cast<float *>(p + o);
  o += align_up((size_t)B * 4, 256);
  w.dzl = reinterpret_cast<float *>(p + o);
  o += align_up(L * (size_t)B * 4, 256);
  w.loss_lb = reinterpret_cast<float *>(p + o);
  o += align_up(L * (size_t)B * 4, 256);
  w.n_split = (B + 127) / 128;
  for (int l = 0; l < mlp->n_layers; ++l) {
    const int in = l == 0 ? mlp->k : mlp->hidden;
    w.ldp[l] = (in + 1 + 3) / 4 * 4;
    w.parts[l] = reinterpret_cast<float *>(p + o);
    o += align_up((size_t)w.n_split * H * w.ldp[l] * 4, 256);
  }
  w.bytes = o;
  return w;
}

template <int AT, int BT, int EPI, bool VEC>
void launch_gemm_v(const GemmArgs &a, dim3 grid, hipStream_t st) {
  static bool raised = false;  // per instantiation: allow the 139 KB of dynamic LDS
  if (!raised) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_mlp_gemm<AT, BT, EPI, VEC>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)G_LDS_BYTES);
    raised = true;
  }
  hipLaunchKernelGGL((k_mlp_gemm<AT, BT, EPI, VEC>), grid, dim3(256), G_LDS_BYTES, st, a);
}

template <int AT, int BT, int EPI>
void launch_gemm(const GemmArgs &a, int n_split, hipStream_t st) {
  const int n_cols = a.N > a.zero_cols_to ? a.N : a.zero_cols_to;
  const dim3 grid((n_cols + G_BN - 1) / G_BN, (a.M + G_BM - 1) / G_BM, n_split);
  if (a.vec) launch_gemm_v<AT, BT, EPI, true>(a, grid, st);
  else launch_gemm_v<AT, BT, EPI, false>(a, grid, st);
}

// 16-byte loads: base pointers, leading dimensions and the extents along the contiguous axes are multiples of 4 floats
inline bool gemm_vec_ok(const GemmArgs &g, int at, int bt) {
  const int a_extent = at == 0 ? g.K : g.M;
  const int b_extent = bt == 1 ? g.K : g.N;
  return g.a_bytes < 0xFFFFFF00u && g.b_bytes < 0xFFFFFF00u && aligned16(g.A) && aligned16(g.Bm) && g.lda % 4 == 0 && g.ldb % 4 == 0 && a_extent % 4 == 0 && b_extent % 4 == 0 &&
         g.k_chunk % 4 == 0;
}
