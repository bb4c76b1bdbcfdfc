// fmx_list_online.hip -- k_fm_list_online: the pure FM's online LIST loop (predict the positive's rank among its negatives, then
// one list step on that list) in one workgroup (fmx_fm_list_online_run; the checks are list_online_call in fmx_list.inc, which
// reaches this unit through list_online_launch, fmx_host.h).  The prefetch of the next list's rows and the forward from registers
// are the pieces of fmx_walk.inc the other walkers use; the gather through LDS-held offsets and the run sums are this kernel's own.

#include "fmx_host.h"

namespace {

#include "fmx_walk.inc"

struct ListOnlineArgs {
  WalkTable t;         // idx, xv: [N G, F], row G i the positive of list i, rows G i + 1 .. G i + G - 1 its negatives.  bias: read once,
                       // never written -- a list step leaves the bias and its state alone (fmx_list.inc)
  uint8_t *rank;       // [N] negatives of list i whose logit is >= the positive's, BEFORE the list's update
  float *logit;        // [N G] or null
  float *loss;         // [N] or null
  int32_t G;
};

// the terms one occurrence adds to its run's sums, as update_body carries them for the pure FM: cV, and the scalars (cA, cw)
struct AW {
  float A, w;
};
__device__ __forceinline__ AW operator+(AW a, AW b) { return {a.A + b.A, a.w + b.w}; }
template <>
__device__ __forceinline__ AW no_terms<AW>() { return {0.f, 0.f}; }
struct Terms {
  float4 V;
  AW S;
};
__device__ __forceinline__ Terms operator+(Terms a, Terms b) { return {a.V + b.V, a.S + b.S}; }
template <>
__device__ __forceinline__ Terms no_terms<Terms>() { return {splat(0.f), {0.f, 0.f}}; }

// ------------------------------------------------------------------------------------------------------------
// k_fm_list_online: k_fm_online for lists (the sampled-softmax loss of fmx_list.inc)
// ------------------------------------------------------------------------------------------------------------
// One workgroup of G waves walks N lists; wave j owns row j of the current list (a single wave cannot hold a list: 16 rows x NP
// RowRegs).  Per list every wave gathers its row's table rows (sc1 loads: the previous list may have written them; the next list's
// indices and values are requested behind them) and evaluates its logit with k_fm_online's forward arithmetic, leaves the logit,
// S and the row's (index, value) per field in LDS; after the barrier every wave evaluates the list loss from the G logits
// (list_loss_dz_of: the operands and the order of list_loss_dz) -- lane j the dz of position j, so a wave reads any member's dz by a
// lane read -- and the fit follows field by field: the occurrences of a field that name the same valid row are ONE run, its head
// the lowest list position, whose wave still holds the row in registers; the head adds the members' terms in k_fm_update's order
// (PlainSum, or RunSum where a run of the wave spans three lane groups) and applies one update_row.  s_waitcnt vmcnt(0) and a
// barrier close the list: the stores are acknowledged before any wave requests the next list's rows (the same-CU visibility
// k_fm_online and k_online_mlp rely on).  The table ends bit-identical to N calls of fmx_fm_list_step with B_lists = 1, inv_b = 1;
// the bias is read once and never written.
// WAVES: the launch bound's class, 8 (G <= 8: 256 registers per wave) or 16 (128 registers per wave).  At 16 waves the rows of the
// FTRL and moments layouts do not fit beside the walk, so there (LATE) the gather requests what the forward reads -- V and w, the
// weights layout's part of the row -- and the fit requests a field's whole row again right before it counts the field's run: the
// bits the gather would have loaded (within a list a row is written by its run's head alone), an L2 hit under the count.
template <int LPR, int LAYOUT, int RULE, int NP, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_fm_list_online(ListOnlineArgs la) {
  const WalkTable &a = la.t;
  constexpr bool LATE = WAVES > 8 && LAYOUT != FMX_LAYOUT_WEIGHTS;
  constexpr int SLOTS = WAVE / LPR, MAXF = NP * SLOTS, MAXG = 16;
  constexpr int kp = LPR * 4;
  __shared__ float z_lds[MAXG];
  __shared__ float S_lds[MAXG][kp];
  __shared__ uint32_t li_lds[MAXG][MAXF];  // the row of field f that list position j names, SENT where it is out of range
  __shared__ float x_lds[MAXG][MAXF];
  __shared__ int64_t foff_lds[MAXF + 1];  // the fields' first rows, read where a row's address is formed instead of held in registers
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // (w: wave-uniform, in a scalar register)
  const int slot = lane / LPR, q = lane % LPR;
  const int G = la.G;
  const float bias_w = bias_weight<LAYOUT>(a.bias[0], LAYOUT != FMX_LAYOUT_WEIGHTS ? a.bias[1] : 0.f, a.h);
  bool live[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) live[p] = p * SLOTS + slot < a.F;
  for (int f = threadIdx.x; f <= MAXF; f += blockDim.x) foff_lds[f] = a.foff[f < a.F ? f : a.F];
  __syncthreads();
  // this wave's row of the next list
  const WalkX xs = walk_x(a);
  WalkInputs<1, NP> next;
  auto fetch_inputs = [&](int i) { walk_fetch<LPR>(next, a, xs, live, slot, i < a.N, [&](int) { return (size_t)G * i + w; }, [] {}); };
  fetch_inputs(0);
  bool bad = false;
  for (int i = 0; i < a.N; ++i) {
    uint32_t li[NP];
    float x[NP];
    RowRegs row[NP];
    bool ok[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      li[p] = next.li[0][p];
      x[p] = next.x[0][p];
      const int64_t lo = foff_lds[p * SLOTS + slot];
      ok[p] = live[p] && li[p] < (uint32_t)(foff_lds[p * SLOTS + slot + 1] - lo);
      row[p] = load_row_sc1<LATE ? FMX_LAYOUT_WEIGHTS : LAYOUT, RULE>(a.rows + (size_t)(ok[p] ? lo + li[p] : 0) * a.stride, q, kp, a.zoff);
      bad = bad || (live[p] && !ok[p]);
    }
    fetch_inputs(i + 1);  // independent of the weights: in flight while this list is processed
    float4 s;
    float sbi, fo;
    walk_forward<LPR>(row, x, ok, lane, s, sbi, fo);  // this wave's row
    const float z = fo + sbi + bias_w;
    if (lane == 0) z_lds[w] = z;
    if (lane < LPR) *reinterpret_cast<float4 *>(&S_lds[w][4 * q]) = s;
    if (q == 0) {
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        li_lds[w][p * SLOTS + slot] = ok[p] ? li[p] : SENT;
        x_lds[w][p * SLOTS + slot] = x[p];
      }
    }
    fmx_hyper_t h = a.h;  // ADAM: list i is step a.h.step + i + 1 (adam_consts, as the host derives them for a launch)
    if (RULE == FMX_RULE_ADAM) {
      adam_consts(a.h.lr, a.h.beta1, a.h.beta2, a.h.step + i + 1, h.lr, h.beta1, h.beta2);
      h.lr = uniform_f(h.lr);  // (the same on every lane: kept in scalar registers)
      h.beta1 = uniform_f(h.beta1);
      h.beta2 = uniform_f(h.beta2);
    }
    __syncthreads();
    // ---- the list loss: lane j evaluates position j (lanes beyond the list repeat position 0 and are not read) ----
    const int pj = lane < G ? lane : 0;
    float loss, dz_all;
    list_loss_dz_of([&](int j) { return z_lds[j]; }, z_lds[pj], pj, G, 1.0f, loss, dz_all);
    const float dz = lane_f(dz_all, w);
    if (w == 0) {
      if (la.logit && lane < G) la.logit[(size_t)G * i + lane] = z_lds[lane];
      if (lane == 0) {
        int r = 0;
        for (int j = 1; j < G; ++j) r += z_lds[j] >= z_lds[0] ? 1 : 0;
        la.rank[i] = (uint8_t)r;
        if (la.loss) la.loss[i] = loss;
      }
    }
    // ---- fit: k_fm_update on the G rows of the list (fmx_fm_list_step with B_lists = 1, inv_b = 1) ----
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int f = p * SLOTS + slot;
      const uint32_t my = ok[p] ? li[p] : SENT;
      float *rp = a.rows + (size_t)(ok[p] ? foff_lds[f] + li[p] : 0) * a.stride;
      RowRegs r = row[p];
      if constexpr (LATE) r = load_row_sc1<LAYOUT, RULE>(rp, q, kp, a.zoff);
      int before = 0, L = 0;  // valid occurrences of the field with a smaller row; members of this row's run
      bool head = ok[p];
      constexpr int U = WAVES <= 8 ? 4 : 2;  // positions whose LDS reads are in flight together (16 waves: the registers allow 2)
      for (int j0 = 0; j0 < G; j0 += U) {    // (a position beyond the list repeats the last one, uncounted)
        uint32_t lj[U];
#pragma unroll
        for (int u = 0; u < U; ++u) lj[u] = li_lds[j0 + u < G ? j0 + u : G - 1][f];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const bool in = j0 + u < G;
          before += in && lj[u] < my ? 1 : 0;
          L += in && lj[u] == my ? 1 : 0;
          head = head && !(in && lj[u] == my && j0 + u < w);
        }
      }
      // the occurrence's terms as update_body forms them (dz_bi == dz_first)
      const float xG = x[p] * dz;
      const float4 ownV = xG * s;
      const AW ownS = {x[p] * xG, x[p] * dz};
      float4 rV = splat(0.f) + ownV;
      AW rS = no_terms<AW>() + ownS;
      if (__ballot(head && L > 1) != 0ull) {  // (wave-uniform) some lane group heads a run of several rows
        // the members behind the head in list order; a member's (row, value, S) are read from LDS one member ahead of their use (AHEAD)
        auto walk = [&](auto rs, auto own, auto term) {
          rs.add(own, head);
          constexpr bool AHEAD = WAVES <= 8;  // (16 waves: no registers for a member in flight)
          auto read = [&](int j, uint32_t &l, float &xx, float4 &S) {
            l = li_lds[j][f];
            xx = x_lds[j][f];
            S = *reinterpret_cast<const float4 *>(&S_lds[j][4 * q]);
          };
          uint32_t ln = 0u;
          float xn = 0.f;
          float4 Sn = splat(0.f);
          if (AHEAD) read(w + 1 < G ? w + 1 : G - 1, ln, xn, Sn);
          for (int j = w + 1; j < G; ++j) {
            if (!AHEAD) read(j, ln, xn, Sn);
            const uint32_t lj = ln;
            const float xj = xn;
            const float4 Sj = Sn;
            if (AHEAD) read(j + 1 < G ? j + 1 : G - 1, ln, xn, Sn);
            rs.add(term(xj, lane_f(dz_all, j), Sj), head && lj == my);
          }
          return rs.g;
        };
        auto all_terms = [](float xj, float dzj, float4 Sj) {
          const float xGj = xj * dzj;
          return Terms{xGj * Sj, AW{xj * xGj, xj * dzj}};
        };
        auto machine = [&](auto zero) {
          RunSum<LPR, decltype(zero)> rs;
          rs.init(before, L);
          return rs;
        };
        const bool wide = head && L > 1 && (before + L - 1) / LPR - before / LPR > 1;  // the run goes over three lane groups or more
        if (__ballot(wide) == 0ull) {  // (wave-uniform) the common case: no run of this wave needs the scan's order
          const Terms r1 = walk(PlainSum<Terms>{no_terms<Terms>()}, Terms{ownV, ownS}, all_terms);
          rV = r1.V;
          rS = r1.S;
        } else if constexpr (WAVES <= 8) {  // one walk for all the sums
          const Terms r1 = walk(machine(no_terms<Terms>()), Terms{ownV, ownS}, all_terms);
          rV = r1.V;
          rS = r1.S;
        } else {  // 128 registers: the vector's walk, then the scalars'
          rV = walk(machine(splat(0.f)), ownV, [](float xj, float dzj, float4 Sj) { return (xj * dzj) * Sj; });
          rS = walk(machine(no_terms<AW>()), ownS, [](float xj, float dzj, float4) { return AW{xj * (xj * dzj), xj * dzj}; });
        }
      }
      if (head) update_row<LAYOUT, RULE>(rp, q, kp, a.zoff, r, rV, splat(rS.A), rS.w, h);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the row stores are acknowledged before any wave loads the next list's rows
    __syncthreads();
  }
  const bool any_bad = __ballot(bad) != 0ull;
  if (lane == 0 && any_bad && a.error) *a.error = 1;
}

template <int LPR, int LAYOUT, int RULE>
void launch_list_online_np(const ListOnlineArgs &a, int np, hipStream_t st) {
  with_walk_np(np, [&](auto NP) {
    if (a.G <= 8) hipLaunchKernelGGL((k_fm_list_online<LPR, LAYOUT, RULE, NP, 8>), dim3(1), dim3(64 * a.G), 0, st, a);
    else hipLaunchKernelGGL((k_fm_list_online<LPR, LAYOUT, RULE, NP, 16>), dim3(1), dim3(64 * a.G), 0, st, a);
  });
}

}  // namespace

namespace fmxd {

int list_online_launch(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const int32_t *idx, const float *xv, int32_t N,
                       int32_t G, uint8_t *rank_out, float *logit_out, float *loss_out, int32_t *error, hipStream_t st) {
  ListOnlineArgs a;
  a.t = walk_table(table, hyper, rule, idx, xv, error, N);
  a.rank = rank_out;
  a.logit = logit_out;
  a.loss = loss_out;
  a.G = G;
  const int np = walk_passes(table);
  with_lpr(table->kp, [&](auto LPR) { with_rule(rule, [&](auto LAYOUT, auto RULE) { launch_list_online_np<LPR, LAYOUT, RULE>(a, np, st); }); });
  return check_launch("k_fm_list_online");
}

}  // namespace fmxd
