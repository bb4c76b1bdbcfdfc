// fmx_afm_pair_online.hip -- k_afm_pair_online: the attentional FM's online PAIR loop (predict z_pos > z_neg, then fit on that pair)
// in one workgroup (fmx_afm_pair_online_run; the host code that decides between this kernel and the queued pair steps is
// afm_pair_online_call in fmx_afm_pair.inc).  The launch takes k_afm_online's arguments, filled by the same fill_afm_online
// (fmx_afm_device.inc) with y null, and the margin beside them.
//
// The kernel is afm_walk<KP, 2> of fmx_afm_device.inc: k_afm_online's walk (afm_walk<KP, 1>) with two rows in every slot.  The
// prologue, the fetch, the forward and its softmax, pass B, the attention rule, the bias step and the epilogue are the onl_ pieces
// both kernels call; the objective and the run logic of the table update are the walk's two `if constexpr` parts (the walk's own
// comment lists a pair's order of forwards and backwards).  Every float is the one fmx_afm_pair_step_opt gives at B_pairs = 1,
// inv_b = 1 -- the sort of two rows, k_afm_pair<BWD>, k_fm_update_occ, k_afm_reduce_opt over one partial.  One code path for every
// shape; the field sums x w are rewritten with e by each forward, so the LDS carving is afm_online_lds' without a word added and
// the buffer decision is afm_online_buffers' itself (afm_online_form, under this entry point's option).
//
// A unit of its own: the walk calls the device functions of k_afm (stage_params, score_pairs, pair_backward, add_tile, ...), and
// compiled inside fmx_afm.hip, where it shares those template instantiations with the other kernels, every kernel of the same kp
// came out of the compiler with its instructions reordered (tools/isa_diff.py: 55 of 60 listings differed; an empty kernel body, or
// the kernel at the end of the unit, changed nothing about that); here fmx_afm.hip's listings are the parent's, instruction for
// instruction.

#include "fmx_host.h"

namespace {

#define FMX_AFM_SHARED_ONLY
#include "fmx_afm_device.inc"

struct AfmPairOnlArgs {
  AfmOnlArgs o;  // N: the number of PAIRS; idx / xv [2 N, F]; logit [2 N]; loss [N]; y is not read
  float margin;
};

template <int KP>
__global__ __launch_bounds__(AFM_ONL_THREADS) void k_afm_pair_online(AfmPairOnlArgs pa) {
  afm_walk<KP, 2>(pa.o, pa.margin);
}

}  // namespace

namespace fmxd {

int afm_pair_online_buffers(int F, int k, int kp, int t, int attn_rule, bool *moments_in_lds) {
  bool mom = false;
  const int nb = afm_online_form(tune().afm_pair_online_persistent, F, k, kp, t, attn_rule, mom);
  if (moments_in_lds) *moments_in_lds = nb > 0 && mom;
  return nb;
}

int afm_pair_online_launch(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_afm_t *afm, const int32_t *idx,
                           const float *xv, int32_t N_pairs, float margin, float *attn_grad_out, const fmx_mlp_opt_t *opt,
                           float *logit_out, float *loss_out, int32_t *error, int nb, bool moments_in_lds, hipStream_t st) {
  AfmPairOnlArgs pa;
  memset(&pa, 0, sizeof(pa));
  pa.o = fill_afm_online(table, hyper, rule, afm, opt, idx, xv, nullptr, N_pairs, attn_grad_out, logit_out, loss_out, error, nb, moments_in_lds);
  pa.margin = margin;
  return with_kp(table->kp, [&](auto KP) { return launch_afm_walk_k<KP, k_afm_pair_online<KP>>(pa, pa.o, "k_afm_pair_online", st); });
}

}  // namespace fmxd
