// fmx_mlp_list.inc -- the listwise (sampled-softmax) loss on the whole network's logit of DeepFM / NFM: k_mlp_list_loss, the
// list counterpart of k_mlp_loss / k_mlp_pair_loss at the loss site between mlp_big_forward and mlp_big_backward, and the section
// around it, fmx_mlp_list_section (fmxd::mlp_list_section_deferred_reduce for fmx_deepfm_list_stream in fmx_kernels.hip).
// Included by fmx_mlp.hip at file scope behind everything else of the unit: it adds code beside the pointwise and the pair
// section and changes none of theirs.  The list section ALWAYS takes the separate-GEMM form (forward x L, this loss kernel,
// dgrad x L, the weight gradients, the reduction), whatever the option "mlp_chain" says: k_mlp_chain has no list mode.
//
// A batch of B_lists lists of G rows is B_lists G rows of bi / base: row G i the positive of list i, rows G i + 1 .. G i + G - 1 its
// negatives (the layout of fmx_fm_list_*).
#include "fmx_host.h"

namespace {

struct MlpListLossArgs {
  const float *H;     // [rows, ldh] last activation
  float *dH;          // [rows, ldh]
  const float *base;  // [rows] the part of the logit that does not come from the MLP
  const float *corr;  // [rows] log Q of every row's item, subtracted in front of the softmax; null: no correction
  float *out;         // [rows] the uncorrected logit (may be null)
  float *dz;          // [rows]
  float *loss_b;      // [rows]: the list's loss in its positive's slot, +0 in its negatives'
  int n_lists, G, hidden, ldh;
  float inv_b;
};

// ONE wave owns a LIST, a workgroup of 256 threads four of them: nothing crosses a wave -- no LDS, no barrier, no atomics.  The
// wave takes the G rows' sums one after the other as k_mlp_loss takes one (mlp_row_sum: every lane ends with the same bits, so
// z_j has k_mlp_loss's), and lane j keeps z_j; the lanes from G on keep z_{G-1} (and its corr), a finite operand whose results are
// never stored.  The only branch in front of a cross-lane read is the wave-uniform exit of a last workgroup's waves without a
// list, and every loop around one runs over j < G, the same count on every lane: all 64 lanes are active at every __shfl, the
// sources 0 .. G - 1 among them.  list_loss_dz_of reads the softmax's operands z_j - corr_j from those lanes in the order
// j = 0 .. G - 1 on every lane.  The logit stored is the uncorrected z_j (the serving score); without corr nothing is subtracted,
// and z - (+0) is z bit for bit, so corr == nullptr and a corr of +0 agree in every bit.
__global__ __launch_bounds__(256) void k_mlp_list_loss(MlpListLossArgs a) {
  const int lane = threadIdx.x & 63;
  const int list = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (list >= a.n_lists) return;  // (wave-uniform: a last workgroup with fewer than four lists)
  const int G = a.G;
  const int b = list * G;         // the list's positive row (n_lists G rows are within int32 and list < n_lists)
  const float *h = a.H + (size_t)b * a.ldh;
  float z = 0.f;
  for (int j = 0; j < G; ++j) {
    const float zj = a.base[b + j] + mlp_row_sum(h + (size_t)j * a.ldh, a.hidden, lane);
    if (lane >= j) z = zj;  // lane j is last written at step j
  }
  const int pos = lane < G ? lane : G - 1;
  float zc = z;  // the softmax's operand
  if (a.corr) zc = z - a.corr[b + pos];
  float loss, dz;
  list_loss_dz_of([&](int j) { return __shfl(zc, j); }, zc, pos, G, a.inv_b, loss, dz);
  if (lane < G) {
    if (a.out) a.out[b + lane] = z;
    a.dz[b + lane] = dz;
    a.loss_b[b + lane] = lane == 0 ? loss : 0.f;
  }
  float *d = a.dH + (size_t)b * a.ldh;
  for (int j = 0; j < G; ++j) {
    const float dzj = __shfl(dz, j);
    const float *hj = h + (size_t)j * a.ldh;
    float *dj = d + (size_t)j * a.ldh;
    for (int c = lane; c < a.hidden; c += 64) dj[c] = hj[c] > 0.f ? dzj : 0.f;
  }
}

}  // namespace

// fmx_mlp_list_section without its last launch (mlp_section_deferred_reduce's contract: `deferred` receives the reduction's
// arguments, null launches it here).  What is refused, in front of any launch: the list's shape, then mlp_big_check, the size of
// the workspace, the null buffers and the leading dimensions
int fmxd::mlp_list_section_deferred_reduce(const fmx_mlp_t *mlp, const float *bi, int32_t ld_bi, const float *base, const float *corr,
                                           int32_t B_lists, int32_t G, float inv_b, void *workspace, int64_t workspace_bytes,
                                           float *logit_out, float *dz_out, float *gbi_out, int32_t ld_gbi, float *grads, float lr_apply,
                                           float *loss_out, hipStream_t st, MlpReduceArgs *deferred, const char *who) {
  if (int rc = mlp_list_shape(B_lists, G, who)) return rc;
  const int32_t B = B_lists * G;
  if (int rc = mlp_big_check(mlp, B, workspace, who)) return rc;
  const int64_t need = (int64_t)mlp_big_carve(mlp, B, nullptr).bytes;
  if (workspace_bytes < need)
    return fail(FMX_ERR_SHAPE, "%s: the MLP workspace holds %lld bytes, fmx_mlp_section_workspace_bytes asks for %lld", who,
                (long long)workspace_bytes, (long long)need);
  if (!bi || !base || !dz_out || !gbi_out || !grads) return fail(FMX_ERR_ARG, "%s: null argument", who);
  if (ld_bi < mlp->k || ld_gbi < mlp->k) return fail(FMX_ERR_SHAPE, "%s: ld_bi / ld_gbi smaller than k", who);
  const MlpBigWs w = mlp_big_carve(mlp, B, workspace);
  const int L = mlp->n_layers, H = mlp->hidden;
  const size_t act = align_up((size_t)B * H * 4, 256) / 4;
  mlp_big_forward(mlp, w, bi, ld_bi, B, st);
  {  // ---- the lists' loss, dL/dlogit, dH_L ----
    MlpListLossArgs a;
    a.H = w.acts + (size_t)(L - 1) * act;
    a.dH = w.dH + (size_t)(L - 1) * act;
    a.base = base;
    a.corr = corr;
    a.out = logit_out;
    a.dz = dz_out;
    a.loss_b = w.loss_b;
    a.n_lists = B_lists;
    a.G = G;
    a.hidden = H;
    a.ldh = H;
    a.inv_b = inv_b;
    hipLaunchKernelGGL(k_mlp_list_loss, dim3((B_lists + 3) / 4), dim3(256), 0, st, a);
  }
  mlp_big_backward(mlp, w, bi, ld_bi, B, nullptr, gbi_out, ld_gbi, grads, lr_apply, loss_out, inv_b, st, false, deferred);
  return check_launch(who);
}

extern "C" int fmx_mlp_list_section(const fmx_mlp_t *mlp, const float *bi, int32_t ld_bi, const float *base, const float *corr,
                                    int32_t B_lists, int32_t G, float inv_b, void *workspace, int64_t workspace_bytes, float *logit_out,
                                    float *dz_out, float *gbi_out, int32_t ld_gbi, float *grads, float lr_apply, const fmx_mlp_opt_t *opt,
                                    float *loss_out, fmx_stream_t stream) {
  const char *who = "fmx_mlp_list_section";
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (!opt)  // the network under SGD by lr_apply, applied in the section's own reduction (fmx_mlp_section)
    return mlp_list_section_deferred_reduce(mlp, bi, ld_bi, base, corr, B_lists, G, inv_b, workspace, workspace_bytes, logit_out, dz_out,
                                            gbi_out, ld_gbi, grads, lr_apply, loss_out, st, nullptr, who);
  // ... or under opt's rule for step t = opt->step + 1 (fmx_mlp_section_opt): the shape first, then opt's own refusals
  if (int rc = mlp_list_shape(B_lists, G, who)) return rc;
  if (int rc = mlp_opt_check(mlp, B_lists * G, workspace, workspace_bytes, grads, opt, 1, who)) return rc;
  MlpReduceArgs red;
  if (int rc = mlp_list_section_deferred_reduce(mlp, bi, ld_bi, base, corr, B_lists, G, inv_b, workspace, workspace_bytes, logit_out, dz_out,
                                                gbi_out, ld_gbi, grads, 0.f, loss_out, st, &red, who))
    return rc;
  mlp_reduce_set_opt(red, *opt, opt->step + 1);
  mlp_launch_reduce(red, st);
  return check_launch(who);
}
