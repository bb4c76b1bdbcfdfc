"""list_mlp_f64 for fmx_mlp_list_fit: the same float64 autograd with the log-Q correction and the rank.  The softmax runs on
z - corr; corr is a constant of the objective, so the corrected problem is list_mlp_f64's on base - corr, and the uncorrected logit
the call stores is that problem's logit plus corr (exact to float64 rounding, 1e-16 of the logit).  rank_i: the negatives of list
i whose uncorrected logit is >= its positive's, with `ties`: whether any such comparison is closer than four times the logits'
fp32 noise (a rank the fp32 kernel may legitimately count the other way).
loss_floor: what fp32 may add to the summed loss beyond test_mlp_gpu.close's relative bound.  loss_i = log(s) - (z_0 - m) with
s = sum_j exp(z_j - m) >= 1: the G exps entering s and its G - 1 additions move s by at most (G + 2) u s (u = 2^-24), which log
passes on as (G + 2) u whatever the size of the loss -- at loss_i near 0 (s near 1) that is all of the error -- and the final
subtraction and the ordered sum add u |loss_i| each; the logits' own noise e_j reaches loss_i through d loss_i / d z_j, which
is dz_j / inv_b.  So loss_floor = inv_b sum_i ((G + 2) u (1 + |loss_i|) + 4 sum_j |dz_ij / inv_b| e_ij).  Helper module, not
collected."""
import numpy as np

from list_mlp_f64 import list_mlp_f64


def list_fit_f64(params, k, H, L, bi, base, G, inv_b, corr=None):
    base = np.asarray(base, dtype=np.float64)
    c = np.zeros_like(base) if corr is None else np.asarray(corr, dtype=np.float64)
    r = list_mlp_f64(params, k, H, L, bi, base - c, G, inv_b)
    r["out"] = r["out"] + c
    z = r["out"].reshape(-1, G)
    gap = z[:, 1:] - z[:, :1]
    r["rank"] = (gap >= 0).sum(1)
    noise = r["logit_noise"].reshape(-1, G)
    r["ties"] = (np.abs(gap) <= 4 * (noise[:, 1:] + noise[:, :1])).any(1)
    slope = np.abs(r["dz"].reshape(-1, G)) / inv_b
    r["loss_floor"] = inv_b * float(((G + 2) * 2.0 ** -24 * (1 + np.abs(r["loss_i"])) + 4 * (slope * noise).sum(1)).sum())
    return r
