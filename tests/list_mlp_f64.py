"""pair_mlp_f64 restated for the list loss: the relu MLP on bi in float64 torch autograd, rows G i .. G i + G - 1 list i with the
positive first, z = base + sum_j x_L[j], loss = inv_b * sum_i CE_i with CE_i = -log softmax(z[G i : G i + G])[0] -- evaluated by
list_f64.list_loss_f64 (the negatives' mass for the positive's derivative), which this module checks its autograd against.  The
rounding noise of every gradient element comes from helpers._mlp_grad_noise and pair_mlp_f64's logit_noise / gbi_noise; a row's
dz depends on every logit of its list, d dz_j / d z_l = inv_b p_j (delta_jl - p_l), so the noise of the list's logits goes into the
row's slope in quadrature.  Helper module, not collected."""
import numpy as np
import torch
import torch.nn.functional as Fn

from helpers import _mlp_grad_noise
from list_f64 import list_loss_f64
from pair_mlp_f64 import U32, gbi_noise, logit_noise


def list_mlp_f64(params, k, H, L, bi, base, G, inv_b):
    """params: the flat layout (W_l [H, in] then b_l [H] per layer); bi [B G, k], base [B G].  -> dict: out [B G] the logits,
    loss_i [B], loss, dz [B G] = dL/dlogit, gbi [B G, k], grads [(dW_l, db_l)], flat, gnoise [(noise dW_l, noise db_l)]; and the
    noise (one standard deviation's worth) of the logits, of dz and of gbi."""
    p = torch.as_tensor(np.asarray(params, dtype=np.float64))
    bi = torch.as_tensor(np.asarray(bi, dtype=np.float64)).requires_grad_(True)
    base = torch.as_tensor(np.asarray(base, dtype=np.float64)).requires_grad_(True)
    N = bi.shape[0]
    assert G >= 2 and N % G == 0 and N == base.shape[0]
    B = N // G
    Ws, bs, off = [], [], 0
    for l in range(L):
        i = k if l == 0 else H
        Ws.append(p[off:off + H * i].view(H, i).clone().requires_grad_(True)); off += H * i
        bs.append(p[off:off + H].clone().requires_grad_(True)); off += H
    xs, x = [bi], bi
    for W, b in zip(Ws, bs):
        x = Fn.relu(x @ W.t() + b)
        xs.append(x)
    out = base + x.sum(1)
    loss_i = -Fn.log_softmax(out.view(B, G), dim=1)[:, 0]
    ls = loss_i.sum() * inv_b
    ls.backward()
    r = dict(out=out.detach().numpy(), loss_i=loss_i.detach().numpy(), loss=float(ls.detach()), dz=base.grad.numpy(), gbi=bi.grad.numpy())
    # the objective is list_loss_f64's: the device's formula in float64, against the autograd of log_softmax
    ref_loss, g = list_loss_f64(r["out"].reshape(B, G))
    np.testing.assert_allclose(ref_loss, r["loss_i"], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose((g * inv_b).reshape(N), r["dz"], rtol=1e-11, atol=1e-15 * inv_b)
    r["grads"] = [(W.grad.numpy(), b.grad.numpy()) for W, b in zip(Ws, bs)]
    r["flat"] = np.concatenate([t.reshape(-1) for pair in r["grads"] for t in pair])
    xs_n, Ws_n, bs_n = [t.detach().numpy() for t in xs], [W.detach().numpy() for W in Ws], [b.detach().numpy() for b in bs]
    e_row = logit_noise(xs_n, Ws_n, bs_n)
    prob = torch.softmax(out.detach().view(B, G), dim=1).numpy()
    hess = inv_b * (prob[:, :, None] * (np.eye(G)[None] - prob[:, None, :]))                                     # [B, j, l]
    e_dz = np.sqrt(((hess * e_row.reshape(B, 1, G)) ** 2).sum(2)).reshape(N)                                     # the list's logit noise in dz_j
    # _mlp_grad_noise multiplies slope by the ROW's logit noise: the factor goes into the slope (as in pair_mlp_f64)
    slope = np.divide(e_dz, e_row, out=np.abs(hess[:, np.arange(G), np.arange(G)]).reshape(N).copy(), where=e_row > 0)
    r["dz_noise"] = 4 * U32 * np.abs(r["dz"]) + e_dz
    r["logit_noise"] = e_row
    r["gbi_noise"] = gbi_noise(xs_n, Ws_n, r["dz"], r["dz_noise"])
    r["gnoise"] = _mlp_grad_noise(xs_n, Ws_n, bs_n, [None] * (L - 1) + [r["dz"]], [None] * (L - 1) + [slope])
    return r
