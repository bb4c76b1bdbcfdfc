"""helpers.mlp_f64 restated for the pair loss: the relu MLP on bi in float64 torch autograd, rows 2i / 2i + 1 the positive /
negative of pair i, z = base + sum_j x_L[j], d_i = z[2i] - z[2i + 1], loss = inv_b * sum_i -log(sigmoid(d_i) + margin)
(margin 0: the stable softplus form).  The rounding noise of every gradient element comes from helpers._mlp_grad_noise, with
the pair loss's slope and the noise of d.  Helper module, not collected."""
import numpy as np
import torch
import torch.nn.functional as Fn

from helpers import _mlp_grad_noise

U32 = 2.0 ** -24


def pair_loss_t(d, margin):
    """-log(sigmoid(d) + margin) per pair, as a float64 torch expression"""
    return -Fn.logsigmoid(d) if margin == 0 else -torch.log(torch.sigmoid(d) + margin)


def logit_noise(xs, Ws, bs):
    """The fp32 rounding noise of every row's logit base + sum_j x_L[j]: _mlp_grad_noise's forward part (each sum's own
    |terms|, the inputs' noise carried through the signed products in quadrature) and its e_out."""
    e = np.zeros_like(xs[0])
    for l, (W, b) in enumerate(zip(Ws, bs)):
        local = U32 * np.sqrt(W.shape[1] + 1) * (np.abs(xs[l]) @ np.abs(W).T + np.abs(b))
        e = (local + np.sqrt((e * e) @ (W * W).T)) * (xs[l + 1] > 0)
    xo = xs[-1]
    return U32 * np.sqrt(xo.shape[1]) * np.abs(xo).sum(1) + np.sqrt((e * e).sum(1))


def gbi_noise(xs, Ws, dz, dz_noise):
    """The fp32 rounding noise of dL/dbi: dz's own noise and every dgrad product's rounding carried down the chain, as
    _mlp_grad_noise carries them (it keeps the weight gradients' noise only)."""
    mask = xs[-1] > 0
    d, e = dz[:, None] * mask, dz_noise[:, None] * mask
    for l in range(len(Ws) - 1, -1, -1):
        W = Ws[l]
        d, e = d @ W, U32 * np.sqrt(W.shape[0]) * (np.abs(d) @ np.abs(W)) + np.sqrt((e * e) @ (W * W))
        if l > 0:
            d, e = d * (xs[l] > 0), e * (xs[l] > 0)
    return e


def pair_mlp_f64(params, k, H, L, bi, base, margin, inv_b):
    """params: the flat layout (W_l [H, in] then b_l [H] per layer); bi [2P, k], base [2P].  -> dict: out [2P] the logits,
    d [P], loss_i [P], loss, dz [2P] = dL/dlogit, gbi [2P, k], grads [(dW_l, db_l)], flat, gnoise [(noise dW_l, noise db_l)];
    and the noise (one standard deviation's worth) of the logits, of dz and of gbi, and hess [2P] = |d dz_b / d z_b|."""
    p = torch.as_tensor(np.asarray(params, dtype=np.float64))
    bi = torch.as_tensor(np.asarray(bi, dtype=np.float64)).requires_grad_(True)
    base = torch.as_tensor(np.asarray(base, dtype=np.float64)).requires_grad_(True)
    assert bi.shape[0] % 2 == 0 and bi.shape[0] == base.shape[0] and margin >= 0
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
    d = out[0::2] - out[1::2]
    loss_i = pair_loss_t(d, margin)
    ls = loss_i.sum() * inv_b
    dz = torch.autograd.grad(ls, out, create_graph=True)[0]
    # |d dz_b / d z_b| (inv_b included): the row's own entry of the Hessian, which is that of its pair's d
    h_pair = torch.autograd.grad(dz[0::2].sum(), d, retain_graph=True)[0].detach().abs().numpy()
    ls.backward()
    r = dict(out=out.detach().numpy(), d=d.detach().numpy(), loss_i=loss_i.detach().numpy(), loss=float(ls.detach()),
             dz=base.grad.numpy(), gbi=bi.grad.numpy())
    r["grads"] = [(W.grad.numpy(), b.grad.numpy()) for W, b in zip(Ws, bs)]
    r["flat"] = np.concatenate([t.reshape(-1) for pair in r["grads"] for t in pair])
    xs_n, Ws_n, bs_n = [t.detach().numpy() for t in xs], [W.detach().numpy() for W in Ws], [b.detach().numpy() for b in bs]
    # _mlp_grad_noise multiplies slope by the ROW's logit noise; the pair loss's dz depends on d, whose noise is both rows'
    # logit noise in quadrature: the factor goes into the slope
    e_row = logit_noise(xs_n, Ws_n, bs_n)
    e_d = np.repeat(np.sqrt(e_row[0::2] ** 2 + e_row[1::2] ** 2), 2)
    slope = np.repeat(h_pair, 2) * np.divide(e_d, e_row, out=np.ones_like(e_d), where=e_row > 0)
    r["dz_noise"] = 4 * U32 * np.abs(r["dz"]) + np.repeat(h_pair, 2) * e_d
    r["logit_noise"], r["hess"] = e_row, np.repeat(h_pair, 2)
    r["gbi_noise"] = gbi_noise(xs_n, Ws_n, r["dz"], r["dz_noise"])
    r["gnoise"] = _mlp_grad_noise(xs_n, Ws_n, bs_n, [None] * (L - 1) + [dz.detach().numpy()], [None] * (L - 1) + [slope])
    return r
