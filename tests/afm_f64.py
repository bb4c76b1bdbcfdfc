"""Float64 torch restatement of the attentional FM (include/fmx.h, fmx_afm_t; DESIGN.md section 3 "AFM") with autograd --
test infrastructure for the AFM kernels, taking the same parameters:

    pair (i<j) in the order i = 0..F-2, j = i+1..F-1;  q_ij = e_i * e_j;  s_ij = h . relu(W q_ij + b);  a = softmax_ij(s)
    logit = bias + sum_f w_f x_f + p . sum_ij a_ij q_ij,   e_f = x_f V[row_f]

Besides the values and gradients it returns fp32 ROUNDING FLOORS: for every output, c u sum|terms| -- u = 2^-24, sum|terms| the
sum of the absolute values of the terms the fp32 kernels add up (each term's own error bound carried), c a count of the
sequential roundings on the longest path (the sqrt of a long sequential sum's length: independent roundings)."""
import math

import numpy as np
import torch

U32 = 2.0 ** -24


def pairs(F):
    I, J = np.triu_indices(F, 1)          # row-major upper triangle: i = 0..F-2, j = i+1..F-1 -- the kernels' pair order
    return torch.as_tensor(I), torch.as_tensor(J)


def split_params(params, k, t):
    p = torch.as_tensor(np.asarray(params, dtype=np.float64))
    W = p[:t * k].reshape(t, k)
    return W, p[t * k:t * k + t], p[t * k + t:t * k + 2 * t], p[t * k + 2 * t:t * k + 2 * t + k]


def afm_f64(V, w, bias, params, k, t, rows, xv=None, y=None, inv_b=None, valid=None, grid=1024):
    """V [R, k], w [R], bias (scalar): the table's weights; params: the flat [W | b | h | p]; rows [B, F] global row numbers;
    xv [B, F] or None (ones); valid [B, F] bool or None: False = an absent row (an index outside its field).
    -> dict(logit [B], floor_logit [B]); with y also loss_b [B], floor_loss [B], loss (inv_b * sum), dz [B], and the gradients of
    the mean loss: dV [R, k], dw [R], dbias, dparams (flat) with floors fl_dV, fl_dw, fl_dbias, fl_dparams."""
    rows = torch.as_tensor(np.asarray(rows, dtype=np.int64))
    B, F = rows.shape
    x = torch.ones(B, F, dtype=torch.float64) if xv is None else torch.as_tensor(np.asarray(xv, dtype=np.float64))
    if valid is not None:
        x = x * torch.as_tensor(np.asarray(valid, dtype=bool)).double()
    Vt = torch.as_tensor(np.asarray(V, dtype=np.float64)).clone().requires_grad_(True)
    wt = torch.as_tensor(np.asarray(w, dtype=np.float64)).clone().requires_grad_(True)
    bt = torch.tensor(float(bias), dtype=torch.float64, requires_grad=True)
    prm = torch.as_tensor(np.asarray(params, dtype=np.float64)).clone().requires_grad_(True)
    W, bW, h, p = prm[:t * k].reshape(t, k), prm[t * k:t * k + t], prm[t * k + t:t * k + 2 * t], prm[t * k + 2 * t:]
    I, J = pairs(F)
    P = len(I)
    e = Vt[rows] * x[..., None]                          # [B, F, k]
    q = e[:, I] * e[:, J]                                # [B, P, k]
    z = q @ W.t() + bW                                   # [B, P, t]
    s = torch.relu(z) @ h                                # [B, P]
    a = torch.softmax(s, dim=1)
    r = q @ p                                            # [B, P]
    att = (a * r).sum(1)
    first = (wt[rows] * x).sum(1)
    logit = bt + first + att
    out = dict(logit=logit.detach().numpy())

    # ---- fp32 floors of the forward ----
    with torch.no_grad():
        R = att[:, None]
        ms = (torch.relu(z).abs() @ h.abs()) + ((bW.abs() + q.abs() @ W.abs().t()) @ h.abs())    # |s| and its terms
        mr = q.abs() @ p.abs()
        Ma = (a * (mr + (r - R).abs() * ms + (r - R).abs())).sum(1)
        c = 2 * (k + t + P // 64 + 8)
        fl = U32 * c * (abs(float(bias)) + (wt[rows] * x).abs().sum(1) + Ma)
    out["floor_logit"] = fl.numpy()
    if y is None:
        return out
    yt = torch.as_tensor(np.asarray(y, dtype=np.float64))
    inv_b = 1.0 / B if inv_b is None else inv_b
    loss_b = torch.nn.functional.binary_cross_entropy_with_logits(logit, yt, reduction="none")
    loss = loss_b.sum() * inv_b
    dz = torch.autograd.grad(loss, logit, retain_graph=True)[0]
    loss.backward()
    out.update(loss_b=loss_b.detach().numpy(), loss=float(loss.detach()), dz=dz.numpy(),
               floor_loss=(fl + 8 * U32 * loss_b.detach().abs()).numpy(),
               dV=Vt.grad.numpy(), dw=wt.grad.numpy(), dbias=float(bt.grad), dparams=prm.grad.numpy())

    # ---- fp32 floors of the gradients: |terms| with each term's own error carried ----
    with torch.no_grad():
        g = dz.abs() + 0.25 * inv_b * fl + 4 * U32 * dz.abs()            # |dlogit| plus the error the logit's floor puts into it
        ga = g[:, None] * a
        dlt = ga * ((r - R).abs() + r.abs() + R.abs() + ms)             # |dL/ds| with the cancellation in r - R and s's noise
        m = (z > 0).double()
        co = dlt[..., None] * h.abs() * m                               # |dL/dz_u|
        n_seq = max(1.0, B * P / min(B, grid))                          # one workgroup's sequential sum, then the workgroups
        cg = 2 * (math.sqrt(n_seq) + math.sqrt(min(B, grid)) + k + t + 8)
        fW = torch.einsum("bpu,bpd->ud", co, q.abs())
        fb = co.sum((0, 1))
        fh = torch.einsum("bp,bpu->u", dlt, torch.relu(z))
        fp = torch.einsum("bp,bpd->d", ga, q.abs())
        out["fl_dparams"] = (U32 * cg * torch.cat([fW.reshape(-1), fb, fh, fp])).numpy()
        cq = ga[..., None] * p.abs() + co @ W.abs()                      # |dL/dq|  [B, P, k]
        Ee = torch.zeros(B, F, k, dtype=torch.float64)
        ea = e.abs()
        Ee.index_add_(1, I, cq * ea[:, J])
        Ee.index_add_(1, J, cq * ea[:, I])
        Ee = Ee * x.abs()[..., None]
        fV = torch.zeros_like(Vt)
        fV.index_add_(0, rows.reshape(-1), Ee.reshape(-1, k))
        cV = 2 * (F + t + k + math.sqrt(B) + 8)
        out["fl_dV"] = (U32 * cV * fV).numpy()
        fw = torch.zeros_like(wt)
        fw.index_add_(0, rows.reshape(-1), (x.abs() * g[:, None]).reshape(-1))
        out["fl_dw"] = (U32 * 2 * (math.sqrt(B) + 8) * fw).numpy()
        out["fl_dbias"] = float(U32 * 2 * (math.sqrt(B) + 8) * g.sum())
    return out


def fm_second_order_f64(V, rows, xv=None):
    """The plain FM second-order term sum_{i<j} <e_i, e_j> = sum_d 0.5 ((sum_f e)^2 - sum_f e^2), float64."""
    rows = torch.as_tensor(np.asarray(rows, dtype=np.int64))
    x = torch.ones(rows.shape, dtype=torch.float64) if xv is None else torch.as_tensor(np.asarray(xv, dtype=np.float64))
    e = torch.as_tensor(np.asarray(V, dtype=np.float64))[rows] * x[..., None]
    return (0.5 * (e.sum(1) ** 2 - (e * e).sum(1))).sum(1).numpy()
