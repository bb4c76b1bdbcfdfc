"""Float64 torch restatement of the listwise (sampled-softmax) objective over the attentional FM's logit, with autograd -- test
infrastructure for fmx_afm_list_* built the way tests/afm_pair_f64.py builds the pair step (afm_f64's pair order, tiles,
live_params and u = 2^-24 are imported, not restated):

    rows G i .. G i + G - 1 of `rows` are list i, the positive first;  z_j the AFM logit of row G i + j,  p = softmax(z);
    loss_i = -log p_0 = log(sum_j exp(z_j - m)) - (z_0 - m);  dz_j = p_j inv_b (j >= 1),  dz_0 = -(sum_{j>=1} p_j) inv_b;
    the gradients are those of inv_b * sum_i loss_i.  The bias has no gradient: dbias is DEFINED as 0.

The fp32 ROUNDING FLOORS follow afm_pair_f64's term by term; only the loss block differs, and it is tests/list_f64.py's (its
docstring derives both lines), over the list's logit floors f_logit_l:
    f_dz     = (sum_l f_logit_l / 4 + (1.5 G + 10) u) inv_b        for every row of the list
    f_loss_i = sum_l f_logit_l + u (1.5 G + 4 + 6 |loss_i|)
f_dz is carried into the gradient floors at first order, as afm_pair_f64 carries dze.  A workgroup owns a LIST: the rounding
estimates count min(B_lists, grid) workgroups.
Helper module, not collected."""
import math

import numpy as np
import torch

from afm_f64 import U32, live_params, pairs, tiles  # noqa: F401  (tiles, live_params: re-exported for the tests)


def list_dz_t(z):
    """z [B, G] float64 -> dloss/dz [B, G] of the softmax cross-entropy against column 0, column 0's as minus the negatives' mass
    (not p_0 - 1, which loses its digits as p_0 -> 1)."""
    e = torch.exp(z - z.max(dim=1, keepdim=True).values)
    s = e.sum(1, keepdim=True)
    g = e / s
    g[:, 0] = -(e[:, 1:].sum(1) / s[:, 0])
    return g


def afm_list_f64(V, w, bias, params, k, t, rows, G, xv=None, inv_b=None, valid=None, grid=1024):
    """V [R, k], w [R], bias, params (flat [W | b | h | p]), rows [B_lists G, F] global row numbers, xv or None, valid
    [B_lists G, F] bool or None (False: an absent row) as afm_f64 takes them.  inv_b: default 1 / B_lists.
    -> what afm_pair_f64 returns: logit, floor_logit [B]; loss_b [B] (loss_i in slot G i, 0 in the others), floor_loss [B];
    loss (inv_b * sum_i loss_i); dz [B] with floor_dz [B]; the gradients dV [R, k], dw [R], dbias (0 by definition), dparams with
    floors fl_dV, fl_dw, fl_dbias, fl_dparams; unit_live [t], pair_live [P], kinks."""
    rows = torch.as_tensor(np.asarray(rows, dtype=np.int64))
    B, F = rows.shape
    G = int(G)
    assert G >= 2 and B % G == 0
    Bl = B // G
    x = torch.ones(B, F, dtype=torch.float64) if xv is None else torch.as_tensor(np.asarray(xv, dtype=np.float64))
    if valid is not None:
        x = x * torch.as_tensor(np.asarray(valid, dtype=bool)).double()
    Vt = torch.as_tensor(np.asarray(V, dtype=np.float64)).clone().requires_grad_(True)
    wt = torch.as_tensor(np.asarray(w, dtype=np.float64)).clone().requires_grad_(True)
    prm = torch.as_tensor(np.asarray(params, dtype=np.float64)).clone().requires_grad_(True)
    W, bW, h, p = prm[:t * k].reshape(t, k), prm[t * k:t * k + t], prm[t * k + t:t * k + 2 * t], prm[t * k + 2 * t:]
    I, J = pairs(F)
    P = len(I)
    inv_b = 1.0 / Bl if inv_b is None else inv_b
    # the counts of sequential roundings, as afm_pair_f64 sets them: a workgroup owns LISTS here, so min(Bl, grid) workgroups
    c = 2 * (k + t + P // 64 + 8)
    n_wg = min(Bl, grid)
    n_seq = max(1.0, B * P / n_wg)
    cg = 2 * (math.sqrt(n_seq) + math.sqrt(n_wg) + k + t + 8)
    cV, cw = 2 * (F + t + k + math.sqrt(B) + 8), 2 * (math.sqrt(B) + 8)

    e = Vt[rows] * x[..., None]                              # [B, F, k]
    q = e[:, I] * e[:, J]                                    # [B, P, k]
    z = q @ W.t() + bW                                       # [B, P, t]
    s = torch.relu(z) @ h                                    # [B, P]
    a = torch.softmax(s, dim=1)
    r = q @ p
    att = (a * r).sum(1)
    logit = float(bias) + (wt[rows] * x).sum(1) + att
    zl = logit.detach().reshape(Bl, G)
    loss_i = torch.logsumexp(zl, dim=1) - zl[:, 0]
    total = loss_i.sum() * inv_b
    dz = (list_dz_t(zl) * inv_b).reshape(B)
    logit.backward(dz)                                       # the gradients of inv_b * sum_i loss_i through its exact dlogit

    with torch.no_grad():
        # ---- fp32 floors of the forward (afm_f64's) ----
        R = att[:, None]
        ms = (torch.relu(z).abs() @ h.abs()) + ((bW.abs() + q.abs() @ W.abs().t()) @ h.abs())
        mr = q.abs() @ p.abs()
        Ma = (a * (mr + (r - R).abs() * ms + (r - R).abs())).sum(1)
        fl = U32 * c * (abs(float(bias)) + (wt[rows] * x).abs().sum(1) + Ma)
        unit_live = (z > 0).any(1).any(0)
        # ---- the list loss block (list_f64's) ----
        f_z = fl.reshape(Bl, G).sum(1)                                            # sum_l f_logit_l of every list
        dze = torch.repeat_interleave((0.25 * f_z + (1.5 * G + 10) * U32) * inv_b, G)
        loss_b = torch.zeros(B, dtype=torch.float64)
        loss_b[0::G] = loss_i
        floor_loss = torch.zeros(B, dtype=torch.float64)
        floor_loss[0::G] = f_z + U32 * (1.5 * G + 4 + 6 * loss_i.abs())

        # ---- fp32 floors of the gradients (afm_pair_f64's, with |dlogit| + its error) ----
        gg = dz.abs() + dze
        ga = gg[:, None] * a
        dlt = ga * ((r - R).abs() + r.abs() + R.abs() + ms)
        m = (z > 0).double()
        co = dlt[..., None] * h.abs() * m
        ea, qa = e.abs(), q.abs()

        def terms(ga, co, dh):
            par = torch.cat([torch.einsum("bpu,bpd->ud", co, qa).reshape(-1), co.sum((0, 1)), dh, torch.einsum("bp,bpd->d", ga, qa)])
            cq = ga[..., None] * p.abs() + co @ W.abs()
            Ee = torch.zeros(B, F, k, dtype=torch.float64)
            Ee.index_add_(1, I, cq * ea[:, J])
            Ee.index_add_(1, J, cq * ea[:, I])
            return par, Ee * x.abs()[..., None]

        par, Ee = terms(ga, co, torch.einsum("bp,bpu->u", dlt, torch.relu(z)))
        gx = x.abs() * gg[:, None]
        amb = (z.abs() <= 2 * (k + 2) * U32 * (bW.abs() + qa @ W.abs().t())).double()
        kinks = int(amb.sum())
        fpar, fE, fwx = U32 * cg * par, U32 * cV * Ee, U32 * cw * gx
        if kinks:
            dk = gg[:, None] * a * (r - R).abs()
            pk, Ek = terms(torch.zeros_like(a), dk[..., None] * h.abs() * amb, torch.einsum("bp,bpu->u", dk, z.abs() * amb))
            fpar, fE = fpar + pk, fE + Ek
        # the absolute dlogit error at first order (afm_f64's dz_abs block, per row)
        gan = dze[:, None] * a
        dn = gan * (r - R).abs()
        pn, En = terms(gan, dn[..., None] * h.abs() * m, torch.einsum("bp,bpu->u", dn, torch.relu(z)))
        fpar, fE, fwx = fpar + pn, fE + En, fwx + x.abs() * dze[:, None]
        fV = torch.zeros_like(Vt)
        fw = torch.zeros_like(wt)
        fV.index_add_(0, rows.reshape(-1), fE.reshape(-1, k))
        fw.index_add_(0, rows.reshape(-1), fwx.reshape(-1))
        dq = dz[:, None, None] * (a[..., None] * p + (m * h * (a * (r - R))[..., None]) @ W)
        pair_live = (dq != 0).any(2).any(0)

    return dict(logit=logit.detach().numpy(), floor_logit=fl.numpy(), loss_b=loss_b.numpy(), floor_loss=floor_loss.numpy(),
                loss=float(total), dz=dz.numpy(), floor_dz=dze.numpy(),
                dV=Vt.grad.numpy(), dw=wt.grad.numpy(), dbias=0.0, dparams=prm.grad.numpy(), fl_dparams=fpar.numpy(),
                fl_dV=fV.numpy(), fl_dw=fw.numpy(), fl_dbias=0.0, unit_live=unit_live.numpy(), pair_live=pair_live.numpy(),
                kinks=kinks)
