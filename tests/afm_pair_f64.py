"""Float64 torch restatement of the pairwise-ranking (BPR) objective over the attentional FM's logit, with autograd -- test
infrastructure for fmx_afm_pair_* built the way tests/afm_f64.py builds the pointwise step (its pair order, tiles, live_params and
u = 2^-24 are imported, not restated):

    rows 2i / 2i + 1 of `rows` are the positive / negative sample of pair i;  d_i = z[2i] - z[2i + 1] over the AFM logit z;
    loss_i = -log(sigmoid(d_i) + margin);  the gradients are those of inv_b * sum_i loss_i.

The fp32 ROUNDING FLOORS follow afm_f64's term by term; only the loss block differs: the floor of d_i is the two logits' floors
(plus the subtraction's rounding), the error of dlogit is that floor times a bound of |dg/dd| for the margin (pair_slope) plus a
few roundings of g itself, and it is carried into the gradient floors at first order, as afm_f64 carries dz_abs / slope.
Helper module, not collected."""
import math

import numpy as np
import torch

from afm_f64 import U32, live_params, pairs, tiles  # noqa: F401  (tiles, live_params: re-exported for the tests)


def pair_loss_t(d, margin):
    """-> loss_i of the logit differences d (a float64 tensor), differentiable (margin 0: the stable softplus form)."""
    if margin == 0:
        return torch.logaddexp(torch.zeros_like(d), -d)
    return -torch.log(torch.sigmoid(d) + margin)


def pair_g(d, margin):
    """dloss/dd in float64 (numpy): -sigmoid(-d) for margin 0, else -sp sn / (sp + margin)."""
    d = np.asarray(d, np.float64)
    sp, sn = 1.0 / (1.0 + np.exp(-d)), 1.0 / (1.0 + np.exp(d))
    return -sn if margin == 0 else -sp * sn / (sp + margin)


def pair_slope(margin):
    """A bound of |dg/dd| over every d for this margin.  With s = sigmoid(d): g = -s (1 - s) / (s + m) and
    dg/dd = -(m - 2 m s - s^2) s (1 - s) / (s + m)^2 -- smooth, -> 0 at both ends; its supremum is taken on a grid of d in
    [-40, 40] at 0.005 spacing in float64 and widened by 1 % (margin 0: sigmoid's 1/4)."""
    if margin == 0:
        return 0.25
    d = np.linspace(-40.0, 40.0, 16001)
    s = 1.0 / (1.0 + np.exp(-d))
    return 1.01 * float(np.abs((margin - 2 * margin * s - s * s) * s * (1 - s) / (s + margin) ** 2).max())


def afm_pair_f64(V, w, bias, params, k, t, rows, xv=None, margin=0.0, inv_b=None, valid=None, grid=1024):
    """V [R, k], w [R], bias, params (flat [W | b | h | p]), rows [2 B_pairs, F] global row numbers, xv or None, valid [2 B_pairs, F]
    bool or None (False: an absent row) as afm_f64 takes them.  inv_b: default 1 / B_pairs.
    -> what afm_f64 returns: logit, floor_logit [2B]; loss_b [2B] (loss_i in the even slots, 0 in the odd), floor_loss [2B];
    loss (inv_b * sum_i loss_i); dz [2B] (dz[2i + 1] = -dz[2i]) with floor_dz [2B]; g [B] = dloss_i/dd_i (unscaled); d [B]; the
    gradients dV [R, k], dw [R], dbias (exactly 0), dparams with floors fl_dV, fl_dw, fl_dbias, fl_dparams; unit_live [t],
    pair_live [P], kinks."""
    rows = torch.as_tensor(np.asarray(rows, dtype=np.int64))
    B, F = rows.shape
    assert B % 2 == 0 and margin >= 0
    Bp = B // 2
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
    inv_b = 1.0 / Bp if inv_b is None else inv_b
    # the counts of sequential roundings, as afm_f64 sets them: a workgroup owns PAIRS here, so min(Bp, grid) workgroups
    c = 2 * (k + t + P // 64 + 8)
    n_wg = min(Bp, grid)
    n_seq = max(1.0, B * P / n_wg)
    cg = 2 * (math.sqrt(n_seq) + math.sqrt(n_wg) + k + t + 8)
    slope = pair_slope(margin)
    cV, cw = 2 * (F + t + k + math.sqrt(B) + 8), 2 * (math.sqrt(B) + 8)

    e = Vt[rows] * x[..., None]                              # [B, F, k]
    q = e[:, I] * e[:, J]                                    # [B, P, k]
    z = q @ W.t() + bW                                       # [B, P, t]
    s = torch.relu(z) @ h                                    # [B, P]
    a = torch.softmax(s, dim=1)
    r = q @ p
    att = (a * r).sum(1)
    logit = bt + (wt[rows] * x).sum(1) + att
    d = logit[0::2] - logit[1::2]
    loss_i = pair_loss_t(d, margin)
    total = loss_i.sum() * inv_b
    dz = torch.autograd.grad(total, logit, retain_graph=True)[0]
    total.backward()

    with torch.no_grad():
        # ---- fp32 floors of the forward (afm_f64's) ----
        R = att[:, None]
        ms = (torch.relu(z).abs() @ h.abs()) + ((bW.abs() + q.abs() @ W.abs().t()) @ h.abs())
        mr = q.abs() @ p.abs()
        Ma = (a * (mr + (r - R).abs() * ms + (r - R).abs())).sum(1)
        fl = U32 * c * (abs(float(bias)) + (wt[rows] * x).abs().sum(1) + Ma)
        unit_live = (z > 0).any(1).any(0)
        # ---- the pair loss block ----
        fd = fl[0::2] + fl[1::2] + U32 * d.abs()                                  # the floor of d: both logits', the subtraction
        g = torch.as_tensor(pair_g(d.numpy(), margin))                            # dloss_i / dd_i, |g| <= 1
        floor_loss = torch.zeros(B, dtype=torch.float64)
        floor_loss[0::2] = g.abs() * fd + slope * fd * fd + 8 * U32 * (loss_i.abs() + (1.0 if margin else 0.0))
        loss_b = torch.zeros(B, dtype=torch.float64)
        loss_b[0::2] = loss_i
        # the error of dlogit per row: d's floor through |dg/dd|, and the roundings of g's own evaluation (exp, reciprocals,
        # product, quotient, inv_b: 8 u relative)
        dze = torch.repeat_interleave((slope * fd + 8 * U32 * g.abs()) * inv_b, 2)
        assert torch.equal(dz[1::2], -dz[0::2])

        # ---- fp32 floors of the gradients (afm_f64's, with |dlogit| + its error) ----
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
        # the bias gradient is sum(dz) = sum_i (g_i - g_i): exactly 0, whatever the order (autograd's own sum may round)
        assert abs(float(bt.grad)) <= 1e-15 * float(dz.abs().sum()) + 1e-300

    return dict(logit=logit.detach().numpy(), floor_logit=fl.numpy(), loss_b=loss_b.numpy(), floor_loss=floor_loss.numpy(),
                loss=float(total.detach()), dz=dz.numpy(), floor_dz=dze.numpy(), g=g.numpy(), d=d.detach().numpy(),
                dV=Vt.grad.numpy(), dw=wt.grad.numpy(), dbias=0.0, dparams=prm.grad.numpy(), fl_dparams=fpar.numpy(),
                fl_dV=fV.numpy(), fl_dw=fw.numpy(), fl_dbias=0.0, unit_live=unit_live.numpy(), pair_live=pair_live.numpy(),
                kinks=kinks)
