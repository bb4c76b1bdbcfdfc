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


def tiles(F, tile=64):
    """The kernels' pair tiles (fmx_afm.hip next_tile): whole pair rows i, at most `tile` pairs each -> [(first pair, pairs)]."""
    out, i0, pb = [], 0, 0
    while i0 < F - 1:
        i1, n = i0, 0
        while i1 < F - 1 and n + (F - 1 - i1) <= tile:
            n += F - 1 - i1
            i1 += 1
        out.append((pb, n))
        pb, i0 = pb + n, i1
    return out


def live_params(params, V, k, t, rows, xv=None, chunk=None):
    """params (fp32) with the weights and bias of every attention unit that is dead (W q + b <= 0 for every sample and pair)
    negated, as test_mlp_gpu.live_units does for the MLP: a dead unit gets an exactly-0 gradient, so a kernel that skipped or
    mis-indexed it would pass unseen.  Negation is exact; units live somewhere are left alone."""
    prm = np.asarray(params, dtype=np.float32).copy()
    W, b = prm[:t * k].reshape(t, k), prm[t * k:t * k + t]
    rows = np.asarray(rows, dtype=np.int64)
    B, F = rows.shape
    x = np.ones((B, F)) if xv is None else np.asarray(xv, dtype=np.float64)
    I, J = np.triu_indices(F, 1)
    live = np.zeros(t, bool)
    Vd, Wd = np.asarray(V, dtype=np.float64), W.astype(np.float64)
    chunk = B if chunk is None else chunk
    for c0 in range(0, B, chunk):
        e = Vd[rows[c0:c0 + chunk]] * x[c0:c0 + chunk, :, None]
        live |= ((e[:, I] * e[:, J]) @ Wd.T + b > 0).any((0, 1))
    W[~live] *= -1
    b[~live] *= -1
    return prm


def afm_f64(V, w, bias, params, k, t, rows, xv=None, y=None, inv_b=None, valid=None, grid=1024, chunk=None, loss="logits",
            dz_abs=0.0):
    """V [R, k], w [R], bias (scalar): the table's weights; params: the flat [W | b | h | p]; rows [B, F] global row numbers;
    xv [B, F] or None (ones); valid [B, F] bool or None: False = an absent row (an index outside its field).
    chunk: samples per autograd evaluation (None: the whole batch) -- the [B, P, max(k, t)] intermediates of a measured shape
    are GBs; the chunks' gradients are summed in float64 and every floor is still that of the whole batch.
    loss: 'logits' (BCE with logits) or 'sigmoid' (BCE with logits of sigmoid(logit): FMX_LOSS_BCE_SIGMOID).
    dz_abs: an absolute error of the kernels' dlogit per sample, in units of inv_b, carried into the gradient floors at first
    order.  sigmoid(logit) - y cancels: where |logit| is large and y = 1 the fp32 sigmoid is a few ulps of 1 from its value,
    which the relative floors do not see.  The default 0 leaves them as they were; ~2^-23 covers that rounding.
    A relu unit whose pre-activation lies within its own fp32 rounding of 0 (|z| <= 2 (k + 2) u (|b| + |W| |q|)) may be taken
    on either side of the kink: the whole of its term in dL/dz goes into the floors of dW, db, dh and dV (no such unit: the
    floors are unchanged; 'kinks' counts them).
    -> dict(logit [B], floor_logit [B]); with y also loss_b [B], floor_loss [B], loss (inv_b * sum), dz [B], and the gradients of
    the mean loss: dV [R, k], dw [R], dbias, dparams (flat) with floors fl_dV, fl_dw, fl_dbias, fl_dparams; unit_live [t]
    (unit u's pre-activation is > 0 for some sample and pair) and pair_live [P] (some sample's dL/dq of the pair is not 0)."""
    assert loss in ("logits", "sigmoid")
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
    inv_b = 1.0 / B if inv_b is None else inv_b
    yt = None if y is None else torch.as_tensor(np.asarray(y, dtype=np.float64))
    chunk = B if chunk is None else max(1, int(chunk))
    c = 2 * (k + t + P // 64 + 8)
    n_seq = max(1.0, B * P / min(B, grid))                              # one workgroup's sequential sum, then the workgroups
    cg = 2 * (math.sqrt(n_seq) + math.sqrt(min(B, grid)) + k + t + 8)
    slope = 0.25 if loss == "logits" else 0.5                           # |d dlogit / d logit| / inv_b at most
    cV, cw = 2 * (F + t + k + math.sqrt(B) + 8), 2 * (math.sqrt(B) + 8)
    pieces = {n: [] for n in ("logit", "floor_logit", "loss_b", "floor_loss", "dz")}
    loss_sum = 0.0
    fpar = torch.zeros(t * k + 2 * t + k, dtype=torch.float64)
    fV = torch.zeros_like(Vt)
    fw = torch.zeros_like(wt)
    fbias = 0.0
    kinks = 0
    unit_live = torch.zeros(t, dtype=torch.bool)
    pair_live = torch.zeros(P, dtype=torch.bool)
    for c0 in range(0, B, chunk):
        rc, xc = rows[c0:c0 + chunk], x[c0:c0 + chunk]
        n = rc.shape[0]
        e = Vt[rc] * xc[..., None]                           # [n, F, k]
        q = e[:, I] * e[:, J]                                # [n, P, k]
        z = q @ W.t() + bW                                   # [n, P, t]
        s = torch.relu(z) @ h                                # [n, P]
        a = torch.softmax(s, dim=1)
        r = q @ p                                            # [n, P]
        att = (a * r).sum(1)
        first = (wt[rc] * xc).sum(1)
        logit = bt + first + att
        pieces["logit"].append(logit.detach())

        # ---- fp32 floors of the forward ----
        with torch.no_grad():
            R = att[:, None]
            ms = (torch.relu(z).abs() @ h.abs()) + ((bW.abs() + q.abs() @ W.abs().t()) @ h.abs())    # |s| and its terms
            mr = q.abs() @ p.abs()
            Ma = (a * (mr + (r - R).abs() * ms + (r - R).abs())).sum(1)
            fl = U32 * c * (abs(float(bias)) + (wt[rc] * xc).abs().sum(1) + Ma)
            unit_live |= (z > 0).any(1).any(0)
        pieces["floor_logit"].append(fl)
        if yt is None:
            continue
        yc = yt[c0:c0 + chunk]
        if loss == "logits":
            loss_b = torch.nn.functional.binary_cross_entropy_with_logits(logit, yc, reduction="none")
            floor_loss = fl + 8 * U32 * loss_b.detach().abs()
        else:                                                # the loss of sigmoid(logit): sigmoid's own rounding is absolute
            loss_b = torch.nn.functional.binary_cross_entropy_with_logits(torch.sigmoid(logit), yc, reduction="none")
            floor_loss = fl + 8 * U32 * (loss_b.detach().abs() + 1)
        lc = loss_b.sum() * inv_b
        dz = torch.autograd.grad(lc, logit, retain_graph=True)[0]
        lc.backward()                                        # the leaves' .grad: the chunks' sum, float64
        loss_sum += float(lc.detach())
        pieces["loss_b"].append(loss_b.detach())
        pieces["floor_loss"].append(floor_loss)
        pieces["dz"].append(dz)

        # ---- fp32 floors of the gradients: |terms| with each term's own error carried ----
        with torch.no_grad():
            g = dz.abs() + slope * inv_b * fl + 4 * U32 * dz.abs()   # |dlogit| plus the error the logit's floor puts into it
            ga = g[:, None] * a
            dlt = ga * ((r - R).abs() + r.abs() + R.abs() + ms)     # |dL/ds| with the cancellation in r - R and s's noise
            m = (z > 0).double()
            co = dlt[..., None] * h.abs() * m                       # |dL/dz_u|
            ea, qa = e.abs(), q.abs()

            def terms(ga, co, dh):
                """sum |term| of [dW | db | dh | dp], and of dV per (sample, field), for |dL/dr| = ga, |dL/dz| = co"""
                par = torch.cat([torch.einsum("bpu,bpd->ud", co, qa).reshape(-1), co.sum((0, 1)), dh,
                                 torch.einsum("bp,bpd->d", ga, qa)])
                cq = ga[..., None] * p.abs() + co @ W.abs()          # |dL/dq|  [n, P, k]
                Ee = torch.zeros(n, F, k, dtype=torch.float64)
                Ee.index_add_(1, I, cq * ea[:, J])
                Ee.index_add_(1, J, cq * ea[:, I])
                return par, Ee * xc.abs()[..., None]

            par, Ee = terms(ga, co, torch.einsum("bp,bpu->u", dlt, torch.relu(z)))
            gx = xc.abs() * g[:, None]
            # the relu kink: units within their fp32 rounding of 0 -- their whole dL/dz term, not a rounding of it
            amb = (z.abs() <= 2 * (k + 2) * U32 * (bW.abs() + qa @ W.abs().t())).double()
            nk = int(amb.sum())
            kinks += nk
            extra = U32 * cg * par, U32 * cV * Ee, U32 * cw * gx
            if nk:
                dk = (dz.abs() + 4 * U32 * dz.abs())[:, None] * a * (r - R).abs()
                co_k = dk[..., None] * h.abs() * amb
                pk, Ek = terms(torch.zeros_like(a), co_k, torch.einsum("bp,bpu->u", dk, z.abs() * amb))
                extra = extra[0] + pk, extra[1] + Ek, extra[2]
            if dz_abs:                                         # an absolute dlogit error, carried at first order
                gn = torch.full_like(dz, dz_abs * inv_b)
                gan = gn[:, None] * a
                dn = gan * (r - R).abs()
                pn, En = terms(gan, dn[..., None] * h.abs() * m, torch.einsum("bp,bpu->u", dn, torch.relu(z)))
                extra = extra[0] + pn, extra[1] + En, extra[2] + xc.abs() * gn[:, None]
                fbias += float(gn.sum())
            fpar += extra[0]
            fV.index_add_(0, rc.reshape(-1), extra[1].reshape(-1, k))
            fw.index_add_(0, rc.reshape(-1), extra[2].reshape(-1))
            fbias += float(U32 * cw * g.sum())
            dq = dz[:, None, None] * (a[..., None] * p + (m * h * (a * (r - R))[..., None]) @ W)
            pair_live |= (dq != 0).any(2).any(0)

    out = {kk: torch.cat(v).numpy() for kk, v in pieces.items() if v}
    out.update(unit_live=unit_live.numpy(), pair_live=pair_live.numpy(), kinks=kinks)
    if yt is None:
        return out
    out.update(loss=loss_sum, dV=Vt.grad.numpy(), dw=wt.grad.numpy(), dbias=float(bt.grad), dparams=prm.grad.numpy(),
               fl_dparams=fpar.numpy(), fl_dV=fV.numpy(), fl_dw=fw.numpy(), fl_dbias=fbias)
    return out


def fm_second_order_f64(V, rows, xv=None):
    """The plain FM second-order term sum_{i<j} <e_i, e_j> = sum_d 0.5 ((sum_f e)^2 - sum_f e^2), float64."""
    rows = torch.as_tensor(np.asarray(rows, dtype=np.int64))
    x = torch.ones(rows.shape, dtype=torch.float64) if xv is None else torch.as_tensor(np.asarray(xv, dtype=np.float64))
    e = torch.as_tensor(np.asarray(V, dtype=np.float64))[rows] * x[..., None]
    return (0.5 * (e.sum(1) ** 2 - (e * e).sum(1))).sum(1).numpy()
