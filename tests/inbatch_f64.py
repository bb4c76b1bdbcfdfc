"""A float64 evaluation of one in-batch sampled-softmax step of the pure FM (fmx_fm_inbatch_*, include/fmx.h) from an fp32 state, with
the fp32 rounding floor of every output -- built the way list_f64.list_step_f64 and listq_f64.listq_step_f64 build theirs: the same
EPS32 and K_FP32, the same forward and rule blocks with their term-by-term floors, the list loss block's floor with the row's eligible
set in the place of the list.  Nothing is tuned.

The objective.  The F fields are item fields and context fields (the complement).  With e_bf = x_bf V[row_bf],
    S_u[i] = sum over context fields of e_if,   a_u[i] = sum of first_if + sum_d bi_u[i, d] + bias       (bi = (S S - sum e e) / 2)
    S_c[j] = sum over item fields of e_jf,      a_c[j] = sum of first_jf + sum_d bi_c[j, d]
    score(i, j) = a_u[i] + a_c[j] + <S_u[i], S_c[j]>,      c_ij = score(i, j) - corr[j]
    E_i = {i} + {j != i : key[j] != key[i]},   p_ij = softmax of c_i. over E_i,   loss_i = -log p_ii
    g_ij = p_ij inv_b (j in E_i, j != i),   g_ii = -(sum of the others' p_ij) inv_b,   g_ij = 0 outside E_i
    gSu[i] = sum_j g_ij S_c[j],   gSc[j] = sum_i g_ij S_u[i],   gac[j] = sum_i g_ij
    occurrence of an item field of row j:     E = x (gac[j] (S_c[j] - x v) + gSc[j]),   its first-order weight: x gac[j]
    occurrence of a context field of row i:   E = x gSu[i],                              its first-order weight: 0 BY DEFINITION
the step is that of inv_b sum_i loss_i with the row sum of g taken as zero: the bias and the context fields' first-order weights have
no gradient (db = 0, the bias is the old value, as in list_f64).

The floors, with u = EPS32.
 (forward)  fS and f_logit are list_f64's, evaluated on each side's own fields: fS_side = (K_FP32 + w_eps u) sum |e|, f_a_side =
     sum_d f_bi + (K_FP32 + w_eps u) (sum |first| + |bias|) + K_FP32 sum |bi| (no bias term on the item side; the device adds
     sfirst + sbi there in one more rounding: u |a_c|).
 (score)  the device's score is (a_u + a_c) + an fma chain over d: the dot of two vectors that carry fS each, accumulated in kp
     roundings, and two more additions:
         f_s_ij = f_au_i + f_ac_j + sum_d (|S_u| fS_c + fS_u |S_c| + fS_u fS_c) + (kp + 2) u (sum_d |S_u S_c| + |a_u| + |a_c|).
     c_ij = fl(score - corr_j) adds u |c_ij| (listq_f64's one term).
 (loss)  list_f64's (a) and (b) with E_i in the place of the list, G_i = |E_i|, p_il the softmax over E_i and x_il = m_i - c_il >= 0.
     list_f64 closes both with p <= 1 (|d dz_j / d z_l| <= inv_b / 4 for EVERY l, (1.5 G + 10) u for the arithmetic), which costs
     nothing at G <= 16; at G_i in the hundreds p_il is of order 1 / G_i and that last step would leave floors a thousand times the
     errors they bound, so the same two derivations are kept one step earlier, with their factors of p:
     (a) d p_ij / d c_il = p_ij (delta_jl - p_il): p_ij moves by at most p_ij (f_c_ij + sum_l p_il f_c_il), and 1 - p_ii (the
         diagonal's mass of the others) by p_ii's; d loss_i / d c_il = p_il - delta_li: the loss moves by sum_l p_il f_c_il + f_c_ii.
     (b) t_il = fl(c_il - m_i) is off by u x_il, which moves e_il = exp(t_il) by u x_il e_il; expf adds 4 u e_il: every e_il is
         within e_il u (x_il + 4).  A sum of G_i such terms in any order adds (G_i - 1) u s, so s_i (and n_i, a part of it) is within
         u s_i A_i, A_i = sum_l p_il x_il + G_i + 3.  A quotient e_ij / s_i is within p_ij u (x_ij + 4 + A_i + 1), n_i / s_i within
         u (2 A_i + 1) (n <= s), and the product with inv_b adds u |g|:
         f_g_ij = (p_ij (f_c_ij + sum_l p_il f_c_il) + p_ij u (x_ij + 6 + A_i)) inv_b    for eligible j != i
         f_g_ii = (p_ii (f_c_ii + sum_l p_il f_c_il) + u (2 A_i + 2)) inv_b
         The loss log(s) - (c_ii - m): log moves by the relative error of s, logf adds 4 u log s, t_ii is off by u x_ii, the
         subtraction adds u |loss|; log s and x_ii are both >= 0 and sum to the loss:
         f_loss_i = sum_l p_il f_c_il + f_c_ii + u (A_i + 6 |loss_i|).
 (side gradients)  a sum of B fma terms g_ij S[j]: each term moves by f_g |S| + |g| fS, and the fp32 accumulation of n terms in ANY
     order is off by at most n u relative to the sum of the absolute terms (one rounding per fma, one per partial-sum addition;
     every partial sum is bounded by that sum).  The order the header states -- `per` terms in a row, then `splits` partial sums --
     has depth per + splits, far below B for large B, and that depth is what the bound needs:
         f_gS = sum_j (f_g |S| + |g| fS) + (per + splits) u sum_j |g S|,        f_gac = sum_i f_g + (per + splits) u sum_i |g|.
 (occurrences)  E = x (gac t + gSc), t = S_c - x v: t carries fS_c (+ w_eps u |x v|) and one rounding, the fma and the product two:
         f_E_item = |x| (f_gac |t| + |gac| (fS_c + (w_eps + 2) u (|S_c| + |x v|)) + f_gSc) + 3 u |E|,   f_E_ctx = |x| f_gSu + u |E|.
 (rows)  dV[row] = sum of its occurrences' E in sample order: fV = sum (f_E + K_FP32 |E|), as list_f64 adds K_FP32 per term;
     dw[row] = sum x gac over its item occurrences: fw = sum |x| (K_FP32 |gac| + f_gac).  The rule blocks are list_f64's.
Helper module, not collected."""
import numpy as np

from oracle.fm_oracle import EPS32, K_FP32, ftrl_weight


def geometry(B):
    """(splits, per) of include/fmx.h: splits = min(32, ceil(B / 64)) ranges of per = ceil(B / splits) rows, empty ranges dropped"""
    s0 = min(32, -(-B // 64))
    per = -(-B // s0)
    return -(-B // per), per


def first_split_threshold():
    """The largest B that is summed as one range: one more row and the sums are cut in two"""
    B = 1
    while geometry(B + 1)[0] == 1:
        B += 1
    return B


def eligible(B, key):
    el = np.ones((B, B), bool)
    if key is not None:
        key = np.asarray(key).reshape(B)
        el = key[None, :] != key[:, None]
        el[np.arange(B), np.arange(B)] = True
    return el


def inbatch_loss_f64(c, el):
    """c [B, B] float64 corrected logits, el [B, B] the eligible set -> (loss [B], g [B, B] = d sum_i loss_i / d c, m [B], s [B], n [B]);
    the diagonal's derivative as minus the others' mass."""
    B = c.shape[0]
    diag = np.arange(B)
    cm = np.where(el, c, -np.inf)
    m = cm.max(axis=1)
    e = np.where(el, np.exp(cm - m[:, None]), 0.0)
    s = e.sum(axis=1)
    off = e.copy()
    off[diag, diag] = 0.0
    n = off.sum(axis=1)
    g = off / s[:, None]
    g[diag, diag] = -(n / s)
    return np.log(s) - (c[diag, diag] - m), g, m, s, n


def inbatch_step_f64(state, rows, x, item_fields, rule, hyper, corr=None, key=None, inv_b=None, kp=None):
    """state (NOT mutated): rule 'sgd': V [R,k], w [R], bias; rule 'ftrl': zV, nV [R,k], zw, nw [R], zb, nb.  rows [B, F] global row
    ids, x [B, F]; item_fields: the item columns; corr [B] (read as fp32) or None; key [B] or None; kp: the device's padded k (the
    length of its product chain; default k).  Returns dict(loss, loss_b, score, Su, au, Sc, ac, m, s, n, g, gSu, gSc, gac, occ
    [B, F, k], urows, dV, dw, db, new, floor)."""
    d = np.float64
    rows = np.asarray(rows, dtype=np.int64)
    x = np.asarray(x, dtype=d)
    B, F = rows.shape
    inv_b = 1.0 / B if inv_b is None else inv_b
    item = np.zeros(F, bool)
    item[list(item_fields)] = True
    ctx = ~item
    if rule == "ftrl":
        # (the hyper-parameters as the fp32 values the device gets: next to the L1 dead zone w = -(z - l1) / (...) is a cancelled
        #  difference, and the float64 value of 0.001 is not the number the kernels subtract)
        a, b_, l1, l2 = (float(np.float32(hyper[n_])) for n_ in ("alpha", "beta", "l1", "l2"))
        V = ftrl_weight(state["zV"], state["nV"], a, b_, l1, l2, dtype=d)
        w = ftrl_weight(state["zw"], state["nw"], a, b_, l1, l2, dtype=d)
        bias = float(ftrl_weight(state["zb"], state["nb"], a, b_, l1, l2, dtype=d))
        w_eps = 4.0
    elif rule == "sgd":
        V, w, bias = np.asarray(state["V"], d), np.asarray(state["w"], d), float(state["bias"])
        w_eps = 0.0
    else:
        raise ValueError(rule)
    k = V.shape[1]
    kp = k if kp is None else kp
    u = EPS32
    # ---- the two masked forwards (list_f64's forward and floors on each side's fields) ----
    e = V[rows] * x[:, :, None]
    first = w[rows] * x

    def side(mask, b):
        es, fs = e[:, mask, :], first[:, mask]
        S, SS = es.sum(axis=1), (es * es).sum(axis=1)
        bi = 0.5 * (S * S - SS)
        av = fs.sum(axis=1) + bi.sum(axis=1) + b
        fS = (K_FP32 + w_eps * u) * np.abs(es).sum(axis=1)
        f_bi = np.abs(S) * fS + K_FP32 * 0.5 * (S * S + SS) + w_eps * u * SS
        f_a = f_bi.sum(axis=1) + (K_FP32 + w_eps * u) * (np.abs(fs).sum(axis=1) + abs(b)) + K_FP32 * np.abs(bi).sum(axis=1)
        return S, av, fS, f_a

    Su, au, fSu, f_au = side(ctx, bias)
    Sc, ac, fSc, f_ac = side(item, 0.0)
    f_ac = f_ac + u * np.abs(ac)                                        # sfirst + sbi: one more fp32 addition
    # ---- scores ----
    score = au[:, None] + ac[None, :] + Su @ Sc.T
    aSu, aSc = np.abs(Su), np.abs(Sc)
    f_s = (f_au[:, None] + f_ac[None, :] + aSu @ fSc.T + fSu @ aSc.T + fSu @ fSc.T
           + (kp + 2) * u * (aSu @ aSc.T + np.abs(au)[:, None] + np.abs(ac)[None, :]))
    if corr is None:
        c, f_c = score, f_s
    else:
        corr = np.asarray(corr, dtype=np.float32).astype(d).reshape(B)
        c = score - corr[None, :]
        f_c = f_s + u * np.abs(c)
    # ---- the loss block ----
    el = eligible(B, key)
    loss_b, g1, m, s, n = inbatch_loss_f64(c, el)
    G = el.sum(axis=1).astype(d)
    diag = np.arange(B)
    p = np.where(el, np.exp(np.where(el, c, -np.inf) - m[:, None]), 0.0) / s[:, None]     # the softmax over E_i, the diagonal included
    xg = np.where(el, m[:, None] - c, 0.0)
    pf = (p * np.where(el, f_c, 0.0)).sum(axis=1)                        # sum_l p_il f_c_il
    A = (p * xg).sum(axis=1) + G + 3
    g = g1 * inv_b
    f_g = (p * (np.where(el, f_c, 0.0) + pf[:, None]) + p * u * (xg + 6 + A[:, None])) * inv_b
    f_g[diag, diag] = (p[diag, diag] * (f_c[diag, diag] + pf) + u * (2 * A + 2)) * inv_b
    f_lb = pf + f_c[diag, diag] + u * (A + 6 * np.abs(loss_b))
    loss = loss_b.sum() * inv_b
    f_loss = (f_lb.sum() + K_FP32 * np.abs(loss_b).sum()) * inv_b
    # ---- the side gradients ----
    splits, per = geometry(B)
    depth = (per + splits) * u
    ag = np.abs(g)
    gSu, gSc, gac = g @ Sc, g.T @ Su, g.sum(axis=0)
    f_gSu = f_g @ aSc + ag @ fSc + depth * (ag @ aSc)
    f_gSc = f_g.T @ aSu + ag.T @ fSu + depth * (ag.T @ aSu)
    f_gac = f_g.sum(axis=0) + depth * ag.sum(axis=0)
    # ---- per-occurrence gradients ----
    xs = x[:, :, None]
    t = Sc[:, None, :] - e
    E_item = xs * (gac[:, None, None] * t + gSc[:, None, :])
    E_ctx = xs * gSu[:, None, :]
    occ = np.where(item[None, :, None], E_item, E_ctx)
    ax = np.abs(xs)
    f_E_item = ax * (f_gac[:, None, None] * np.abs(t) + np.abs(gac)[:, None, None] * (fSc[:, None, :] + (w_eps + 2) * u * (aSc[:, None, :] + np.abs(e)))
                     + f_gSc[:, None, :]) + 3 * u * np.abs(E_item)
    f_E_ctx = ax * f_gSu[:, None, :] + u * np.abs(E_ctx)
    f_occ = np.where(item[None, :, None], f_E_item, f_E_ctx)
    # ---- row gradients ----
    flat = rows.reshape(-1)
    urows, inv = np.unique(flat, return_inverse=True)
    inv = inv.reshape(-1)
    U = len(urows)
    dV = np.zeros((U, k), d)
    np.add.at(dV, inv, occ.reshape(-1, k))
    fV = np.zeros((U, k), d)
    np.add.at(fV, inv, (f_occ + K_FP32 * np.abs(occ)).reshape(-1, k))
    dw1 = np.where(item[None, :], x * gac[:, None], 0.0)
    f_dw1 = np.where(item[None, :], np.abs(x) * (K_FP32 * np.abs(gac) + f_gac)[:, None], 0.0)
    dw = np.zeros(U, d)
    np.add.at(dw, inv, dw1.reshape(-1))
    fw = np.zeros(U, d)
    np.add.at(fw, inv, f_dw1.reshape(-1))
    db = 0.0                                                            # by definition: the bias is not part of an in-batch step
    out = dict(loss=loss, loss_b=loss_b, score=score, Su=Su, au=au, Sc=Sc, ac=ac, m=m, s=s, n=n, g=g, gSu=gSu, gSc=gSc, gac=gac,
               occ=occ, urows=urows, dV=dV, dw=dw, db=db, V=V, w=w, bias=bias, eligible=el)
    floor = dict(loss=f_loss, loss_b=f_lb, score=f_s, Su=fSu, au=f_au, Sc=fSc, ac=f_ac, g=f_g, gSu=f_gSu, gSc=f_gSc, gac=f_gac,
                 occ=f_occ, dV=fV, dw=fw, db=0.0)
    new = {}
    if rule == "ftrl":
        def upd(z, n_, g_, fg, wt):
            z, n_ = np.asarray(z, d), np.asarray(n_, d)
            n2 = n_ + g_ * g_
            sig = (np.sqrt(n2) - np.sqrt(n_)) / a
            z2 = z + g_ - sig * wt
            f_n = 2 * np.abs(g_) * fg + fg * fg + 2 * EPS32 * n2
            f_sig = fg / a + 4 * EPS32 * (np.sqrt(n2) + np.sqrt(n_)) / a
            f_z_ = fg + np.abs(wt) * f_sig + (w_eps + 4) * EPS32 * np.abs(sig * wt) + 2 * EPS32 * (np.abs(z2) + np.abs(z) + np.abs(g_))
            return z2, n2, f_z_, f_n
        new["zV"], new["nV"] = np.array(state["zV"], d), np.array(state["nV"], d)
        new["zw"], new["nw"] = np.array(state["zw"], d), np.array(state["nw"], d)
        zV, nV, floor["zV"], floor["nV"] = upd(new["zV"][urows], new["nV"][urows], dV, fV, V[urows])
        zw, nw, floor["zw"], floor["nw"] = upd(new["zw"][urows], new["nw"][urows], dw, fw, w[urows])
        new["zV"][urows], new["nV"][urows], new["zw"][urows], new["nw"][urows] = zV, nV, zw, nw
        new["zb"], new["nb"], floor["zb"], floor["nb"] = d(state["zb"]), d(state["nb"]), 0.0, 0.0
    else:
        lr = hyper["lr"]
        new["V"], new["w"] = np.array(state["V"], d), np.array(state["w"], d)
        new["V"][urows] -= lr * dV
        new["w"][urows] -= lr * dw
        new["bias"] = d(state["bias"])
        floor["V"], floor["w"] = lr * fV + 2 * EPS32 * np.abs(new["V"][urows]), lr * fw + 2 * EPS32 * np.abs(new["w"][urows])
        floor["bias"] = 0.0
    out["new"], out["floor"] = new, floor
    return out


def assembled_lists(rows, x, item_fields, corr=None):
    """The B B explicit rows of the same batch as B lists of G = B, the positive first: list i is context i with the items of rows
    i, then 0 .. B - 1 without i.  -> (rows [B B, F], x [B B, F], corr [B B] or None, order [B, B]: order[i, p] = the batch row whose
    item sits at position p of list i)"""
    rows, x = np.asarray(rows), np.asarray(x)
    B, F = rows.shape
    item = list(item_fields)
    order = np.stack([np.concatenate([[i], np.delete(np.arange(B), i)]) for i in range(B)])
    lr, lx = np.repeat(rows[:, None, :], B, axis=1), np.repeat(x[:, None, :], B, axis=1)
    lr[:, :, item] = rows[order][:, :, item]
    lx[:, :, item] = x[order][:, :, item]
    lc = None if corr is None else np.asarray(corr, np.float32)[order].reshape(B * B)
    return lr.reshape(B * B, F), lx.reshape(B * B, F), lc, order
