"""A float64 evaluation of one listwise (sampled-softmax) step of the pure FM from an fp32 state, with the fp32 rounding floor of
every output -- built the way pair_f64.pair_step_f64 builds the pair step: the same EPS32 and K_FP32, the same forward, row-gradient
and rule blocks with their term-by-term floors (f_logit, fS, fV, fw and the rule floors are taken over unchanged); only the loss
block differs, and the bias.

Rows G i .. G i + G - 1 of `rows` are list i, the positive first.  With z_j the logit of row G i + j and p = softmax(z):
    loss_i = -log p_0 = log(sum_j exp(z_j - m)) - (z_0 - m),   dz_j = p_j inv_b (j >= 1),   dz_0 = -(sum_{j>=1} p_j) inv_b,
the step is that of inv_b * sum_i loss_i.  The bias has no gradient (a softmax does not move under a shift of its logits) and the
device step keeps it bit-unchanged: db is DEFINED as 0 here and new["bias"] (new["zb"], new["nb"]) is the old value.

The list floor.  Two sources, added:
 (a) the logits arrive with the forward's floor f_logit.  d p_j / d z_l = p_j (delta_jl - p_l), and p_j (1 - p_j) <= 1/4 as well as
     p_j p_l <= 1/4, so |d dz_j / d z_l| <= inv_b / 4 for every j, l (dz_0 = (p_0 - 1) inv_b has p_0's derivative): dz_j moves by at
     most inv_b / 4 * sum_l f_logit_l over the list's rows.  d loss / d z_l = p_l - delta_l0, of absolute value <= 1: the loss moves by
     at most sum_l f_logit_l.
 (b) the epilogue's own fp32 arithmetic on exact logits, u = EPS32.  t_j = fl(z_j - m) is off by <= u |z_j - m|, which moves
     e_j = exp(t_j) by <= u x exp(-x) <= u / e (x = |z_j - m|); an expf and a logf of <= 2 ulp add 4 u e_j and 4 u |log s|: every e_j is
     within u (0.37 + 4 e_j).  The sum of G such terms, s >= 1, is within u (0.37 G + 4 s) + (G - 1) u s, relative to s within
     u (1.37 G + 3); the negatives' mass likewise.  A quotient e_j / s (one more rounding) is then within
     u (0.37 + 4 p_j) + p_j u (1.37 G + 3) + u p_j <= u (1.37 G + 8.4), and the product with inv_b adds u |dz_j|:
         f_dz  = (sum_l f_logit_l / 4 + (1.5 G + 10) EPS32) inv_b.
     The loss log(s) - (z_0 - m): log moves by the relative error of s, logf adds 4 u log s, t_0 is off by u (m - z_0), the
     subtraction adds u |loss|; log s and m - z_0 are both >= 0 and sum to the loss:
         f_loss_i = sum_l f_logit_l + EPS32 (1.5 G + 4 + 6 |loss_i|).
Helper module, not collected."""
import numpy as np

from oracle.fm_oracle import EPS32, K_FP32, ftrl_weight


def list_loss_f64(z):
    """z [B, G] float64 logits, the positive in column 0 -> (loss [B], dloss/dz [B, G]): softmax cross-entropy against column 0,
    column 0's derivative as minus the negatives' mass."""
    z = np.asarray(z, np.float64)
    m = z.max(axis=1, keepdims=True)
    e = np.exp(z - m)
    s = e.sum(axis=1, keepdims=True)
    g = e / s
    g[:, 0] = -(e[:, 1:].sum(axis=1) / s[:, 0])
    return np.log(s[:, 0]) - (z[:, 0] - m[:, 0]), g


def list_step_f64(state, rows, x, G, rule, hyper, inv_b=None):
    """state (NOT mutated): rule 'sgd': V [R,k], w [R], bias; rule 'ftrl': zV, nV [R,k], zw, nw [R], zb, nb.  rows [B G, F]
    global row ids, x [B G, F].  Returns what pair_step_f64 returns: dict(loss, logit, dz, S, urows, dV, dw, db, new, floor), with
    loss_b [B G] (the per-row loss slots) and floor["loss_b"] besides."""
    d = np.float64
    rows = np.asarray(rows, dtype=np.int64)
    x = np.asarray(x, dtype=d)
    N, F = rows.shape
    assert G >= 2 and N % G == 0
    B = N // G
    inv_b = 1.0 / B if inv_b is None else inv_b
    if rule == "ftrl":
        a, b_, l1, l2 = hyper["alpha"], hyper["beta"], hyper["l1"], hyper["l2"]
        V = ftrl_weight(state["zV"], state["nV"], a, b_, l1, l2, dtype=d)
        w = ftrl_weight(state["zw"], state["nw"], a, b_, l1, l2, dtype=d)
        bias = float(ftrl_weight(state["zb"], state["nb"], a, b_, l1, l2, dtype=d))
        w_eps = 4.0
    elif rule == "sgd":
        V, w, bias = np.asarray(state["V"], d), np.asarray(state["w"], d), float(state["bias"])
        w_eps = 0.0
    else:
        raise ValueError(rule)
    # ---- forward (pair_step_f64's, with its floors) ----
    e = V[rows] * x[:, :, None]
    S = e.sum(axis=1)
    SS = (e * e).sum(axis=1)
    bi = 0.5 * (S * S - SS)
    first = w[rows] * x
    logit = first.sum(axis=1) + bi.sum(axis=1) + bias
    aS = np.abs(e).sum(axis=1)
    fS = (K_FP32 + w_eps * EPS32) * aS
    f_bi = np.abs(S) * fS + K_FP32 * 0.5 * (S * S + SS) + w_eps * EPS32 * SS
    f_logit = f_bi.sum(axis=1) + (K_FP32 + w_eps * EPS32) * (np.abs(first).sum(axis=1) + abs(bias)) + K_FP32 * np.abs(bi).sum(axis=1)
    # ---- the list loss block (the floors: the docstring) ----
    loss_i, g = list_loss_f64(logit.reshape(B, G))
    f_z = f_logit.reshape(B, G).sum(axis=1)                           # sum_l f_logit_l of every list
    dz = (g * inv_b).reshape(N)
    f_dz = np.repeat((0.25 * f_z + (1.5 * G + 10) * EPS32) * inv_b, G)
    loss_b = np.zeros(N, d)
    loss_b[0::G] = loss_i
    f_lb = np.zeros(N, d)
    f_lb[0::G] = f_z + EPS32 * (1.5 * G + 4 + 6 * np.abs(loss_i))
    loss = loss_b.sum() * inv_b
    f_loss = (f_lb.sum() + K_FP32 * np.abs(loss_b).sum()) * inv_b
    # ---- row gradients (pair_step_f64's) ----
    flat = rows.reshape(-1)
    urows, inv = np.unique(flat, return_inverse=True)
    inv = inv.reshape(-1)
    U, k = len(urows), V.shape[1]
    xe = x.reshape(-1, 1)
    Sb, dzb = np.repeat(S, F, axis=0), np.repeat(dz, F)[:, None]
    fSb, fdzb = np.repeat(fS, F, axis=0), np.repeat(f_dz, F)[:, None]
    ee = e.reshape(-1, k)
    dV = np.zeros((U, k), d)
    np.add.at(dV, inv, xe * (Sb - ee) * dzb)
    dw = np.zeros(U, d)
    np.add.at(dw, inv, (xe * dzb)[:, 0])
    db = 0.0                                                          # by definition: the bias is not part of a list step
    fV = np.zeros((U, k), d)
    np.add.at(fV, inv, np.abs(xe) * ((np.abs(Sb) + np.abs(ee)) * (K_FP32 * np.abs(dzb) + fdzb)
                                     + np.abs(dzb) * (fSb + w_eps * EPS32 * np.abs(ee))))
    fw = np.zeros(U, d)
    np.add.at(fw, inv, (np.abs(xe) * (K_FP32 * np.abs(dzb) + fdzb))[:, 0])
    out = dict(loss=loss, logit=logit, dz=dz, loss_b=loss_b, S=S, urows=urows, dV=dV, dw=dw, db=db, V=V, w=w, bias=bias)
    floor = dict(loss=f_loss, logit=f_logit, dz=f_dz, loss_b=f_lb, S=fS, dV=fV, dw=fw, db=0.0)
    new = {}
    if rule == "ftrl":
        def upd(z, n, g_, fg, wt):
            z, n = np.asarray(z, d), np.asarray(n, d)
            n2 = n + g_ * g_
            sig = (np.sqrt(n2) - np.sqrt(n)) / a
            z2 = z + g_ - sig * wt
            f_n = 2 * np.abs(g_) * fg + fg * fg + 2 * EPS32 * n2
            f_sig = fg / a + 4 * EPS32 * (np.sqrt(n2) + np.sqrt(n)) / a
            f_z = fg + np.abs(wt) * f_sig + (w_eps + 4) * EPS32 * np.abs(sig * wt) + 2 * EPS32 * (np.abs(z2) + np.abs(z) + np.abs(g_))
            return z2, n2, f_z, f_n
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
