"""A float64 evaluation of one pairwise-ranking (BPR) step of the pure FM from an fp32 state, with the fp32 rounding floor of
every output -- built the way oracle.fm_oracle.flat_fm_step_f64 builds the pointwise step: the same EPS32 and K_FP32, the same
term-by-term floors (f_logit, fS, fV, fw, f_db and the rule floors are taken over unchanged); only the loss block differs.

Rows 2i / 2i + 1 of `rows` are the positive / negative sample of pair i; d_i = z[2i] - z[2i + 1],
loss_i = -log(sigmoid(d_i) + margin), the step is that of inv_b * sum_i loss_i.  Helper module, not collected."""
import numpy as np

from oracle.fm_oracle import EPS32, K_FP32, ftrl_weight


def pair_loss_f64(d, margin):
    """-> (loss, dloss/dd) of the logit differences d, in float64 (margin 0: the stable softplus form)."""
    d = np.asarray(d, np.float64)
    sp = 1.0 / (1.0 + np.exp(-d))
    sn = 1.0 / (1.0 + np.exp(d))
    if margin == 0:
        return np.log1p(np.exp(-np.abs(d))) + np.maximum(-d, 0), -sn
    return -np.log(sp + margin), -sp * sn / (sp + margin)


def pair_step_f64(state, rows, x, margin, rule, hyper, inv_b=None):
    """state (NOT mutated): rule 'sgd': V [R,k], w [R], bias; rule 'ftrl': zV, nV [R,k], zw, nw [R], zb, nb.  rows [2B, F]
    global row ids, x [2B, F].  Returns what flat_fm_step_f64 returns: dict(loss, logit, dz, S, urows, dV, dw, db, new, floor)."""
    d = np.float64
    rows = np.asarray(rows, dtype=np.int64)
    x = np.asarray(x, dtype=d)
    B2, F = rows.shape
    assert B2 % 2 == 0 and margin >= 0
    inv_b = 2.0 / B2 if inv_b is None else inv_b
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
    # ---- forward (flat_fm_step_f64's, with its floors) ----
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
    # ---- the pair loss block ----
    dd = logit[0::2] - logit[1::2]
    f_d = f_logit[0::2] + f_logit[1::2]
    loss_i, g = pair_loss_f64(dd, margin)
    dz = np.zeros(B2, d)
    dz[0::2], dz[1::2] = g * inv_b, -(g * inv_b)
    f_dz = np.repeat((0.25 * f_d + 4 * EPS32) * inv_b, 2)             # |dg/dd| <= 1/4 for every margin >= 0
    loss_b = np.zeros(B2, d)
    loss_b[0::2] = loss_i
    f_lb = np.zeros(B2, d)
    f_lb[0::2] = f_d + 4 * EPS32 * (1 + np.abs(loss_i))               # |dloss/dd| <= 1, as in the `logits` branch
    loss = loss_b.sum() * inv_b
    f_loss = (f_lb.sum() + K_FP32 * np.abs(loss_b).sum()) * inv_b
    # ---- row gradients (flat_fm_step_f64's) ----
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
    db = dz.sum()
    fV = np.zeros((U, k), d)
    np.add.at(fV, inv, np.abs(xe) * ((np.abs(Sb) + np.abs(ee)) * (K_FP32 * np.abs(dzb) + fdzb)
                                     + np.abs(dzb) * (fSb + w_eps * EPS32 * np.abs(ee))))
    fw = np.zeros(U, d)
    np.add.at(fw, inv, (np.abs(xe) * (K_FP32 * np.abs(dzb) + fdzb))[:, 0])
    f_db = K_FP32 * np.abs(dz).sum() + f_dz.sum()
    out = dict(loss=loss, logit=logit, dz=dz, S=S, urows=urows, dV=dV, dw=dw, db=db, V=V, w=w, bias=bias)
    floor = dict(loss=f_loss, logit=f_logit, dz=f_dz, S=fS, dV=fV, dw=fw, db=f_db)
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
        new["zb"], new["nb"], floor["zb"], floor["nb"] = upd(d(state["zb"]), d(state["nb"]), db, f_db, bias)
    else:
        lr = hyper["lr"]
        new["V"], new["w"] = np.array(state["V"], d), np.array(state["w"], d)
        new["V"][urows] -= lr * dV
        new["w"][urows] -= lr * dw
        new["bias"] = bias - lr * db
        floor["V"], floor["w"] = lr * fV + 2 * EPS32 * np.abs(new["V"][urows]), lr * fw + 2 * EPS32 * np.abs(new["w"][urows])
        floor["bias"] = lr * f_db + 2 * EPS32 * abs(new["bias"])
    out["new"], out["floor"] = new, floor
    return out
