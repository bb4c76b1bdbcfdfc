"""A float64 evaluation of one log-Q corrected list step of the pure FM (fmx_fm_list_forward_q / _step_q) from an fp32 state, with
the fp32 rounding floor of every output: list_f64.list_step_f64 with c_j = z_j - corr_j in the place of z_j in the loss block.  The
forward, the row gradients, the rule blocks and their floors are list_f64's, line for line; `logit` stays the UNCORRECTED z (the
serving score).

The floors.  list_f64's derivation holds with c in the place of z: (b), the epilogue's own arithmetic, is a function of the G values
handed to it whatever they are called.  (a) changes by ONE term: the device forms c_j = fl(z_j - corr_j), one fp32 subtraction of
two fp32 values, off by at most EPS32 |c_j|; corr itself is an fp32 input, exact.  So c_j arrives with the floor
    f_c_j = f_logit_j + EPS32 |c_j|,
and f_c takes f_logit's place in both sums:  f_dz = (sum_l f_c_l / 4 + (1.5 G + 10) EPS32) inv_b  and
f_loss_i = sum_l f_c_l + EPS32 (1.5 G + 4 + 6 |loss_i|).  Nothing is tuned.
Helper module, not collected."""
import numpy as np

from list_f64 import list_loss_f64
from oracle.fm_oracle import EPS32, K_FP32, ftrl_weight


def listq_step_f64(state, rows, x, G, corr, rule, hyper, inv_b=None):
    """list_f64.list_step_f64's arguments and result, with corr [B G] (finite; read as the fp32 values the device gets) subtracted
    from every row's logit in front of the softmax.  out["logit"] and floor["logit"] are the uncorrected forward's."""
    d = np.float64
    rows = np.asarray(rows, dtype=np.int64)
    x = np.asarray(x, dtype=d)
    N, F = rows.shape
    assert G >= 2 and N % G == 0
    corr = np.asarray(corr, dtype=np.float32).astype(d).reshape(N)
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
    c = logit - corr
    loss_i, g = list_loss_f64(c.reshape(B, G))
    f_z = (f_logit + EPS32 * np.abs(c)).reshape(B, G).sum(axis=1)     # sum_l f_c_l of every list: f_logit_l + EPS32 |c_l|
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
