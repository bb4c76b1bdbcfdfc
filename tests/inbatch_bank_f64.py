"""A float64 evaluation of one in-batch step WITH a cross-batch item bank (fmx_fm_inbatch_bank_*, include/fmx.h) from an fp32 state,
with the fp32 rounding floor of every output.  Built on inbatch_f64: the forwards, the in-batch scores and their floors are
inbatch_step_f64's own (it is called, not restated); the loss block, the side gradients and what follows are its blocks run over
E_i + Q_i, term for term.  Nothing is tuned.

What the bank adds.  bank = dict(S [count, >= k] fp32, a [count] fp32, corr [count] fp32 or None, key [count] or None, M): the VALID
slots in slot order and the capacity.  S, a and corr are fp32 DATA: they carry no forward floor.
 (score)  score(i, q) = (a_u[i] + bank.a[q]) + the fma chain: inbatch_f64's f_s with f_ac = 0 and fS_c = 0,
         f_s_iq = f_au_i + sum_d fS_u |bank.S| + (kp + 2) u (sum_d |S_u bank.S| + |a_u| + |bank.a|),
     and c_iq = fl(score - bank.corr[q]) adds u |c_iq| (corr's one rounding).
 (loss)  inbatch_f64's (a) and (b) over E_i + Q_i: G_i = |E_i| + |Q_i|, the same A_i, f_g and f_loss; a bank column is never the
     diagonal, so f_g_iq is the off-diagonal form.
 (side gradients)  gSu[i] = sum_j g_ij S_c[j] + sum_q g_iq bank.S[q]: the bank's terms move by f_g |bank.S| alone (bank.S is exact),
     and the sum's order is the batch's ranges then the bank's: per + splits terms, then per_q + splits_q more, so the depth is
     (per + splits) + (per_q + splits_q).  gSc and gac keep inbatch_f64's form and depth; they change only through g.
Helper module, not collected."""
import numpy as np

from inbatch_f64 import eligible, geometry, inbatch_step_f64
from oracle.fm_oracle import EPS32, K_FP32


def bank_geometry(M):
    """(splits_q, per_q) of include/fmx.h: the in-batch formula on the capacity M, whatever the count"""
    return geometry(M)


def ring_push(ring, B):
    """The numpy model of the ring: ring = dict(M, head, count, slots: list of length M) -> the slots batch rows 0 .. B - 1 are
    written to; head and count advance (B <= M)."""
    M = ring["M"]
    assert 1 <= B <= M
    slots = [(ring["head"] + j) % M for j in range(B)]
    ring["head"] = (ring["head"] + B) % M
    ring["count"] = min(M, ring["count"] + B)
    return slots


def inbatch_bank_step_f64(state, rows, x, item_fields, rule, hyper, bank, corr=None, key=None, inv_b=None, kp=None):
    """inbatch_step_f64's arguments and `bank` (above).  Returns its dict with the loss block and everything behind it evaluated
    over E_i + Q_i, plus bank_score [B, count] and its floor."""
    d = np.float64
    u = EPS32
    base = inbatch_step_f64(state, rows, x, item_fields, rule, hyper, corr=corr, key=key, inv_b=inv_b, kp=kp)
    rows = np.asarray(rows, dtype=np.int64)
    x = np.asarray(x, dtype=d)
    B, F = rows.shape
    inv_b = 1.0 / B if inv_b is None else inv_b
    item = np.zeros(F, bool)
    item[list(item_fields)] = True
    V, w = base["V"], base["w"]
    k = V.shape[1]
    kp = k if kp is None else kp
    w_eps = 4.0 if rule == "ftrl" else 0.0
    bf = base["floor"]
    Su, au, Sc = base["Su"], base["au"], base["Sc"]
    fSu, f_au, fSc = bf["Su"], bf["au"], bf["Sc"]
    aSu, aSc = np.abs(Su), np.abs(Sc)
    # ---- the scores: the batch's are inbatch_f64's, the bank's have an exact item side ----
    score, f_s = base["score"], bf["score"]
    if corr is None:
        c, f_c = score, f_s
    else:
        cr = np.asarray(corr, dtype=np.float32).astype(d).reshape(B)
        c = score - cr[None, :]
        f_c = f_s + u * np.abs(c)
    bS = np.asarray(bank["S"], dtype=np.float32).astype(d)[:, :k]
    ba = np.asarray(bank["a"], dtype=np.float32).astype(d).reshape(-1)
    Q = ba.shape[0]
    assert bS.shape[0] == Q and Q <= bank["M"]
    assert (bank.get("corr") is None) == (corr is None) and (bank.get("key") is None) == (key is None)
    abS = np.abs(bS)
    bscore = au[:, None] + ba[None, :] + Su @ bS.T
    f_bs = f_au[:, None] + fSu @ abS.T + (kp + 2) * u * (aSu @ abS.T + np.abs(au)[:, None] + np.abs(ba)[None, :])
    if corr is None:
        cq, f_cq = bscore, f_bs
    else:
        bcr = np.asarray(bank["corr"], dtype=np.float32).astype(d).reshape(Q)
        cq = bscore - bcr[None, :]
        f_cq = f_bs + u * np.abs(cq)
    el_q = np.ones((B, Q), bool)
    if key is not None:
        el_q = np.asarray(key).reshape(B)[:, None] != np.asarray(bank["key"]).reshape(Q)[None, :]
    C = np.concatenate([c, cq], axis=1)
    FC = np.concatenate([f_c, f_cq], axis=1)
    EL = np.concatenate([eligible(B, key), el_q], axis=1)
    # ---- the loss block over E_i + Q_i (inbatch_loss_f64 and inbatch_step_f64's floors, the diagonal at column i) ----
    diag = np.arange(B)
    cm = np.where(EL, C, -np.inf)
    m = cm.max(axis=1)
    e = np.where(EL, np.exp(cm - m[:, None]), 0.0)
    s = e.sum(axis=1)
    off = e.copy()
    off[diag, diag] = 0.0
    n = off.sum(axis=1)
    g1 = off / s[:, None]
    g1[diag, diag] = -(n / s)
    loss_b = np.log(s) - (C[diag, diag] - m)
    G = EL.sum(axis=1).astype(d)
    p = e / s[:, None]
    xg = np.where(EL, m[:, None] - C, 0.0)
    fce = np.where(EL, FC, 0.0)
    pf = (p * fce).sum(axis=1)
    A = (p * xg).sum(axis=1) + G + 3
    g = g1 * inv_b
    f_g = (p * (fce + pf[:, None]) + p * u * (xg + 6 + A[:, None])) * inv_b
    f_g[diag, diag] = (p[diag, diag] * (FC[diag, diag] + pf) + u * (2 * A + 2)) * inv_b
    f_lb = pf + FC[diag, diag] + u * (A + 6 * np.abs(loss_b))
    loss = loss_b.sum() * inv_b
    f_loss = (f_lb.sum() + K_FP32 * np.abs(loss_b).sum()) * inv_b
    # ---- the side gradients ----
    splits, per = geometry(B)
    splits_q, per_q = bank_geometry(bank["M"])
    depth_c = (per + splits) * u
    depth_u = ((per + splits) + (per_q + splits_q)) * u
    gb, gq, fgb, fgq = g[:, :B], g[:, B:], f_g[:, :B], f_g[:, B:]
    agb, agq = np.abs(gb), np.abs(gq)
    gSu = gb @ Sc + gq @ bS
    f_gSu = fgb @ aSc + agb @ fSc + fgq @ abS + depth_u * (agb @ aSc + agq @ abS)
    gSc, gac = gb.T @ Su, gb.sum(axis=0)
    f_gSc = fgb.T @ aSu + agb.T @ fSu + depth_c * (agb.T @ aSu)
    f_gac = fgb.sum(axis=0) + depth_c * agb.sum(axis=0)
    # ---- per-occurrence gradients, row gradients, the rule: inbatch_step_f64's blocks ----
    ev = V[rows] * x[:, :, None]
    xs = x[:, :, None]
    t = Sc[:, None, :] - ev
    E_item = xs * (gac[:, None, None] * t + gSc[:, None, :])
    E_ctx = xs * gSu[:, None, :]
    occ = np.where(item[None, :, None], E_item, E_ctx)
    ax = np.abs(xs)
    f_E_item = ax * (f_gac[:, None, None] * np.abs(t) + np.abs(gac)[:, None, None] * (fSc[:, None, :] + (w_eps + 2) * u * (aSc[:, None, :] + np.abs(ev)))
                     + f_gSc[:, None, :]) + 3 * u * np.abs(E_item)
    f_E_ctx = ax * f_gSu[:, None, :] + u * np.abs(E_ctx)
    f_occ = np.where(item[None, :, None], f_E_item, f_E_ctx)
    urows, inv = np.unique(rows.reshape(-1), return_inverse=True)
    inv = inv.reshape(-1)
    U = len(urows)
    dV, fV = np.zeros((U, k), d), np.zeros((U, k), d)
    np.add.at(dV, inv, occ.reshape(-1, k))
    np.add.at(fV, inv, (f_occ + K_FP32 * np.abs(occ)).reshape(-1, k))
    dw1 = np.where(item[None, :], x * gac[:, None], 0.0)
    f_dw1 = np.where(item[None, :], np.abs(x) * (K_FP32 * np.abs(gac) + f_gac)[:, None], 0.0)
    dw, fw = np.zeros(U, d), np.zeros(U, d)
    np.add.at(dw, inv, dw1.reshape(-1))
    np.add.at(fw, inv, f_dw1.reshape(-1))
    out = dict(base)
    out.update(loss=loss, loss_b=loss_b, m=m, s=s, n=n, g=g, gSu=gSu, gSc=gSc, gac=gac, occ=occ, urows=urows, dV=dV, dw=dw, db=0.0,
               eligible=EL, bank_score=bscore)
    floor = dict(bf)
    floor.update(loss=f_loss, loss_b=f_lb, g=f_g, gSu=f_gSu, gSc=f_gSc, gac=f_gac, occ=f_occ, dV=fV, dw=fw, db=0.0, bank_score=f_bs)
    new = {}
    if rule == "ftrl":
        a = float(np.float32(hyper["alpha"]))

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
