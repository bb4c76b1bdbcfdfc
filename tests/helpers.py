"""Shared helpers for the tests (fixture loading, tolerant comparisons)."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CLASS_NAMES = ["FMAdam", "DeepFMAdam", "NFMAdam", "DeepFMOnn", "NFMOnn"]
TAGS = ["criteo39s", "tiny4"]


def load_model_fixture(name, tag):
    z = np.load(os.path.join(GOLDEN, f"{name}_{tag}.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    return z, meta


def sub(z, prefix):
    p = prefix + "/"
    return {k[len(p):]: z[k] for k in z.files if k.startswith(p)}


def assert_close(a, b, rtol=1e-5, atol=0.0, what=""):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, f"{what}: shape {a.shape} vs {b.shape}"
    if a.size == 0:
        return
    scale = max(float(np.max(np.abs(b))), 1e-30)
    err = np.abs(a - b)
    tol = atol + rtol * np.maximum(np.abs(b), 0.0)
    bad = err > tol
    assert not bad.any(), (f"{what}: {int(bad.sum())}/{a.size} off; max abs err {err.max():.3e}, "
                           f"max |ref| {scale:.3e}, worst rel {np.max(err / np.maximum(np.abs(b), 1e-30)):.3e}")


def assert_state_close(sd_a, sd_b, sd_prev=None, rtol=1e-5, what="", sign_rule=None):
    """Parameters after a step: compare the *deltas* (after - before) when the previous state is given, with an
    absolute floor of rtol * lr-sized steps, plus the values themselves.

    sign_rule = (lr, eps, g_noise): the step was p -= lr g / (|g| + eps) (the reference's fresh Adam).  Where |g| is of
    the order of eps the step is as sensitive as a sign function: a gradient that differs by fp32 cancellation noise
    g_noise moves the step by lr eps g_noise / (|g| + eps)^2.  |g| is recovered from the reference's own step
    (|delta| / lr = |g| / (|g| + eps)) and that much is added to the tolerance, element by element."""
    assert set(sd_a.keys()) == set(sd_b.keys()), f"{what}: keys differ: {set(sd_a) ^ set(sd_b)}"
    for k in sd_b:
        a = np.asarray(sd_a[k], dtype=np.float64)
        b = np.asarray(sd_b[k], dtype=np.float64)
        assert a.shape == b.shape, f"{what}/{k}: {a.shape} vs {b.shape}"
        extra = 0.0
        if sd_prev is not None and sign_rule is not None and a.size:
            lr, eps, g_noise = sign_rule
            r = np.minimum(np.abs(b - np.asarray(sd_prev[k], dtype=np.float64)) / lr, 1.0 - 1e-6)
            g = eps * r / (1.0 - r)
            extra = np.minimum(lr * eps * g_noise / (g + eps) ** 2, 2 * lr) * (r > 0)
        err = np.abs(a - b)
        tol = 1e-7 + rtol * np.abs(b) + extra
        assert not (err > tol).any(), (f"{what}/{k}: {int((err > tol).sum())}/{a.size} off; max abs err {err.max():.3e}")
        if sd_prev is not None:
            p = np.asarray(sd_prev[k], dtype=np.float64)
            da, db = a - p, b - p
            dscale = float(np.max(np.abs(db))) if db.size else 0.0
            # deltas are O(lr); fp32 cancellation in (after - before) leaves ~1e-7 * |param| of noise
            atol = max(1e-6 * dscale, 3e-7 * float(np.max(np.abs(b)) if b.size else 0))
            derr = np.abs(da - db)
            dtol = atol + 1e-4 * np.abs(db) + extra
            assert not (derr > dtol).any(), (f"{what}/{k} (delta): {int((derr > dtol).sum())}/{a.size} off; max abs err "
                                             f"{derr.max():.3e}, max |ref delta| {dscale:.3e}")



def assert_within_f64(a, ref, floor, what, rtol=1e-5):
    """|a - ref| <= 1e-5 |ref| + floor, element by element: north_star's tolerance against a float64 evaluation, with the
    fp32 rounding floor of the quantity (oracle.fm_oracle.flat_fm_step_f64 derives it term by term) where the value is a
    cancelled difference."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, f"{what}: shape {a.shape} vs {ref.shape}"
    err = np.abs(a - ref)
    tol = rtol * np.abs(ref) + floor
    bad = err > tol
    assert not bad.any(), (f"{what}: {int(bad.sum())}/{a.size} beyond {rtol:g} rel + fp32 floor; worst err/tol "
                           f"{float((err / np.maximum(tol, 1e-300)).max()):.2f}, max abs err {float(err.max()):.3e}")


def assert_ftrl_step_within_f64(hip, ref, what="", before=None):
    """hip: the (z, n) state after the HIP step as dict(zV [R,k], nV, zw [R], nw, zb, nb); ref: flat_fm_step_f64's result
    for the same step.  Touched rows within 1e-5 + floor of the float64 step, untouched rows bit-identical.
    before: the state the step started from -- then the STEP itself is checked too, |(hip - before) - (ref - before)| <=
    1e-5 |ref - before| + floor: at the headline batch a rarely hit row moves by ~1e-4 in z with |z| ~ 10, inside 1e-5 |z|, so
    the check on values alone would pass a skipped update; the check on the step does not (the floors are those of the
    step's own terms)."""
    u, new, fl = ref["urows"], ref["new"], ref["floor"]
    for kk in ("zV", "nV", "zw", "nw"):
        assert_within_f64(np.asarray(hip[kk])[u], new[kk][u], fl[kk], f"{what}{kk}")
        if before is not None:
            b0 = np.asarray(before[kk], np.float64)[u]
            assert_within_f64(np.asarray(hip[kk], np.float64)[u] - b0, new[kk][u] - b0, fl[kk], f"{what}{kk} (the step)")
        mask = np.ones(len(new[kk]), dtype=bool)
        mask[u] = False
        np.testing.assert_array_equal(np.asarray(hip[kk])[mask], new[kk][mask].astype(np.float32), err_msg=f"{what}{kk} untouched rows")
    assert_within_f64(hip["zb"], new["zb"], fl["zb"], f"{what}zb")
    assert_within_f64(hip["nb"], new["nb"], fl["nb"], f"{what}nb")


def oracle_float64():
    """The oracle's restatement evaluated in FLOAT64: the same source (oracle/fm_oracle.py) with its working type `f32` bound to
    numpy.float64, as a module of its own.  What an fp32 implementation approximates, free of any fp32 summation order -- the
    reference for "within 1e-5 of the float64 value + the fp32 rounding floor" checks of the paths the oracle only has in fp32
    (Hedge backprop).  Test infrastructure, like the oracle itself."""
    import types
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "fm_oracle.py")
    src = open(path).read()
    assert src.count("f32 = np.float32") == 1
    mod = types.ModuleType("fm_oracle_f64")
    mod.__file__ = path
    exec(compile(src.replace("f32 = np.float32", "f32 = np.float64"), path, "exec"), mod.__dict__)
    return mod


def mlp_f64(params, k, H, L, bi, base, y=None, loss="logits", inv_b=1.0, hedge_alpha=None):
    """Float64 torch autograd statement of the relu MLP on bi (reference deepfm_adam.py:79-89,106-119; Hedge backprop
    deepfm_onn.py:109-154).  params: the flat layout (W_l [H, in] then b_l [H] per layer).  Returns a dict:
      out [B] = base + sum x_L ; layers [L, B] = sigmoid(base + sum x_l) ; and with y:
      loss (mean: inv_b * sum), dz [B] = dL/dlogit, gbi [B, k] = dL/dbi, grads = [(dW_l, db_l)], flat (grads in the params
      layout), gnoise = [(noise of dW_l, noise of db_l)]: the fp32 rounding noise to expect in every gradient element
      (_mlp_grad_noise).
    hedge_alpha [L]: Hedge instead -- losses [L] (BCELoss of each layer's sigmoid, mean over the batch) and the gradient of
    sum_l alpha_l losses_l."""
    import torch
    import torch.nn.functional as Fn
    p = torch.as_tensor(np.asarray(params, dtype=np.float64))
    bi = torch.as_tensor(np.asarray(bi, dtype=np.float64)).requires_grad_(True)
    base = torch.as_tensor(np.asarray(base, dtype=np.float64)).requires_grad_(True)
    Ws, bs, off = [], [], 0
    for l in range(L):
        i = k if l == 0 else H
        Ws.append(p[off:off + H * i].view(H, i).clone().requires_grad_(True)); off += H * i
        bs.append(p[off:off + H].clone().requires_grad_(True)); off += H
    xs, x = [bi], bi
    for W, b in zip(Ws, bs):
        x = Fn.relu(x @ W.t() + b)
        xs.append(x)
    r = dict(out=(base + x.sum(1)).detach().numpy(),
             layers=torch.stack([torch.sigmoid(base + a.sum(1)) for a in xs[1:]]).detach().numpy())
    if y is None:
        return r
    yt = torch.as_tensor(np.asarray(y, dtype=np.float64))
    if hedge_alpha is None:
        out = base + x.sum(1)
        z = torch.sigmoid(out) if loss == "sigmoid" else out
        ls = Fn.binary_cross_entropy_with_logits(z, yt, reduction="sum") * inv_b
        r["loss"] = float(ls.detach())
        dlog = [None] * (L - 1) + [torch.autograd.grad(ls, out, retain_graph=True)[0].detach()]
        ls.backward()
        r["dz"] = base.grad.numpy()
        r["gbi"] = bi.grad.numpy()
    else:
        outs = [base + a.sum(1) for a in xs[1:]]
        losses = torch.stack([Fn.binary_cross_entropy(torch.sigmoid(o), yt) for o in outs])
        tot = (torch.as_tensor(np.asarray(hedge_alpha, dtype=np.float64)) * losses).sum()
        dlog = [g.detach() for g in torch.autograd.grad(tot, outs, retain_graph=True)]
        tot.backward()
        r["losses"] = losses.detach().numpy()
    r["grads"] = [(W.grad.numpy(), b.grad.numpy()) for W, b in zip(Ws, bs)]
    r["flat"] = np.concatenate([t.reshape(-1) for pair in r["grads"] for t in pair])
    # |d dL/dlogit_l / d logit_l|: p (1 - p) times alpha_l (Hedge), 1 (logits) or at most 5/4 (the double sigmoid)
    slope = [None if g is None else
             torch.sigmoid(o) * (1 - torch.sigmoid(o)) * (abs(float(hedge_alpha[l])) if hedge_alpha is not None else
                                                          1.25 if loss == "sigmoid" else 1.0)
             for l, (g, o) in enumerate(zip(dlog, [base + a.sum(1) for a in xs[1:]]))]
    r["gnoise"] = _mlp_grad_noise([t.detach().numpy() for t in xs], [W.detach().numpy() for W in Ws],
                                  [b.detach().numpy() for b in bs], [None if g is None else g.numpy() for g in dlog],
                                  [None if c is None else c.detach().numpy() * inv_b for c in slope])
    return r


def _mlp_grad_noise(xs, Ws, bs, dlog, slope):
    """The fp32 rounding noise to expect in each gradient element of the MLP (one standard deviation's worth, per element):
    every sum of n terms adds EPS32 sqrt(n) times the sum of ITS OWN |terms| (a layer's own products, not a chain of |W|),
    and the noise already in its inputs is carried through the same signed products in quadrature (independent roundings:
    sqrt(e^2 . W^2)), forward through the activations and the logit, then backward through dL/dlogit (slope[l]: its
    derivative by logit l, inv_b included) and the dgrad chain.  -> [(noise of dW_l [H, in], noise of db_l [H])]."""
    u = 2.0 ** -24
    L = len(Ws)
    ex = [np.zeros_like(xs[0])]                        # noise of x_l (the input itself is exact)
    for l in range(L):
        W, b, x, e = Ws[l], bs[l], xs[l], ex[l]
        local = u * np.sqrt(W.shape[1] + 1) * (np.abs(x) @ np.abs(W).T + np.abs(b))
        ex.append((local + np.sqrt((e * e) @ (W * W).T)) * (xs[l + 1] > 0))
    def dlog_noise(l):                                 # dL/dlogit_l's own rounding + the logit's noise times its slope
        xo, eo = xs[l + 1], ex[l + 1]
        e_out = u * np.sqrt(xo.shape[1]) * np.abs(xo).sum(1) + np.sqrt((eo * eo).sum(1))
        return 4 * u * np.abs(dlog[l]) + slope[l] * e_out
    d = np.zeros_like(xs[-1])
    e = np.zeros_like(xs[-1])
    out = [None] * L
    for l in range(L - 1, -1, -1):
        if dlog[l] is not None:
            d = d + dlog[l][:, None]
            e = e + dlog_noise(l)[:, None]
        mask = xs[l + 1] > 0
        d, e = d * mask, e * mask
        x, exl, W = xs[l], ex[l], Ws[l]
        B = x.shape[0]
        nW = u * np.sqrt(B) * (np.abs(d).T @ np.abs(x)) + np.sqrt((e * e).T @ (x * x) + (d * d).T @ (exl * exl))
        nb = u * np.sqrt(B) * np.abs(d).sum(0) + np.sqrt((e * e).sum(0))
        out[l] = (nW, nb)
        d, e = d @ W, u * np.sqrt(W.shape[0]) * (np.abs(d) @ np.abs(W)) + np.sqrt((e * e) @ (W * W))
    return out
