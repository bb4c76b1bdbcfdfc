"""The one-workgroup MLP kernels (k_mlp_small: fmx_mlp_forward, fmx_mlp_fit, fmx_mlp_hedge_fit) against a float64 autograd
statement of the same network (helpers.mlp_f64), across the shapes the host accepts and one past each limit; and the online loop
(fmx_online_run_mlp: k_online_mlp, one workgroup walking the stream, or per-sample launches) on both sides of its thresholds, bit
for bit against the per-sample launches and, step by step, against the float64 oracle."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import assert_state_close, mlp_f64, oracle_float64

pytestmark = pytest.mark.gpu
LR, EPS = 0.01, 1e-8


@pytest.fixture(scope="module")
def fmx():
    import fmx as _fmx
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _fmx


def make_net(B, k, kp, H, L, seed):
    """Parameters scaled layer by layer so that every layer's output sum (what the logit and Hedge's per-layer sigmoids see)
    is O(1) on these inputs: no saturated sigmoid, live gradients through every layer; biases mostly positive (few dead units)."""
    rng = np.random.default_rng(seed)
    bi = np.zeros((B, kp), np.float32)
    bi[:, :k] = rng.normal(size=(B, k)) * 0.5
    x, parts = bi[:, :k].astype(np.float64), []
    for l in range(L):
        i = k if l == 0 else H
        W = (rng.normal(size=(H, i)) + 0.4) * np.sqrt(2.0 / i)    # mostly positive: sums that do not cancel to noise
        pre = x @ W.T
        b = np.abs(rng.normal(size=H)) * 0.3 * max(float(pre.std()), float(np.abs(pre).mean()), 1e-3)
        if not (pre + b > 0).any(axis=0).all():     # a unit dead for every sample would hide its whole row of the gradient
            W, pre = -W, -pre
        h = np.maximum(pre + b, 0.0)
        s = 0.7 / max(float(np.abs(h.sum(1)).mean()), 1e-3)
        W, b = (W * s).astype(np.float32), (b * s).astype(np.float32)
        x = np.maximum(x @ W.astype(np.float64).T + b, 0.0)
        parts += [W.reshape(-1), b]
    params = np.concatenate(parts).astype(np.float32)
    base = (rng.normal(size=B) * 0.3).astype(np.float32)
    y = (rng.uniform(size=B) < 0.4).astype(np.float32)
    return params, bi, base, y


def split(flat, k, H, L):
    """flat parameters (or gradients) -> {"W0": [H, k], "b0": [H], ...}"""
    out, off = {}, 0
    for l in range(L):
        i = k if l == 0 else H
        out[f"W{l}"] = np.asarray(flat[off:off + H * i]).reshape(H, i); off += H * i
        out[f"b{l}"] = np.asarray(flat[off:off + H]); off += H
    return out


def close(a, b, what, rel=2e-5, floor=0.0):
    """|a - b| <= rel * max |b| (the tensor's own maximum) + floor, element by element."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, f"{what}: shape {a.shape} vs {b.shape}"
    err = np.abs(a - b)
    tol = rel * max(float(np.abs(b).max()), 1e-30) + floor
    assert (err <= tol).all(), f"{what}: max err {err.max():.3e}, max |ref| {np.abs(b).max():.3e}"


def check_params(got, p0, ref_grads, gnoise, k, H, L, rule, lr, what):
    """Parameters after the step against p0 - lr * rule(g) of the float64 gradients, layer by layer (helpers.assert_state_close
    with the previous state).  Under the sign rule the tolerance widens where |g| ~ eps by four times the fp32 rounding noise
    expected in g (helpers.mlp_f64's gnoise)."""
    got, prev = split(got, k, H, L), split(p0, k, H, L)
    for l in range(L):
        for key, g, gn in ((f"W{l}", ref_grads[l][0], gnoise[l][0]), (f"b{l}", ref_grads[l][1], gnoise[l][1])):
            p = prev[key].astype(np.float64)
            step = g if rule == "sgd" else g / (np.abs(g) + EPS)
            sign = (lr, EPS, 4 * gn) if rule == "signadam" else None
            assert_state_close({key: got[key]}, {key: p - lr * step}, {key: prev[key]}, what=what, sign_rule=sign)


def assert_live(r, L, what):
    """Every layer's float64 gradient has non-zero W and b entries: no dead layer that a skipped or mis-indexed one would match."""
    for l in range(L):
        assert np.any(r["grads"][l][0]) and np.any(r["grads"][l][1]), f"{what}: layer {l} has no live unit"


def alloc(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


FIT_SHAPES = [  # B, k, kp, H, L
    (1, 1, 4, 1, 1),        # every dimension at its smallest
    (16, 63, 64, 64, 1),    # the fit limits: B = 16, k = 63 (the loss parked in column 63), H = 64
    (16, 10, 16, 64, 8),    # eight layers at the widest
    (5, 4, 4, 33, 3),       # odd widths
    (16, 62, 64, 64, 2),    # 8,192 parameters
]


@pytest.mark.parametrize("loss", ["logits", "sigmoid"])
@pytest.mark.parametrize("rule", ["signadam", "sgd"])
@pytest.mark.parametrize("B,k,kp,H,L", FIT_SHAPES)
def test_mlp_fit_vs_f64(fmx, B, k, kp, H, L, rule, loss):
    """fmx_mlp_fit: dz, gbi (padding columns exactly 0), the mean loss and the parameters after the step under the fresh-Adam
    sign rule and SGD, both losses."""
    params, bi, base, y = make_net(B, k, kp, H, L, seed=B * 1000 + k * 10 + L)
    p_d, bi_d, base_d, y_d = alloc(params, bi, base, y)
    dz, gbi, loss_out = torch.full((B,), 7.0, device="cuda"), torch.full((B, kp), 7.0, device="cuda"), torch.zeros(1, device="cuda")
    lib = fmx._lib.load()
    m = fmx._lib.Mlp(p_d.data_ptr(), L, k, H, 0)
    h = fmx.Hyper(lr=LR, eps=EPS)
    fmx._lib.check(lib.fmx_mlp_fit(C.byref(m), h.ref(), fmx._lib.RULES[rule], fmx._lib.LOSSES[loss], bi_d.data_ptr(), kp,
                                   base_d.data_ptr(), y_d.data_ptr(), B, 1.0 / B, dz.data_ptr(), gbi.data_ptr(), loss_out.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    r = mlp_f64(params, k, H, L, bi[:, :k], base, y, loss, 1.0 / B)
    assert_live(r, L, "fit")
    close(dz.cpu().numpy(), r["dz"], "dz")
    close(loss_out.item(), r["loss"], "loss")
    g = gbi.cpu().numpy()
    for c in range(k):
        close(g[:, c], r["gbi"][:, c], f"gbi column {c}")
    assert (g[:, k:] == 0).all(), "gbi padding columns must be exactly 0"
    check_params(p_d.cpu().numpy(), params, r["grads"], r["gnoise"], k, H, L, rule, LR, f"fit {rule} {loss}")


HEDGE_SHAPES = [
    (16, 56, 64, 64, 8),    # k + L = 64: the per-layer losses parked in columns 63 .. 56, next to the last input column
    (1, 4, 4, 10, 5),       # the ONN classes' online step (batch_size 1)
    (5, 4, 4, 33, 3),
    (16, 10, 16, 64, 8),
]


@pytest.mark.parametrize("B,k,kp,H,L", HEDGE_SHAPES)
def test_mlp_hedge_fit_vs_f64(fmx, B, k, kp, H, L):
    """fmx_mlp_hedge_fit: per-layer losses, alpha after the Hedge update and the hidden layers after lr * the gradient of
    sum_l alpha_l loss_l (reference deepfm_onn.py:109-154)."""
    params, bi, base, y = make_net(B, k, kp, H, L, seed=7 + B + k + L)
    alpha0 = np.linspace(0.5, 1.5, L).astype(np.float32)
    alpha0 /= alpha0.sum() * 1.1
    hb, hs = 0.99, 0.2
    p_d, bi_d, base_d, y_d, a_d = alloc(params, bi, base, y, alpha0)
    lout = torch.full((L,), 7.0, device="cuda")
    lib = fmx._lib.load()
    m = fmx._lib.Mlp(p_d.data_ptr(), L, k, H, 0)
    fmx._lib.check(lib.fmx_mlp_hedge_fit(C.byref(m), LR, hb, hs, a_d.data_ptr(), bi_d.data_ptr(), kp, base_d.data_ptr(),
                                         y_d.data_ptr(), B, lout.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    r = mlp_f64(params, k, H, L, bi[:, :k], base, y, hedge_alpha=alpha0)
    assert_live(r, L, "hedge")
    close(lout.cpu().numpy(), r["losses"], "per-layer losses")
    a1 = np.maximum(alpha0.astype(np.float64) * hb ** r["losses"], hs / L)
    close(a_d.cpu().numpy(), a1 / a1.sum(), "alpha")
    check_params(p_d.cpu().numpy(), params, r["grads"], r["gnoise"], k, H, L, "sgd", LR, "hedge")


@pytest.mark.parametrize("want_layers", [False, True])
@pytest.mark.parametrize("B,k,kp,H,L", [(16, 64, 64, 64, 3), (3, 64, 64, 20, 2), (1, 1, 4, 1, 1), (16, 10, 16, 64, 8),
                                        (5, 4, 8, 33, 3)])
def test_mlp_forward_vs_f64(fmx, B, k, kp, H, L, want_layers):
    """fmx_mlp_forward (k = 64 is taken here): the logit and, when asked for, every layer's sigmoid."""
    params, bi, base, _ = make_net(B, k, kp, H, L, seed=B + k + H)
    p_d, bi_d, base_d = alloc(params, bi, base)
    out = torch.full((B,), 7.0, device="cuda")
    layers = torch.full((L, B), 7.0, device="cuda") if want_layers else None
    lib = fmx._lib.load()
    m = fmx._lib.Mlp(p_d.data_ptr(), L, k, H, 0)
    fmx._lib.check(lib.fmx_mlp_forward(C.byref(m), bi_d.data_ptr(), kp, base_d.data_ptr(), B, out.data_ptr(),
                                       layers.data_ptr() if want_layers else None, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    r = mlp_f64(params, k, H, L, bi[:, :k], base)
    assert np.all(r["out"] != base), "the network must contribute to every sample's logit"
    close(out.cpu().numpy(), r["out"], "out")
    if want_layers:
        for l in range(L):
            close(layers.cpu().numpy()[l], r["layers"][l], f"layers_out[{l}]")
    np.testing.assert_array_equal(p_d.cpu().numpy(), params)


@pytest.mark.parametrize("entry,B,k,H,L", [
    ("fit", 17, 4, 8, 2), ("fit", 4, 4, 65, 2), ("fit", 4, 4, 8, 9), ("fit", 4, 64, 8, 1),
    ("hedge", 17, 4, 8, 2), ("hedge", 4, 4, 65, 2), ("hedge", 4, 4, 8, 9), ("hedge", 4, 60, 8, 5),
    ("forward", 17, 4, 8, 2), ("forward", 4, 4, 65, 2), ("forward", 4, 4, 8, 9), ("forward", 4, 65, 8, 1)])
def test_mlp_small_rejects_one_past_each_limit(fmx, entry, B, k, H, L):
    """One past each limit of the one-workgroup kernel (B 17, hidden 65, 9 layers, k 64 for fit / 65 for forward, k + L = 65
    for Hedge): FMX_ERR_UNSUPPORTED, no launch, parameters and alpha bit-unchanged.  Every buffer is sized for the shape asked."""
    kp = max(4, -(-k // 4) * 4)
    params, bi, base, y = make_net(B, k, kp, H, L, seed=3)
    p_d, bi_d, base_d, y_d = alloc(params, bi, base, y)
    alpha = torch.full((L,), 1.0 / (L + 1), device="cuda")
    out = torch.zeros(max(B * kp, L * B), device="cuda")
    out2 = torch.zeros(max(B * kp, L * B), device="cuda")
    lib = fmx._lib.load()
    m = fmx._lib.Mlp(p_d.data_ptr(), L, k, H, 0)
    st = torch.cuda.current_stream().cuda_stream
    if entry == "fit":
        rc = lib.fmx_mlp_fit(C.byref(m), fmx.Hyper(lr=LR).ref(), fmx._lib.RULE_SGD, fmx._lib.LOSS_BCE_LOGITS, bi_d.data_ptr(), kp,
                             base_d.data_ptr(), y_d.data_ptr(), B, 1.0 / B, out.data_ptr(), out2.data_ptr(), None, st)
    elif entry == "hedge":
        rc = lib.fmx_mlp_hedge_fit(C.byref(m), LR, 0.99, 0.2, alpha.data_ptr(), bi_d.data_ptr(), kp, base_d.data_ptr(),
                                   y_d.data_ptr(), B, out.data_ptr(), st)
    else:
        rc = lib.fmx_mlp_forward(C.byref(m), bi_d.data_ptr(), kp, base_d.data_ptr(), B, out.data_ptr(), out2.data_ptr(), st)
    torch.cuda.synchronize()
    assert rc == fmx._lib.ERR_UNSUPPORTED, (entry, rc)
    np.testing.assert_array_equal(p_d.cpu().numpy(), params)
    assert (alpha.cpu().numpy() == np.float32(1.0 / (L + 1))).all()


# ---- the online loop (fmx_online_run_mlp) through the classes ----

def make_model(name, sizes, k, H, L, rule, seed):
    from models.models_online_deep.deepfm_adam import DeepFMAdam
    from models.models_online_deep.nfm_adam import NFMAdam
    from models.models_online_deep.deepfm_onn import DeepFMOnn
    from models.models_online_deep.nfm_onn import NFMOnn
    cls = dict(DeepFMAdam=DeepFMAdam, NFMAdam=NFMAdam, DeepFMOnn=DeepFMOnn, NFMOnn=NFMOnn)[name]
    torch.manual_seed(seed)
    extra = dict(batch_size=1) if name.endswith("Onn") else {}
    m = cls(sizes, embedding_size=k, num_hidden_layers=L, neuron_per_hidden_layer=H, n=LR, update_rule=rule, **extra)
    with torch.no_grad():     # tables small enough that the FM logit stays away from sigmoid's flat ends at every k
        m._table.rows.mul_(0.3)
        m._mlp_flat.mul_(0.5)
    return m


def samples(sizes, N, seed):
    rng = np.random.default_rng(seed)
    Xi = np.stack([rng.integers(0, s, size=N) for s in sizes], axis=1).reshape(N, -1, 1)
    Xv = rng.uniform(0.5, 1.5, size=(N, len(sizes))).astype(np.float32)
    Y = (rng.uniform(size=N) < 0.4).astype(np.float32)
    return Xi, Xv, Y


def online(m, Xi, Xv, Y):
    """fmx_online_run_mlp through the class's engine, as run_experiment calls it -> what forward() returned per sample."""
    idx_d, xv_d, y_d = m._inputs(Xi.tolist(), Xv.tolist(), Y.tolist())
    pred = m._engine.online_run_mlp(m._hyper, m.update_rule, m._loss_fit, m._mlp_flat, m.embedding_size, m.neuron_per_hidden_layer,
                                    m.num_hidden_layers, m._onn, m._fm_term_in_forward, float(m.b.detach()) if m._onn else 0.0,
                                    float(m.s.detach()) if m._onn else 0.0, m.alpha if m._onn else None, idx_d, xv_d, y_d)
    torch.cuda.synchronize()
    m._engine.check_error_flag()
    return pred.cpu().numpy()


def sd_np(m):
    return {kk: v.detach().cpu().numpy() for kk, v in m.state_dict().items()}


ONLINE_CASES = [  # name, fields, k, H, L, rule
    ("DeepFMAdam", 8, 62, 64, 2, "signadam"),     # 8,192 parameters: the last shape kept in LDS
    ("DeepFMAdam", 8, 63, 64, 2, "signadam"),     # 8,256: per-sample launches
    ("NFMAdam", 64, 16, 16, 2, "sgd"),            # kp = 16: 64 fields fill four passes of a wavefront
    ("NFMAdam", 65, 16, 16, 2, "sgd"),            # one field more: per-sample launches
    ("DeepFMAdam", 6, 10, 32, 8, "sgd"),          # eight layers
    ("DeepFMOnn", 6, 56, 16, 8, "signadam"),      # Hedge at k + L = 64
    ("NFMOnn", 65, 16, 8, 3, "signadam"),         # Hedge, one field more than a wavefront takes at kp = 16
]


@pytest.mark.parametrize("name,F,k,H,L,rule", ONLINE_CASES)
def test_online_loop_persistent_equals_per_sample_launches(fmx, name, F, k, H, L, rule):
    """online_persistent 1 (k_online_mlp where the network fits 8,192 floats of LDS and the fields one wavefront) against 0
    (per-sample launches of the forward, k_mlp_small, the sort and the update): predictions, tables, MLP parameters, alpha
    identical bits, on both sides of each threshold."""
    lib = fmx._lib.load()
    sizes = [7 + (3 * f) % 23 for f in range(F)]
    Xi, Xv, Y = samples(sizes, 24, seed=F + k)
    res = []
    for persistent in (1, 0):
        prev = lib.fmx_set_option(b"online_persistent", persistent)
        try:
            m = make_model(name, sizes, k, H, L, rule, seed=11)
            sd0 = sd_np(m)
            pred = online(m, Xi, Xv, Y)
            res.append((pred, sd_np(m)))
        finally:
            lib.fmx_set_option(b"online_persistent", prev)
    np.testing.assert_array_equal(res[0][0], res[1][0], err_msg="predictions")
    for kk in res[1][1]:
        np.testing.assert_array_equal(res[0][1][kk], res[1][1][kk], err_msg=kk)
    assert not np.array_equal(res[0][1]["hidden_layers.0.weight"], sd0["hidden_layers.0.weight"])
    if name.endswith("Onn"):
        assert not np.array_equal(res[0][1]["alpha"], sd0["alpha"])


@pytest.mark.parametrize("name,F,k,H,L", [("DeepFMAdam", 10, 16, 64, 2), ("NFMOnn", 10, 10, 32, 4)])
def test_online_loop_steps_vs_f64_oracle(fmx, name, F, k, H, L):
    """The persistent kernel's state after each of the first 4 samples (one call per sample) against the float64 oracle's
    predict + fit on the same sample: fit under SGD (tables, bias, hidden layers) and Hedge (hidden layers, alpha)."""
    lib = fmx._lib.load()
    sizes = [5 + 2 * f for f in range(F)]
    Xi, Xv, Y = samples(sizes, 4, seed=5)
    prev = lib.fmx_set_option(b"online_persistent", 1)
    try:
        m = make_model(name, sizes, k, H, L, "sgd", seed=13)
        om = oracle_float64().OracleModel(name, sd_np(m), update_rule="sgd")
        for i in range(4):
            before = om.state_dict()
            before = {kk: np.array(v, copy=True) for kk, v in before.items()}
            ref_out = om.forward(Xi[i:i + 1], Xv[i:i + 1])
            ref_pred = ref_out[0] if isinstance(ref_out, tuple) else ref_out
            pred = online(m, Xi[i:i + 1], Xv[i:i + 1], Y[i:i + 1])
            np.testing.assert_allclose(pred, np.asarray(ref_pred, np.float64).reshape(-1), rtol=1e-5, atol=1e-6,
                                       err_msg=f"sample {i}: prediction")
            om.fit(Xi[i:i + 1], Xv[i:i + 1], Y[i:i + 1])
            got, ref = sd_np(m), om.state_dict()
            keys = [kk for kk in ref if kk in got and kk not in ("n", "b", "s")]
            assert_state_close({kk: got[kk] for kk in keys}, {kk: ref[kk] for kk in keys}, {kk: before[kk] for kk in keys},
                               what=f"{name} sample {i}")
    finally:
        lib.fmx_set_option(b"online_persistent", prev)
