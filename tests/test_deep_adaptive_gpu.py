"""DeepFM / NFM with the network under a persistent rule of its own, on the MI355X: fmx_mlp_section_opt and
fmx_deepfm_stream_opt, the trainer backend and the model classes' fused_optimizer=True.

The float64 statement of a step is torch itself: nn.Linear layers in float64 under torch.optim.Adam / Adagrad / SGD, and
(for whole models) test_adaptive_rules_gpu.TorchDeepFM, synchronised before every step to the device's parameters, moments
and step counts.  Tolerance (test_deepfm_fit_adam_vs_float64_torch's): |delta - delta_ref| <= 1e-4 |delta_ref| + floor +
3e-7 |ref| + 1e-12, floor = the matching one of the three (p, m, v) that _floors returns for g_noise = 1e-6 (|g| + max |g|) per
tensor.  The network's adam is torch.optim.Adam, whose eps enters as eps sqrt(1 - beta2^t) once the denominator is multiplied
through: _floors is handed that eps.  SGD is not one of _floors' rules: p -= lr g has dp/dg = lr, so its floor is lr g_noise
(and under SGD the parameters also equal fmx_mlp_section(lr_apply = lr) bit for bit).
Everything else is bit-level: grads / dz / gbi / loss against fmx_mlp_section(lr_apply = 0), stream == steps, halves == whole,
determinism, guard bands, pickling."""
import ctypes as C
import io
import pickle

import numpy as np
import pytest
import torch

from abi_geometry import Guarded
from test_adaptive_rules_gpu import (CRITEO_SIZES, F32, MIXED_SIZES, TorchDeepFM, _floors, _model_state, moments_table, problem,
                                     state_of)
from test_mlp_gpu import live_units

pytestmark = pytest.mark.gpu

B1, B2 = F32(0.9), F32(0.999)
# the network's learning rates: adam's and adagrad's first steps move EVERY coordinate by about lr, which a unit of fan-in 256
# feels as 256 lr -- at 0.01 the float64 network itself is dead (every relu off, every gradient exactly 0) by the third step
NET_HYP = {"adam": dict(lr=F32(0.001), eps=F32(1e-8), beta1=B1, beta2=B2), "adagrad": dict(lr=F32(0.002), eps=F32(1e-10), beta1=B1, beta2=B2),
           "sgd": dict(lr=F32(0.05), eps=F32(1e-8), beta1=B1, beta2=B2)}


@pytest.fixture(scope="module")
def fmx():
    import fmx as _fmx
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _fmx


def n_params(k, H, L):
    return sum(H * (k if l == 0 else H) + H for l in range(L))


def tensors_of(flat, k, H, L):
    """The flat layout cut into [W_0, b_0, W_1, b_1, ...] (views)."""
    out, off = [], 0
    for l in range(L):
        i = k if l == 0 else H
        out.append(flat[off:off + H * i].reshape(H, i))
        off += H * i
        out.append(flat[off:off + H])
        off += H
    assert off == flat.shape[0]
    return out


def net_floor_hyper(rule, h, t):
    """The hyper-parameters _floors takes for the network: dense adam's eps stands as eps sqrt(1 - beta2^t)."""
    if rule != "adam":
        return h
    return dict(h, eps=h["eps"] * np.sqrt(1.0 - float(h["beta2"]) ** t))


def assert_close(name, a, r, b0, floor):
    a, r, b0 = (np.asarray(v, np.float64) for v in (a, r, b0))
    da, dr = a - b0, r - b0
    tol = 1e-4 * np.abs(dr) + floor + 3e-7 * np.abs(r) + 1e-12
    err = np.abs(da - dr)
    print(f"{name}: max err {err.max():.3e}, max err / tol {np.max(err / tol):.3f}, max |ref delta| {np.abs(dr).max():.3e}")
    assert np.all(err <= tol), f"{name}: {int(np.sum(err > tol))} off, max err {err.max():.3e}, max err / tol {np.max(err / tol):.2f}"


def assert_net_step(what, rule, h, t, before, after, ref, grads, k, H, L):
    """The network's p, m, v after a step (flat float64 arrays in dicts) against the float64 torch step, tensor by tensor."""
    hf = net_floor_hyper(rule, h, t)
    cut = lambda a: tensors_of(np.asarray(a, np.float64), k, H, L)
    for j, (g, m2, v2) in enumerate(zip(cut(grads), cut(ref["m"]), cut(ref["v"]))):
        g_noise = 1e-6 * (np.abs(g) + np.max(np.abs(g)))
        if rule == "sgd":
            floors = (h["lr"] * g_noise, None, None)
        else:
            floors = _floors(rule, hf, t, g, g_noise, m2, v2)
        for name, f in zip(("p", "m", "v"), floors):
            if rule == "sgd" and name != "p":
                np.testing.assert_array_equal(cut(after[name])[j], cut(before[name])[j], err_msg=f"{what}: sgd moved {name}")
                continue
            if rule == "adagrad" and name == "m":
                np.testing.assert_array_equal(cut(after[name])[j], cut(before[name])[j], err_msg=f"{what}: adagrad moved m")
                continue
            assert_close(f"{what} tensor {j} {name}", cut(after[name])[j], cut(ref[name])[j], cut(before[name])[j], f)


def unsafe_samples(p, k, H, L, bi, dbi=None):
    """Samples whose fp32 forward could take a relu on the other side than the float64 forward does.  Across a relu's kink the
    gradient jumps by that sample's whole contribution (1 / B of the batch's: 2.4e-4 at B = 4096), which no rounding floor
    covers -- torch's own fp32 autograd differs from its float64 by that much on such a batch -- so float64 states what the fp32
    kernels must compute only on batches that stay clear of every kink.  The error model is the usual one of fp32 dot products
    with independent roundings, carried through the layers: dz_l^2 = W_l^2 dx_{l-1}^2 + (in_l + 2) 2^-48 (|W_l| |x_{l-1}| + |b_l|)^2,
    dx_l = dz_l on live units, 0 on dead ones (relu), dx_0 = dbi (0 for inputs given in fp32); a sample is unsafe when some
    |z| <= 16 dz (sixteen standard deviations; the worst-case bound, linear in the fan-in at every layer, leaves no sample of
    an 8-layer network)."""
    x = np.asarray(bi, np.float64)
    dx = np.zeros_like(x) if dbi is None else np.asarray(dbi, np.float64)
    bad = np.zeros(x.shape[0], bool)
    ts = tensors_of(np.asarray(p, np.float64), k, H, L)
    for l in range(L):
        W, b = ts[2 * l], ts[2 * l + 1]
        z = x @ W.T + b
        dz = np.sqrt((dx * dx) @ (W * W).T + (W.shape[1] + 2) * 2.0 ** -48 * (np.abs(x) @ np.abs(W).T + np.abs(b)) ** 2)
        bad |= (np.abs(z) <= 16 * dz).any(1)
        x, dx = np.maximum(z, 0.0), np.where(z > 0, dz, 0.0)
    return bad


def draw_clear_of_kinks(rng, p, k, H, L, B, kp):
    """bi [B, kp] (fp32, N(0, 0.25) in the first k columns) with every unsafe sample (unsafe_samples) drawn again."""
    bi = np.zeros((B, kp), np.float32)
    bi[:, :k] = rng.normal(size=(B, k)) * 0.5
    for _ in range(200):
        bad = unsafe_samples(p, k, H, L, bi[:, :k])
        if not bad.any():
            return bi
        bi[bad, :k] = rng.normal(size=(int(bad.sum()), k)) * 0.5
    raise AssertionError("no batch clear of the relu kinks in 200 rounds")


def torch_net_step(rule, h, t, p, m, v, k, H, L, bi, base, y, loss, inv_b):
    """One float64 step of the relu network under torch's own optimizer from (p, m, v, t - 1 steps taken).
    -> (ref dict of flat p, m, v after the step, flat gradient)."""
    pt = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in tensors_of(np.asarray(p, np.float64), k, H, L)]
    if rule == "adam":
        opt = torch.optim.Adam(pt, lr=h["lr"], betas=(h["beta1"], h["beta2"]), eps=h["eps"])
        for q, mm, vv in zip(pt, tensors_of(np.asarray(m, np.float64), k, H, L), tensors_of(np.asarray(v, np.float64), k, H, L)):
            opt.state[q] = dict(step=torch.tensor(float(t - 1)), exp_avg=torch.tensor(mm), exp_avg_sq=torch.tensor(vv))
    elif rule == "adagrad":
        opt = torch.optim.Adagrad(pt, lr=h["lr"], eps=h["eps"])
        for q, vv in zip(pt, tensors_of(np.asarray(v, np.float64), k, H, L)):
            opt.state[q]["sum"] = torch.tensor(vv)
            opt.state[q]["step"] = torch.tensor(float(t - 1))
    else:
        opt = torch.optim.SGD(pt, lr=h["lr"])
    x = torch.tensor(np.asarray(bi, np.float64))
    for l in range(L):
        x = torch.relu(x @ pt[2 * l].t() + pt[2 * l + 1])
    out = torch.tensor(np.asarray(base, np.float64)) + x.sum(1)
    z = torch.sigmoid(out) if loss == "sigmoid" else out
    ls = torch.nn.functional.binary_cross_entropy_with_logits(z, torch.tensor(np.asarray(y, np.float64)), reduction="sum") * inv_b
    ls.backward()
    g = np.concatenate([q.grad.numpy().reshape(-1) for q in pt])
    opt.step()
    flat = lambda ts: np.concatenate([a.detach().numpy().reshape(-1) for a in ts])
    ref = dict(p=flat(pt), m=np.asarray(m, np.float64).copy(), v=np.asarray(v, np.float64).copy())
    if rule == "adam":
        ref["m"], ref["v"] = flat([opt.state[q]["exp_avg"] for q in pt]), flat([opt.state[q]["exp_avg_sq"] for q in pt])
    elif rule == "adagrad":
        ref["v"] = flat([opt.state[q]["sum"] for q in pt])
    return ref, g


# ---------------------------------------------------------------------------------------------------------------
# 1 - 3: fmx_mlp_section_opt
# ---------------------------------------------------------------------------------------------------------------
# (64, 10, 10, 5): the reference's own network, entirely on the scalar path, W_1 at float 110 of the flat buffer (110 % 4 = 2).
# (48, 8, 6, 3): layer 0 on the 16-byte path (in = 8), layers 1 and 2 at floats 54 and 96 with in = 6 (scalar), 54 % 4 = 2.
SHAPES = [(4096, 16, 256, 3), (100, 16, 256, 8), (64, 10, 10, 5), (33, 8, 16, 2), (257, 16, 64, 1), (48, 8, 6, 3)]


@pytest.mark.parametrize("rule", ["adam", "adagrad", "sgd"])
@pytest.mark.parametrize("B,k,H,L", SHAPES)
def test_section_opt_four_steps_vs_float64_torch(fmx, B, k, H, L, rule):
    """Four consecutive fmx_mlp_section_opt steps; before each a float64 torch network + optimizer synchronised to the device's
    params, m, v, step.  On the same inputs grads, dz, gbi, logit and loss equal fmx_mlp_section(lr_apply = 0) bit for bit, and
    under sgd params equal fmx_mlp_section(lr_apply = lr).  params, grads, m and v sit in guard bands."""
    L_ = fmx._lib
    lib = L_.load()
    kp = (k + 3) // 4 * 4
    n = n_params(k, H, L)
    offs = np.cumsum([0] + [H * (k if l == 0 else H) + H for l in range(L)])[:-1]
    if (k, H) in ((10, 10), (8, 6)):
        assert any(o % 4 for o in offs), "this case is here for a layer whose offset in the flat buffer is not a multiple of 4"
    h = NET_HYP[rule]
    torch.manual_seed(B + H + L)
    rng = np.random.default_rng(B * 7 + H)
    p0 = (torch.randn(n) * (1.0 / np.sqrt(H))).numpy()
    bufs = {name: Guarded(4 * n, name=name) for name in ("params", "grads", "m", "v")}
    stream = torch.cuda.current_stream().cuda_stream
    loss_kind = "sigmoid" if H == 10 else "logits"
    for t in range(1, 5):
        if t == 1:
            first = np.zeros((B, kp), np.float32)
            first[:, :k] = rng.normal(size=(B, k)) * 0.5
            bufs["params"].t.copy_(torch.from_numpy(live_units(p0, k, H, L, first[:, :k])))
        bi = draw_clear_of_kinks(rng, bufs["params"].t.cpu().numpy(), k, H, L, B, kp)
        base = (rng.normal(size=B) * 0.3).astype(np.float32)
        y = (rng.uniform(size=B) < 0.3).astype(np.float32)
        bi_d, base_d, y_d = (torch.from_numpy(a).cuda() for a in (bi, base, y))
        before = {name: bufs[kk].t.cpu().numpy().astype(np.float64) for name, kk in (("p", "params"), ("m", "m"), ("v", "v"))}
        # ---- fmx_mlp_section on copies: lr_apply = 0 (the gradient's bits) and, for sgd, lr_apply = lr (the parameters' bits) ----
        outs = {}
        for tag, lr_apply in (("zero", 0.0),) + ((("sgd", h["lr"]),) if rule == "sgd" else ()):
            pc = bufs["params"].t.clone()
            mc = L_.Mlp(pc.data_ptr(), L, k, H, 0)
            ws = torch.empty(int(lib.fmx_mlp_section_workspace_bytes(C.byref(mc), B)) // 4, device="cuda")
            o = dict(grads=torch.zeros(n, device="cuda"), dz=torch.empty(B, device="cuda"), gbi=torch.full((B, kp), 7.0, device="cuda"),
                     logit=torch.empty(B, device="cuda"), loss=torch.zeros(1, device="cuda"), params=pc)
            L_.check(lib.fmx_mlp_section(C.byref(mc), L_.LOSSES[loss_kind], bi_d.data_ptr(), kp, base_d.data_ptr(), y_d.data_ptr(), B,
                                         1.0 / B, ws.data_ptr(), o["logit"].data_ptr(), o["dz"].data_ptr(), o["gbi"].data_ptr(), kp,
                                         o["grads"].data_ptr(), lr_apply, o["loss"].data_ptr(), stream))
            outs[tag] = o
        # ---- the call under test, on the guarded buffers ----
        mg = L_.Mlp(bufs["params"].ptr, L, k, H, 0)
        ws_bytes = int(lib.fmx_mlp_section_workspace_bytes(C.byref(mg), B))
        ws = Guarded(ws_bytes, torch.int32, name="workspace")
        dz, gbi = torch.empty(B, device="cuda"), torch.full((B, kp), 7.0, device="cuda")
        logit, loss_out = torch.empty(B, device="cuda"), torch.zeros(1, device="cuda")
        opt = L_.MlpOpt(bufs["m"].ptr, bufs["v"].ptr, h["lr"], h["eps"], h["beta1"], h["beta2"], L_.RULES[rule], t - 1)
        L_.check(lib.fmx_mlp_section_opt(C.byref(mg), L_.LOSSES[loss_kind], bi_d.data_ptr(), kp, base_d.data_ptr(), y_d.data_ptr(), B,
                                         1.0 / B, ws.ptr, ws_bytes, logit.data_ptr(), dz.data_ptr(), gbi.data_ptr(), kp,
                                         bufs["grads"].ptr, C.byref(opt), loss_out.data_ptr(), stream))
        torch.cuda.synchronize()
        assert opt.step == t - 1, "the step count is the caller's: never written back"
        for g in (*bufs.values(), ws):
            g.check()
        z = outs["zero"]
        for name, got in (("grads", bufs["grads"].t), ("dz", dz), ("gbi", gbi), ("logit", logit), ("loss", loss_out)):
            assert torch.equal(got, z[name]), f"step {t}: {name} differs from fmx_mlp_section(lr_apply = 0)"
        assert torch.equal(z["params"], torch.from_numpy(before["p"].astype(np.float32)).cuda())
        if rule == "sgd":
            assert torch.equal(bufs["params"].t, outs["sgd"]["params"]), f"step {t}: sgd differs from fmx_mlp_section(lr_apply = lr)"
        # ---- float64 torch ----
        ref, g64 = torch_net_step(rule, h, t, before["p"], before["m"], before["v"], k, H, L, bi[:, :k], base, y, loss_kind, 1.0 / B)
        assert all(np.any(a) for a in tensors_of(g64, k, H, L)), "a layer without a live unit"
        after = {name: bufs[kk].t.cpu().numpy().astype(np.float64) for name, kk in (("p", "params"), ("m", "m"), ("v", "v"))}
        assert_net_step(f"{rule} B={B} k={k} H={H} L={L} step {t}", rule, h, t, before, after, ref, g64, k, H, L)


# ---------------------------------------------------------------------------------------------------------------
# 4: fmx_deepfm_stream_opt
# ---------------------------------------------------------------------------------------------------------------
TABLE_HYP = dict(lr=F32(0.01), eps=F32(1e-8), alpha=F32(0.05), beta=F32(1.0), l1=F32(0.001), l2=F32(0.01), beta1=B1, beta2=B2)


def stream_setup(fmx, table_rule, net_rule, k, H, L, B, seed=0):
    """-> (table, engine, hyper, flat params, grads, MlpOpt): seeded, identical for equal arguments."""
    sizes = MIXED_SIZES
    rng = np.random.default_rng(seed)
    if table_rule in ("adam", "adagrad"):
        t = moments_table(fmx, sizes, k, seed=seed)
    else:
        R = sum(sizes)
        V, w = (rng.normal(size=(R, k)) * 0.3).astype(np.float32), (rng.normal(size=R) * 0.3).astype(np.float32)
        if table_rule == "ftrl":
            from oracle import fm_oracle as orc
            hf = {kk: TABLE_HYP[kk] for kk in ("alpha", "beta", "l1", "l2")}
            t = fmx.FlatTable(sizes, k, layout="ftrl", ftrl=hf)
            t.load_ftrl_state(orc.ftrl_z_for_weight(V, **hf), np.full_like(V, 0.1), orc.ftrl_z_for_weight(w, **hf), np.full_like(w, 0.1))
        else:
            t = fmx.FlatTable(sizes, k, layout="weights")
            t.rows[:, :k] = torch.from_numpy(V).cuda()
            t.rows[:, t.kp] = torch.from_numpy(w).cuda()
            t.bias[0] = 0.37
    e = fmx.FMEngine(t, max_batch=B)
    hyp = fmx.Hyper(**TABLE_HYP)
    gen = torch.Generator().manual_seed(seed + 1)
    params = (torch.randn(n_params(k, H, L), generator=gen) * (1.0 / np.sqrt(H))).cuda()
    h = NET_HYP[net_rule]
    opt = fmx.MlpOpt(params.numel(), net_rule, lr=h["lr"], eps=h["eps"], beta1=h["beta1"], beta2=h["beta2"], device="cuda")
    return t, e, hyp, params, torch.zeros_like(params), opt


def snapshot(t, params, opt, losses):
    torch.cuda.synchronize()
    return dict(rows=t.rows.cpu().numpy().copy(), bias=t.bias.cpu().numpy().copy(), params=params.cpu().numpy().copy(),
                m=opt.m.cpu().numpy().copy(), v=opt.v.cpu().numpy().copy(), losses=losses.cpu().numpy().copy(),
                steps=(t.step if t.layout == "moments" else None, opt.step))


def assert_same(a, b, what):
    for kk in a:
        np.testing.assert_array_equal(a[kk], b[kk], err_msg=f"{what}: {kk}")


STREAM_RULES = [("adam", "adam"), ("adagrad", "adagrad"), ("ftrl", "adam"), ("signadam", "sgd")]


@pytest.mark.parametrize("B", [1024, 96])
@pytest.mark.parametrize("table_rule,net_rule", STREAM_RULES)
@pytest.mark.parametrize("fm_term", [True, False], ids=["deepfm", "nfm"])
def test_stream_opt_equals_steps_halves_and_itself(fmx, fm_term, table_rule, net_rule, B):
    """n steps in one fmx_deepfm_stream_opt call == n x (fmx_fm_forward, fmx_mlp_section_opt, fmx_sort_occurrences, fmx_fm_update)
    with both step counts advanced by hand == two calls of n / 2 == a second run from the same state, bit for bit in rows, bias,
    params, m, v and the per-step losses; (signadam, sgd) also equals fmx_deepfm_stream.  NFM on FTRL tables stays refused.
    B = 1024: the sorts on the side stream; B = 96: everything on one stream."""
    k, H, L, n_pool, n = 16, 64, 2, 3, 6
    loss = "sigmoid"
    pool = [problem(MIXED_SIZES, k, B, 4000 + B + j) for j in range(n_pool)]
    idx_pool = torch.from_numpy(np.stack([p[1] for p in pool])).cuda()
    y_pool = torch.from_numpy(np.stack([p[3] for p in pool])).cuda()

    def run_stream(calls, use_opt=True):
        t, e, hyp, params, grads, opt = stream_setup(fmx, table_rule, net_rule, k, H, L, B)
        losses = torch.zeros(n, device="cuda")
        done = 0
        for c in calls:
            ip, yp = torch.roll(idx_pool, -(done % n_pool), 0).contiguous(), torch.roll(y_pool, -(done % n_pool), 0).contiguous()
            run = e.prepare_deepfm_stream(hyp, table_rule, loss, params, grads, k, H, L, NET_HYP[net_rule]["lr"], ip, yp,
                                          loss_out=losses[done:done + c], fm_term=fm_term, mlp_opt=opt if use_opt else None)
            run(c)
            done += c
        e.check_error_flag()
        if not use_opt:
            opt.step = n
        return snapshot(t, params, opt, losses)

    if not fm_term and table_rule == "ftrl":
        with pytest.raises(fmx._lib.FmxError) as ei:
            run_stream([n])
        assert ei.value.code == fmx._lib.ERR_UNSUPPORTED
        return
    whole = run_stream([n])
    assert whole["steps"] == (n if table_rule in ("adam", "adagrad") else None, n)
    # ---- the same steps call by call ----
    t, e, hyp, params, grads, opt = stream_setup(fmx, table_rule, net_rule, k, H, L, B)
    losses = torch.zeros(n, device="cuda")
    for s in range(n):
        idx, y = idx_pool[s % n_pool], y_pool[s % n_pool]
        e.forward(hyp, idx, None, want_first=False, want_bi=True)
        base = e.logit[:B] if fm_term else e.sfirst[:B] + t.bias[0]
        loss_s, dz, gbi = e.mlp_section(params, grads, k, H, L, loss, e.bi[:B], base.contiguous(), y, B, 1.0 / B, mlp_opt=opt)
        losses[s] = loss_s[0]
        e.sort(idx)
        e.update(hyp, table_rule, B, None, dz, dz if fm_term else None, gbi, with_loss=False)
        assert opt.step == s + 1
    e.check_error_flag()
    assert_same(whole, snapshot(t, params, opt, losses), "one call vs steps")
    assert_same(whole, run_stream([n // 2, n - n // 2]), "one call vs two halves")
    assert_same(whole, run_stream([n]), "two runs")
    assert np.any(whole["m"]) == (net_rule == "adam") and np.any(whole["v"]) == (net_rule != "sgd")
    if (table_rule, net_rule) == ("signadam", "sgd"):
        assert_same(whole, run_stream([n], use_opt=False), "fmx_deepfm_stream_opt vs fmx_deepfm_stream")


# ---------------------------------------------------------------------------------------------------------------
# 5, 6: the model classes (fused_optimizer=True) and the trainer against TorchDeepFM in float64
# ---------------------------------------------------------------------------------------------------------------
class TorchNFM(TorchDeepFM):
    """NFMAdam's forward on TorchDeepFM's modules: first-order + bias + the network on bi (no sum of bi itself)."""

    def forward(self, idx, x):
        F = idx.shape[1]
        e = torch.stack([self.second[f](idx[:, f]) * x[:, f:f + 1] for f in range(F)], 1)
        fo = sum(self.first[f](idx[:, f])[:, 0] * x[:, f] for f in range(F))
        S = e.sum(1)
        h = 0.5 * (S * S - (e * e).sum(1))
        for layer in self.hidden:
            h = torch.relu(layer(h))
        return fo + self.bias(torch.zeros(idx.shape[0], dtype=torch.long))[:, 0] + h.sum(1)


def float64_model_step(sizes, k, H, L, fm_term, loss_kind, rule, th, nh, s, st, net, idx, x, y):
    """One float64 step of the whole model from the device's state: st (state_of the table), net (flat p, m, v as float64), s - 1
    steps taken.  Tables: SparseAdam / Adagrad (th); hidden layers: Adam / Adagrad (nh).
    -> dict(V, w, bias: (new, grad, m2, v2); net: (ref dict, flat grad))."""
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    ref = (TorchDeepFM if fm_term else TorchNFM)(sizes, k, [(k, H)] + [(H, H)] * (L - 1))
    with torch.no_grad():
        for f in range(len(sizes)):
            lo, hi = int(offs[f]), int(offs[f + 1])
            ref.first[f].weight.copy_(torch.from_numpy(st["w"][lo:hi]).reshape(-1, 1))
            ref.second[f].weight.copy_(torch.from_numpy(st["V"][lo:hi]))
        ref.bias.weight.fill_(float(st["bias"]))
        for a, src in zip(ref.hidden.parameters(), tensors_of(net["p"], k, H, L)):
            a.copy_(torch.from_numpy(np.ascontiguousarray(src)))
    tp = [p for mod in (*ref.first, *ref.second, ref.bias) for p in mod.parameters()]
    hp = list(ref.hidden.parameters())
    if rule == "adam":
        sp = torch.optim.SparseAdam(tp, lr=th["lr"], betas=(th["beta1"], th["beta2"]), eps=th["eps"])
        ad = torch.optim.Adam(hp, lr=nh["lr"], betas=(nh["beta1"], nh["beta2"]), eps=nh["eps"])
    else:
        sp = torch.optim.Adagrad(tp, lr=th["lr"], eps=th["eps"])
        ad = torch.optim.Adagrad(hp, lr=nh["lr"], eps=nh["eps"])
    mk, vk = ("exp_avg", "exp_avg_sq") if rule == "adam" else (None, "sum")

    def put(opt, p, mm, vv, step):
        stt = dict(step=step, **{vk: torch.from_numpy(np.ascontiguousarray(vv, dtype=np.float64)).reshape(p.shape).clone()})
        if mk:
            stt[mk] = torch.from_numpy(np.ascontiguousarray(mm, dtype=np.float64)).reshape(p.shape).clone()
        opt.state[p] = stt
    if s > 1:
        tstep = (s - 1) if rule == "adam" else torch.tensor(float(s - 1))
        for f in range(len(sizes)):
            lo, hi = int(offs[f]), int(offs[f + 1])
            put(sp, ref.first[f].weight, st["mw"][lo:hi, None], st["vw"][lo:hi, None], tstep)
            put(sp, ref.second[f].weight, st["mV"][lo:hi], st["vV"][lo:hi], tstep)
        put(sp, ref.bias.weight, np.array([[st["mb"]]]), np.array([[st["vb"]]]), tstep)
        for a, mm, vv in zip(hp, tensors_of(net["m"], k, H, L), tensors_of(net["v"], k, H, L)):
            put(ad, a, mm, vv, torch.tensor(float(s - 1)))
    z = ref(torch.from_numpy(idx.astype(np.int64)), torch.from_numpy(x.astype(np.float64)))
    yy = torch.from_numpy(y.astype(np.float64))
    loss = torch.nn.functional.binary_cross_entropy_with_logits(torch.sigmoid(z) if loss_kind == "sigmoid" else z, yy)
    loss.backward()
    dense = lambda mods: torch.cat([mod.weight.grad.to_dense() for mod in mods]).numpy()
    gV, gw, gb = dense(ref.second), dense(ref.first)[:, 0], float(ref.bias.weight.grad.to_dense()[0, 0])
    gnet = np.concatenate([p.grad.numpy().reshape(-1) for p in hp])
    sp.step()
    ad.step()
    dn = lambda v: (v.to_dense() if v.is_sparse else v).numpy()
    cat = lambda mods, kk: np.concatenate([dn(sp.state[mod.weight][kk]) for mod in mods]) if kk else None
    flat = lambda ts: np.concatenate([t_.detach().numpy().reshape(-1) for t_ in ts])
    netref = dict(p=flat(hp), m=net["m"].copy(), v=flat([ad.state[p][vk] for p in hp]))
    if mk:
        netref["m"] = flat([ad.state[p][mk] for p in hp])
    first = lambda a: None if a is None else a[:, 0]
    return dict(V=(torch.cat([mod.weight.detach() for mod in ref.second]).numpy(), gV, cat(ref.second, mk), cat(ref.second, vk)),
                w=(torch.cat([mod.weight.detach()[:, 0] for mod in ref.first]).numpy(), gw, first(cat(ref.first, mk)), first(cat(ref.first, vk))),
                bias=(float(ref.bias.weight.detach()[0, 0]), gb, None if not mk else dn(sp.state[ref.bias.weight][mk]),
                      dn(sp.state[ref.bias.weight][vk])),
                net=(netref, gnet))


def assert_model_step(what, rule, th, nh, s, st, after, net_before, net_after, r, k, H, L):
    """Tables vs SparseAdam / Adagrad (the parameters, as test_deepfm_fit_adam_vs_float64_torch), hidden vs Adam / Adagrad (p, m, v)."""
    for name in ("V", "w", "bias"):
        new, g, m2, v2 = r[name]
        g = np.asarray(g, np.float64)
        g_noise = 1e-6 * (np.abs(g) + np.max(np.abs(g)))
        m2 = np.zeros_like(g) if m2 is None else np.asarray(m2, np.float64).reshape(g.shape)
        fp = _floors(rule, th, s, g, g_noise, m2, np.asarray(v2, np.float64).reshape(g.shape))[0]
        assert_close(f"{what} {name}", after[name], new, st[name], fp)
    assert_net_step(f"{what} hidden", rule, nh, s, net_before, net_after, r["net"][0], r["net"][1], k, H, L)


def model_net(m):
    f = m._mlp_fused
    return {"p": m._mlp_flat.detach().cpu().numpy().astype(np.float64), "m": f.m.cpu().numpy().astype(np.float64),
            "v": f.v.cpu().numpy().astype(np.float64)}


def model_hypers(rule, lr, b1, b2):
    eps = F32(1e-8) if rule == "adam" else F32(1e-10)
    h = dict(lr=F32(lr), beta1=b1, beta2=b2, eps=eps)
    return h, dict(h)


@pytest.mark.parametrize("rule", ["adam", "adagrad"])
@pytest.mark.parametrize("cls", ["DeepFMAdam", "NFMAdam"])
def test_model_fit_fused_vs_float64_torch(fmx, cls, rule):
    """Three fit() steps at B = 64 of DeepFMAdam / NFMAdam(fused_optimizer=True): the tables through fmx_fm_update, the hidden
    layers through fmx_mlp_section_opt, each step against TorchDeepFM in float64 synchronised to the model before it (the loss
    is the class's own: BCEwl(sigmoid(forward)) for DeepFMAdam, BCEwl(forward) for NFMAdam)."""
    from models.models_online_deep.deepfm_adam import DeepFMAdam
    from models.models_online_deep.nfm_adam import NFMAdam
    M = {"DeepFMAdam": DeepFMAdam, "NFMAdam": NFMAdam}[cls]
    sizes, k, H, L, B, lr = MIXED_SIZES, 8, 16, 2, 64, 0.01
    torch.manual_seed(1)
    m = M(sizes, embedding_size=k, num_hidden_layers=L, neuron_per_hidden_layer=H, n=lr, batch_size=B, update_rule=rule,
          fused_optimizer=True)
    assert m._mlp_opt is None and m._mlp_fused is not None, "fused_optimizer=True: no torch optimizer"
    th, nh = model_hypers(rule, lr, *m._betas())
    for s in range(1, 4):
        _, idx, x, y = problem(sizes, k, B, 40 + s)
        st, nb = _model_state(m), model_net(m)
        m.fit(idx, x, y)
        torch.cuda.synchronize()
        assert m._table.step == s and m._mlp_fused.step == s
        r = float64_model_step(sizes, k, H, L, m._fm_term_in_forward, m._loss_fit, rule, th, nh, s, st, nb, idx, x, y)
        assert_model_step(f"{cls} {rule} step {s}", rule, th, nh, s, st, _model_state(m), nb, model_net(m), r, k, H, L)
    osd = m.optimizer_state_dict()["mlp"]
    assert set(osd) == {"m", "v", "step"} and osd["step"] == 3 and osd["m"].device.type == "cpu" and osd["m"].dim() == 1
    assert osd["v"].numel() == m._mlp_flat.numel()


@pytest.mark.parametrize("cls,rule", [("DeepFMAdam", "adam"), ("DeepFMAdam", "adagrad"), ("NFMAdam", "adam")])
def test_pickle_mid_run_resumes_bit_for_bit_fused(fmx, cls, rule):
    from models.models_online_deep.deepfm_adam import DeepFMAdam
    from models.models_online_deep.nfm_adam import NFMAdam
    M = {"DeepFMAdam": DeepFMAdam, "NFMAdam": NFMAdam}[cls]
    sizes, k, B = MIXED_SIZES, 8, 32
    torch.manual_seed(3)
    m = M(sizes, embedding_size=k, n=0.01, update_rule=rule, num_hidden_layers=2, neuron_per_hidden_layer=16, batch_size=B,
          fused_optimizer=True)
    batches = [problem(sizes, k, B, 600 + s) for s in range(6)]
    for _, idx, x, y in batches[:3]:
        m.fit(idx, x, y)
    buf = io.BytesIO()
    pickle.dump(m, buf)
    m2 = pickle.loads(buf.getvalue())
    assert m2.fused_optimizer and m2._mlp_opt is None
    assert m2._table.step == m._table.step == 3 and m2._mlp_fused.step == m._mlp_fused.step == 3
    for mm in (m, m2):
        for _, idx, x, y in batches[3:]:
            mm.fit(idx, x, y)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(m._table.rows.cpu().numpy(), m2._table.rows.cpu().numpy())
    np.testing.assert_array_equal(m._table.bias.cpu().numpy(), m2._table.bias.cpu().numpy())
    np.testing.assert_array_equal(m._mlp_flat.cpu().numpy(), m2._mlp_flat.cpu().numpy())
    np.testing.assert_array_equal(m._mlp_fused.m.cpu().numpy(), m2._mlp_fused.m.cpu().numpy())
    np.testing.assert_array_equal(m._mlp_fused.v.cpu().numpy(), m2._mlp_fused.v.cpu().numpy())
    st = m.optimizer_state_dict()
    assert st["table"]["step"] == 6 and st["mlp"]["step"] == 6 and set(m.state_dict()) == set(m2.state_dict())


def test_default_keeps_the_torch_optimizer(fmx):
    from models.models_online_deep.deepfm_adam import DeepFMAdam
    from models.models_online_deep.fm_adam import FMAdam
    torch.manual_seed(0)
    m = DeepFMAdam(MIXED_SIZES, embedding_size=8, num_hidden_layers=2, neuron_per_hidden_layer=16, update_rule="adam")
    assert not m.fused_optimizer and isinstance(m._mlp_opt, torch.optim.Adam) and m._mlp_fused is None
    m = DeepFMAdam(MIXED_SIZES, embedding_size=8, num_hidden_layers=2, neuron_per_hidden_layer=16, update_rule="adagrad",
                   fused_optimizer=False)
    assert isinstance(m._mlp_opt, torch.optim.Adagrad) and m._mlp_fused is None
    for bad in (lambda: DeepFMAdam(MIXED_SIZES, embedding_size=8, update_rule="signadam", fused_optimizer=True),
                lambda: FMAdam(MIXED_SIZES, embedding_size=8, update_rule="adam", fused_optimizer=True)):
        with pytest.raises(ValueError):
            bad()


def test_full_size_trainer_adam_step_vs_float64(fmx):
    """BASELINE configs[3] once: the Criteo-39 table (1,006,628 rows), k = 16, 3 x 256, B = 4096; one adam step through
    DeepFMTrainer on a HipDeepOptBackend against float64, every row compared (the untouched ones must not move)."""
    sizes, k, H, L, B, lr = CRITEO_SIZES, 16, 256, 3, 4096, F32(0.01)
    t = moments_table(fmx, sizes, k, seed=3)
    eng = fmx.FMEngine(t, max_batch=B)
    th = dict(lr=lr, eps=F32(1e-8), beta1=B1, beta2=B2)
    hyp = fmx.Hyper(**th)
    torch.manual_seed(7)
    layers = [torch.nn.Linear(k if l == 0 else H, H).cuda() for l in range(L)]
    opt = fmx.MlpOpt(n_params(k, H, L), "adam", lr=lr, eps=th["eps"], beta1=B1, beta2=B2, device="cuda")
    tr = fmx.DeepFMTrainer(fmx.HipDeepOptBackend(eng, hyp, "adam", opt), layers, k, t.kp, mlp_lr=lr, fm_term=True, loss="logits")
    assert tr.native
    _, idx, _, y = problem(sizes, k, B, 71)
    x = np.ones(idx.shape, np.float32)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    st = state_of(t)
    for rnd in range(1, 50):      # samples that could cross a relu's kink in fp32 (unsafe_samples) are drawn again
        e_ = st["V"][idx.astype(np.int64) + offs[:-1][None, :]]                    # [B, F, k], x = 1
        S_, Sa_, ss_ = e_.sum(1), np.abs(e_).sum(1), (e_ * e_).sum(1)
        dbi = np.sqrt(len(sizes) + 2.0) * 2.0 ** -24 * 0.5 * (Sa_ * Sa_ + ss_)     # bi = 0.5 (S^2 - sum e^2) in fp32, the same model
        bad = unsafe_samples(tr.flat.cpu().numpy(), k, H, L, 0.5 * (S_ * S_ - ss_), dbi)
        if not bad.any():
            break
        idx[bad] = problem(sizes, k, B, 71 + 1000 * rnd)[1][bad]
    assert not bad.any()
    idx_d, _, y_d = eng.to_device(idx, None, y)
    net = lambda: {"p": tr.flat.cpu().numpy().astype(np.float64), "m": opt.m.cpu().numpy().astype(np.float64),
                   "v": opt.v.cpu().numpy().astype(np.float64)}
    nb = net()
    tr.step(idx_d, y_d)
    torch.cuda.synchronize()
    eng.check_error_flag()
    assert t.step == 1 and opt.step == 1
    after = state_of(t)
    touched = np.unique(idx.astype(np.int64) + offs[:-1][None, :])
    untouched = np.setdiff1d(np.arange(t.n_rows), touched)
    for kk in ("V", "w", "mV", "vV", "mw", "vw"):
        np.testing.assert_array_equal(after[kk][untouched], st[kk][untouched], err_msg=f"untouched rows moved ({kk})")
    r = float64_model_step(sizes, k, H, L, True, "logits", "adam", th, dict(th), 1, st, nb, idx, x, y)
    assert_model_step("criteo trainer adam", "adam", th, dict(th), 1, st, after, nb, net(), r, k, H, L)
