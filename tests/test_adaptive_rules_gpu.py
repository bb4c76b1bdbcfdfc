"""The persistent adaptive rules on the MI355X: FMX_RULE_ADAGRAD / FMX_RULE_ADAM on FMX_LAYOUT_MOMENTS tables against the
float64 statement of test_adaptive_rules_cpu.py (itself pinned to torch.optim.SparseAdam / Adagrad), and the bit-level
contracts: untouched rows and pad components, stream == steps, online run == per-sample steps, determinism, resumption."""
import io
import pickle

import numpy as np
import pytest
import torch

from test_adaptive_rules_cpu import flat_adaptive_step, adam_consts

pytestmark = pytest.mark.gpu

CRITEO_SIZES = [63, 113, 126, 51, 224, 148, 100, 79, 104, 9, 32, 57, 82, 1457, 555, 176373, 129683, 305, 19, 11887,
                632, 3, 41738, 5170, 175446, 3170, 27, 11356, 165602, 10, 4641, 2030, 4, 172761, 18, 15, 57903, 86,
                44549]
MIXED_SIZES = [3, 9, 1000, 50000, 4, 17, 200, 31, 7, 2, 1]
# the hyper-parameters as the kernels see them (fp32): the oracle takes the same values
F32 = lambda v: float(np.float32(v))
HYP = {"adam": dict(lr=F32(0.01), beta1=F32(0.9), beta2=F32(0.999), eps=F32(1e-8)),
       "adagrad": dict(lr=F32(0.05), eps=F32(1e-10), beta1=F32(0.9), beta2=F32(0.999))}


@pytest.fixture(scope="module")
def fmx():
    import fmx as _fmx
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _fmx


def problem(sizes, k, B, seed):
    """Zipf-skewed indices (duplicates), real x in [-1, 1] with about 10 % exact zeros."""
    rng = np.random.default_rng(seed)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    idx = np.stack([np.minimum(rng.zipf(1.3, size=B) - 1, s - 1) for s in sizes], axis=1).astype(np.int32)
    x = rng.uniform(-1, 1, size=(B, len(sizes))).astype(np.float32)
    x[rng.uniform(size=x.shape) < 0.1] = 0.0
    y = (rng.uniform(size=B) < 0.3).astype(np.float32)
    return offs, idx, x, y


def moments_table(fmx, sizes, k, seed=0):
    rng = np.random.default_rng(seed)
    t = fmx.FlatTable(sizes, k, layout="moments")
    R = t.n_rows
    t.rows[:, :k] = torch.from_numpy((rng.normal(size=(R, k)) * 0.3).astype(np.float32)).cuda()
    t.rows[:, t.kp] = torch.from_numpy((rng.normal(size=R) * 0.3).astype(np.float32)).cuda()
    t.bias[0] = 0.37
    return t


def state_of(t):
    """The table's parameters and moments as float64 arrays (the oracle's state names)."""
    r = t.rows.detach().cpu().numpy()
    kp, k, zo = t.kp, t.k, t.z_offset
    b = t.bias.detach().cpu().numpy()
    return dict(V=r[:, :k].astype(np.float64), w=r[:, kp].astype(np.float64), bias=np.float64(b[0]),
                mV=r[:, zo:zo + k].astype(np.float64), vV=r[:, zo + kp:zo + kp + k].astype(np.float64),
                mw=r[:, kp + 1].astype(np.float64), vw=r[:, kp + 2].astype(np.float64), mb=np.float64(b[1]), vb=np.float64(b[2]))


def hyper(fmx, rule):
    h = HYP[rule]
    return fmx.Hyper(lr=h["lr"], eps=h["eps"], beta1=h["beta1"], beta2=h["beta2"])


def _floors(rule, h, t, g, g_noise, m2, v2):
    """fp32 floors of one application of the rule, element by element: the step's sensitivity to the gradient's fp32 noise
    (as helpers.assert_state_close(sign_rule=...) does for the fresh-Adam rule: where |g| is of the order of eps the step is
    as sensitive as a sign function) and the moments' own."""
    D = np.sqrt(np.maximum(v2, 0)) + h["eps"]
    if rule == "adam":
        ss, c1, c2 = adam_consts(h["lr"], h["beta1"], h["beta2"], t)
        dstep = ss * (c1 / D + np.abs(m2) * c2 * np.abs(g) / (np.maximum(np.sqrt(v2), 1e-30) * D * D)) * g_noise
        return np.minimum(dstep, 4 * ss), c1 * g_noise, c2 * 2 * np.abs(g) * g_noise
    dstep = 2 * h["lr"] / D * g_noise
    return np.minimum(dstep, 4 * h["lr"]), 0 * g_noise, 2 * np.abs(g) * g_noise


def assert_step(before, after, ref, urows, ex, rule, h, t, what=""):
    """after (the GPU) against ref (the float64 statement applied to `before`): 1e-5 relative on the deltas plus the floors;
    untouched rows bit for bit."""
    R = before["V"].shape[0]
    untouched = np.setdiff1d(np.arange(R), urows)
    for kk in ("V", "w", "mV", "vV", "mw", "vw"):
        np.testing.assert_array_equal(after[kk][untouched], before[kk][untouched], err_msg=f"{what}: untouched rows moved ({kk})")
    for p, m, v, g, gn in (("V", "mV", "vV", ex["gV"], ex["gnoise_V"]), ("w", "mw", "vw", ex["gw"], ex["gnoise_w"]),
                           ("bias", "mb", "vb", np.float64(ex["gb"]), np.float64(ex["gnoise_b"]))):
        sel = (lambda a: a[urows]) if p != "bias" else (lambda a: a)
        g_noise = gn + 1e-30
        fp, fm, fv = _floors(rule, h, t, g, g_noise, sel(ref[m]), sel(ref[v]))
        for name, f in ((p, fp), (m, fm), (v, fv)):
            if rule == "adagrad" and name == m:
                continue
            a, r, b0 = sel(after[name]), sel(ref[name]), sel(before[name])
            da, dr = a - b0, r - b0
            tol = 1e-5 * np.abs(dr) + f + 2.5e-7 * np.abs(r) + 1e-12
            bad = np.abs(da - dr) > tol
            assert not np.any(bad), (f"{what}/{name}: {int(np.sum(bad))} off, max err {np.max(np.abs(da - dr)):.3e}, "
                                     f"max |ref delta| {np.max(np.abs(dr)):.3e}")


def assert_pads_zero(t):
    r = t.rows.detach().cpu().numpy()
    kp, k, zo = t.kp, t.k, t.z_offset
    assert not r[:, k:kp].any() and not r[:, kp + 3:zo].any() and not r[:, zo + k:zo + kp].any()
    assert not r[:, zo + kp + k:].any(), "pad components must stay zero"
    if t.layout == "moments":
        assert float(t.bias[3]) == 0.0


@pytest.mark.parametrize("rule", ["adam", "adagrad"])
@pytest.mark.parametrize("k,B", [(4, 1), (4, 33), (16, 33), (16, 4096), (64, 1), (64, 4096), (4, 4096), (16, 1), (64, 33)])
def test_step_trajectory_vs_float64(fmx, rule, k, B):
    """20 fmx_fm_step calls; every step compared with the float64 statement applied to the GPU's state before it."""
    sizes, T = MIXED_SIZES, 20
    t = moments_table(fmx, sizes, k, seed=k + B)
    eng = fmx.FMEngine(t, max_batch=B)
    hyp, h = hyper(fmx, rule), HYP[rule]
    for s in range(1, T + 1):
        offs, idx, x, y = problem(sizes, k, B, 1000 * k + B + s)
        before = state_of(t)
        idx_d, xv_d, y_d = eng.to_device(idx, x, y)
        eng.step(hyp, rule, "logits", idx_d, xv_d, y_d)
        torch.cuda.synchronize()
        assert t.step == s
        rows = idx.astype(np.int64) + offs[:-1][None, :]
        ref, urows, ex = flat_adaptive_step(before, rows, x, y, "logits", rule, h, s)
        assert_step(before, state_of(t), ref, urows, ex, rule, h, s, what=f"{rule} k={k} B={B} step {s}")
    eng.check_error_flag()
    assert_pads_zero(t)


@pytest.mark.parametrize("rule", ["adam", "adagrad"])
def test_full_size_step_vs_float64(fmx, rule):
    """bench.py's configs[1]+[2] shape: Criteo-39 (1,006,628 rows), k = 16, B = 4096, x = 1; 3 steps."""
    k, B = 16, 4096
    t = moments_table(fmx, CRITEO_SIZES, k, seed=3)
    eng = fmx.FMEngine(t, max_batch=B)
    hyp, h = hyper(fmx, rule), HYP[rule]
    for s in range(1, 4):
        offs, idx, _, y = problem(CRITEO_SIZES, k, B, 70 + s)
        x = np.ones(idx.shape, np.float32)
        before = state_of(t)
        idx_d, _, y_d = eng.to_device(idx, None, y)
        eng.step(hyp, rule, "logits", idx_d, None, y_d)
        torch.cuda.synchronize()
        rows = idx.astype(np.int64) + offs[:-1][None, :]
        ref, urows, ex = flat_adaptive_step(before, rows, x, y, "logits", rule, h, s)
        assert_step(before, state_of(t), ref, urows, ex, rule, h, s, what=f"criteo {rule} step {s}")
    eng.check_error_flag()


@pytest.mark.parametrize("rule", ["adam", "adagrad"])
def test_stream_equals_repeated_steps_across_calls(fmx, rule):
    """fmx_fm_stream over two calls (3 + 2 steps, and a prepared stream run twice) gives the bits of 5 fmx_fm_step calls."""
    sizes, k, B, n_pool = MIXED_SIZES, 16, 1024, 3
    pool = [problem(sizes, k, B, 500 + j) for j in range(n_pool)]
    idx_pool = torch.from_numpy(np.stack([p[1] for p in pool])).cuda()
    y_pool = torch.from_numpy(np.stack([p[3] for p in pool])).cuda()
    hyp = hyper(fmx, rule)
    t1 = moments_table(fmx, sizes, k, seed=9)
    e1 = fmx.FMEngine(t1, max_batch=B)
    for s in range(5):
        e1.step(hyp, rule, "logits", idx_pool[s % n_pool], None, y_pool[s % n_pool])
    t2 = moments_table(fmx, sizes, k, seed=9)
    e2 = fmx.FMEngine(t2, max_batch=B)
    e2.stream(hyp, rule, "logits", idx_pool, y_pool, 3)
    e2.stream(hyp, rule, "logits", torch.roll(idx_pool, -3 % n_pool, 0).contiguous(), torch.roll(y_pool, -3 % n_pool, 0).contiguous(), 2)
    t3 = moments_table(fmx, sizes, k, seed=9)
    e3 = fmx.FMEngine(t3, max_batch=B)
    run = e3.prepare_stream(hyp, rule, "logits", idx_pool, y_pool)
    run(3)
    run2 = e3.prepare_stream(hyp, rule, "logits", torch.roll(idx_pool, -3 % n_pool, 0).contiguous(),
                             torch.roll(y_pool, -3 % n_pool, 0).contiguous())
    run2(2)
    torch.cuda.synchronize()
    assert t1.step == t2.step == t3.step == 5
    for t in (t2, t3):
        np.testing.assert_array_equal(t.rows.cpu().numpy(), t1.rows.cpu().numpy())
        np.testing.assert_array_equal(t.bias.cpu().numpy(), t1.bias.cpu().numpy())


@pytest.mark.parametrize("rule", ["adam", "adagrad"])
def test_prepared_stream_continues_the_count(fmx, rule):
    sizes, k, B = MIXED_SIZES, 8, 64
    p = problem(sizes, k, B, 61)
    idx_pool, y_pool = torch.from_numpy(p[1][None]).cuda(), torch.from_numpy(p[3][None]).cuda()
    hyp = hyper(fmx, rule)
    ta, tb = moments_table(fmx, sizes, k, seed=2), moments_table(fmx, sizes, k, seed=2)
    ea, eb = fmx.FMEngine(ta, max_batch=B), fmx.FMEngine(tb, max_batch=B)
    run = ea.prepare_stream(hyp, rule, "logits", idx_pool, y_pool)
    run(2)
    run(2)
    eb.stream(hyp, rule, "logits", idx_pool, y_pool, 4)
    torch.cuda.synchronize()
    assert ta.step == tb.step == 4
    np.testing.assert_array_equal(ta.rows.cpu().numpy(), tb.rows.cpu().numpy())
    np.testing.assert_array_equal(ta.bias.cpu().numpy(), tb.bias.cpu().numpy())


@pytest.mark.parametrize("rule,k", [("adam", 16), ("adagrad", 4), ("adam", 64)])
def test_online_run_equals_single_sample_steps(fmx, rule, k):
    """fmx_fm_online_run derives ADAM's constants per sample on the device: the same bits as N steps with B = 1."""
    sizes, N = MIXED_SIZES, 200
    _, idx, x, y = problem(sizes, k, N, 77)
    hyp = hyper(fmx, rule)
    t1 = moments_table(fmx, sizes, k, seed=4)
    e1 = fmx.FMEngine(t1, max_batch=N)
    idx_d, xv_d, y_d = e1.to_device(idx, x, y)
    pred, loss_b = e1.online_run(hyp, rule, "sigmoid", idx_d, xv_d, y_d, want_loss=True)
    t2 = moments_table(fmx, sizes, k, seed=4)
    e2 = fmx.FMEngine(t2, max_batch=8)
    losses = []
    for i in range(N):
        e2.step(hyp, rule, "sigmoid", idx_d[i:i + 1], xv_d[i:i + 1], y_d[i:i + 1])
        losses.append(e2.loss_out.clone())
    torch.cuda.synchronize()
    e1.check_error_flag()
    assert t1.step == t2.step == N
    np.testing.assert_array_equal(t1.rows.cpu().numpy(), t2.rows.cpu().numpy())
    np.testing.assert_array_equal(t1.bias.cpu().numpy(), t2.bias.cpu().numpy())
    np.testing.assert_array_equal(loss_b.cpu().numpy(), torch.cat(losses).cpu().numpy())


@pytest.mark.parametrize("rule", ["adam", "adagrad"])
def test_deterministic(fmx, rule):
    sizes, k, B = MIXED_SIZES, 16, 4096
    pool = [problem(sizes, k, B, 900 + j) for j in range(4)]
    idx_pool = torch.from_numpy(np.stack([p[1] for p in pool])).cuda()
    y_pool = torch.from_numpy(np.stack([p[3] for p in pool])).cuda()
    res = []
    for _ in range(2):
        t = moments_table(fmx, sizes, k, seed=1)
        e = fmx.FMEngine(t, max_batch=B)
        e.stream(hyper(fmx, rule), rule, "logits", idx_pool, y_pool, 8)
        torch.cuda.synchronize()
        res.append((t.rows.cpu().numpy(), t.bias.cpu().numpy()))
    np.testing.assert_array_equal(res[0][0], res[1][0])
    np.testing.assert_array_equal(res[0][1], res[1][1])


def test_wrong_layout_or_rule_refused(fmx):
    sizes, k, B = MIXED_SIZES, 16, 64
    _, idx, _, y = problem(sizes, k, B, 5)
    for layout, rule in (("weights", "adam"), ("ftrl", "adagrad"), ("moments", "signadam"), ("moments", "ftrl")):
        t = fmx.FlatTable(sizes, k, layout=layout)
        e = fmx.FMEngine(t, max_batch=B)
        idx_d, _, y_d = e.to_device(idx, None, y)
        with pytest.raises(fmx._lib.FmxError) as ei:
            e.step(fmx.Hyper(), rule, "logits", idx_d, None, y_d)
        assert ei.value.code == fmx._lib.ERR_ARG
        assert t.step == 0


# ---------------------------------------------------------------------------------------------------------------
# the model classes
# ---------------------------------------------------------------------------------------------------------------
def _model_state(m):
    return state_of(m._table)


@pytest.mark.parametrize("rule", ["adam", "adagrad"])
def test_fmadam_update_embedding_vs_float64(fmx, rule):
    from models.models_online_deep.fm_adam import FMAdam
    sizes, k, B = MIXED_SIZES, 8, 256
    torch.manual_seed(0)
    lr = 0.01
    m = FMAdam(sizes, embedding_size=k, n=lr, update_rule=rule)
    h = dict(HYP[rule], lr=F32(lr))
    h["eps"] = F32(1e-8 if rule == "adam" else 1e-10)
    for s in range(1, 11):
        offs, idx, x, y = problem(sizes, k, B, 300 + s)
        before = _model_state(m)
        m.update_embedding(idx, x, y)
        torch.cuda.synchronize()
        rows = idx.astype(np.int64) + offs[:-1][None, :]
        ref, urows, ex = flat_adaptive_step(before, rows, x, y, "logits", rule, h, s)
        assert_step(before, _model_state(m), ref, urows, ex, rule, h, s, what=f"FMAdam {rule} batch {s}")


class TorchDeepFM(torch.nn.Module):
    """DeepFMAdam in float64 on per-field nn.Embedding(sparse=True) tables (SparseAdam) and nn.Linear hidden layers (Adam)."""

    def __init__(self, sizes, k, layers):
        super().__init__()
        self.first = torch.nn.ModuleList([torch.nn.Embedding(s, 1, sparse=True).double() for s in sizes])
        self.second = torch.nn.ModuleList([torch.nn.Embedding(s, k, sparse=True).double() for s in sizes])
        self.bias = torch.nn.Embedding(1, 1, sparse=True).double()
        self.hidden = torch.nn.ModuleList([torch.nn.Linear(a, b).double() for a, b in layers])

    def forward(self, idx, x):
        F = idx.shape[1]
        e = torch.stack([self.second[f](idx[:, f]) * x[:, f:f + 1] for f in range(F)], 1)
        fo = sum(self.first[f](idx[:, f])[:, 0] * x[:, f] for f in range(F))
        S = e.sum(1)
        bi = 0.5 * (S * S - (e * e).sum(1))
        h = bi
        for layer in self.hidden:
            h = torch.relu(layer(h))
        return fo + bi.sum(1) + self.bias(torch.zeros(idx.shape[0], dtype=torch.long))[:, 0] + h.sum(1)


def test_deepfm_fit_adam_vs_float64_torch(fmx):
    """DeepFMAdam.fit under 'adam': the tables through fmx_fm_update (SparseAdam on every touched row and the bias), the hidden
    layers through the model's one persistent torch.optim.Adam.  Each step against a float64 torch model synchronised to the
    GPU model's parameters and optimizer state before it."""
    from models.models_online_deep.deepfm_adam import DeepFMAdam
    sizes, k, H, L, B, lr = MIXED_SIZES, 8, 16, 2, 64, 0.01
    torch.manual_seed(1)
    m = DeepFMAdam(sizes, embedding_size=k, num_hidden_layers=L, neuron_per_hidden_layer=H, n=lr, batch_size=B, update_rule="adam")
    assert not m._device_loop_ok()
    b1, b2 = m._betas()
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    for s in range(1, 4):
        _, idx, x, y = problem(sizes, k, B, 40 + s)
        st = _model_state(m)
        ref = TorchDeepFM(sizes, k, [(k, H)] + [(H, H)] * (L - 1))
        with torch.no_grad():
            for f in range(len(sizes)):
                lo, hi = int(offs[f]), int(offs[f + 1])
                ref.first[f].weight.copy_(torch.from_numpy(st["w"][lo:hi]).reshape(-1, 1))
                ref.second[f].weight.copy_(torch.from_numpy(st["V"][lo:hi]))
            ref.bias.weight.fill_(float(st["bias"]))
            for a, g in zip(ref.hidden, m.hidden_layers):
                a.weight.copy_(g.weight.detach().double().cpu())
                a.bias.copy_(g.bias.detach().double().cpu())
        sp = torch.optim.SparseAdam([p for mod in (*ref.first, *ref.second, ref.bias) for p in mod.parameters()], lr=lr,
                                    betas=(b1, b2), eps=1e-8)
        ad = torch.optim.Adam(ref.hidden.parameters(), lr=lr, betas=(b1, b2), eps=1e-8)
        if s > 1:      # the moments and the step count as the GPU model holds them
            for f in range(len(sizes)):
                lo, hi = int(offs[f]), int(offs[f + 1])
                for p, mm, vv in ((ref.first[f].weight, st["mw"][lo:hi, None], st["vw"][lo:hi, None]),
                                  (ref.second[f].weight, st["mV"][lo:hi], st["vV"][lo:hi])):
                    sp.state[p] = dict(step=s - 1, exp_avg=torch.from_numpy(np.ascontiguousarray(mm)),
                                       exp_avg_sq=torch.from_numpy(np.ascontiguousarray(vv)))
            sp.state[ref.bias.weight] = dict(step=s - 1, exp_avg=torch.tensor([[st["mb"]]]),
                                             exp_avg_sq=torch.tensor([[st["vb"]]]))
            for a, g in zip(ref.hidden.parameters(), m.hidden_layers.parameters()):
                gs = m._mlp_opt.state[g]
                ad.state[a] = dict(step=torch.tensor(float(gs["step"])), exp_avg=gs["exp_avg"].double().cpu(),
                                   exp_avg_sq=gs["exp_avg_sq"].double().cpu())
        before_h = [p.detach().double().cpu().clone() for p in m.hidden_layers.parameters()]
        m.fit(idx, x, y)
        torch.cuda.synchronize()
        z = ref(torch.from_numpy(idx.astype(np.int64)), torch.from_numpy(x.astype(np.float64)))
        loss = torch.nn.functional.binary_cross_entropy_with_logits(torch.sigmoid(z), torch.from_numpy(y.astype(np.float64)))
        sp.zero_grad()
        ad.zero_grad()
        loss.backward()
        grads = [p.grad.clone() for p in ref.hidden.parameters()]
        dense = lambda mods: torch.cat([mod.weight.grad.to_dense() for mod in mods]).numpy()
        gV, gw, gb = dense(ref.second), dense(ref.first)[:, 0], float(ref.bias.weight.grad.to_dense()[0, 0])
        sp.step()
        ad.step()
        after = _model_state(m)
        assert m._table.step == s
        h = dict(lr=lr, beta1=b1, beta2=b2, eps=1e-8)

        def check(name, a, r, b0, g, st_ref):
            """1e-4 relative on the deltas plus the adam step's sensitivity to the fp32 gradient through the network
            (noise: 1e-6 of the tensor's largest gradient), as assert_step's floors"""
            a, r, b0, g = (np.asarray(v, np.float64) for v in (a, r, b0, g))
            g_noise = 1e-6 * (np.abs(g) + np.max(np.abs(g)))
            m2, v2 = (np.asarray(st_ref[kk], np.float64).reshape(g.shape) for kk in ("exp_avg", "exp_avg_sq"))
            fp = _floors("adam", h, s, g, g_noise, m2, v2)[0]
            da, dr = a - b0, r - b0
            tol = 1e-4 * np.abs(dr) + fp + 3e-7 * np.abs(r) + 1e-12
            assert np.all(np.abs(da - dr) <= tol), f"DeepFM step {s} {name}: max err {np.max(np.abs(da - dr)):.3e}"

        cat = lambda mods, kk: torch.cat([sp.state[mod.weight][kk] for mod in mods]).numpy()
        V = torch.cat([mod.weight.detach() for mod in ref.second]).numpy()
        w = torch.cat([mod.weight.detach()[:, 0] for mod in ref.first]).numpy()
        check("V", after["V"], V, st["V"], gV, {kk: cat(ref.second, kk) for kk in ("exp_avg", "exp_avg_sq")})
        check("w", after["w"], w, st["w"], gw, {kk: cat(ref.first, kk)[:, 0] for kk in ("exp_avg", "exp_avg_sq")})
        check("bias", after["bias"], float(ref.bias.weight.detach()[0, 0]), st["bias"], gb,
              {kk: sp.state[ref.bias.weight][kk].numpy() for kk in ("exp_avg", "exp_avg_sq")})
        for j, (a, r, b0, g) in enumerate(zip(m.hidden_layers.parameters(), ref.hidden.parameters(), before_h, grads)):
            check(f"hidden {j}", a.detach().double().cpu().numpy(), r.detach().numpy(), b0.numpy(), g.numpy(),
                  {kk: ad.state[r][kk].numpy() for kk in ("exp_avg", "exp_avg_sq")})


@pytest.mark.parametrize("cls,rule", [("FMAdam", "adam"), ("FMAdam", "adagrad"), ("DeepFMAdam", "adam")])
def test_pickle_mid_run_resumes_bit_for_bit(fmx, cls, rule):
    from models.models_online_deep.fm_adam import FMAdam
    from models.models_online_deep.deepfm_adam import DeepFMAdam
    M = {"FMAdam": FMAdam, "DeepFMAdam": DeepFMAdam}
    sizes, k, B = MIXED_SIZES, 8, 32
    torch.manual_seed(3)
    kw = dict(num_hidden_layers=2, neuron_per_hidden_layer=16, batch_size=B) if cls != "FMAdam" else {}
    m = M[cls](sizes, embedding_size=k, n=0.01, update_rule=rule, **kw)
    batches = [problem(sizes, k, B, 600 + s) for s in range(6)]
    for _, idx, x, y in batches[:3]:
        m.fit(idx, x, y)
    buf = io.BytesIO()
    pickle.dump(m, buf)
    m2 = pickle.loads(buf.getvalue())
    assert m2._table.step == m._table.step == 3
    for mm in (m, m2):
        for _, idx, x, y in batches[3:]:
            mm.fit(idx, x, y)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(m._table.rows.cpu().numpy(), m2._table.rows.cpu().numpy())
    np.testing.assert_array_equal(m._table.bias.cpu().numpy(), m2._table.bias.cpu().numpy())
    if cls != "FMAdam":
        np.testing.assert_array_equal(m._mlp_flat.cpu().numpy(), m2._mlp_flat.cpu().numpy())
    st = m.optimizer_state_dict()
    assert st["table"]["step"] == 6 and set(m.state_dict()) == set(m2.state_dict())


@pytest.mark.parametrize("rule", ["adam", "adagrad"])
def test_recommend_on_a_moments_model_agrees_with_forward(fmx, rule):
    from models.models_online_deep.fm_adam import FMAdam
    sizes, k, B, K, item = MIXED_SIZES, 8, 256, 5, 2
    torch.manual_seed(5)
    m = FMAdam(sizes, embedding_size=k, n=0.05, update_rule=rule)
    for s in range(5):
        _, idx, x, y = problem(sizes, k, B, 800 + s)
        m.update_embedding(idx, x, y)
    _, ctx, _, _ = problem(sizes, k, 4, 99)
    pos, logit = m.recommend(ctx, None, item, K)
    N = sizes[item]
    for u in range(ctx.shape[0]):
        full = np.repeat(ctx[u:u + 1], N, axis=0)
        full[:, item] = np.arange(N)
        z = m.forward(full, np.ones(full.shape, np.float32)).cpu().numpy()
        order = np.lexsort((np.arange(N), -z))[:K]
        np.testing.assert_array_equal(pos[u], order)
        np.testing.assert_allclose(logit[u], z[order], rtol=1e-5, atol=1e-6)
