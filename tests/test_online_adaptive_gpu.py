"""The online predict-then-fit loop of DeepFM / NFM under the persistent adaptive rules, on the MI355X: fmx_mlp_fit_opt,
fmx_online_run_mlp_opt (one workgroup walking the stream, or the queued per-sample launches) and run_experiment of the model
classes with fused_optimizer=True.

Bit-level: the one-workgroup form == the queued form == per-sample calls from outside (fmx_fm_forward, fmx_mlp_fit_opt,
fmx_sort_occurrences, fmx_fm_update, both step counts advanced by hand) in rows (moments included), bias words, params, m, v
and pred_out; halves == whole; fmx_mlp_fit_opt's outputs == fmx_mlp_fit's; (sgd, sgd) == fmx_online_run_mlp(sgd); guard bands;
pickling mid-stream.
Against float64: test_deep_adaptive_gpu's float64_model_step / assert_model_step (torch's SparseAdam / Adagrad on the tables,
Adam / Adagrad on the hidden layers, synchronised to the device before each sample) with exactly their tolerance,
|delta - delta_ref| <= 1e-4 |delta_ref| + floor + 3e-7 |ref| + 1e-12, floor from _floors at g_noise = 1e-6 (|g| + max |g|).
Every test runs the kernels once and compares."""
import ctypes as C
import io
import pickle

import numpy as np
import pytest
import torch

from abi_geometry import Guarded
from helpers import load_model_fixture
from test_adaptive_rules_gpu import MIXED_SIZES, moments_table, problem, state_of
from test_deep_adaptive_gpu import (B1, B2, NET_HYP, TABLE_HYP, assert_model_step, float64_model_step, model_hypers, n_params,
                                    tensors_of, unsafe_samples)

pytestmark = pytest.mark.gpu

RULE_PAIRS = [("adam", "adam"), ("adagrad", "adagrad"), ("adam", "sgd"), ("signadam", "adam"), ("sgd", "adagrad")]
K_OF_KP = {4: 4, 16: 16, 64: 60}         # the fit step takes k <= 63
T_STEP0, NET_STEP0 = 7, 11               # non-zero (and different) starting step counts


@pytest.fixture(scope="module")
def fmx():
    import fmx as _fmx
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _fmx


class persistent:
    """fmx_set_option("online_persistent", v) for a block, restored on the way out."""

    def __init__(self, fmx, v):
        self.lib, self.v = fmx._lib.load(), int(v)

    def __enter__(self):
        self.old = self.lib.fmx_set_option(b"online_persistent", self.v)
        assert self.old in (0, 1)

    def __exit__(self, *exc):
        self.lib.fmx_set_option(b"online_persistent", self.old)


def setup(fmx, table_rule, net_rule, k, H, L, seed=0, sizes=MIXED_SIZES, steps=(T_STEP0, NET_STEP0)):
    """-> (table, engine, hyper, flat params, MlpOpt): seeded, identical for equal arguments.  Moments tables and the network's
    moments start from non-zero values (v >= 0), as after the steps the counts claim."""
    rng = np.random.default_rng(seed)
    if table_rule in ("adam", "adagrad"):
        t = moments_table(fmx, sizes, k, seed=seed)
        R, zo, kp = t.n_rows, t.z_offset, t.kp
        t.rows[:, zo:zo + k] = torch.from_numpy((rng.normal(size=(R, k)) * 1e-3).astype(np.float32)).cuda()
        t.rows[:, zo + kp:zo + kp + k] = torch.from_numpy((rng.normal(size=(R, k)) ** 2 * 1e-5).astype(np.float32)).cuda()
        t.rows[:, kp + 1] = torch.from_numpy((rng.normal(size=R) * 1e-3).astype(np.float32)).cuda()
        t.rows[:, kp + 2] = torch.from_numpy((rng.normal(size=R) ** 2 * 1e-5).astype(np.float32)).cuda()
        t.bias[1], t.bias[2] = 2e-3, 3e-5
        t.step = steps[0]
    else:
        R = sum(sizes)
        t = fmx.FlatTable(sizes, k, layout="weights")
        t.rows[:, :k] = torch.from_numpy((rng.normal(size=(R, k)) * 0.3).astype(np.float32)).cuda()
        t.rows[:, t.kp] = torch.from_numpy((rng.normal(size=R) * 0.3).astype(np.float32)).cuda()
        t.bias[0] = 0.37
    e = fmx.FMEngine(t, max_batch=8)
    hyp = fmx.Hyper(**TABLE_HYP)
    gen = torch.Generator().manual_seed(seed + 1)
    n = n_params(k, H, L)
    params = (torch.randn(n, generator=gen) * (1.0 / np.sqrt(H))).cuda()
    h = NET_HYP[net_rule]
    opt = fmx.MlpOpt(n, net_rule, lr=h["lr"], eps=h["eps"], beta1=h["beta1"], beta2=h["beta2"], device="cuda", step=steps[1])
    if net_rule != "sgd":
        opt.v.copy_((torch.randn(n, generator=gen) ** 2 * 1e-5).cuda())
    if net_rule == "adam":
        opt.m.copy_((torch.randn(n, generator=gen) * 1e-3).cuda())
    return t, e, hyp, params, opt


def snapshot(t, params, opt, pred):
    torch.cuda.synchronize()
    return dict(rows=t.rows.cpu().numpy().copy(), bias=t.bias.cpu().numpy().copy(), params=params.cpu().numpy().copy(),
                m=opt.m.cpu().numpy().copy(), v=opt.v.cpu().numpy().copy(), pred=pred.cpu().numpy().copy(),
                steps=np.array([t.step if t.layout == "moments" else -1, opt.step]))


def assert_same(a, b, what):
    for kk in a:
        np.testing.assert_array_equal(a[kk].view(np.int32) if a[kk].dtype == np.float32 else a[kk],
                                      b[kk].view(np.int32) if b[kk].dtype == np.float32 else b[kk], err_msg=f"{what}: {kk}")


def per_sample(e, t, hyp, table_rule, loss, params, k, H, L, fm_term, idx_d, xv_d, y_d, opt):
    """The N per-sample sequences from outside: fmx_fm_forward, (fmx_mlp_forward for the value forward() returns: read only,)
    fmx_mlp_fit_opt, fmx_sort_occurrences, fmx_fm_update; FMEngine advances the table's and the network's counts per call."""
    N = idx_d.shape[0]
    pred = torch.empty(N, device="cuda")
    for i in range(N):
        xi = None if xv_d is None else xv_d[i:i + 1]
        e.forward(hyp, idx_d[i:i + 1], xi, want_first=False, want_bi=True)
        base = (e.logit[:1] if fm_term else e.sfirst[:1] + t.bias[0]).contiguous()
        out, _ = e.mlp_forward(params, k, H, L, base, 1, False)
        pred[i] = out[0]
        dz, gbi = e.mlp_fit(params, k, H, L, hyp, "sgd", loss, base, y_d[i:i + 1], 1, mlp_opt=opt)
        e.sort(idx_d[i:i + 1])
        e.update(hyp, table_rule, 1, xi, dz, dz if fm_term else None, gbi, inv_b=1.0, with_loss=False)
    return pred


def run(e, hyp, table_rule, loss, params, k, H, L, fm_term, idx_d, xv_d, y_d, opt):
    return e.online_run_mlp(hyp, table_rule, loss, params, k, H, L, False, fm_term, 0.0, 0.0, None, idx_d, xv_d, y_d, mlp_opt=opt)


# ---------------------------------------------------------------------------------------------------------------
# 1: identical bits three ways
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kp", [4, 16, 64])
@pytest.mark.parametrize("table_rule,net_rule", RULE_PAIRS)
@pytest.mark.parametrize("fm_term", [1, 0], ids=["deepfm", "nfm"])
def test_one_workgroup_equals_queued_equals_per_sample_calls(fmx, fm_term, table_rule, net_rule, kp):
    k, H, L, N = K_OF_KP[kp], 32, 2, 200
    with_x = (RULE_PAIRS.index((table_rule, net_rule)) + [4, 16, 64].index(kp) + fm_term) % 2 == 0     # xv given / null (all ones)
    loss = "sigmoid" if fm_term else "logits"
    _, idx, x, y = problem(MIXED_SIZES, k, N, 5100 + kp)       # zipf: the same rows again and again
    assert len(np.unique(idx[:, 3])) < N
    res = {}
    for form in ("one workgroup", "queued", "per sample"):
        t, e, hyp, params, opt = setup(fmx, table_rule, net_rule, k, H, L, seed=kp)
        assert t.kp == kp
        idx_d, xv_d, y_d = e.to_device(idx, x if with_x else None, y)
        if form == "per sample":
            pred = per_sample(e, t, hyp, table_rule, loss, params, k, H, L, fm_term, idx_d, xv_d, y_d, opt)
        else:
            with persistent(fmx, form == "one workgroup"):
                pred = run(e, hyp, table_rule, loss, params, k, H, L, fm_term, idx_d, xv_d, y_d, opt)
        e.check_error_flag()
        res[form] = snapshot(t, params, opt, pred)
    whole = res["one workgroup"]
    assert list(whole["steps"]) == [T_STEP0 + N if table_rule in ("adam", "adagrad") else -1, NET_STEP0 + N]
    assert_same(whole, res["queued"], "one workgroup vs queued launches")
    assert_same(whole, res["per sample"], "one workgroup vs per-sample calls")
    t0, _, _, p0, o0 = setup(fmx, table_rule, net_rule, k, H, L, seed=kp)
    assert not np.array_equal(whole["params"], p0.cpu().numpy()), "the network did not move"
    if net_rule == "sgd":
        np.testing.assert_array_equal(whole["m"], o0.m.cpu().numpy())
        np.testing.assert_array_equal(whole["v"], o0.v.cpu().numpy())
    elif net_rule == "adagrad":
        np.testing.assert_array_equal(whole["m"], o0.m.cpu().numpy(), err_msg="adagrad neither loads nor stores m")
        assert not np.array_equal(whole["v"], o0.v.cpu().numpy())
    else:
        assert not np.array_equal(whole["m"], o0.m.cpu().numpy()) and not np.array_equal(whole["v"], o0.v.cpu().numpy())
    # untouched rows keep their bits
    offs = np.concatenate([[0], np.cumsum(MIXED_SIZES)]).astype(np.int64)
    untouched = np.setdiff1d(np.arange(t0.n_rows), np.unique(idx.astype(np.int64) + offs[:-1][None, :]))
    assert untouched.size > 0
    np.testing.assert_array_equal(whole["rows"][untouched].view(np.int32), t0.rows.cpu().numpy()[untouched].view(np.int32))


@pytest.mark.parametrize("form", ["one workgroup", "queued"])
def test_two_halves_equal_one_call(fmx, form):
    k, H, L, N = 16, 32, 2, 200
    _, idx, x, y = problem(MIXED_SIZES, k, N, 5200)
    res = []
    for cuts in ([N], [N // 2, N - N // 2]):
        t, e, hyp, params, opt = setup(fmx, "adam", "adam", k, H, L, seed=2)
        idx_d, xv_d, y_d = e.to_device(idx, x, y)
        preds, lo = [], 0
        with persistent(fmx, form == "one workgroup"):
            for c in cuts:
                preds.append(run(e, hyp, "adam", "sigmoid", params, k, H, L, 1, idx_d[lo:lo + c], xv_d[lo:lo + c], y_d[lo:lo + c], opt))
                lo += c
                assert t.step == T_STEP0 + lo and opt.step == NET_STEP0 + lo
        e.check_error_flag()
        res.append(snapshot(t, params, opt, torch.cat(preds)))
    assert_same(res[0], res[1], f"{form}: one call vs two halves")


# ---------------------------------------------------------------------------------------------------------------
# 2: against float64
# ---------------------------------------------------------------------------------------------------------------
def sample_clear_of_kinks(sizes, k, H, L, st, p, seed, fm_term, loss):
    """One sample (idx [1, F], x, y) on which float64 states what the fp32 kernels must compute, drawn again until it is:
    * no relu input at a kink: draw_clear_of_kinks' criterion (unsafe_samples) on the bi-interaction vector the TABLE gives for
      the sample, with the fp32 noise of that vector (test_full_size_trainer_adam_step_vs_float64's model) as its input noise;
    * no saturated logit.  A batch of ONE sample has one dL/dlogit, a factor of every gradient of the step, and fp32 evaluates it
      through a cancelled difference: 1 - p in p (1 - p) (the "sigmoid" loss) or p - y (the "logits" loss), whose relative
      rounding error is that of p = sigmoid(z), a few 2^-24, times amp = p / (1 - p) resp. p / |p - y|.  The tolerance's floors
      model the gradient's noise as g_noise = 1e-6 (|g| + max |g|), i.e. at least 1e-6 |g|: with four roundings in sigmoid's
      chain (negate, expf, add, divide) that holds where 4 * 2^-24 * (1 + amp) <= 1e-6, amp <= 3.19.  At mini-batch sizes (the
      tests this tolerance comes from) the saturated samples' share of a summed gradient is negligible; here it is everything."""
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    ts = tensors_of(np.asarray(p, np.float64), k, H, L)
    amp_max = 1e-6 / (4 * 2.0 ** -24) - 1
    for rnd in range(400):
        _, idx, x, y = problem(sizes, k, 1, seed + 1000 * rnd)
        rows = idx.astype(np.int64) + offs[:-1][None, :]
        e_ = st["V"][rows] * x.astype(np.float64)[:, :, None]       # [1, F, k]
        S_, Sa_, ss_ = e_.sum(1), np.abs(e_).sum(1), (e_ * e_).sum(1)
        bi = 0.5 * (S_ * S_ - ss_)
        dbi = np.sqrt(len(sizes) + 2.0) * 2.0 ** -24 * 0.5 * (Sa_ * Sa_ + ss_)
        if unsafe_samples(p, k, H, L, bi, dbi).any():
            continue
        h = bi
        for l in range(L):
            h = np.maximum(h @ ts[2 * l].T + ts[2 * l + 1], 0.0)
        z = float((st["w"][rows] * x).sum() + st["bias"] + (bi.sum() if fm_term else 0.0) + h.sum())
        pz = 1.0 / (1.0 + np.exp(-z))
        amp = pz / (1.0 - pz) if loss == "sigmoid" else pz / abs(pz - float(y[0]))
        if amp <= amp_max:
            return idx, x, y
    raise AssertionError("no sample clear of the relu kinks and of saturation in 400 draws")


@pytest.mark.parametrize("rule", ["adam", "adagrad"])
@pytest.mark.parametrize("cls", ["DeepFM", "NFM"])
def test_first_four_samples_vs_float64_torch(fmx, cls, rule):
    """The first 4 samples of a stream, one fmx_online_run_mlp_opt call each (the one-workgroup form), each against the float64
    torch model synchronised to the device's tables, network, moments and step counts before it.  The loss is the class's
    own: BCEwl(sigmoid(forward)) for DeepFMAdam, BCEwl(forward) for NFMAdam."""
    sizes, k, H, L, lr = MIXED_SIZES, 8, 16, 2, 0.01
    fm_term, loss = (True, "sigmoid") if cls == "DeepFM" else (False, "logits")
    th, nh = model_hypers(rule, lr, B1, B2)
    t = moments_table(fmx, sizes, k, seed=5)
    e = fmx.FMEngine(t, max_batch=8)
    hyp = fmx.Hyper(lr=th["lr"], eps=th["eps"], beta1=th["beta1"], beta2=th["beta2"])
    n = n_params(k, H, L)
    gen = torch.Generator().manual_seed(17)
    params = (torch.randn(n, generator=gen) * (1.0 / np.sqrt(H))).cuda()
    opt = fmx.MlpOpt(n, rule, lr=nh["lr"], eps=nh["eps"], beta1=nh["beta1"], beta2=nh["beta2"], device="cuda")
    net = lambda: {"p": params.cpu().numpy().astype(np.float64), "m": opt.m.cpu().numpy().astype(np.float64),
                   "v": opt.v.cpu().numpy().astype(np.float64)}
    for s in range(1, 5):
        st, nb = state_of(t), net()
        idx, x, y = sample_clear_of_kinks(sizes, k, H, L, st, nb["p"], 7000 + s, fm_term, loss)
        idx_d, xv_d, y_d = e.to_device(idx, x, y)
        pred = run(e, hyp, rule, loss, params, k, H, L, fm_term, idx_d, xv_d, y_d, opt)
        torch.cuda.synchronize()
        e.check_error_flag()
        assert t.step == s and opt.step == s and np.isfinite(float(pred[0]))
        r = float64_model_step(sizes, k, H, L, fm_term, loss, rule, th, nh, s, st, nb, idx, x, y)
        assert np.any(r["net"][1]), "a sample that leaves the whole network without a gradient shows nothing"
        assert_model_step(f"{cls} {rule} sample {s}", rule, th, nh, s, st, state_of(t), nb, net(), r, k, H, L)


# ---------------------------------------------------------------------------------------------------------------
# 3: cross-checks that need no oracle
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net_rule", ["adam", "adagrad", "sgd"])
@pytest.mark.parametrize("B", [1, 5, 16])
def test_mlp_fit_opt_outputs_equal_mlp_fit(fmx, B, net_rule):
    """dz_out, gbi_out, loss_out of fmx_mlp_fit_opt == fmx_mlp_fit's bit for bit (the update does not feed them); under
    opt->rule = SGD the parameters too are those of fmx_mlp_fit(rule = SGD, lr = opt->lr); opt->step is never written."""
    L_ = fmx._lib
    lib = L_.load()
    k, kp, H, L = 10, 16, 10, 5
    n = n_params(k, H, L)
    rng = np.random.default_rng(B)
    gen = torch.Generator().manual_seed(B + 3)
    p0 = (torch.randn(n, generator=gen) * (1.0 / np.sqrt(H))).cuda()
    bi = torch.zeros((B, kp), device="cuda")
    bi[:, :k] = torch.from_numpy((rng.normal(size=(B, k)) * 0.5).astype(np.float32)).cuda()
    base = torch.from_numpy((rng.normal(size=B) * 0.3).astype(np.float32)).cuda()
    y = torch.from_numpy((rng.uniform(size=B) < 0.4).astype(np.float32)).cuda()
    h = NET_HYP[net_rule]
    stream = torch.cuda.current_stream().cuda_stream
    hyp = fmx.Hyper(lr=h["lr"], eps=1e-8)
    outs = {}
    for tag in ("fit", "opt"):
        p = Guarded(4 * n, name="params")
        p.t.copy_(p0)
        m, v = Guarded(4 * n, name="m"), Guarded(4 * n, name="v")
        o = dict(dz=torch.full((B,), 7.0, device="cuda"), gbi=torch.full((B, kp), 7.0, device="cuda"), loss=torch.zeros(1, device="cuda"))
        mc = L_.Mlp(p.ptr, L, k, H, 0)
        if tag == "fit":
            L_.check(lib.fmx_mlp_fit(C.byref(mc), hyp.ref(), L_.RULE_SGD, L_.LOSS_BCE_SIGMOID, bi.data_ptr(), kp, base.data_ptr(),
                                     y.data_ptr(), B, 1.0 / B, o["dz"].data_ptr(), o["gbi"].data_ptr(), o["loss"].data_ptr(), stream))
        else:
            opt = L_.MlpOpt(m.ptr, v.ptr, h["lr"], h["eps"], h["beta1"], h["beta2"], L_.RULES[net_rule], 4)
            L_.check(lib.fmx_mlp_fit_opt(C.byref(mc), None, L_.LOSS_BCE_SIGMOID, bi.data_ptr(), kp, base.data_ptr(), y.data_ptr(), B,
                                         1.0 / B, o["dz"].data_ptr(), o["gbi"].data_ptr(), o["loss"].data_ptr(), C.byref(opt), stream))
            assert opt.step == 4
        torch.cuda.synchronize()
        for g in (p, m, v):
            g.check()
        o.update(params=p.t.clone(), m=m.t.clone(), v=v.t.clone())
        outs[tag] = o
    for name in ("dz", "gbi", "loss"):
        assert torch.equal(outs["fit"][name], outs["opt"][name]), name
    assert not torch.equal(outs["opt"]["params"], p0)
    if net_rule == "sgd":
        assert torch.equal(outs["fit"]["params"], outs["opt"]["params"])
        assert not outs["opt"]["m"].any() and not outs["opt"]["v"].any()
    else:
        assert outs["opt"]["v"].any() and bool(outs["opt"]["m"].any()) == (net_rule == "adam")


@pytest.mark.parametrize("form", ["one workgroup", "queued"])
@pytest.mark.parametrize("fm_term", [1, 0], ids=["deepfm", "nfm"])
def test_sgd_sgd_equals_the_old_call(fmx, fm_term, form):
    """(sgd tables, sgd network at the same lr) through fmx_online_run_mlp_opt == fmx_online_run_mlp(rule = SGD), bit for bit."""
    k, H, L, N = 16, 32, 2, 200
    _, idx, x, y = problem(MIXED_SIZES, k, N, 5300)
    res = []
    for use_opt in (True, False):
        t, e, hyp, params, opt = setup(fmx, "sgd", "sgd", k, H, L, seed=4)
        opt.c.lr = hyp.c.lr
        idx_d, xv_d, y_d = e.to_device(idx, x, y)
        with persistent(fmx, form == "one workgroup"):
            pred = e.online_run_mlp(hyp, "sgd", "sigmoid", params, k, H, L, False, fm_term, 0.0, 0.0, None, idx_d, xv_d, y_d,
                                    mlp_opt=opt if use_opt else None)
        e.check_error_flag()
        if not use_opt:
            opt.step += N
        res.append(snapshot(t, params, opt, pred))
    assert_same(res[0], res[1], "fmx_online_run_mlp_opt(sgd, sgd) vs fmx_online_run_mlp(sgd)")


@pytest.mark.parametrize("form", ["one workgroup", "queued"])
@pytest.mark.parametrize("table_rule,net_rule", [("adam", "adam"), ("adagrad", "adagrad"), ("signadam", "adam")])
def test_guard_bands_survive(fmx, table_rule, net_rule, form):
    """params, m, v, pred_out and the table's rows in guard bands: the pattern around them survives a call on each path, and the
    guarded call gives the bits of the plain one."""
    L_ = fmx._lib
    lib = L_.load()
    k, H, L, N = 16, 32, 2, 64
    n = n_params(k, H, L)
    _, idx, x, y = problem(MIXED_SIZES, k, N, 5400)
    t, e, hyp, params, opt = setup(fmx, table_rule, net_rule, k, H, L, seed=6)
    idx_d, xv_d, y_d = e.to_device(idx, x, y)
    with persistent(fmx, form == "one workgroup"):
        pred = run(e, hyp, table_rule, "sigmoid", params, k, H, L, 1, idx_d, xv_d, y_d, opt)
    plain = snapshot(t, params, opt, pred)
    # ---- the same call on guarded buffers ----
    t, e, hyp, params, opt = setup(fmx, table_rule, net_rule, k, H, L, seed=6)
    g = {name: Guarded(4 * n, name=name) for name in ("params", "m", "v")}
    g["params"].t.copy_(params)
    g["m"].t.copy_(opt.m)
    g["v"].t.copy_(opt.v)
    g["pred"] = Guarded(4 * N, name="pred_out")
    g["rows"] = Guarded(4 * t.rows.numel(), name="table rows")
    g["bias"] = Guarded(4 * t.bias.numel(), name="bias")
    g["rows"].t.copy_(t.rows.reshape(-1))
    g["bias"].t.copy_(t.bias)
    t.rows, t.bias, t._cstruct = g["rows"].t.view(t.n_rows, t.row_stride), g["bias"].t, None
    e._ensure(1)
    out = e._fwd_out(want_first=False, want_bi=True)
    scratch = torch.zeros(t.kp + 8, device="cuda")
    mc = L_.Mlp(g["params"].ptr, L, k, H, 0)
    oc = L_.MlpOpt(g["m"].ptr, g["v"].ptr, opt.c.lr, opt.c.eps, opt.c.beta1, opt.c.beta2, opt.c.rule, opt.step)
    hyp.c.step = T_STEP0
    with persistent(fmx, form == "one workgroup"):
        L_.check(lib.fmx_online_run_mlp_opt(t.c_struct(), hyp.ref(), L_.RULES[table_rule], L_.LOSS_BCE_SIGMOID, C.byref(mc), 1,
                                            idx_d.data_ptr(), xv_d.data_ptr(), y_d.data_ptr(), N, e.workspace.data_ptr(), e._ws_bytes(),
                                            C.byref(out), scratch.data_ptr(), g["pred"].ptr, C.byref(oc), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    e.check_error_flag()
    for gg in g.values():
        gg.check()
    assert oc.step == opt.step and hyp.c.step == T_STEP0, "the step counts are the caller's: never written back"
    for name, got in (("rows", g["rows"].t.view(t.n_rows, t.row_stride)), ("bias", g["bias"].t), ("params", g["params"].t), ("m", g["m"].t),
                      ("v", g["v"].t), ("pred", g["pred"].t)):
        np.testing.assert_array_equal(got.cpu().numpy().view(np.int32), plain[name].view(np.int32), err_msg=f"guarded vs plain: {name}")


# ---------------------------------------------------------------------------------------------------------------
# 4: the class surface
# ---------------------------------------------------------------------------------------------------------------
def _classes():
    from models.models_online_deep.deepfm_adam import DeepFMAdam
    from models.models_online_deep.nfm_adam import NFMAdam
    return {"DeepFMAdam": DeepFMAdam, "NFMAdam": NFMAdam}


def _criteo_model(cls, rule, seed=1, **kw):
    _, meta = load_model_fixture(cls, "criteo39s")
    torch.manual_seed(seed)
    m = _classes()[cls](meta["feature_sizes"], embedding_size=meta["k"], num_hidden_layers=meta["L"], neuron_per_hidden_layer=meta["H"],
                        n=meta["n"], update_rule=rule, **kw)
    return m, meta


def _criteo_stream(meta, N, seed):
    rng = np.random.default_rng(seed)
    sizes = meta["feature_sizes"]
    idx = np.stack([rng.integers(0, s, size=N) for s in sizes], axis=1).astype(np.int32)
    x = rng.uniform(-1, 1, size=idx.shape).astype(np.float32)
    y = (rng.uniform(size=N) < 0.4).astype(np.float32)
    return idx, x, y


def _model_bits(m):
    torch.cuda.synchronize()
    osd = m.optimizer_state_dict()
    out = dict(rows=m._table.rows.cpu().numpy().copy(), bias=m._table.bias.cpu().numpy().copy(), flat=m._mlp_flat.cpu().numpy().copy(),
               m=osd["mlp"]["m"].numpy().copy(), v=osd["mlp"]["v"].numpy().copy(),
               steps=np.array([m._table.step, m._mlp_fused.step, osd["table"]["step"], osd["mlp"]["step"]]))
    for kk, vv in osd["table"].items():
        if kk != "step":
            out["table_" + kk] = np.asarray(vv).copy()
    for kk, vv in m.state_dict().items():
        out["sd_" + kk] = np.asarray(vv.cpu() if torch.is_tensor(vv) else vv).copy()
    return out


@pytest.mark.parametrize("rule", ["adam", "adagrad"])
@pytest.mark.parametrize("cls", ["DeepFMAdam", "NFMAdam"])
def test_run_experiment_on_the_device_equals_per_sample_calls(fmx, cls, rule):
    """DeepFMAdam / NFMAdam(update_rule=rule, fused_optimizer=True) on the criteo39s fixture's sizes: run_experiment takes the
    device loop and ends in the bits of the engine's per-sample calls driven by hand (fmx_mlp_fit_opt's arithmetic -- NOT
    fit()'s, which keeps fmx_mlp_section_opt: the two differ in fp32 summation order)."""
    N = 300
    m, meta = _criteo_model(cls, rule, fused_optimizer=True)
    idx, x, y = _criteo_stream(meta, N, 81)
    assert m._device_loop_ok()
    res = m.run_experiment(idx, x, y)
    assert isinstance(res, tuple) and len(res) == 4
    secs, acc, roc, cm = res
    assert secs > 0 and 0.0 <= acc <= 100.0 and set(roc) == {"tpr", "fpr"} and sum(cm.values()) == N
    assert m._table.step == N and m._mlp_fused.step == N
    # ---- the same stream through the engine's per-sample calls ----
    m2, _ = _criteo_model(cls, rule, fused_optimizer=True)
    e, k, H, L = m2._engine, m2.embedding_size, m2.neuron_per_hidden_layer, m2.num_hidden_layers
    idx_d, xv_d, y_d = e.to_device(idx, x, y)
    fm_term = m2._fm_term_in_forward
    pred = per_sample(e, m2._table, m2._hyper, rule, m2._loss_fit, m2._mlp_flat, k, H, L, fm_term, idx_d, xv_d, y_d, m2._mlp_fused)
    e.check_error_flag()
    a, b = _model_bits(m), _model_bits(m2)
    assert_same(a, b, f"{cls} {rule}: run_experiment vs per-sample calls")
    hits = (torch.sigmoid(pred) > 0.5).cpu().numpy() == (y == 1)
    assert cm["tp"] + cm["tn"] == int(hits.sum())
    # device_online_loop = False: today's path (predict + fit per sample, fmx_mlp_section_opt)
    m3, _ = _criteo_model(cls, rule, fused_optimizer=True)
    m3.device_online_loop = False
    assert not m3._device_loop_ok()
    r3 = m3.run_experiment(idx[:12], x[:12], y[:12])
    assert len(r3) == 4 and m3._table.step == 12 and m3._mlp_fused.step == 12


@pytest.mark.parametrize("cls,rule", [("DeepFMAdam", "adam"), ("NFMAdam", "adagrad")])
def test_pickle_mid_stream_resumes_bit_for_bit(fmx, cls, rule):
    N = 200
    m, meta = _criteo_model(cls, rule, seed=2, fused_optimizer=True)
    idx, x, y = _criteo_stream(meta, N, 82)
    m.run_experiment(idx, x, y)
    h, _ = _criteo_model(cls, rule, seed=2, fused_optimizer=True)
    h.run_experiment(idx[:N // 2], x[:N // 2], y[:N // 2])
    buf = io.BytesIO()
    pickle.dump(h, buf)
    h2 = pickle.loads(buf.getvalue())
    assert h2.fused_optimizer and h2._device_loop_ok() and h2._table.step == N // 2 and h2._mlp_fused.step == N // 2
    h2.run_experiment(idx[N // 2:], x[N // 2:], y[N // 2:])
    assert_same(_model_bits(m), _model_bits(h2), f"{cls} {rule}: uninterrupted vs pickled mid-stream")


def test_default_models_keep_todays_loop(fmx):
    """fused_optimizer=False (the default) under the adaptive rules: the hidden layers are on a torch optimizer, which cannot
    run in the device loop."""
    for cls in ("DeepFMAdam", "NFMAdam"):
        for rule in ("adam", "adagrad"):
            m, _ = _criteo_model(cls, rule)
            assert not m.fused_optimizer and not m._device_loop_ok()
        m, _ = _criteo_model(cls, "signadam")
        assert m._device_loop_ok()


# ---------------------------------------------------------------------------------------------------------------
# 5: limits
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,where", [(61, "the largest network of this shape under the cap: 96 KB of parameters and moments in LDS"),
                                     (63, "just above the cap: the queued form")])
def test_networks_around_the_lds_cap(fmx, k, where):
    """H = 64, L = 2: 8,128 parameters at k = 61, 8,256 at k = 63, around the one-workgroup form's 8,192.  Either way a call ends
    in the bits of per-sample calls, with online_persistent on or off."""
    H, L, N = 64, 2, 40
    n = n_params(k, H, L)
    assert (n <= 8192) == (k == 61) and abs(n - 8192) <= 64
    _, idx, x, y = problem(MIXED_SIZES, k, N, 5500 + k)
    res = {}
    for form in ("default", "queued", "per sample"):
        t, e, hyp, params, opt = setup(fmx, "adam", "adam", k, H, L, seed=k)
        idx_d, xv_d, y_d = e.to_device(idx, x, y)
        if form == "per sample":
            pred = per_sample(e, t, hyp, "adam", "sigmoid", params, k, H, L, 1, idx_d, xv_d, y_d, opt)
        else:
            with persistent(fmx, form == "default"):
                pred = run(e, hyp, "adam", "sigmoid", params, k, H, L, 1, idx_d, xv_d, y_d, opt)
        e.check_error_flag()
        res[form] = snapshot(t, params, opt, pred)
    assert_same(res["default"], res["queued"], f"{where}: default vs queued")
    assert_same(res["default"], res["per sample"], f"{where}: default vs per-sample calls")


@pytest.mark.parametrize("form", ["one workgroup", "queued"])
def test_out_of_range_index_raises_the_flag(fmx, form):
    k, H, L, N = 16, 32, 2, 20
    _, idx, x, y = problem(MIXED_SIZES, k, N, 5600)
    idx[7, 4] = MIXED_SIZES[4]          # one past the field's last row
    t, e, hyp, params, opt = setup(fmx, "adam", "adam", k, H, L, seed=8)
    idx_d, xv_d, y_d = e.to_device(idx, x, y)
    with persistent(fmx, form == "one workgroup"):
        run(e, hyp, "adam", "sigmoid", params, k, H, L, 1, idx_d, xv_d, y_d, opt)
    with pytest.raises(IndexError):
        e.check_error_flag()
    e.check_error_flag()                 # the flag is cleared by the read


def test_out_of_range_index_through_the_class(fmx):
    m, meta = _criteo_model("DeepFMAdam", "adam", fused_optimizer=True)
    idx, x, y = _criteo_stream(meta, 30, 83)
    idx[11, 2] = meta["feature_sizes"][2]
    assert m._device_loop_ok()
    with pytest.raises(IndexError):
        m.run_experiment(idx, x, y)


def test_an_empty_stream_is_a_checked_no_op(fmx):
    L_ = fmx._lib
    lib = L_.load()
    k, H, L = 16, 32, 2
    t, e, hyp, params, opt = setup(fmx, "adam", "adam", k, H, L, seed=9)
    before = snapshot(t, params, opt, torch.zeros(1))
    idx_d, xv_d, y_d = e.to_device(problem(MIXED_SIZES, k, 4, 1)[1], None, np.zeros(4, np.float32))
    e._ensure(1)
    out = e._fwd_out(want_first=False, want_bi=True)
    scratch, pred = torch.zeros(t.kp + 8, device="cuda"), torch.zeros(4, device="cuda")
    mc = L_.Mlp(params.data_ptr(), L, k, H, 0)
    hyp.c.step = t.step

    def call(o, N=0):
        return lib.fmx_online_run_mlp_opt(t.c_struct(), hyp.ref(), L_.RULE_ADAM, L_.LOSS_BCE_SIGMOID, C.byref(mc), 1, idx_d.data_ptr(), None,
                                          y_d.data_ptr(), N, e.workspace.data_ptr(), e._ws_bytes(), C.byref(out), scratch.data_ptr(),
                                          pred.data_ptr(), o, torch.cuda.current_stream().cuda_stream)
    for on in (1, 0):
        with persistent(fmx, on):
            assert call(opt.ref()) == L_.OK
            assert call(None) == L_.ERR_ARG and b"fmx_online_run_mlp_opt" in lib.fmx_last_error_string()
            assert call(opt.ref(), N=-1) == L_.ERR_ARG
    assert_same(before, snapshot(t, params, opt, torch.zeros(1)), "N = 0")
    assert not pred.any()
