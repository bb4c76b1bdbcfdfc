"""The one-workgroup pair step of DeepFM / NFM (fmx_mlp_pair_fit: k_mlp_small_pair) and the online pair loop on top of it
(fmx_online_run_mlp_pair: k_online_mlp_pair walking the stream, or the queued per-pair launches), on the MI355X; and
run_pair_experiment(full=True) of the classes with pair_loop_on_device = True.

Bit-level: logit_out == fmx_mlp_forward's out; dz[2i + 1] == -dz[2i]; dz / gbi / logit / loss across the rules; the
one-workgroup form == the queued form == the per-pair sequence from outside (fmx_fm_forward at B = 2, the NFM base add,
fmx_mlp_pair_fit, fmx_sort_occurrences, fmx_fm_update at B = 2, both step counts advanced by the engine) in rows (moments
included), bias words, params, m, v, pred_out, logit_out and loss_out; halves == whole; guard bands.
Against float64, with the bounds of the files the helpers come from, restated:
* the epilogue from the device's own logits (test_pair_mlp_gpu.check_section_epilogue): |dz - ref| <= 1e-5 |ref| + 4 EPS32 inv_b;
  loss_out within inv_b (sum_i (1e-5 |l_i| + 4 EPS32 (1 + |l_i|)) + 2 P EPS32 sum_i |l_i|) of the float64 sum;
* logit, loss, dz, gbi against tests/pair_mlp_f64.py with test_mlp_gpu.close: 2e-5 of the tensor's largest magnitude;
* the SGD step of every parameter tensor against -lr times the float64 gradient with test_mlp_gpu.close_per_tensor's bound on
  the gradient, 2e-5 of the tensor's largest gradient + 4 gnoise, plus one rounding of the parameter, EPS32 |p|.
Every test runs its kernels once and compares."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from abi_geometry import Guarded
from oracle.fm_oracle import EPS32
from pair_f64 import pair_loss_f64
from pair_mlp_f64 import pair_mlp_f64
from test_adaptive_rules_gpu import MIXED_SIZES, problem
from test_deep_adaptive_gpu import n_params
from test_kernels_gpu import HYP
from test_mlp_gpu import close, live_units
from test_online_adaptive_gpu import K_OF_KP, NET_STEP0, T_STEP0, persistent, setup
from test_pair_gpu import build_table, same_bits
from test_pair_mlp_gpu import class_data, model_words, new_model

pytestmark = pytest.mark.gpu

SIZES = MIXED_SIZES[:-1]          # ten fields, none with a single row: a negative can differ from its positive in every column
ITEM = (2, 3)                     # the item columns (1000 and 50000 rows, zipf-drawn: the same rows again and again)
FIT_SHAPES = [(4, 4, 1, 1), (10, 12, 33, 2), (16, 16, 64, 3), (63, 64, 64, 8)]        # k, kp, hidden, layers
FIT_PAIRS = [1, 3, 8]             # one pair, an odd count, the cap
MARGINS = [0.0, 0.1]
LR = 0.05


@pytest.fixture(scope="module")
def fmx():
    import fmx as _fmx
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _fmx


def stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------------------------
# 1: fmx_mlp_pair_fit alone
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fit_problem(P, k, kp, H, L):
    """-> (params, bi [2P, kp], base [2P]) as CPU tensors: no layer dead (live_units)"""
    g = torch.Generator().manual_seed(1000 * P + H + L + k)
    params = torch.randn(n_params(k, H, L), generator=g) * (1.0 / np.sqrt(H))
    bi = torch.zeros(2 * P, kp)
    bi[:, :k] = torch.randn(2 * P, k, generator=g) * 0.5
    params = torch.from_numpy(live_units(params.numpy(), k, H, L, bi[:, :k].numpy()))
    base = torch.randn(2 * P, generator=g) * 0.3
    return params, bi, base


@functools.lru_cache(maxsize=None)
def fit_reference(P, k, kp, H, L, margin):
    """the float64 reference of a case: computed once, shared by the tests, never written to"""
    params, bi, base = fit_problem(P, k, kp, H, L)
    return pair_mlp_f64(params.numpy(), k, H, L, bi[:, :k].numpy(), base.numpy(), margin, 1.0 / P)


class PairFit:
    """fmx_mlp_pair_fit on one case's device buffers; run() starts from the case's parameters every time"""

    def __init__(self, fmx, P, k, kp, H, L):
        self.fmx, self.lib = fmx, fmx._lib.load()
        self.P, self.k, self.kp, self.H, self.L = P, k, kp, H, L
        params, bi, base = fit_problem(P, k, kp, H, L)
        self.p0, self.bi, self.base = params.cuda(), bi.cuda(), base.cuda()
        self.params = self.p0.clone()
        self.m = fmx._lib.Mlp(self.params.data_ptr(), L, k, H, 0)
        f = dict(device="cuda")
        self.dz, self.logit = torch.empty(2 * P, **f), torch.empty(2 * P, **f)
        self.gbi, self.loss = torch.full((2 * P, kp), 7.0, **f), torch.zeros(1, **f)
        self.hyper = fmx.Hyper(lr=LR, eps=1e-8)

    def run(self, margin, rule="sgd", opt=None, base=None):
        base = self.base if base is None else base
        self.params.copy_(self.p0)
        for t in (self.dz, self.logit, self.gbi, self.loss):
            t.fill_(float("nan"))
        self.fmx._lib.check(self.lib.fmx_mlp_pair_fit(
            C.byref(self.m), self.hyper.ref(), self.fmx._lib.RULES[rule], self.bi.data_ptr(), self.kp, base.data_ptr(), self.P, margin,
            1.0 / self.P, self.logit.data_ptr(), self.dz.data_ptr(), self.gbi.data_ptr(), self.loss.data_ptr(),
            None if opt is None else opt.ref(), stream()))
        torch.cuda.synchronize()

    def forward_logit(self, base=None):
        """fmx_mlp_forward's out on the same bi / base and the case's parameters"""
        base = self.base if base is None else base
        m0 = self.fmx._lib.Mlp(self.p0.data_ptr(), self.L, self.k, self.H, 0)      # (read only)
        out = torch.empty_like(self.logit)
        self.fmx._lib.check(self.lib.fmx_mlp_forward(C.byref(m0), self.bi.data_ptr(), self.kp, base.data_ptr(), 2 * self.P,
                                                     out.data_ptr(), None, stream()))
        torch.cuda.synchronize()
        return out

    def outputs(self):
        return [t.clone() for t in (self.dz, self.gbi, self.logit, self.loss)]


def check_fit_epilogue(s, margin, what):
    """check_section_epilogue's bounds (the module docstring) on fmx_mlp_pair_fit's outputs, from the device's own logits"""
    P, inv_b = s.P, 1.0 / s.P
    z = s.logit.double().cpu().numpy()
    dz = s.dz.cpu()
    assert np.isfinite(z).all() and np.isfinite(dz.numpy()).all() and np.isfinite(s.gbi.cpu().numpy()).all(), what
    assert np.isfinite(s.params.cpu().numpy()).all() and np.isfinite(s.loss.item()), what
    ref_loss, g = pair_loss_f64(z[0::2] - z[1::2], margin)
    ref_dz = g * inv_b
    err, tol = np.abs(dz[0::2].double().numpy() - ref_dz), 1e-5 * np.abs(ref_dz) + 4 * EPS32 * inv_b
    print(f"{what} dz: worst err/tol {float((err / tol).max()):.3f}")
    assert (err <= tol).all(), f"{what} dz: worst err/tol {float((err / tol).max()):.3f}"
    same_bits(dz[1::2], -dz[0::2], what + " dz[2i+1] == -dz[2i]")
    want = ref_loss.sum() * inv_b
    tol = inv_b * ((1e-5 * np.abs(ref_loss) + 4 * EPS32 * (1 + np.abs(ref_loss))).sum() + 2 * P * EPS32 * np.abs(ref_loss).sum())
    err = abs(s.loss.item() - want)
    print(f"{what} loss_out: err/tol {err / tol:.3f}")
    assert err <= tol, f"{what} loss_out {s.loss.item()} vs {want}: err/tol {err / tol:.3f}"
    return z


@pytest.mark.parametrize("margin", MARGINS)
@pytest.mark.parametrize("k,kp,H,L", FIT_SHAPES)
@pytest.mark.parametrize("P", FIT_PAIRS)
def test_pair_fit_forward_identity_epilogue_and_float64(fmx, P, k, kp, H, L, margin):
    s = PairFit(fmx, P, k, kp, H, L)
    what = f"P={P} k={k} H={H} L={L}"
    s.run(margin)
    same_bits(s.logit, s.forward_logit(), "logit_out vs fmx_mlp_forward")
    z = check_fit_epilogue(s, margin, what)
    # ---- against float64 ----
    r = fit_reference(P, k, kp, H, L, margin)
    for l in range(L):   # every layer is exercised (a bias gradient sums +g and -g: at hidden = 1 with one pair it is exactly 0 in float64 too)
        assert np.any(r["grads"][l][0]) and (np.any(r["grads"][l][1]) or H == 1), f"layer {l} has no live unit (a dead network)"
    close(s.logit.cpu().numpy(), r["out"], "logit")
    close(s.loss.item(), r["loss"], "loss")
    close(s.dz.cpu().numpy(), r["dz"], "dz")
    gbi = s.gbi.cpu().numpy()
    close(gbi[:, :k], r["gbi"], "gbi")
    assert (gbi[:, k:] == 0).all(), "padding columns of gbi must be zeroed"
    # the SGD step: -lr times the float64 gradient, close_per_tensor's bound on the gradient plus one rounding of the parameter
    p0, p1 = s.p0.cpu().numpy().astype(np.float64), s.params.cpu().numpy().astype(np.float64)
    assert not np.array_equal(p0, p1), "the network did not move"
    off = 0
    for l in range(L):
        i = k if l == 0 else H
        for name, n, g_ref, g_noise in (("W", H * i, r["grads"][l][0], r["gnoise"][l][0]), ("b", H, r["grads"][l][1], r["gnoise"][l][1])):
            close(p1[off:off + n] - p0[off:off + n], -LR * g_ref.reshape(-1), f"{what}: step of {name}{l}",
                  floor=LR * 4 * g_noise.reshape(-1) + EPS32 * np.abs(p1[off:off + n]))
            off += n
    assert off == p0.size
    # ---- logit differences from -30 to 30: the positives' base moved so that d_i becomes the target ----
    target = np.linspace(-30.0, 30.0, P) if P > 1 else np.array([30.0])
    wide = s.base.clone()
    wide[0::2] += torch.from_numpy(target - (z[0::2] - z[1::2])).float().cuda()
    s.run(margin, base=wide)
    same_bits(s.logit, s.forward_logit(wide), "logit_out vs fmx_mlp_forward (wide)")
    z = check_fit_epilogue(s, margin, what + " wide")
    d = z[0::2] - z[1::2]
    assert P == 1 or (d.min() < -25 and d.max() > 25)


@pytest.mark.parametrize("k,kp,H,L", FIT_SHAPES)
@pytest.mark.parametrize("P", FIT_PAIRS)
def test_pair_fit_rules(fmx, P, k, kp, H, L):
    """dz, gbi, logit and loss do not depend on the rule; opt (SGD) is rule SGD at the same lr; opt->step is read only; under
    opt ADAM m and v move, under ADAGRAD m keeps its bits."""
    margin = 0.1
    s = PairFit(fmx, P, k, kp, H, L)
    s.run(margin, rule="sgd")
    first, by_rule_sgd = s.outputs(), s.params.clone()
    s.run(margin, rule="signadam")
    for name, a, b in zip(("dz", "gbi", "logit", "loss"), first, s.outputs()):
        same_bits(a, b, f"rule signadam: {name}")
    assert not torch.equal(s.params, s.p0) and not torch.equal(s.params, by_rule_sgd)
    n = s.p0.numel()
    g = torch.Generator().manual_seed(n)
    for rule in ("sgd", "adagrad", "adam"):
        opt = fmx.MlpOpt(n, rule, lr=LR, device="cuda", step=5)
        opt.m.copy_((torch.randn(n, generator=g) * 1e-3).cuda())
        opt.v.copy_((torch.randn(n, generator=g) ** 2 * 1e-5).cuda())
        m0, v0 = opt.m.clone(), opt.v.clone()
        s.run(margin, rule="signadam", opt=opt)            # (`rule` is not read with opt)
        for name, a, b in zip(("dz", "gbi", "logit", "loss"), first, s.outputs()):
            same_bits(a, b, f"opt {rule}: {name}")
        assert opt.c.step == 5 and opt.step == 5, "opt->step is read, never written"
        if rule == "sgd":
            same_bits(s.params, by_rule_sgd, "opt (SGD) vs rule SGD at the same lr")
            same_bits(opt.m, m0, "opt (SGD): m")
            same_bits(opt.v, v0, "opt (SGD): v")
        else:
            assert not torch.equal(s.params, s.p0) and not torch.equal(opt.v, v0), rule
            if rule == "adagrad":
                same_bits(opt.m, m0, "adagrad neither loads nor stores m")
            else:
                assert not torch.equal(opt.m, m0)


# ---------------------------------------------------------------------------------------------------------------
# 2: the loop, three ways
# ---------------------------------------------------------------------------------------------------------------
RULE_PAIRS = [("signadam", None), ("sgd", None), ("adam", "adam"), ("adagrad", "adagrad"), ("signadam", "adam"), ("sgd", "adagrad"),
              ("adam", "sgd")]
MARGIN = 0.1


def pair_stream(sizes, k, N, seed, item=ITEM, with_x=True):
    """-> (rows int32 [2N, F], x float32 [2N, F] or None): zipf-drawn positives (the same rows again and again); the negative is
    the positive with one item column (even pairs) or both (odd pairs) redrawn from the same law; pair 5's negative is its
    positive in every column (and in x), pair 6's differs from its positive in every column; about 10 % of x is exactly 0."""
    _, idx, x, _ = problem(sizes, k, 2 * N, seed)
    rows = idx.copy()
    rows[1::2] = rows[0::2]
    rows[1::2, item[1]] = idx[1::2, item[1]]
    rows[3::4, item[0]] = idx[3::4, item[0]]
    if N > 6:
        rows[11], x[11] = rows[10], x[10]
        rows[13] = (rows[12] + 1) % np.asarray(sizes, dtype=np.int32)
    return rows, (x if with_x else None)


def assert_stream_has_the_cases(rows, sizes, N):
    pos, neg = rows[0::2], rows[1::2]
    differ = (pos != neg).sum(1)
    assert len(np.unique(pos[:, ITEM[1]])) < N, "zipf: rows repeat across pairs"
    assert (differ == 1).sum() > 5 and (differ == 2).sum() > 5, "pairs with one and with two item columns replaced"
    assert (differ == 0).any(), "a pair whose negative is its positive: every field a run of two"
    assert (differ == len(sizes)).any(), "a pair that differs in every column"


def snapshot(t, params, opt, outs):
    torch.cuda.synchronize()
    pred, logit, loss = outs
    s = dict(rows=t.rows.cpu().numpy().copy(), bias=t.bias.cpu().numpy().copy(), params=params.cpu().numpy().copy(),
             pred=pred.cpu().numpy().copy(), logit=logit.cpu().numpy().copy(), loss=loss.cpu().numpy().copy(),
             steps=np.array([t.step if t.layout == "moments" else -1, -1 if opt is None else opt.step]))
    if opt is not None:
        s.update(m=opt.m.cpu().numpy().copy(), v=opt.v.cpu().numpy().copy())
    return s


def assert_same(a, b, what):
    for kk in a:
        np.testing.assert_array_equal(a[kk].view(np.int32) if a[kk].dtype == np.float32 else a[kk],
                                      b[kk].view(np.int32) if b[kk].dtype == np.float32 else b[kk], err_msg=f"{what}: {kk}")


def per_pair(e, t, hyp, table_rule, params, k, H, L, fm_term, idx_d, xv_d, opt, margin=MARGIN):
    """The N per-pair sequences from outside: fmx_fm_forward (B = 2, no loss), the NFM base add, fmx_mlp_pair_fit (B_pairs = 1,
    inv_b = 1), fmx_sort_occurrences (B = 2), fmx_fm_update (B = 2); FMEngine advances the table's and the network's counts."""
    N = idx_d.shape[0] // 2
    pred = torch.empty(N, dtype=torch.uint8, device="cuda")
    logit, loss = torch.empty(2 * N, device="cuda"), torch.empty(N, device="cuda")
    for i in range(N):
        r = idx_d[2 * i:2 * i + 2]
        xi = None if xv_d is None else xv_d[2 * i:2 * i + 2]
        e.forward(hyp, r, xi, want_first=False, want_bi=True)
        base = (e.logit[:2] if fm_term else e.sfirst[:2] + t.bias[0]).contiguous()
        dz, gbi, z = e.mlp_pair_fit(params, k, H, L, hyp, table_rule if opt is None else "sgd", base, 1, margin=margin, inv_b=1.0,
                                    mlp_opt=opt, want_logit=True)
        pred[i] = z[0] > z[1]
        logit[2 * i:2 * i + 2] = z
        loss[i] = e.loss_out[0]
        e.sort(r)
        e.update(hyp, table_rule, 2, xi, dz, dz if fm_term else None, gbi, inv_b=1.0, with_loss=False)
    return pred, logit, loss


def loop(e, hyp, table_rule, params, k, H, L, fm_term, idx_d, xv_d, opt, margin=MARGIN):
    return e.online_run_mlp_pair(hyp, table_rule, params, k, H, L, fm_term, idx_d, xv_d, margin=margin, mlp_opt=opt, want_logit=True,
                                 want_loss=True)


def three_ways(fmx, make, table_rule, k, H, L, fm_term, rows, x, forms=("one workgroup", "queued", "per pair"), flag=False):
    """make() -> (table, engine, hyper, params, opt or None), identical every time.  -> {form: snapshot}"""
    res = {}
    for form in forms:
        t, e, hyp, params, opt = make()
        idx_d, xv_d, _ = e.to_device(rows, x)
        if form == "per pair":
            outs = per_pair(e, t, hyp, table_rule, params, k, H, L, fm_term, idx_d, xv_d, opt)
        else:
            with persistent(fmx, form != "queued"):
                outs = loop(e, hyp, table_rule, params, k, H, L, fm_term, idx_d, xv_d, opt)
        torch.cuda.synchronize()
        if flag:
            assert int(e.error.item()) == 1, f"{form}: the index flag was not raised"
            e.error.zero_()
        else:
            e.check_error_flag()
        res[form] = snapshot(t, params, opt, outs)
    return res


def maker(fmx, table_rule, net_rule, k, H, L, seed, sizes=SIZES):
    def make():
        t, e, hyp, params, opt = setup(fmx, table_rule, net_rule or "sgd", k, H, L, seed=seed, sizes=sizes)
        return t, e, hyp, params, (opt if net_rule else None)
    return make


@pytest.mark.parametrize("kp", [4, 16, 64])
@pytest.mark.parametrize("table_rule,net_rule", RULE_PAIRS)
@pytest.mark.parametrize("fm_term", [1, 0], ids=["deepfm", "nfm"])
def test_one_workgroup_equals_queued_equals_per_pair_calls(fmx, fm_term, table_rule, net_rule, kp):
    k, H, L, N = K_OF_KP[kp], 32, 2, 200
    with_x = (RULE_PAIRS.index((table_rule, net_rule)) + [4, 16, 64].index(kp) + fm_term) % 2 == 0     # xv given / null (all ones)
    rows, x = pair_stream(SIZES, k, N, 6100 + kp, with_x=with_x)
    assert_stream_has_the_cases(rows, SIZES, N)
    assert x is None or (x == 0).any()
    make = maker(fmx, table_rule, net_rule, k, H, L, seed=kp)
    res = three_ways(fmx, make, table_rule, k, H, L, fm_term, rows, x)
    whole = res["one workgroup"]
    moments = table_rule in ("adam", "adagrad")
    assert list(whole["steps"]) == [T_STEP0 + N if moments else -1, NET_STEP0 + N if net_rule else -1]
    assert_same(whole, res["queued"], "one workgroup vs queued launches")
    assert_same(whole, res["per pair"], "one workgroup vs per-pair calls")
    # the pair whose negative is its positive: d = 0 exactly, predicted "not above"
    assert whole["logit"][10].view(np.int32) == whole["logit"][11].view(np.int32) and whole["pred"][5] == 0
    assert 0 < whole["pred"].sum() < N and np.isfinite(whole["loss"]).all() and np.isfinite(whole["logit"]).all()
    t0, _, _, p0, o0 = make()
    assert not np.array_equal(whole["params"], p0.cpu().numpy()), "the network did not move"
    if net_rule == "adagrad":
        np.testing.assert_array_equal(whole["m"], o0.m.cpu().numpy(), err_msg="adagrad neither loads nor stores m")
        assert not np.array_equal(whole["v"], o0.v.cpu().numpy())
    elif net_rule == "adam":
        assert not np.array_equal(whole["m"], o0.m.cpu().numpy()) and not np.array_equal(whole["v"], o0.v.cpu().numpy())
    elif net_rule == "sgd":
        np.testing.assert_array_equal(whole["m"], o0.m.cpu().numpy())
        np.testing.assert_array_equal(whole["v"], o0.v.cpu().numpy())
    # untouched rows keep their bits; the bias gradient is exactly +0: only ADAM (whose moments decay) moves the bias words
    offs = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    touched = np.unique(rows.astype(np.int64) + offs[:-1][None, :])
    untouched = np.setdiff1d(np.arange(t0.n_rows), touched)
    assert untouched.size > 0
    rows0 = t0.rows.cpu().numpy()
    np.testing.assert_array_equal(whole["rows"][untouched].view(np.int32), rows0[untouched].view(np.int32))
    assert not np.array_equal(whole["rows"][touched], rows0[touched])
    if table_rule != "adam":
        np.testing.assert_array_equal(whole["bias"].view(np.int32), t0.bias.cpu().numpy().view(np.int32))
    else:
        assert not np.array_equal(whole["bias"], t0.bias.cpu().numpy())


# ---------------------------------------------------------------------------------------------------------------
# 3: field counts at the edges of the wavefront form; FTRL tables
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [4, 16, 17])
def test_field_counts_around_the_wavefront_form(fmx, F):
    """kp = 64: four rows per pass, four passes.  F = 4 is one pass, F = 16 the most one wavefront holds per sample; F = 17 takes
    the queued form whatever online_persistent says, and still equals the per-pair sequence."""
    k, H, L, N = 60, 32, 2, 40
    sizes = [5 + i % 7 for i in range(F)]
    rows, x = pair_stream(sizes, k, N, 6300 + F, item=(F - 2, F - 1))
    make = maker(fmx, "adam", "adam", k, H, L, seed=F, sizes=sizes)
    assert make()[0].kp == 64 and fmx.FMEngine.online_run_fits(F, 64) == (F <= 16)
    res = three_ways(fmx, make, "adam", k, H, L, 1, rows, x)
    assert_same(res["one workgroup"], res["per pair"], f"F = {F}: online_persistent on vs per-pair calls")
    assert_same(res["queued"], res["per pair"], f"F = {F}: queued vs per-pair calls")


@pytest.mark.parametrize("net_rule", ["adam", "sgd"])
def test_ftrl_table_with_opt_takes_the_queued_form(fmx, net_rule):
    k, H, L, N = 16, 32, 2, 40
    rows, x = pair_stream(SIZES, k, N, 6400)

    def make():
        t, _ = build_table(fmx, SIZES, k, "ftrl")
        e, hyp = fmx.FMEngine(t, max_batch=8), fmx.Hyper(**HYP)
        _, _, _, params, opt = setup(fmx, "sgd", net_rule, k, H, L, seed=3, sizes=SIZES)
        return t, e, hyp, params, opt
    res = three_ways(fmx, make, "ftrl", k, H, L, 1, rows, x)
    assert_same(res["one workgroup"], res["per pair"], "FTRL tables: online_persistent on vs per-pair calls")
    assert_same(res["queued"], res["per pair"], "FTRL tables: queued vs per-pair calls")
    t0 = make()[0]
    assert not np.array_equal(res["queued"]["rows"], t0.rows.cpu().numpy())
    np.testing.assert_array_equal(res["queued"]["bias"].view(np.int32), t0.bias.cpu().numpy().view(np.int32))


# ---------------------------------------------------------------------------------------------------------------
# 4: halves equal the whole
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["one workgroup", "queued"])
def test_two_halves_equal_one_call(fmx, form):
    k, H, L, N = 16, 32, 2, 200
    rows, x = pair_stream(SIZES, k, N, 6500)
    res = []
    for cuts in ([N], [N // 2, N - N // 2]):
        t, e, hyp, params, opt = setup(fmx, "adam", "adam", k, H, L, seed=2, sizes=SIZES)
        idx_d, xv_d, _ = e.to_device(rows, x)
        outs, lo = [], 0
        with persistent(fmx, form == "one workgroup"):
            for c in cuts:
                outs.append(loop(e, hyp, "adam", params, k, H, L, 1, idx_d[2 * lo:2 * (lo + c)], xv_d[2 * lo:2 * (lo + c)], opt))
                lo += c
                assert t.step == T_STEP0 + lo and opt.step == NET_STEP0 + lo
        e.check_error_flag()
        res.append(snapshot(t, params, opt, [torch.cat(o) for o in zip(*outs)]))
    assert_same(res[0], res[1], f"{form}: one call vs two halves")


# ---------------------------------------------------------------------------------------------------------------
# 5: guard bands
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["one workgroup", "queued"])
@pytest.mark.parametrize("fm_term", [1, 0], ids=["deepfm", "nfm"])
def test_guard_bands(fmx, form, fm_term):
    """Every buffer the call writes sits between NaN-patterned bands that must survive: pred_out, logit_out, loss_out, scratch,
    the fwd buffers, the workspace, params, m, v."""
    L_ = fmx._lib
    lib = L_.load()
    k, H, L, N = 16, 32, 2, 40
    rows, x = pair_stream(SIZES, k, N, 6600)
    t, e, hyp, params, opt = setup(fmx, "adam", "adam", k, H, L, seed=4, sizes=SIZES)
    idx_d, xv_d, _ = e.to_device(rows, x)
    kp, n = t.kp, params.numel()
    g = {name: Guarded(4 * words, name=name) for name, words in
         (("logit_out", 2 * N), ("loss_out", N), ("scratch", 2 * kp + 8), ("S", 2 * kp), ("bi", 2 * kp), ("sfirst", 2), ("logit", 2),
          ("params", n), ("m", n), ("v", n))}
    g["pred_out"] = Guarded(N, dtype=torch.uint8, name="pred_out")
    g["error"] = Guarded(4, dtype=torch.int32, name="error")
    g["workspace"] = Guarded(int(lib.fmx_workspace_bytes(t.c_struct(), 2)), dtype=torch.int32, name="workspace")
    g["params"].t.copy_(params)
    g["m"].t.copy_(opt.m)
    g["v"].t.copy_(opt.v)
    out = L_.FwdOut()
    out.S, out.bi, out.sfirst, out.logit, out.error = g["S"].ptr, g["bi"].ptr, g["sfirst"].ptr, g["logit"].ptr, g["error"].ptr
    mlp = L_.Mlp(g["params"].ptr, L, k, H, 0)
    o = L_.MlpOpt(g["m"].ptr, g["v"].ptr, opt.c.lr, opt.c.eps, opt.c.beta1, opt.c.beta2, opt.c.rule, NET_STEP0)
    hyp.c.step = t.step
    with persistent(fmx, form == "one workgroup"):
        L_.check(lib.fmx_online_run_mlp_pair(t.c_struct(), hyp.ref(), L_.RULES["adam"], C.byref(mlp), fm_term, idx_d.data_ptr(),
                                             xv_d.data_ptr(), N, MARGIN, g["workspace"].ptr, g["workspace"].nbytes, C.byref(out),
                                             g["scratch"].ptr, g["pred_out"].ptr, g["logit_out"].ptr, g["loss_out"].ptr, C.byref(o),
                                             stream()))
    torch.cuda.synchronize()
    for b in g.values():
        b.check()
    assert int(g["error"].t[0].item()) == 0
    assert not torch.equal(g["params"].t, params) and np.isfinite(g["loss_out"].t.cpu().numpy()).all() and np.isfinite(g["logit_out"].t.cpu().numpy()).all()


# ---------------------------------------------------------------------------------------------------------------
# 6: the index flag
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["positive", "negative"])
def test_out_of_range_index_in_one_sample_only(fmx, where):
    """An index past its field in ONE sample of a pair: the flag is raised in both forms, that occurrence is dropped and the
    other sample's row of the field is a run of one -- the bits of the per-pair sequence, whose sort drops the occurrence.
    The rows no valid index names keep their bits (the row the bad index would alias among them)."""
    k, H, L, N = 16, 32, 2, 20
    rows, x = pair_stream(SIZES, k, N, 6700)
    f, i = 4, 7
    rows[2 * i] = rows[2 * i + 1]                     # the same row in both samples of every field: without the bad index, runs of two
    bad = 2 * i + (where == "negative")
    rows[bad, f] = SIZES[f] + 5                       # would alias row 5 of the next field
    rows[:, f + 1] = np.minimum(rows[:, f + 1], 4)    # ... which nothing else names
    make = maker(fmx, "adam", "adam", k, H, L, seed=8)
    res = three_ways(fmx, make, "adam", k, H, L, 1, rows, x, flag=True)
    assert_same(res["one workgroup"], res["per pair"], f"bad index in the {where}: one workgroup vs per-pair calls")
    assert_same(res["queued"], res["per pair"], f"bad index in the {where}: queued vs per-pair calls")
    t0 = make()[0]
    offs = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    valid = rows.astype(np.int64) < np.asarray(SIZES)[None, :]
    touched = np.unique((rows.astype(np.int64) + offs[:-1][None, :])[valid])
    untouched = np.setdiff1d(np.arange(t0.n_rows), touched)
    assert offs[f + 1] + 5 in untouched
    np.testing.assert_array_equal(res["one workgroup"]["rows"][untouched].view(np.int32), t0.rows.cpu().numpy()[untouched].view(np.int32))
    # the other sample's row of that field moved
    other = offs[f] + rows[bad ^ 1, f]
    assert not np.array_equal(res["one workgroup"]["rows"][other], t0.rows.cpu().numpy()[other])


# ---------------------------------------------------------------------------------------------------------------
# 7: the LDS cap
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,where", [(61, "the largest network of this shape under the cap: 96 KB of parameters and moments in LDS"),
                                     (63, "just above the cap: the queued form")])
def test_networks_around_the_lds_cap(fmx, k, where):
    """H = 64, L = 2: 8,128 parameters at k = 61, 8,256 at k = 63, around the one-workgroup form's 8,192 (the shapes of
    test_online_adaptive_gpu.test_networks_around_the_lds_cap), with the network under ADAM: params, v and m in LDS."""
    H, L, N = 64, 2, 40
    n = n_params(k, H, L)
    assert (n <= 8192) == (k == 61) and abs(n - 8192) <= 64
    rows, x = pair_stream(SIZES, k, N, 6800 + k)
    res = three_ways(fmx, maker(fmx, "adam", "adam", k, H, L, seed=k), "adam", k, H, L, 1, rows, x)
    assert_same(res["one workgroup"], res["queued"], f"{where}: default vs queued")
    assert_same(res["one workgroup"], res["per pair"], f"{where}: default vs per-pair calls")


# ---------------------------------------------------------------------------------------------------------------
# 8: the classes
# ---------------------------------------------------------------------------------------------------------------
def by_hand_loop(m, Xi, Xv, item, neg, margin):
    """run_pair_experiment(full=True)'s device loop restated with the engine's per-pair sequence -> correct predictions"""
    import fmx
    e = m._engine
    rows, xv = fmx.pairwise.assemble_pairs(torch.from_numpy(Xi).cuda(), torch.from_numpy(Xv).cuda(), item, torch.from_numpy(neg).cuda())
    pred, _, loss = per_pair(e, m._table, m._hyper, m.update_rule, m._mlp_flat, m.embedding_size, m.neuron_per_hidden_layer,
                             m.num_hidden_layers, m._fm_term_in_forward, rows.contiguous(), None if xv is None else xv.contiguous(),
                             m._mlp_fused, margin=margin)
    return int(pred.sum().item()), loss


@pytest.mark.parametrize("cls,rule", [("DeepFMAdam", "signadam"), ("NFMAdam", "adam")])
def test_run_pair_experiment_on_the_device_is_the_per_pair_sequence(fmx, cls, rule):
    N = 30
    Xi, Xv, item, neg = class_data(N, seed=8)
    a, b, c = new_model(cls, rule), new_model(cls, rule), new_model(cls, rule)
    assert a.pair_loop_on_device is False
    a.pair_loop_on_device = True
    assert a._pair_device_loop_ok()
    secs, acc, checkpoints, counts = a.run_pair_experiment(Xi, Xv, item, negatives=neg, margin=0.0, full=True)
    correct, _ = by_hand_loop(b, Xi, Xv, item, neg, 0.0)
    torch.cuda.synchronize()
    for (name, wa), (_, wb) in zip(model_words(a), model_words(b)):
        same_bits(wa, wb, f"{cls} {rule}: {name}")
    assert counts == {"correct": correct, "wrong": N - correct} and a._table.step == b._table.step
    assert a._mlp_fused is None or a._mlp_fused.step == b._mlp_fused.step == N
    assert acc == checkpoints[-1] == pytest.approx(100.0 * correct / N) and len(checkpoints) == 2 and secs > 0
    # with the attribute False the model takes the path it takes today: the host loop of one-pair fit_pairs(full=True) calls
    d = new_model(cls, rule)
    c.run_pair_experiment(Xi, Xv, item, negatives=neg, margin=0.0, full=True)
    for i in range(N):
        d.fit_pairs(Xi[i:i + 1], Xv[i:i + 1], item, negatives=neg[i:i + 1], full=True)
    torch.cuda.synchronize()
    for (name, wc), (_, wd) in zip(model_words(c), model_words(d)):
        same_bits(wc, wd, f"{cls} {rule}, attribute False: {name}")


@pytest.mark.parametrize("cls,rule", [("DeepFMAdam", "signadam"), ("NFMAdam", "adam")])
def test_the_device_loop_learns(fmx, cls, rule):
    """Thirty pairs repeated over a few passes bring the mean pair loss of the device loop down."""
    N = 30
    Xi, Xv, item, neg = class_data(N, seed=9)
    m = new_model(cls, rule)
    rows, xv = fmx.pairwise.assemble_pairs(torch.from_numpy(Xi).cuda(), torch.from_numpy(Xv).cuda(), item, torch.from_numpy(neg).cuda())
    means = []
    for _ in range(6):
        _, _, loss = m._engine.online_run_mlp_pair(m._hyper, m.update_rule, m._mlp_flat, m.embedding_size, m.neuron_per_hidden_layer,
                                                   m.num_hidden_layers, m._fm_term_in_forward, rows.contiguous(), xv.contiguous(),
                                                   margin=0.0, mlp_opt=m._mlp_fused, want_loss=True)
        means.append(float(loss.mean().item()))
    m._engine.check_error_flag()
    print("mean pair loss per pass:", means)
    assert means[-1] < means[0]
