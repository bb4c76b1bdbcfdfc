"""fmx_afm_step_opt (the AFM step with the attention parameters under their rule inside the gradient reduction) and fmx_afm_stream
(many steps in one call) on the GPU: the step against fmx_afm_step bit for bit and against the float64 rules on afm_f64's
gradients, adam / adagrad trajectories against float64 torch.optim.Adam / Adagrad (a dead unit's parameters still move), the
stream against step-by-step calls bit for bit, and AFMAdam(fused_optimizer=True): update_embedding, fit, pickling, the index flag."""
import contextlib
import functools
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from afm_f64 import afm_f64  # noqa: E402
from helpers import assert_within_f64  # noqa: E402
from test_afm_gpu import (AHYP, DZ_ABS, HYP, _assert_delta, _check_rule, _chunk, _floors_gn, _live, _model_state, _sizes,  # noqa: E402
                          assert_exercised, batch, engine, make, state_of)
from test_afm_stream_cpu import torch_dense_step  # noqa: E402

pytestmark = pytest.mark.gpu

LAYOUT = {"sgd": "weights", "signadam": "weights", "ftrl": "ftrl", "adam": "moments", "adagrad": "moments"}
ATTN_RULE = {"sgd": "sgd", "signadam": "signadam", "ftrl": "signadam", "adam": "adam", "adagrad": "adagrad"}   # AFMAdam's policy


def _fmx():
    import fmx
    return fmx


def attn_opt(arule, n, step=0):
    """The attention parameters' state under `arule` with the hyper-parameters the float64 checks use: HYP's for the rules
    test_afm_gpu._check_rule restates (sgd, signadam), test_adaptive_rules_gpu.HYP's for adam / adagrad."""
    fmx = _fmx()
    if arule in ("adam", "adagrad"):
        h = AHYP[arule]
        return fmx.AfmOpt(n, arule, lr=float(h["lr"]), eps=float(h["eps"]), beta1=float(h["beta1"]), beta2=float(h["beta2"]),
                          device="cuda", step=step)
    return fmx.AfmOpt(n, arule, lr=HYP["lr"], eps=HYP["eps"], device="cuda", step=step)


def f64(t):
    return t.detach().double().cpu().numpy()


def check_attention(arule, h, s, before, after, ref, what):
    """The attention parameters (and moments) after step s against the float64 rule on afm_f64's gradient from the state before
    it.  before / after: (p, m, v) float64.  The gradient's bound is 1e-5 relative plus afm_f64's floor, carried through the rule
    as test_afm_gpu does: _check_rule for sgd / signadam, _floors_gn + _assert_delta for adam / adagrad (torch.optim.Adam's eps
    enters as eps sqrt(1 - beta2^s) in _floors' form of the rule)."""
    g = ref["dparams"]
    gn = 1e-5 * np.abs(g) + ref["fl_dparams"] + 1e-30
    if arule in ("sgd", "signadam"):
        _check_rule(arule, after[0], before[0], g, gn, f"{what} attention parameters")
        return
    p2, m2, v2 = torch_dense_step(arule, h, s, before[0], before[1], before[2], g)
    ha = dict(h, eps=h["eps"] * (np.sqrt(1 - float(h["beta2"]) ** s) if arule == "adam" else 1.0))
    fp, fm, fv = _floors_gn(arule, ha, s, g, gn, m2, v2)
    _assert_delta(after[0], before[0], p2, fp, f"{what} attention parameters")
    _assert_delta(after[2], before[2], v2, fv, f"{what} attention second moments")
    if arule == "adam":
        _assert_delta(after[1], before[1], m2, fm, f"{what} attention first moments")


def opt_state(params, opt):
    return f64(params), f64(opt.m), f64(opt.v)


# ---- one step: fmx_afm_step_opt against fmx_afm_step (bits) and against float64 (the attention parameters) ----
@pytest.mark.parametrize("F,k,t,B", [pytest.param(39, 16, 16, 300, id="F39-k16-t16-multi_tile"), pytest.param(3, 4, 4, 64, id="F3-k4-t4")])
@pytest.mark.parametrize("rule", ["sgd", "signadam", "ftrl", "adagrad", "adam"])
def test_step_opt_matches_step_and_f64(rule, F, k, t, B):
    fmx = _fmx()
    sizes, arule = _sizes(F, F + 5), ATTN_RULE[rule]
    idx, xv, y, rows = batch(sizes, B, seed=F + 11, xv_kind="random", hot=True)
    runs = []
    for with_opt in (False, True):
        tb, params, st = make(sizes, k, t, layout=LAYOUT[rule], seed=F + 3)
        _live(tb, params, st, k, t, rows, xv)
        eng = engine(tb, params, t, B)
        opt = attn_opt(arule, params.numel()) if with_opt else None
        idx_d, xv_d, y_d = eng.to_device(idx, xv, y)
        eng.step(fmx.Hyper(**HYP), rule, idx_d, xv_d, y_d, opt=opt)
        torch.cuda.synchronize()
        assert int(eng.error.item()) == 0
        runs.append(dict(tb=tb, params=params, st=st, eng=eng, opt=opt))
    a, b = runs
    for what, x, z in (("attn_grad_out", a["eng"].grad, b["eng"].grad), ("loss", a["eng"].loss_out, b["eng"].loss_out),
                       ("table rows", a["tb"].rows, b["tb"].rows), ("bias words", a["tb"].bias, b["tb"].bias)):
        assert torch.equal(x, z), f"{rule}: {what} differs from fmx_afm_step's"
    assert a["tb"].step == b["tb"].step and b["opt"].step == 1
    before = a["st"]["params"]
    np.testing.assert_array_equal(a["params"].cpu().numpy(), before, err_msg="fmx_afm_step moved the attention parameters")
    ref = afm_f64(a["st"]["V"], a["st"]["w"], a["st"]["bias"], before, k, t, rows, xv, y, chunk=_chunk(F, k, t),
                  dz_abs=DZ_ABS if arule in ("adam", "adagrad") else 0.0)
    assert_exercised(ref, F, f"{rule} F={F}")
    assert_within_f64(b["eng"].grad.cpu().numpy(), ref["dparams"], ref["fl_dparams"], "attention gradient")
    zero = np.zeros(before.size)
    check_attention(arule, AHYP.get(arule), 1, (before.astype(np.float64), zero, zero), opt_state(b["params"], b["opt"]), ref,
                    f"{rule} F={F}")
    assert (b["params"].cpu().numpy() != before).any()
    if arule in ("sgd", "signadam"):          # no moments: m, v are never written
        assert not b["opt"].m.any() and not b["opt"].v.any()
    if arule == "adagrad":
        assert not b["opt"].m.any()


# ---- several steps of the persistent rules against float64 torch.optim.Adam / Adagrad ----
def _trajectory(rule, T, kill_unit_after=None):
    fmx = _fmx()
    F, k, t, B = 20, 16, 16, 300
    sizes, h = _sizes(F, 23), AHYP[rule]
    hyp = fmx.Hyper(lr=h["lr"], eps=h["eps"], beta1=h["beta1"], beta2=h["beta2"])
    tb, params, st = make(sizes, k, t, layout="moments", seed=17)
    data = [batch(sizes, B, seed=200 + s, xv_kind="random", hot=True) for s in range(T)]
    _live(tb, params, st, k, t, np.concatenate([d[3] for d in data]), np.concatenate([d[1] for d in data]))
    eng = engine(tb, params, t, B)
    opt = attn_opt(rule, params.numel())
    u = 5                                            # the unit that dies
    unit = np.concatenate([np.arange(u * k, (u + 1) * k), [t * k + u], [t * k + t + u]])      # its W row, b and h
    for s, (idx, xv, y, rows) in enumerate(data, start=1):
        dead = kill_unit_after is not None and s > kill_unit_after
        if dead and s == kill_unit_after + 1:
            params[t * k + u] = -1.0e3               # W q + b < 0 for every pair from here on
        tbl = state_of(tb)
        before = opt_state(params, opt)
        idx_d, xv_d, y_d = eng.to_device(idx, xv, y)
        eng.step(hyp, rule, idx_d, xv_d, y_d, opt=opt)
        torch.cuda.synchronize()
        assert tb.step == s and opt.step == s and int(eng.error.item()) == 0
        ref = afm_f64(tbl["V"], tbl["w"], tbl["bias"], before[0], k, t, rows, xv, y, chunk=_chunk(F, k, t), dz_abs=DZ_ABS)
        live = ref["unit_live"]
        if dead:
            assert not live[u] and live[np.arange(t) != u].all()
            assert not eng.grad.cpu().numpy()[unit].any(), "a dead unit takes an exactly-zero gradient"
        else:
            assert live.all(), f"step {s}: dead attention units {np.flatnonzero(~live)}"
        assert_within_f64(eng.grad.cpu().numpy(), ref["dparams"], ref["fl_dparams"], f"step {s} attention gradient")
        after = opt_state(params, opt)
        check_attention(rule, h, s, before, after, ref, f"{rule} step {s}")
        if dead:      # dense Adam: the moments of the live step decay and keep moving the unit's parameters
            assert (before[1][unit] != 0).all()
            assert (after[0][unit] != before[0][unit]).all(), "a dead unit's parameters stopped moving"
            assert (np.abs(after[1][unit]) < np.abs(before[1][unit])).all() and (after[2][unit] < before[2][unit]).all()


@pytest.mark.parametrize("rule", ["adam", "adagrad"])
def test_step_opt_trajectory_tracks_torch_f64(rule):
    _trajectory(rule, 4)


def test_step_opt_adam_moves_a_dead_units_parameters():
    _trajectory("adam", 3, kill_unit_after=1)


# ---- the stream ----
def _stream_start(rule, sizes, k, t, B, seed):
    tb, params, st = make(sizes, k, t, layout=LAYOUT[rule], seed=seed)
    eng = engine(tb, params, t, B)
    opt = attn_opt(ATTN_RULE[rule], params.numel(), step=2)      # the two step counts differ: each must advance on its own
    return tb, params, eng, opt


def _everything(tb, params, opt, losses):
    return dict(rows=tb.rows.cpu(), bias=tb.bias.cpu(), params=params.cpu(), m=opt.m.cpu(), v=opt.v.cpu(), losses=losses.cpu())


def _hyper(rule):
    fmx = _fmx()
    if rule in ("adam", "adagrad"):
        h = AHYP[rule]
        return fmx.Hyper(lr=h["lr"], eps=h["eps"], beta1=h["beta1"], beta2=h["beta2"])
    return fmx.Hyper(**HYP)


@pytest.mark.parametrize("rule,with_xv,B", [("sgd", False, 64), ("signadam", True, 600), ("ftrl", False, 130), ("adagrad", True, 64),
                                            ("adam", True, 128), ("adam", False, 1030)])
def test_stream_equals_step_by_step_bit_for_bit(rule, with_xv, B):
    """n_steps = 7 over a pool of 3: the stream against 7 fmx_afm_step_opt calls, against two calls of 3 + 4 steps, and against
    itself -- table (moments and bias words), params, m, v and every step's loss.  Under adam the table's count and the
    attention parameters' (started 2 apart) both advance: a stream that held either still would part from the single steps."""
    F, k, t, n_pool, n_steps = 10, 8, 8, 3, 7
    sizes = _sizes(F, 31)
    pool = [batch(sizes, B, seed=300 + j, xv_kind="random" if with_xv else "ones", hot=True) for j in range(n_pool)]
    idx_pool = torch.from_numpy(np.stack([p[0] for p in pool])).cuda().contiguous()
    xv_pool = torch.from_numpy(np.stack([p[1] for p in pool])).cuda().contiguous() if with_xv else None
    y_pool = torch.from_numpy(np.stack([p[2] for p in pool])).cuda().contiguous()
    hyp = _hyper(rule)

    tb, params, eng, opt = _stream_start(rule, sizes, k, t, B, seed=41)
    losses = torch.zeros(n_steps, device="cuda")
    for s in range(n_steps):
        j = s % n_pool
        eng.step(hyp, rule, idx_pool[j], None if xv_pool is None else xv_pool[j], y_pool[j], opt=opt)
        losses[s] = eng.loss_out[0]
    torch.cuda.synchronize()
    assert int(eng.error.item()) == 0 and opt.step == 2 + n_steps
    want = _everything(tb, params, opt, losses)
    assert bool((want["losses"] > 0).all())
    moments = LAYOUT[rule] == "moments"
    assert tb.step == (n_steps if moments else 0)

    for split in ((n_steps,), (3, 4), (n_steps,)):
        tb, params, eng, opt = _stream_start(rule, sizes, k, t, B, seed=41)
        losses = torch.full((n_steps,), -1.0, device="cuda")
        done = 0
        for n in split:
            eng.stream(hyp, rule, idx_pool, xv_pool, y_pool, B, n, opt, losses=losses[done:])
            done += n
        torch.cuda.synchronize()
        assert int(eng.error.item()) == 0 and opt.step == 2 + n_steps and tb.step == (n_steps if moments else 0)
        got = _everything(tb, params, opt, losses)
        for key in want:
            assert torch.equal(got[key], want[key]), f"{rule} stream {split}: {key} differs from the single steps'"


# ---- the one queue of steps behind the stream and the queued online run, at its smallest: kp = 4, 3 samples a step, a pool of
#      3 walked twice and a step more, 5 samples online -- without xv, and issued from a stream that is not torch's default.
#      (test_afm_pair_gpu and test_afm_list_gpu run the pair and list forms at the same shape.) ----
SMALL = dict(F=5, k=3, t=4, units=3, n_pool=3, n_steps=7, N=5)
SMALL_CASES = pytest.mark.parametrize("with_xv,side", [(False, False), (True, True)], ids=["no_xv", "side_stream"])
SMALL_RULES = pytest.mark.parametrize("rule", ["sgd", "adam"])


def issue(side, call):
    """call(stream) behind everything queued so far and waited for: stream None (torch's current, the default one) or, side, a
    stream of its own.  The comparison side of these tests is always single steps on the default stream."""
    torch.cuda.synchronize()
    stream = torch.cuda.Stream() if side else None
    call(stream)
    torch.cuda.synchronize()


@contextlib.contextmanager
def queued_online_form(option):
    """Inside, the online run whose one-workgroup kernel `option` switches takes its queued form"""
    lib = _fmx()._lib.load()
    assert lib.fmx_set_option(option, 0) == 1
    try:
        yield
    finally:
        lib.fmx_set_option(option, 1)


@functools.lru_cache(maxsize=None)
def _small_bce(rule, with_xv):
    """(sizes, pool and stream on the device, what the single steps on the default stream leave): computed once per case"""
    F, k, t, B, n_pool, n_steps, N = (SMALL[kk] for kk in ("F", "k", "t", "units", "n_pool", "n_steps", "N"))
    sizes, kind = _sizes(F, 31), "random" if with_xv else "ones"
    pool = [batch(sizes, B, seed=300 + j, xv_kind=kind) for j in range(n_pool)]
    idx_pool = torch.from_numpy(np.stack([p[0] for p in pool])).cuda().contiguous()
    xv_pool = torch.from_numpy(np.stack([p[1] for p in pool])).cuda().contiguous() if with_xv else None
    y_pool = torch.from_numpy(np.stack([p[2] for p in pool])).cuda().contiguous()
    hyp = _hyper(rule)
    tb, params, eng, opt = _stream_start(rule, sizes, k, t, B, seed=41)
    losses = torch.zeros(n_steps, device="cuda")
    for s in range(n_steps):
        j = s % n_pool
        eng.step(hyp, rule, idx_pool[j], None if xv_pool is None else xv_pool[j], y_pool[j], opt=opt)
        losses[s] = eng.loss_out[0]
    torch.cuda.synchronize()
    assert int(eng.error.item()) == 0 and opt.step == 2 + n_steps
    want_stream = _everything(tb, params, opt, losses)

    idx, xv, y, _ = batch(sizes, N, seed=340, xv_kind=kind)
    tb, params, eng, opt = _stream_start(rule, sizes, k, t, 1, seed=41)
    idx_d, xv_d, y_d = eng.to_device(idx, xv, y)
    logits, losses = torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda")
    for i in range(N):
        xi = None if xv_d is None else xv_d[i:i + 1]
        eng.forward(hyp, idx_d[i:i + 1], xi)                       # the sample's logit before its update
        logits[i] = eng.logit[0]
        eng.step(hyp, rule, idx_d[i:i + 1], xi, y_d[i:i + 1], inv_b=1.0, opt=opt)
        losses[i] = eng.loss_out[0]
    torch.cuda.synchronize()
    assert int(eng.error.item()) == 0 and opt.step == 2 + N
    want_online = dict(_everything(tb, params, opt, losses), logits=logits.cpu(), grad=eng.grad.cpu())
    return sizes, (idx_pool, xv_pool, y_pool), (idx_d, xv_d, y_d), want_stream, want_online


@SMALL_CASES
@SMALL_RULES
def test_small_stream_is_its_single_steps(rule, with_xv, side):
    k, t, B, n_steps = (SMALL[kk] for kk in ("k", "t", "units", "n_steps"))
    sizes, (idx_pool, xv_pool, y_pool), _, want, _ = _small_bce(rule, with_xv)
    assert bool((want["losses"] > 0).all())
    tb, params, eng, opt = _stream_start(rule, sizes, k, t, B, seed=41)
    losses = torch.full((n_steps,), -1.0, device="cuda")
    issue(side, lambda st: eng.stream(_hyper(rule), rule, idx_pool, xv_pool, y_pool, B, n_steps, opt, losses=losses, stream=st))
    assert int(eng.error.item()) == 0 and opt.step == 2 + n_steps and tb.step == (n_steps if LAYOUT[rule] == "moments" else 0)
    got = _everything(tb, params, opt, losses)
    for key in want:
        assert torch.equal(got[key], want[key]), f"{rule} stream: {key} differs from the single steps'"


@SMALL_CASES
@SMALL_RULES
def test_small_queued_online_run_is_its_single_steps(rule, with_xv, side):
    """The queued form in two calls of 1 and N - 1 samples: the second call's logits and losses start one sample in."""
    k, t, N = (SMALL[kk] for kk in ("k", "t", "N"))
    sizes, _, (idx_d, xv_d, y_d), _, want = _small_bce(rule, with_xv)
    assert bool((want["losses"] > 0).all())
    tb, params, eng, opt = _stream_start(rule, sizes, k, t, 1, seed=41)
    logits, losses = torch.full((N,), -7.0, device="cuda"), torch.full((N,), -7.0, device="cuda")
    hyp = _hyper(rule)

    def run(st):
        for o, n in ((0, 1), (1, N - 1)):
            eng.online_run(hyp, rule, idx_d[o:o + n], None if xv_d is None else xv_d[o:o + n], y_d[o:o + n], opt, logits=logits[o:],
                           losses=losses[o:], stream=st)
    with queued_online_form(b"afm_online_persistent"):
        issue(side, run)
    assert int(eng.error.item()) == 0 and opt.step == 2 + N and tb.step == (N if LAYOUT[rule] == "moments" else 0)
    got = dict(_everything(tb, params, opt, losses), logits=logits.cpu(), grad=eng.grad.cpu())
    for key in want:
        assert torch.equal(got[key], want[key]), f"{rule} queued online run: {key} differs from the single steps'"


def test_stream_of_zero_steps_launches_nothing():
    rule, F, k, t, B = "adam", 6, 8, 4, 64
    sizes = _sizes(F, 7)
    idx, xv, y, _ = batch(sizes, B, seed=5)
    tb, params, eng, opt = _stream_start(rule, sizes, k, t, B, seed=3)
    before = _everything(tb, params, opt, torch.zeros(1))
    idx_d, _, y_d = eng.to_device(idx, None, y)
    eng.stream(_hyper(rule), rule, idx_d, None, y_d, B, 0, opt)
    torch.cuda.synchronize()
    after = _everything(tb, params, opt, torch.zeros(1))
    assert all(torch.equal(before[key], after[key]) for key in before) and opt.step == 2 and tb.step == 0


def test_stream_flags_a_bad_index_anywhere_in_the_pool():
    rule, F, k, t, B, n_pool = "sgd", 6, 8, 4, 64, 3
    sizes = _sizes(F, 9)
    pool = [batch(sizes, B, seed=400 + j) for j in range(n_pool)]
    idx_pool = np.stack([p[0] for p in pool])
    idx_pool[2, 17, 4] = sizes[4] + 2                      # the last batch of the pool
    y_pool = torch.from_numpy(np.stack([p[2] for p in pool])).cuda()
    tb, params, eng, opt = _stream_start(rule, sizes, k, t, B, seed=3)
    eng.stream(_hyper(rule), rule, torch.from_numpy(idx_pool).cuda(), None, y_pool, B, 2, opt)
    eng.check_error_flag()                                 # steps 0 and 1 never saw it
    eng.stream(_hyper(rule), rule, torch.from_numpy(idx_pool).cuda(), None, y_pool, B, 3, opt)
    with pytest.raises(IndexError):
        eng.check_error_flag()


# ---- the class ----
def _afm_adam():
    from models.models_online_deep.afm_adam import AFMAdam
    return AFMAdam


@pytest.mark.parametrize("rule", ["adam", "adagrad", "signadam"])
def test_class_fused_steps_track_f64(rule):
    """AFMAdam(fused_optimizer=True) over 4 update_embedding calls (F = 14: 2 pair tiles): the loss and the attention parameters
    (with their moments) against float64 from the model's own state before each step.  (The tables of a fused step are
    fmx_afm_step's, bit for bit: test_step_opt_matches_step_and_f64.)"""
    AFMAdam = _afm_adam()
    sizes, k, t, B = _sizes(14, 14), 8, 8, 256
    n = HYP["lr"] if rule == "signadam" else 0.01         # signadam: the learning rate _check_rule restates
    torch.manual_seed(5)
    m = AFMAdam(sizes, embedding_size=k, attention_size=t, batch_size=B, n=n, update_rule=rule, fused_optimizer=True)
    assert m._attn_opt is None and m._attn_fused is not None and m._attn_fused.rule == rule
    F32 = lambda v: float(np.float32(v))
    b1, b2 = m._betas()
    h = dict(lr=F32(n), eps=F32(m._adam["eps"] if rule == "adam" else m._adagrad["eps"]), beta1=b1, beta2=b2)
    for s in range(1, 5):
        idx, xv, y, rows = batch(sizes, B, seed=80 + s, xv_kind="random")
        V, w, bias, params = _model_state(m)
        before = opt_state(m._attn_flat, m._attn_fused)
        np.testing.assert_array_equal(before[0], params.astype(np.float64))
        ref = afm_f64(V, w, bias, params, k, t, rows, xv, y, dz_abs=DZ_ABS)
        loss = float(m.update_embedding(idx, xv, y))
        torch.cuda.synchronize()
        assert m._attn_fused.step == s and (rule == "signadam" or m._table.step == s)
        assert_within_f64(loss, ref["loss"], float(np.mean(ref["floor_loss"])), f"step {s} loss")
        check_attention(rule, h, s, before, opt_state(m._attn_flat, m._attn_fused), ref, f"{rule} step {s}")


def _same_models(a, b):
    for key, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[key]), key
    oa, ob = a.optimizer_state_dict(), b.optimizer_state_dict()
    assert set(oa) == set(ob) == {"table", "attention"} and set(oa["attention"]) == {"m", "v", "step"}
    assert oa["attention"]["step"] == ob["attention"]["step"]
    assert torch.equal(oa["attention"]["m"], ob["attention"]["m"]) and torch.equal(oa["attention"]["v"], ob["attention"]["v"])
    assert (oa["table"] is None) == (ob["table"] is None)
    if oa["table"] is not None:
        for kk in ("mV", "vV", "mw", "vw", "bias_mv"):
            assert torch.equal(oa["table"][kk], ob["table"][kk]), kk
        assert oa["table"]["step"] == ob["table"]["step"]
    fa, fb = a.ftrl_state_dict(), b.ftrl_state_dict()
    if fa is not None:
        for kk in fa:
            assert torch.equal(fa[kk], fb[kk]), kk


@pytest.mark.parametrize("rule", ["adam", "ftrl"])
def test_class_fused_fit_equals_update_embedding_batch_by_batch(rule):
    """fit() on 300 samples at batch_size 128 (two full batches in one fmx_afm_stream call, a ragged batch of 44 in one
    fmx_afm_step_opt call, for 2 epochs) against the same model driven by update_embedding over the same slices."""
    AFMAdam = _afm_adam()
    sizes, k, t, N, B = [20, 300, 5, 64, 9], 8, 4, 300, 128
    idx, xv, y, _ = batch(sizes, N, seed=3, xv_kind="random")
    models = []
    for _ in range(2):
        torch.manual_seed(1)
        models.append(AFMAdam(sizes, embedding_size=k, attention_size=t, n_epochs=2, batch_size=B, n=0.01, update_rule=rule,
                              fused_optimizer=True))
    a, b = models
    train, valid = a.fit(idx, xv, y)
    assert len(train) == 2 and valid == []
    for _ in range(2):
        for o in range(0, N, B):
            b.update_embedding(idx[o:o + B], xv[o:o + B], y[o:o + B])
    _same_models(a, b)
    steps = 2 * 3
    assert a._attn_fused.step == steps and (rule != "adam" or a._table.step == steps)


@pytest.mark.parametrize("rule", ["adam", "adagrad", "signadam", "sgd", "ftrl"])
def test_class_fused_pickle_resumes_bit_for_bit(rule):
    AFMAdam = _afm_adam()
    sizes, k, t, B = [20, 300, 5, 64, 9], 8, 4, 128
    torch.manual_seed(2)
    m = AFMAdam(sizes, embedding_size=k, attention_size=t, batch_size=B, update_rule=rule, n=0.01, fused_optimizer=True)
    data = [batch(sizes, B, seed=60 + s, xv_kind="random") for s in range(3)]
    for idx, xv, y, _ in data[:2]:
        m.update_embedding(idx, xv, y)
    m3 = pickle.loads(pickle.dumps(m))
    assert m3.fused_optimizer and m3._attn_opt is None and m3._attn_fused.step == 2
    _same_models(m, m3)
    idx, xv, y, _ = data[2]
    l1, l3 = m.update_embedding(idx, xv, y), m3.update_embedding(idx, xv, y)
    assert torch.equal(l1, l3)
    _same_models(m, m3)
    assert m._attn_fused.step == 3


def test_class_default_constructor_keeps_the_torch_optimizer():
    AFMAdam = _afm_adam()
    m = AFMAdam([7, 30, 4, 12], embedding_size=6, attention_size=5)
    assert m.fused_optimizer is False and m._attn_fused is None and isinstance(m._attn_opt, torch.optim.Adam)
    m = AFMAdam([7, 30, 4, 12], embedding_size=6, attention_size=5, update_rule="adagrad")
    assert m._attn_fused is None and isinstance(m._attn_opt, torch.optim.Adagrad)
    m = AFMAdam([7, 30, 4, 12], embedding_size=6, attention_size=5, update_rule="signadam")
    assert m._attn_fused is None and m._attn_opt is None and m.optimizer_state_dict() is None


def test_class_fused_fit_raises_on_a_bad_index():
    AFMAdam = _afm_adam()
    sizes, k, t = [20, 300, 5, 64], 8, 4
    idx, xv, y, _ = batch(sizes, 300, seed=3, xv_kind="random")
    idx[200, 2] = sizes[2] + 1                             # in the second full batch of the stream call
    torch.manual_seed(1)
    m = AFMAdam(sizes, embedding_size=k, attention_size=t, n_epochs=1, batch_size=128, fused_optimizer=True)
    with pytest.raises(IndexError):
        m.fit(idx, xv, y)
