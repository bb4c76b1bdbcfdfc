"""fmx_afm_online_run on the GPU: the one-workgroup walk of a stream against N calls of fmx_afm_step_opt(B = 1, inv_b = 1), bit
for bit -- rows, bias words, params, m, v, every sample's logit and loss, the last gradient, the error word -- under every table
rule, with and without feature values, over one-tile, multi-tile and fall-back shapes; the queued form against the one-workgroup
form; a bad index in mid-stream; N = 0; run-to-run determinism; AFMAdam.run_online_experiment against a loop of predict() and
update_embedding(); and one float64 anchor of the first sample (the per-sample step it must equal is pinned to float64 by
test_afm_gpu / test_afm_stream_gpu)."""
import ctypes as C
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from afm_f64 import afm_f64  # noqa: E402
from helpers import assert_within_f64  # noqa: E402
from test_afm_gpu import batch, engine, make  # noqa: E402
from test_afm_pair_online_cpu import MOMENTS_IN_GLOBAL  # noqa: E402
from test_afm_stream_gpu import LAYOUT, _hyper, _same_models, attn_opt, check_attention, opt_state  # noqa: E402

pytestmark = pytest.mark.gpu

N_STREAM = 200


def _fmx():
    import fmx
    return fmx


def small_sizes(F, seed):
    """A few rows per field: consecutive samples share rows."""
    return [int(s) for s in np.random.default_rng(seed).integers(2, 5, size=F)]


def stream_data(sizes, N, seed, with_xv):
    idx, xv, y, rows = batch(sizes, N, seed=seed, xv_kind="random" if with_xv else "ones")
    if N >= 60:                       # one sample repeated back to back: every row is gathered right after it was stored
        idx[50:55] = idx[50]
        if xv is not None:
            xv[50:55] = xv[50]
    return idx, xv, y, rows


def start(rule, arule, sizes, k, t, seed=41):
    tb, params, st = make(sizes, k, t, layout=LAYOUT[rule], seed=seed)
    eng = engine(tb, params, t, 64)
    opt = attn_opt(arule, params.numel(), step=2)      # the two step counts differ: each must advance on its own
    return tb, params, eng, opt, st


def everything(tb, params, eng, opt, logits, losses):
    torch.cuda.synchronize()
    return dict(rows=tb.rows.cpu(), bias=tb.bias.cpu(), params=params.cpu(), m=opt.m.cpu(), v=opt.v.cpu(), logits=logits.cpu(),
                losses=losses.cpu(), grad=eng.grad.cpu(), error=eng.error.cpu())


def per_sample(rule, arule, sizes, k, t, data, seed=41):
    """N calls of fmx_afm_step_opt(B = 1, inv_b = 1), each behind a forward for the sample's logit."""
    idx, xv, y, _ = data
    tb, params, eng, opt, _ = start(rule, arule, sizes, k, t, seed)
    idx_d, xv_d, y_d = eng.to_device(idx, xv, y)
    N = idx.shape[0]
    logits, losses = torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda")
    hyp = _hyper(rule)
    for i in range(N):
        xi = None if xv_d is None else xv_d[i:i + 1]
        eng.forward(hyp, idx_d[i:i + 1], xi)
        logits[i] = eng.logit[0]
        eng.step(hyp, rule, idx_d[i:i + 1], xi, y_d[i:i + 1], inv_b=1.0, opt=opt)
        losses[i] = eng.loss_out[0]
    out = everything(tb, params, eng, opt, logits, losses)
    assert opt.step == 2 + N and tb.step == (N if LAYOUT[rule] == "moments" else 0)
    return out


def online(rule, arule, sizes, k, t, data, seed=41, splits=None):
    idx, xv, y, _ = data
    tb, params, eng, opt, _ = start(rule, arule, sizes, k, t, seed)
    idx_d, xv_d, y_d = eng.to_device(idx, xv, y)
    N = idx.shape[0]
    logits, losses = torch.full((N,), -7.0, device="cuda"), torch.full((N,), -7.0, device="cuda")
    hyp = _hyper(rule)
    o = 0
    for n in splits or (N,):
        eng.online_run(hyp, rule, idx_d[o:o + n], None if xv_d is None else xv_d[o:o + n], y_d[o:o + n], opt,
                       logits=logits[o:o + n], losses=losses[o:o + n])
        o += n
    assert o == N
    out = everything(tb, params, eng, opt, logits, losses)
    assert opt.step == 2 + N and tb.step == (N if LAYOUT[rule] == "moments" else 0)
    return out


def assert_same(got, want, what):
    for key in want:
        assert got[key].shape == want[key].shape, (what, key)
        assert torch.equal(got[key], want[key]), f"{what}: {key} differs ({int((got[key] != want[key]).sum())} words)"


RULES = [("sgd", "sgd", True), ("signadam", "signadam", False), ("ftrl", "signadam", True), ("adagrad", "adagrad", False),
         ("adam", "adam", True), ("sgd", "adam", False), ("signadam", "adagrad", True), ("ftrl", "sgd", False),
         ("adagrad", "signadam", True), ("adam", "adam", False)]
SHAPES = [pytest.param(39, 16, 16, id="F39-k16-t16-multi_tile"), pytest.param(3, 4, 4, id="F3-k4-t4")]


@pytest.mark.parametrize("F,k,t", SHAPES)
@pytest.mark.parametrize("rule,arule,with_xv", RULES)
def test_online_run_equals_per_sample_steps_bit_for_bit(rule, arule, with_xv, F, k, t):
    sizes = small_sizes(F, F + 1)
    data = stream_data(sizes, N_STREAM, seed=500 + F, with_xv=with_xv)
    want = per_sample(rule, arule, sizes, k, t, data)
    assert int(want["error"]) == 0 and bool((want["losses"] >= 0).all()) and bool((want["losses"] > 0).any())
    assert_same(online(rule, arule, sizes, k, t, data), want, f"{rule}/{arule} one call")
    assert_same(online(rule, arule, sizes, k, t, data, splits=(1, 120, 79)), want, f"{rule}/{arule} three calls")


@pytest.mark.parametrize("F,k,t,rule,arule", [pytest.param(64, 64, 64, "adam", "adam", id="F64-k64-t64-largest-queued_form"),
                                              pytest.param(64, 33, 7, "ftrl", "signadam", id="F64-k33-t7-kp64-two_rows_a_thread"),
                                              pytest.param(40, 20, 64, "adagrad", "adagrad", id="F40-k20-t64-kp32"),
                                              pytest.param(12, 10, 4, "sgd", "sgd", id="F12-k10-t4-two_tiles"),
                                              pytest.param(2, 1, 1, "signadam", "signadam", id="F2-k1-t1-one_pair")])
def test_online_run_other_shapes(F, k, t, rule, arule):
    """The largest shape leaves no room in LDS for two tile buffers and takes the queued per-sample launches; the others pin
    kp = 64 (two rows per thread), kp = 32, kp != k padding and a single pair."""
    sizes = small_sizes(F, F + 2)
    data = stream_data(sizes, N_STREAM, seed=600 + F, with_xv=True)
    want = per_sample(rule, arule, sizes, k, t, data)
    assert int(want["error"]) == 0
    assert_same(online(rule, arule, sizes, k, t, data), want, f"F={F} k={k} t={t}")


def test_moments_in_global_memory():
    """At this shape the attention moments would cost a tile buffer, so k_afm_online reads and writes them in global memory through
    the pointer that elsewhere names LDS (the walk's shared mm / vv path; the pair kernel's test of the same name runs it for
    pairs).  The witness that the shape takes that path is fmx_afm_pair_online_form: both entry points take the decision from
    afm_online_buffers, each under its own option, and both options are on here."""
    F, k, t = MOMENTS_IN_GLOBAL
    sizes = small_sizes(F, F + 4)
    _, _, eng, _, _ = start("adam", "adam", sizes, k, t)
    nb, mom_lds = eng.pair_online_form("adam")
    assert nb > 0 and not mom_lds, f"{nb} tile buffers, moments in LDS {mom_lds}: not the form this test is about"
    data = stream_data(sizes, N_STREAM, seed=700 + F, with_xv=True)
    want = per_sample("adam", "adam", sizes, k, t, data)
    assert int(want["error"]) == 0
    got = online("adam", "adam", sizes, k, t, data)
    assert_same(got, want, "moments in global memory")
    assert bool((got["m"] != 0).any()) and bool((got["v"] != 0).any())


@pytest.mark.parametrize("rule,arule", [("adam", "adam"), ("ftrl", "signadam")])
def test_queued_form_and_one_workgroup_form_give_the_same_bits(rule, arule):
    lib = _fmx()._lib.load()
    F, k, t = 39, 16, 16
    sizes = small_sizes(F, 5)
    data = stream_data(sizes, N_STREAM, seed=77, with_xv=True)
    one = online(rule, arule, sizes, k, t, data)
    try:
        assert lib.fmx_set_option(b"afm_online_persistent", 0) == 1
        queued = online(rule, arule, sizes, k, t, data)
    finally:
        lib.fmx_set_option(b"afm_online_persistent", 1)
    assert_same(queued, one, f"{rule}: queued against one workgroup")
    assert_same(online(rule, arule, sizes, k, t, data), one, f"{rule}: a second run from the same start")


@pytest.mark.parametrize("rule,arule", [("adam", "adam"), ("sgd", "sgd")])
def test_a_bad_index_in_mid_stream_is_an_absent_row(rule, arule):
    F, k, t = 14, 8, 8
    sizes = small_sizes(F, 9)
    data = stream_data(sizes, N_STREAM, seed=88, with_xv=True)
    data[0][N_STREAM // 2, 3] = sizes[3] + 2
    data[0][N_STREAM // 2 + 7, 0] = -1
    want = per_sample(rule, arule, sizes, k, t, data)
    assert int(want["error"]) == 1
    got = online(rule, arule, sizes, k, t, data)
    assert int(got["error"]) == 1
    assert_same(got, want, f"{rule}: bad index")
    clean = stream_data(sizes, N_STREAM, seed=88, with_xv=True)
    assert not torch.equal(online(rule, arule, sizes, k, t, clean)["rows"], got["rows"])


def test_an_empty_stream_changes_nothing():
    fmx = _fmx()
    rule, F, k, t = "adam", 6, 8, 4
    sizes = small_sizes(F, 7)
    idx, xv, y, _ = stream_data(sizes, 8, seed=5, with_xv=False)
    tb, params, eng, opt, _ = start(rule, "adam", sizes, k, t, seed=3)
    idx_d, _, y_d = eng.to_device(idx, None, y)
    z = torch.zeros(8, device="cuda")
    before = everything(tb, params, eng, opt, z, z)
    hyp = _hyper(rule)
    rc = eng.lib.fmx_afm_online_run(tb.c_struct(), hyp.ref(), fmx._lib.RULES[rule], C.byref(eng.c_afm), idx_d.data_ptr(), None,
                                    y_d.data_ptr(), 0, eng.workspace.data_ptr(), eng.workspace.numel() * 4, eng.grad.data_ptr(),
                                    opt.ref(), None, None, eng.error.data_ptr(), None)
    assert rc == 0
    assert_same(everything(tb, params, eng, opt, z, z), before, "N = 0")


def test_first_sample_against_float64():
    """The logit, the loss and the attention parameters' step of a one-sample stream against afm_f64 with its own floors."""
    rule, F, k, t = "sgd", 12, 10, 4
    sizes = small_sizes(F, 3)
    idx, xv, y, rows = stream_data(sizes, 1, seed=9, with_xv=True)
    tb, params, eng, opt, st = start(rule, "sgd", sizes, k, t, seed=13)
    idx_d, xv_d, y_d = eng.to_device(idx, xv, y)
    logits, losses = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
    before = opt_state(params, opt)
    eng.online_run(_hyper(rule), rule, idx_d, xv_d, y_d, opt, logits=logits, losses=losses)
    torch.cuda.synchronize()
    ref = afm_f64(st["V"], st["w"], st["bias"], st["params"], k, t, rows, xv, y)
    assert_within_f64(logits.cpu().numpy(), ref["logit"], ref["floor_logit"], "logit")
    assert_within_f64(losses.cpu().numpy(), ref["loss_b"], ref["floor_loss"], "loss")
    assert_within_f64(eng.grad.cpu().numpy(), ref["dparams"], ref["fl_dparams"], "attention gradient")
    check_attention("sgd", None, 1, before, opt_state(params, opt), ref, "first sample")
    assert (params.cpu().numpy() != st["params"]).any()


# ---- the class ----
def _afm_adam():
    from models.models_online_deep.afm_adam import AFMAdam
    return AFMAdam


def _loop(m, idx, xv, y):
    """predict, then update_embedding, one sample at a time -> the predictions"""
    pred = np.zeros(len(y), dtype=bool)
    for i in range(len(y)):
        pred[i] = bool(np.asarray(m.predict(idx[i:i + 1], xv[i:i + 1])).reshape(-1)[0])
        m.update_embedding(idx[i:i + 1], xv[i:i + 1], y[i:i + 1])
    return pred


def _cm(pred, y):
    pos, hit = y == 1, pred == (y == 1)
    return {"tp": int((pos & hit).sum()), "fp": int((~pos & ~hit).sum()), "tn": int((~pos & hit).sum()), "fn": int((pos & ~hit).sum())}


@pytest.mark.parametrize("rule", ["adam", "signadam", "ftrl"])
def test_class_online_experiment_equals_the_loop_and_survives_pickling(rule):
    AFMAdam = _afm_adam()
    sizes, k, t, N = small_sizes(12, 21), 8, 4, 150
    idx, xv, y, _ = stream_data(sizes, 2 * N, seed=31, with_xv=True)
    models = []
    for _ in range(2):
        torch.manual_seed(1)
        models.append(AFMAdam(sizes, embedding_size=k, attention_size=t, batch_size=64, n=0.01, update_rule=rule, fused_optimizer=True))
    a, b = models
    out = a.run_online_experiment(idx[:N], xv[:N], y[:N])
    pred = _loop(b, idx[:N], xv[:N], y[:N])
    _same_models(a, b)
    assert a._attn_fused.step == N and (rule != "adam" or a._table.step == N)
    seconds, acc, roc, cm = out
    assert seconds >= 0 and cm == _cm(pred, y[:N]) and sum(cm.values()) == N
    assert abs(acc - (cm["tp"] + cm["tn"]) / N * 100) < 1e-9 and set(roc) == {"tpr", "fpr"}
    a2, b2 = pickle.loads(pickle.dumps(a)), pickle.loads(pickle.dumps(b))
    _same_models(a2, b2)
    out_a, out_b = a2.run_online_experiment(idx[N:], xv[N:], y[N:]), b2.run_online_experiment(idx[N:], xv[N:], y[N:])
    assert out_a[1:] == out_b[1:]
    _same_models(a2, b2)
    assert out_a[3] == _cm(_loop(b, idx[N:], xv[N:], y[N:]), y[N:])
    _same_models(a2, b)
    assert a2._attn_fused.step == 2 * N


def test_class_online_experiment_without_the_fused_optimizer():
    AFMAdam = _afm_adam()
    sizes, k, t, N = small_sizes(6, 4), 8, 4, 40
    idx, xv, y, _ = stream_data(sizes, N, seed=2, with_xv=True)
    torch.manual_seed(1)
    m = AFMAdam(sizes, embedding_size=k, attention_size=t, update_rule="adam")
    before = m.state_dict()
    seconds, acc, roc, cm = m.run_online_experiment(idx, xv, y)
    assert isinstance(seconds, float) and 0.0 <= acc <= 100.0 and set(roc) == {"tpr", "fpr"}
    assert set(cm) == {"tp", "fp", "tn", "fn"} and sum(cm.values()) == N
    assert not torch.equal(before["attention_linear.weight"], m.state_dict()["attention_linear.weight"])


def test_class_online_experiment_raises_on_a_bad_index():
    AFMAdam = _afm_adam()
    sizes, k, t, N = small_sizes(6, 4), 8, 4, 40
    idx, xv, y, _ = stream_data(sizes, N, seed=2, with_xv=True)
    idx[17, 2] = sizes[2] + 1
    torch.manual_seed(1)
    m = AFMAdam(sizes, embedding_size=k, attention_size=t, fused_optimizer=True)
    with pytest.raises(IndexError):
        m.run_online_experiment(idx, xv, y)
