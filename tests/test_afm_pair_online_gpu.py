"""k_afm_pair_online on the GPU: fmx_afm_pair_online_run's one-workgroup form against the loop of fmx_afm_forward +
fmx_afm_pair_step_opt(B_pairs = 1, inv_b = 1) issued from outside, bit for bit -- rows, bias words, params, m, v, all 2 N logits, the
N losses, the last gradient, the error word, compared as int32 words.  Every stream is 200 pairs over vocabularies of 2 - 4 rows per
field (consecutive pairs share rows) with five consecutive identical pairs (rows gathered right after being stored).  Every test
first asserts, through fmx_afm_pair_online_form, which form it ran."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_afm_online_gpu import RULES, small_sizes, start  # noqa: E402
from test_afm_pair_gpu import _assert_same, _class_data, _models  # noqa: E402
from test_afm_pair_online_cpu import MOMENTS_IN_GLOBAL  # noqa: E402
from test_afm_stream_gpu import LAYOUT, _hyper, _same_models  # noqa: E402

pytestmark = pytest.mark.gpu

N_PAIRS = 200
OPTION = b"afm_pair_online_persistent"


def _lib():
    import fmx
    return fmx._lib.load()


def pair_stream(sizes, N, seed, with_xv, kind="mixed"):
    """N pairs in the interleaved layout -> (idx int32 [2 N, F], xv [2 N, F] or None).  mixed: every field of the negative keeps the
    positive's row with probability 1/2 (runs of two and runs of one in every pair), the two sides' values drawn apart.
    Pairs 50 .. 54 are one pair repeated."""
    rng = np.random.default_rng(seed)
    F = len(sizes)
    pos = np.stack([rng.integers(0, s, size=N) for s in sizes], axis=1).astype(np.int32)
    other = np.stack([(pos[:, f] + 1 + rng.integers(0, sizes[f] - 1, size=N)) % sizes[f] for f in range(F)], axis=1).astype(np.int32)
    xp = rng.uniform(0.2, 1.8, size=pos.shape).astype(np.float32)
    xn = rng.uniform(0.2, 1.8, size=pos.shape).astype(np.float32)
    if kind == "mixed":
        neg = np.where(rng.uniform(size=pos.shape) < 0.5, pos, other)
    elif kind == "last_field":                 # the negative differs in the last field only; the values kept
        neg, xn = pos.copy(), xp.copy()
        neg[:, -1] = other[:, -1]
    elif kind == "every_field":                # no shared row
        neg = other
    elif kind == "identical":                  # the same rows and values on both sides
        neg, xn = pos.copy(), xp.copy()
    elif kind == "same_index_other_value":     # one run of two occurrences in every field, the values apart
        neg = pos.copy()
    else:
        raise ValueError(kind)
    idx = np.empty((2 * N, F), np.int32)
    idx[0::2], idx[1::2] = pos, neg
    xv = np.empty((2 * N, F), np.float32)
    xv[0::2], xv[1::2] = xp, xn
    if N >= 60:
        idx[100:110], xv[100:110] = np.tile(idx[100:102], (5, 1)), np.tile(xv[100:102], (5, 1))
    return idx, (xv if with_xv else None)


def _everything(tb, params, eng, opt, logits, losses):
    torch.cuda.synchronize()
    return dict(rows=tb.rows.cpu(), bias=tb.bias.cpu(), params=params.cpu(), m=opt.m.cpu(), v=opt.v.cpu(), logits=logits.cpu(),
                losses=losses.cpu(), grad=eng.grad.cpu(), error=eng.error.cpu())


def pair_loop(rule, arule, sizes, k, t, idx, xv, margin, seed=41):
    """The yardstick: for every pair a forward (its two logits before the update), then fmx_afm_pair_step_opt(B_pairs = 1,
    inv_b = 1), from outside."""
    tb, params, eng, opt, _ = start(rule, arule, sizes, k, t, seed)
    idx_d, xv_d, _ = eng.to_device(idx, xv)
    N = idx.shape[0] // 2
    logits, losses = torch.zeros(2 * N, device="cuda"), torch.zeros(N, device="cuda")
    hyp = _hyper(rule)
    for i in range(N):
        xi = None if xv_d is None else xv_d[2 * i:2 * i + 2]
        eng.forward(hyp, idx_d[2 * i:2 * i + 2], xi)
        logits[2 * i:2 * i + 2] = eng.logit[:2]
        eng.pair_step(hyp, rule, idx_d[2 * i:2 * i + 2], xi, margin=margin, inv_b=1.0, opt=opt)
        losses[i] = eng.loss_out[0]
    out = _everything(tb, params, eng, opt, logits, losses)
    assert opt.step == 2 + N and tb.step == (N if LAYOUT[rule] == "moments" else 0)
    return out


def pair_online(rule, arule, sizes, k, t, idx, xv, margin, seed=41, splits=None, want_form=True, want_mom=None):
    """fmx_afm_pair_online_run from the same start, as one call or as the calls `splits`; asserts the form it ran first."""
    tb, params, eng, opt, _ = start(rule, arule, sizes, k, t, seed)
    nb, mom = eng.pair_online_form(arule)
    assert (nb > 0) == want_form, f"F={len(sizes)} k={k} t={t}: {nb} tile buffers -- not the form this test is about"
    assert want_mom is None or mom == want_mom
    idx_d, xv_d, _ = eng.to_device(idx, xv)
    N = idx.shape[0] // 2
    logits, losses = torch.full((2 * N,), -7.0, device="cuda"), torch.full((N,), -7.0, device="cuda")
    hyp = _hyper(rule)
    o = 0
    for n in splits or (N,):
        eng.pair_online_run(hyp, rule, idx_d[2 * o:2 * (o + n)], None if xv_d is None else xv_d[2 * o:2 * (o + n)], opt, margin=margin,
                            logits=logits[2 * o:], losses=losses[o:])
        o += n
    assert o == N
    out = _everything(tb, params, eng, opt, logits, losses)
    assert opt.step == 2 + N and tb.step == (N if LAYOUT[rule] == "moments" else 0)
    return out


@functools.lru_cache(maxsize=None)
def _case(rule, arule, F, k, t, with_xv, margin, kind="mixed", n=N_PAIRS, bad=False):
    """(sizes, idx, xv, the yardstick's results) of one stream: computed once, shared by the tests that need it."""
    sizes = small_sizes(F, F + 3)
    idx, xv = pair_stream(sizes, n, seed=700 + F, with_xv=with_xv, kind=kind)
    if bad:
        mid = n // 2
        idx[2 * mid, 3] = sizes[3] + 2                   # in the positive only
        idx[2 * (mid + 7) + 1, 0] = -1                   # in the negative only
        idx[2 * (mid + 11), 5] = idx[2 * (mid + 11) + 1, 5] = sizes[5]   # in both, at the same field
    return sizes, idx, xv, pair_loop(rule, arule, sizes, k, t, idx, xv, margin)


# ---- 1. every pairing of the rules ----
SHAPES = [pytest.param(39, 16, 16, id="F39-k16-t16-two_rounds_of_8"), pytest.param(3, 4, 4, id="F3-k4-t4")]


@pytest.mark.parametrize("F,k,t", SHAPES)
@pytest.mark.parametrize("n,pairing", list(enumerate(RULES)), ids=[f"{r}-{a}-{'xv' if x else 'ones'}" for r, a, x in RULES])
def test_pair_online_run_equals_the_loop_bit_for_bit(n, pairing, F, k, t):
    rule, arule, with_xv = pairing
    margin = 0.1 if n % 2 == 0 else 0.0
    sizes, idx, xv, want = _case(rule, arule, F, k, t, with_xv, margin)
    assert int(want["error"]) == 0 and bool(torch.isfinite(want["losses"]).all()) and bool((want["losses"] != 0).any())
    _assert_same(pair_online(rule, arule, sizes, k, t, idx, xv, margin), want, f"{rule}/{arule} one call")
    _assert_same(pair_online(rule, arule, sizes, k, t, idx, xv, margin, splits=(1, 120, 79)), want, f"{rule}/{arule} three calls")


# ---- 2. other shapes ----
@pytest.mark.parametrize("F,k,t,rule,arule,n", [
    pytest.param(64, 33, 7, "ftrl", "signadam", N_PAIRS, id="F64-k33-t7-kp64-four_slices_a_thread"),
    pytest.param(40, 20, 64, "adagrad", "adagrad", N_PAIRS, id="F40-k20-t64-kp32"),
    pytest.param(12, 10, 4, "sgd", "sgd", N_PAIRS, id="F12-k10-t4-two_tiles"),
    pytest.param(2, 1, 1, "signadam", "signadam", N_PAIRS, id="F2-k1-t1-one_field_pair")])
def test_pair_online_run_other_shapes(F, k, t, rule, arule, n):
    sizes, idx, xv, want = _case(rule, arule, F, k, t, True, 0.1, n=n)
    assert int(want["error"]) == 0
    _assert_same(pair_online(rule, arule, sizes, k, t, idx, xv, 0.1), want, f"F={F} k={k} t={t}")


def test_the_largest_shape_takes_the_queued_form():
    F, k, t, rule, arule = 64, 64, 64, "adam", "adam"
    # (60 pairs, the repeated block kept: at this shape the loop and the queued form run 32 tiles of 64 x 64 on one wave, 15 ms a pair)
    sizes, idx, xv, want = _case(rule, arule, F, k, t, True, 0.1, n=60)
    assert int(want["error"]) == 0
    _assert_same(pair_online(rule, arule, sizes, k, t, idx, xv, 0.1, want_form=False), want, "F=64 k=64 t=64: the queued form")


# ---- 3. the run logic ----
@pytest.mark.parametrize("rule,arule", [("adam", "adam"), ("ftrl", "signadam")])
def test_runs_of_two_and_runs_of_one(rule, arule):
    F, k, t, margin = 12, 10, 4, 0.1
    sizes = small_sizes(F, F + 3)
    parts = [pair_stream(sizes, 50, seed=800 + j, with_xv=True, kind=kind)
             for j, kind in enumerate(("last_field", "every_field", "identical", "same_index_other_value"))]
    idx, xv = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    idx[100:110], xv[100:110] = np.tile(idx[100:102], (5, 1)), np.tile(xv[100:102], (5, 1))
    assert (idx[0:100:2, :-1] == idx[1:100:2, :-1]).all() and (idx[0:100:2, -1] != idx[1:100:2, -1]).all()
    assert (idx[110:200:2] != idx[111:200:2]).all()
    assert (idx[200:300:2] == idx[201:300:2]).all() and (xv[200:300:2] == xv[201:300:2]).all()
    assert (idx[300::2] == idx[301::2]).all() and (xv[300::2] != xv[301::2]).all()
    want = pair_loop(rule, arule, sizes, k, t, idx, xv, margin)
    assert int(want["error"]) == 0
    _assert_same(pair_online(rule, arule, sizes, k, t, idx, xv, margin), want, f"{rule}: the four kinds of pairs")


@pytest.mark.parametrize("rule,arule", [("adam", "adam"), ("ftrl", "signadam")])
def test_identical_rows_leave_every_table_word_as_it_was(rule, arule):
    """A stream of pairs whose two sides are one row set with one set of values: every field is one run of two occurrences whose
    terms cancel exactly -- (0 + c) + (-c) = +0 -- so the tables take zero gradients.  adam (moments zero at the start: the step is
    lr 0 / (sqrt(0) + eps) = 0): every word of the table keeps the bits it started with.  ftrl: every (z, n) word keeps the bits it
    started with; the weights are re-derived from them by the kernel's closed form on a row's first update (the table was loaded
    with weights rounded by another route), so the words that must not move are those the first pass over the stream left -- a
    second pass over it changes none.  Also the loop's bits."""
    F, k, t, margin = 12, 10, 4, 0.0
    sizes = small_sizes(F, F + 3)
    idx, xv = pair_stream(sizes, N_PAIRS, seed=900, with_xv=True, kind="identical")
    tb, params, eng, opt, _ = start(rule, arule, sizes, k, t, 41)
    rows_before = tb.rows.cpu().view(torch.int32)
    got = pair_online(rule, arule, sizes, k, t, idx, xv, margin)
    rows = got["rows"].view(torch.int32)
    if rule == "ftrl":
        kp, zo = tb.kp, tb.z_offset
        zn = lambda r: torch.cat([r[:, kp + 1:kp + 3], r[:, zo:zo + 2 * kp]], dim=1)     # (z, n) of w and of V
        assert torch.equal(zn(rows), zn(rows_before)), "a (z, n) word moved"
        twice = pair_online(rule, arule, sizes, k, t, np.concatenate([idx, idx]), np.concatenate([xv, xv]), margin)
        assert torch.equal(twice["rows"].view(torch.int32), rows), "a table word moved in the second pass"
    else:
        assert torch.equal(rows, rows_before), "a table word moved"
    assert bool((got["logits"][0::2] == got["logits"][1::2]).all())
    _assert_same(got, pair_loop(rule, arule, sizes, k, t, idx, xv, margin), f"{rule}: identical rows")


# ---- 4. bad indices ----
@pytest.mark.parametrize("rule,arule", [("adam", "adam"), ("sgd", "sgd")])
def test_bad_indices_in_mid_stream_are_absent_rows(rule, arule):
    F, k, t, margin = 14, 8, 8, 0.1
    sizes, idx, xv, want = _case(rule, arule, F, k, t, True, margin, bad=True)
    assert int(want["error"]) == 1
    got = pair_online(rule, arule, sizes, k, t, idx, xv, margin)
    assert int(got["error"]) == 1
    _assert_same(got, want, f"{rule}: bad indices")
    _, idx_c, xv_c, _ = _case(rule, arule, F, k, t, True, margin)
    clean = pair_online(rule, arule, sizes, k, t, idx_c, xv_c, margin)
    assert int(clean["error"]) == 0 and not torch.equal(clean["rows"], got["rows"])


# ---- 5. the two forms ----
@pytest.mark.parametrize("rule,arule", [("adam", "adam"), ("ftrl", "signadam")])
def test_queued_form_and_one_workgroup_form_give_the_same_bits(rule, arule):
    lib = _lib()
    F, k, t, margin = 39, 16, 16, 0.1
    sizes, idx, xv, want = _case(rule, arule, F, k, t, True, margin)
    one = pair_online(rule, arule, sizes, k, t, idx, xv, margin)
    try:
        assert lib.fmx_set_option(OPTION, 0) == 1
        queued = pair_online(rule, arule, sizes, k, t, idx, xv, margin, want_form=False)
    finally:
        lib.fmx_set_option(OPTION, 1)
    _assert_same(queued, one, f"{rule}: queued against one workgroup")
    _assert_same(pair_online(rule, arule, sizes, k, t, idx, xv, margin), one, f"{rule}: a second run from the same start")
    _assert_same(one, want, f"{rule}: against the loop")


def test_zero_pairs_touch_nothing():
    import ctypes as C
    import fmx
    rule, arule, F, k, t = "adam", "adam", 6, 8, 4
    sizes = small_sizes(F, 7)
    tb, params, eng, opt, _ = start(rule, arule, sizes, k, t, seed=3)
    assert eng.pair_online_form(arule)[0] > 0
    z = torch.zeros(2, device="cuda")
    before = _everything(tb, params, eng, opt, z, z)
    idx_d = torch.zeros((2, F), dtype=torch.int32, device="cuda")       # (an empty tensor has no address to pass)
    hyp = _hyper(rule)
    rc = eng.lib.fmx_afm_pair_online_run(tb.c_struct(), hyp.ref(), fmx._lib.RULES[rule], C.byref(eng.c_afm), idx_d.data_ptr(), None, 0,
                                         0.0, eng.workspace.data_ptr(), eng.workspace.numel() * 4, eng.grad.data_ptr(), opt.ref(), None,
                                         None, eng.error.data_ptr(), None)
    assert rc == 0
    _assert_same(_everything(tb, params, eng, opt, z, z), before, "N_pairs = 0")


# ---- 6. the moments in global memory; the class ----
def test_moments_in_global_memory():
    """At this shape the attention moments would cost a tile buffer, so the kernel reads and writes them in global memory through
    the pointer that elsewhere names LDS."""
    F, k, t = MOMENTS_IN_GLOBAL
    sizes, idx, xv, want = _case("adam", "adam", F, k, t, True, 0.1)
    assert int(want["error"]) == 0
    got = pair_online("adam", "adam", sizes, k, t, idx, xv, 0.1, want_mom=False)
    _assert_same(got, want, "moments in global memory")
    assert bool((got["m"] != 0).any()) and bool((got["v"] != 0).any())


@pytest.mark.parametrize("rule", ["adam", "ftrl"])
def test_class_pair_experiment_on_the_one_workgroup_form_equals_the_host_loop(rule):
    F, k, t, N, margin = 39, 16, 16, 60, 0.1
    sizes = small_sizes(F, F + 3)
    a, b = _models(2, sizes, k, t, rule)
    assert a._engine.pair_online_form(a._attn_fused.rule if hasattr(a._attn_fused, "rule") else "adam")[0] > 0
    pos, xv, fields, neg = _class_data(sizes, N, seed=23)
    ra = a.run_pair_experiment(pos, xv, fields, negatives=neg, margin=margin, attention=True)
    pred = []
    for i in range(N):
        b.fit_pairs(pos[i:i + 1], xv[i:i + 1], fields, negatives=neg[i:i + 1], margin=margin, attention=True)
        pred.append(bool(b._engine.logit[0] > b._engine.logit[1]))
    _same_models(a, b)
    assert a._attn_fused.step == N
    pred = np.array(pred)
    assert ra[3] == {"correct": int(pred.sum()), "wrong": int(N - pred.sum())}
