"""fmx_afm_pair_* on the GPU: the pair forward's logits against fmx_afm_forward bit for bit and its loss / dlogit against the
float64 restatement in tests/afm_pair_f64.py; one pair step against float64 across the pair-tile geometries and under every
update rule (the bias word keeps its bits: its gradient is exactly +0); exact cancellation when a pair's rows coincide; an
index outside its field; determinism; the stream against its steps and the online run against single-pair steps, bit for bit;
AFMAdam.fit_pairs / run_pair_experiment(attention=True); and sixty steps that bring the pair loss down."""
import ctypes as C
import functools
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from afm_pair_f64 import U32, afm_pair_f64, live_params  # noqa: E402
from helpers import assert_within_f64  # noqa: E402
from test_adaptive_rules_cpu import rule_apply  # noqa: E402
from test_afm_gpu import (HYP, _attn_state, _check_rule, _model_state, _sizes, _touched, assert_exercised, engine,  # noqa: E402
                          make)
from test_afm_stream_gpu import (ATTN_RULE, LAYOUT, SMALL, SMALL_CASES, SMALL_RULES, _hyper, _same_models, _stream_start,  # noqa: E402
                                 check_attention, issue, opt_state, queued_online_form)

pytestmark = pytest.mark.gpu

MARGINS = [0.0, 0.1]


def _fmx():
    import fmx
    return fmx


def pair_batch(sizes, Bp, seed=1, xv_kind="ones", hot=False, share_item=False):
    """Bp pairs in the interleaved layout -> (idx int32 [2 Bp, F], xv [2 Bp, F] or None, global rows [2 Bp, F]).  The item is
    the last field; a pair's negative is its positive with another index of that field (the values kept); every third pair takes
    pair 0's whole context (share_item: and its positive item), so every context field has runs of two and longer."""
    rng = np.random.default_rng(seed)
    F = len(sizes)
    pos = np.stack([rng.integers(0, s, size=Bp) for s in sizes], axis=1).astype(np.int32)
    if hot:
        pos[:, 0] = rng.integers(0, 2, size=Bp)          # two rows of field 0 take every occurrence: runs cross 64-entry tiles
    pos[::3, :F - 1] = pos[0, :F - 1]
    if share_item:
        pos[::3, F - 1] = pos[0, F - 1]
    neg = pos.copy()
    neg[:, F - 1] = (pos[:, F - 1] + 1 + rng.integers(0, sizes[-1] - 1, size=Bp)) % sizes[-1]
    idx = np.empty((2 * Bp, F), np.int32)
    idx[0::2], idx[1::2] = pos, neg
    xv = None
    if xv_kind != "ones":
        xp = rng.uniform(0.2, 1.8, size=pos.shape).astype(np.float32)
        if xv_kind == "zeros":
            xp[:, ::3] = 0.0
        xv = np.repeat(xp, 2, axis=0)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return idx, xv, idx.astype(np.int64) + offs[:-1][None, :]


def _live(params, st, k, t, rows, xv, valid=None):
    x = np.ones(rows.shape) if xv is None else xv
    fixed = live_params(st["params"], st["V"], k, t, rows, x if valid is None else x * valid)
    params.copy_(torch.from_numpy(fixed))
    st["params"] = fixed


def assert_precheck(ref, F, what):
    """What every float64-tolerance test asserts of its own data: no pair near the loss's flat end, no dead attention unit,
    every pair tile carrying gradient."""
    assert (np.abs(ref["g"]) >= 0.05).all(), f"{what}: min |g| {np.abs(ref['g']).min():.3g}"
    assert_exercised(ref, F, what)


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


# ---- 1. the forward ----
FORWARD_CASES = [(2, 4, 1, 1, "ones"), (3, 10, 4, 33, "random"), (39, 16, 16, 257, "zeros"), (3, 4, 4, 1025, "ones")]


@pytest.mark.parametrize("margin", MARGINS)
@pytest.mark.parametrize("F,k,t,Bp,xv_kind", FORWARD_CASES)
def test_pair_forward(F, k, t, Bp, xv_kind, margin):
    fmx = _fmx()
    sizes = _sizes(F, F + Bp)
    tb, params, st = make(sizes, k, t, seed=F + k)
    idx, xv, rows = pair_batch(sizes, Bp, seed=Bp, xv_kind=xv_kind)
    _live(params, st, k, t, rows, xv)
    eng = engine(tb, params, t, 2 * Bp)
    idx_d, xv_d, _ = eng.to_device(idx, xv)
    hyp = fmx.Hyper(**HYP)
    eng.forward(hyp, idx_d, xv_d)
    plain = eng.logit[:2 * Bp].cpu().numpy().copy()
    eng.logit.fill_(-7.0)
    dz = torch.full((2 * Bp,), -7.0, device="cuda")
    assert eng.pair_forward(hyp, idx_d, xv_d, margin=margin, dz=dz) == Bp
    torch.cuda.synchronize()
    logit, loss, dz = eng.logit[:2 * Bp].cpu().numpy(), eng.loss_b[:2 * Bp].cpu().numpy(), dz.cpu().numpy()
    assert int(eng.error.item()) == 0
    np.testing.assert_array_equal(bits(logit), bits(plain), err_msg="the pair forward's logits are not fmx_afm_forward's")
    np.testing.assert_array_equal(bits(dz[1::2]), bits(dz[0::2]) ^ np.uint32(0x80000000), err_msg="dz[2i+1] is not dz[2i] negated")
    assert not bits(loss[1::2]).any(), "loss[2i+1] is not +0"
    ref = afm_pair_f64(st["V"], st["w"], st["bias"], st["params"], k, t, rows, xv, margin=margin)
    assert_precheck(ref, F, f"forward F={F} Bp={Bp}")
    assert_within_f64(logit, ref["logit"], ref["floor_logit"], "logit")
    assert_within_f64(loss, ref["loss_b"], ref["floor_loss"], "pair loss")
    assert_within_f64(dz, ref["dz"], ref["floor_dz"], "dlogit")


def test_pair_forward_stays_finite_at_large_differences():
    fmx = _fmx()
    F, k, t, Bp = 6, 8, 4, 64
    sizes = _sizes(F, 3)
    tb, params, st = make(sizes, k, t, seed=2, scale=4.0)
    idx, xv, rows = pair_batch(sizes, Bp, seed=5, xv_kind="random")
    eng = engine(tb, params, t, 2 * Bp)
    idx_d, xv_d, _ = eng.to_device(idx, xv)
    for margin in MARGINS:
        dz = torch.zeros(2 * Bp, device="cuda")
        eng.pair_forward(fmx.Hyper(**HYP), idx_d, xv_d, margin=margin, dz=dz)
        logit = eng.logit[:2 * Bp].cpu().numpy()
        d = logit[0::2] - logit[1::2]
        assert (np.abs(d) > 30).any() and d.max() > 30 and d.min() < -30, (d.min(), d.max())
        assert np.isfinite(logit).all() and np.isfinite(eng.loss_b[:2 * Bp].cpu().numpy()).all() and np.isfinite(dz.cpu().numpy()).all()


# ---- 2. / 3. / 5. one step against float64 ----
def _pair_step_and_check(rule, sizes, k, t, Bp, xv_kind="random", margin=0.0, hot=False, seed=0, bad=None):
    """test_afm_gpu._step_and_check for a pair step: the mean loss, the attention gradient, every touched row's V and w under
    the rule, the untouched rows bit for bit; the bias words as the exactly-zero gradient leaves them.  bad = (row, field): that
    index is put outside its field."""
    fmx = _fmx()
    F = len(sizes)
    tb, params, st = make(sizes, k, t, layout=LAYOUT[rule], seed=seed)
    idx, xv, rows = pair_batch(sizes, Bp, seed=seed + 7, xv_kind=xv_kind, hot=hot)
    valid = None
    if bad is not None:
        valid = np.ones(idx.shape, bool)
        valid[bad] = False
        idx[bad] = sizes[bad[1]] + 3
        rows[bad] = 0
    _live(params, st, k, t, rows, xv, valid)
    if rule == "adam":                                     # non-zero bias moments: a zero gradient still moves the word along them
        tb.bias[1], tb.bias[2] = 0.01, 1e-4
    eng = engine(tb, params, t, 2 * Bp)
    rows_before = tb.rows.detach().cpu().numpy().copy()
    bias_before = tb.bias.detach().cpu().numpy().copy()
    idx_d, xv_d, _ = eng.to_device(idx, xv)
    eng.pair_step(fmx.Hyper(**HYP), rule, idx_d, xv_d, margin=margin)
    torch.cuda.synchronize()
    assert int(eng.error.item()) == (0 if bad is None else 1)
    ref = afm_pair_f64(st["V"], st["w"], st["bias"], st["params"], k, t, rows, xv, margin=margin, valid=valid)
    assert_precheck(ref, F, f"F={F} k={k} t={t} Bp={Bp}")
    assert_within_f64(float(eng.loss_out.item()), ref["loss"], float(np.sum(ref["floor_loss"])) / Bp, "mean pair loss")
    assert_within_f64(eng.logit[:2 * Bp].cpu().numpy(), ref["logit"], ref["floor_logit"], "logits before the update")
    assert_within_f64(eng.grad.cpu().numpy(), ref["dparams"], ref["fl_dparams"], "attention gradient")
    R = int(sum(sizes))
    u = _touched(rows if valid is None else rows[valid], R)
    rows_after = tb.rows.detach().cpu().numpy()
    bias_after = tb.bias.detach().cpu().numpy()
    np.testing.assert_array_equal(bits(rows_after[~u]), bits(rows_before[~u]), err_msg="untouched rows moved")
    # ---- the bias: its gradient is the sum of (g, -g) over the pairs, exactly +0 ----
    if rule == "adam":
        p2, m2, v2 = rule_apply(np.float64(bias_before[0]), np.float64(bias_before[1]), np.float64(bias_before[2]), 0.0, "adam",
                                {kk: float(np.float32(HYP[kk])) for kk in ("lr", "eps", "beta1", "beta2")}, 1)
        for got, want, what in ((bias_after[0], p2, "bias"), (bias_after[1], m2, "bias m"), (bias_after[2], v2, "bias v")):
            assert abs(float(got) - want) <= 8 * U32 * abs(want), (what, float(got), want)
        assert bias_after[0] != bias_before[0] and bias_after[1] != bias_before[1]
    else:
        np.testing.assert_array_equal(bits(bias_after), bits(bias_before), err_msg=f"{rule}: the bias words moved")
    gV, gw = ref["dV"][u], ref["dw"][u]
    tV, tw = 1e-5 * np.abs(gV) + ref["fl_dV"][u], 1e-5 * np.abs(gw) + ref["fl_dw"][u]
    kp = tb.kp
    if rule == "ftrl":   # test_afm_gpu._step_and_check's (z, n) checks
        zo = tb.z_offset
        zV0, nV0 = rows_before[u, zo:zo + k].astype(np.float64), rows_before[u, zo + kp:zo + kp + k].astype(np.float64)
        Vw = rows_before[u, :k].astype(np.float64)

        def z_of(g):
            return zV0 + g - (np.sqrt(nV0 + g * g) - np.sqrt(nV0)) / HYP["alpha"] * Vw

        zr, lo, hi = z_of(gV), z_of(gV - tV), z_of(gV + tV)
        got = rows_after[u, zo:zo + k].astype(np.float64)
        tol = (np.abs(hi - lo) / 2 + 1e-5 * np.abs(zr - zV0)
               + 8 * U32 * (np.abs(zr) + np.abs(zV0) + np.abs(Vw) * np.sqrt(nV0 + gV * gV) / HYP["alpha"]))
        assert (np.abs(got - zr) <= tol).all(), "ftrl z"
        nr = nV0 + gV * gV
        assert (np.abs(rows_after[u, zo + kp:zo + kp + k] - nr) <= 2 * np.abs(gV) * tV + tV * tV + 8 * U32 * nr).all(), "ftrl n"
        return
    _check_rule(rule, rows_after[u, :k], rows_before[u, :k].astype(np.float64), gV, tV, f"{rule} V")
    _check_rule(rule, rows_after[u, kp], rows_before[u, kp].astype(np.float64), gw, tw, f"{rule} w")


# (F, k -> kp, t, B_pairs, xv, margin)
STEP_GEOMETRY = [
    pytest.param(12, 10, 4, 130, "random", 0.0, id="F12-k10-t4-P130-two_tiles"),
    pytest.param(12, 10, 4, 130, "random", 0.1, id="F12-k10-t4-P130-two_tiles-margin"),
    pytest.param(13, 3, 1, 1, "ones", 0.0, id="F13-k3-t1-P1-kp4"),
    pytest.param(2, 1, 64, 33, "random", 0.0, id="F2-k1-t64-P33-one_field_pair"),
    pytest.param(20, 16, 16, 200, "ones", 0.0, id="F20-k16-t16-P200-four_tiles"),
    pytest.param(39, 16, 16, 257, "random", 0.0, id="F39-k16-t16-P257-criteo_width"),
    pytest.param(39, 16, 16, 257, "random", 0.1, id="F39-k16-t16-P257-criteo_width-margin"),
    pytest.param(64, 64, 64, 33, "random", 0.0, id="F64-k64-t64-P33-largest_lds"),
    pytest.param(3, 4, 4, 1025, "random", 0.0, id="F3-k4-t4-P1025-two_pairs_a_workgroup"),
]


@pytest.mark.parametrize("F,k,t,Bp,xv_kind,margin", STEP_GEOMETRY)
def test_pair_step_geometry(F, k, t, Bp, xv_kind, margin):
    _pair_step_and_check("sgd", _sizes(F, F + Bp), k, t, Bp, xv_kind=xv_kind, margin=margin, seed=F + t)


@pytest.mark.parametrize("rule", ["signadam", "ftrl", "adam", "adagrad"])
def test_pair_step_rules_multi_tile(rule):
    # F = 20: 190 pairs in 4 tiles; two hot rows of field 0 take all 400 rows (runs cross 64-entry update tiles)
    _pair_step_and_check(rule, _sizes(20, 20), 16, 16, 200, hot=True, seed=9)


@pytest.mark.parametrize("bad", [(2 * 5, 3), (2 * 7 + 1, 9)], ids=["in_a_positive", "in_a_negative"])
def test_pair_step_bad_index(bad):
    _pair_step_and_check("sgd", _sizes(12, 12), 10, 4, 33, seed=4, bad=bad)


# ---- 4. exact cancellation ----
def _workspace_sections(eng, tb, B):
    """dz [B], loss [B], E [B, F kp] of the step's workspace (fmx_afm.hip carve_afm: 256-byte sections behind the table's)."""
    lib = _fmx()._lib.load()
    up = lambda n: (n + 255) // 256 * 256
    o = up(int(lib.fmx_workspace_bytes(tb.c_struct(), B)))
    ws = eng.workspace.view(torch.float32)
    dz = ws[o // 4:o // 4 + B]
    o += up(B * 4)
    loss = ws[o // 4:o // 4 + B]
    o += up(B * 4)
    n = B * tb.n_fields * tb.kp
    return dz.cpu().numpy(), loss.cpu().numpy(), ws[o // 4:o // 4 + n].cpu().numpy().reshape(B, tb.n_fields, tb.kp)


def test_pair_step_identical_rows_cancel_exactly():
    fmx = _fmx()
    F, k, t, Bp = 12, 10, 4, 33
    sizes = _sizes(F, 12)
    tb, params, st = make(sizes, k, t, seed=6)
    idx, xv, rows = pair_batch(sizes, Bp, seed=8, xv_kind="random")
    idx[1::2] = idx[0::2]
    eng = engine(tb, params, t, 2 * Bp)
    rows_before, bias_before = tb.rows.cpu().numpy().copy(), tb.bias.cpu().numpy().copy()
    idx_d, xv_d, _ = eng.to_device(idx, xv)
    eng.pair_step(fmx.Hyper(**HYP), "sgd", idx_d, xv_d, margin=0.0)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bits(tb.rows.cpu().numpy()), bits(rows_before), err_msg="a row moved")
    np.testing.assert_array_equal(bits(tb.bias.cpu().numpy()), bits(bias_before), err_msg="the bias moved")
    dz, loss, E = _workspace_sections(eng, tb, 2 * Bp)
    assert E[0::2].any()
    np.testing.assert_array_equal(E[1::2], -E[0::2])
    np.testing.assert_array_equal(dz[1::2], -dz[0::2])
    ln2 = np.float32(np.log(2.0))                          # pair_loss_dz(0): log1p(exp(-0)) + 0
    ulp = np.spacing(ln2)
    assert (np.abs(loss[0::2] - ln2) <= ulp).all() and not bits(loss[1::2]).any()
    assert abs(np.float32(eng.loss_out.item()) - ln2) <= ulp, float(eng.loss_out.item())


# ---- 6. determinism ----
@pytest.mark.parametrize("F,k,t,Bp", [(39, 16, 16, 257), (3, 4, 4, 1025)])
def test_pair_step_is_deterministic(F, k, t, Bp):
    fmx = _fmx()
    sizes = _sizes(F, F)
    outs = []
    for _ in range(2):
        tb, params, eng, opt = _stream_start("sgd", sizes, k, t, 2 * Bp, seed=11)
        idx, xv, rows = pair_batch(sizes, Bp, seed=12, xv_kind="random", hot=True)
        idx_d, xv_d, _ = eng.to_device(idx, xv)
        eng.pair_step(fmx.Hyper(**HYP), "sgd", idx_d, xv_d, margin=0.1, opt=opt)
        eng.pair_step(fmx.Hyper(**HYP), "sgd", idx_d, xv_d, margin=0.1, opt=opt)
        torch.cuda.synchronize()
        outs.append((tb.rows.cpu().numpy().copy(), tb.bias.cpu().numpy().copy(), params.cpu().numpy().copy(),
                     eng.grad.cpu().numpy().copy(), eng.loss_out.cpu().numpy().copy()))
    for a, b in zip(*outs):
        np.testing.assert_array_equal(bits(a), bits(b))


# ---- 7. the stream is its steps ----
def _everything(tb, params, opt, losses, extra=None):
    torch.cuda.synchronize()
    out = dict(rows=tb.rows.cpu(), bias=tb.bias.cpu(), params=params.cpu(), m=opt.m.cpu(), v=opt.v.cpu(), losses=losses.cpu())
    if extra is not None:
        out.update({kk: v.cpu() for kk, v in extra.items()})
    return out


def _assert_same(got, want, what):
    for key in want:
        assert got[key].shape == want[key].shape, (what, key)
        assert torch.equal(got[key].view(torch.int32), want[key].view(torch.int32)), \
            f"{what}: {key} differs ({int((got[key] != want[key]).sum())} words)"


@pytest.mark.parametrize("F,k,t,Bp", [(12, 10, 4, 33), (39, 16, 16, 64)])
@pytest.mark.parametrize("rule", ["signadam", "ftrl", "adam", "adagrad", "sgd"])
def test_pair_stream_equals_its_steps_bit_for_bit(rule, F, k, t, Bp):
    n_pool, n_steps, margin = 3, 5, 0.1
    sizes = _sizes(F, 31)
    pool = [pair_batch(sizes, Bp, seed=300 + j, xv_kind="random", hot=True) for j in range(n_pool)]
    idx_pool = torch.from_numpy(np.stack([p[0] for p in pool])).cuda().contiguous()
    xv_pool = torch.from_numpy(np.stack([p[1] for p in pool])).cuda().contiguous()
    hyp = _hyper(rule)
    moments = LAYOUT[rule] == "moments"

    tb, params, eng, opt = _stream_start(rule, sizes, k, t, 2 * Bp, seed=41)
    losses = torch.zeros(n_steps, device="cuda")
    for s in range(n_steps):
        eng.pair_step(hyp, rule, idx_pool[s % n_pool], xv_pool[s % n_pool], margin=margin, opt=opt)
        losses[s] = eng.loss_out[0]
    want = _everything(tb, params, opt, losses)
    assert int(eng.error.item()) == 0 and opt.step == 2 + n_steps and tb.step == (n_steps if moments else 0)
    assert bool(torch.isfinite(want["losses"]).all()) and bool((want["losses"] != 0).all())    # (a margin lets a loss go below 0)

    for split in ((n_steps,), (2, 3)):
        tb, params, eng, opt = _stream_start(rule, sizes, k, t, 2 * Bp, seed=41)
        losses = torch.full((n_steps,), -1.0, device="cuda")
        done = 0
        for n in split:
            # a call starts at batch 0 of the pool it is given: the second call's pool is the first's, rotated by `done`
            order = [(done + j) % n_pool for j in range(n_pool)]
            eng.pair_stream(hyp, rule, idx_pool[order].contiguous(), xv_pool[order].contiguous(), Bp, n, opt, margin=margin,
                            losses=losses[done:])
            done += n
        got = _everything(tb, params, opt, losses)
        assert int(eng.error.item()) == 0 and opt.step == 2 + n_steps and tb.step == (n_steps if moments else 0)
        _assert_same(got, want, f"{rule} pair stream {split}")


# ---- 8. the online run is single-pair steps ----
@pytest.mark.parametrize("F,k,t", [pytest.param(5, 3, 4, id="kp4"), pytest.param(12, 10, 4, id="kp16")])
@pytest.mark.parametrize("rule", ["signadam", "ftrl", "adam", "adagrad", "sgd"])
def test_pair_online_run_equals_single_pair_steps_bit_for_bit(rule, F, k, t):
    N, margin = 40, 0.1
    sizes = [int(s) for s in np.random.default_rng(F).integers(2, 6, size=F)]
    idx, xv, rows = pair_batch(sizes, N, seed=500 + F, xv_kind="random", share_item=True)
    hyp = _hyper(rule)
    moments = LAYOUT[rule] == "moments"

    tb, params, eng, opt = _stream_start(rule, sizes, k, t, 2, seed=41)
    idx_d, xv_d, _ = eng.to_device(idx, xv)
    logits, losses = torch.zeros(2 * N, device="cuda"), torch.zeros(N, device="cuda")
    for i in range(N):
        eng.forward(hyp, idx_d[2 * i:2 * i + 2], xv_d[2 * i:2 * i + 2])            # the pair's logits before its update
        before = eng.logit[:2].clone()
        eng.pair_step(hyp, rule, idx_d[2 * i:2 * i + 2], xv_d[2 * i:2 * i + 2], margin=margin, inv_b=1.0, opt=opt)
        assert torch.equal(eng.logit[:2], before)
        logits[2 * i:2 * i + 2] = eng.logit[:2]
        losses[i] = eng.loss_out[0]
    want = _everything(tb, params, opt, losses, dict(logits=logits, grad=eng.grad, error=eng.error))
    assert opt.step == 2 + N and tb.step == (N if moments else 0) and int(want["error"]) == 0
    assert bool(torch.isfinite(want["losses"]).all()) and bool((want["losses"] != 0).all())    # (a margin lets a loss go below 0)

    for split in ((N,), (1, 25, 14)):
        tb, params, eng, opt = _stream_start(rule, sizes, k, t, 2, seed=41)
        logits, losses = torch.full((2 * N,), -7.0, device="cuda"), torch.full((N,), -7.0, device="cuda")
        o = 0
        for n in split:
            eng.pair_online_run(hyp, rule, idx_d[2 * o:2 * (o + n)], xv_d[2 * o:2 * (o + n)], opt, margin=margin,
                                logits=logits[2 * o:], losses=losses[o:])
            o += n
        got = _everything(tb, params, opt, losses, dict(logits=logits, grad=eng.grad, error=eng.error))
        assert opt.step == 2 + N and tb.step == (N if moments else 0)
        _assert_same(got, want, f"{rule} pair online run {split}")


# ---- the one queue of steps at its smallest (test_afm_stream_gpu's SMALL): 3 pairs a step, a pool of 3 walked twice and a step
#      more, 5 pairs online in the queued form -- without xv, and from a stream that is not torch's default ----
@functools.lru_cache(maxsize=None)
def _small_pairs(rule, with_xv):
    """(sizes, pool and stream on the device, what the single pair steps on the default stream leave): computed once per case"""
    F, k, t, P, n_pool, n_steps, N = (SMALL[kk] for kk in ("F", "k", "t", "units", "n_pool", "n_steps", "N"))
    sizes, kind, margin = _sizes(F, 31), "random" if with_xv else "ones", 0.1
    pool = [pair_batch(sizes, P, seed=300 + j, xv_kind=kind) for j in range(n_pool)]
    idx_pool = torch.from_numpy(np.stack([p[0] for p in pool])).cuda().contiguous()
    xv_pool = torch.from_numpy(np.stack([p[1] for p in pool])).cuda().contiguous() if with_xv else None
    hyp = _hyper(rule)
    tb, params, eng, opt = _stream_start(rule, sizes, k, t, 2 * P, seed=41)
    losses = torch.zeros(n_steps, device="cuda")
    for s in range(n_steps):
        j = s % n_pool
        eng.pair_step(hyp, rule, idx_pool[j], None if xv_pool is None else xv_pool[j], margin=margin, opt=opt)
        losses[s] = eng.loss_out[0]
    want_stream = _everything(tb, params, opt, losses)
    assert int(eng.error.item()) == 0 and opt.step == 2 + n_steps

    idx, xv, _ = pair_batch(sizes, N, seed=340, xv_kind=kind, share_item=True)
    tb, params, eng, opt = _stream_start(rule, sizes, k, t, 2, seed=41)
    idx_d, xv_d, _ = eng.to_device(idx, xv)
    logits, losses = torch.zeros(2 * N, device="cuda"), torch.zeros(N, device="cuda")
    for i in range(N):
        sl = slice(2 * i, 2 * i + 2)
        eng.pair_step(hyp, rule, idx_d[sl], None if xv_d is None else xv_d[sl], margin=margin, inv_b=1.0, opt=opt)
        logits[sl] = eng.logit[:2]                                 # (the step's own forward: the logits before its update)
        losses[i] = eng.loss_out[0]
    want_online = _everything(tb, params, opt, losses, dict(logits=logits, grad=eng.grad, error=eng.error))
    assert opt.step == 2 + N and int(want_online["error"]) == 0
    for want in (want_stream, want_online):
        assert bool(torch.isfinite(want["losses"]).all()) and bool((want["losses"] != 0).all())
    return sizes, margin, (idx_pool, xv_pool), (idx_d, xv_d), want_stream, want_online


@SMALL_CASES
@SMALL_RULES
def test_small_pair_stream_is_its_single_steps(rule, with_xv, side):
    k, t, P, n_steps = (SMALL[kk] for kk in ("k", "t", "units", "n_steps"))
    sizes, margin, (idx_pool, xv_pool), _, want, _ = _small_pairs(rule, with_xv)
    tb, params, eng, opt = _stream_start(rule, sizes, k, t, 2 * P, seed=41)
    losses = torch.full((n_steps,), -1.0, device="cuda")
    issue(side, lambda st: eng.pair_stream(_hyper(rule), rule, idx_pool, xv_pool, P, n_steps, opt, margin=margin, losses=losses,
                                           stream=st))
    got = _everything(tb, params, opt, losses)
    assert int(eng.error.item()) == 0 and opt.step == 2 + n_steps and tb.step == (n_steps if LAYOUT[rule] == "moments" else 0)
    _assert_same(got, want, f"{rule} pair stream")


@SMALL_CASES
@SMALL_RULES
def test_small_queued_pair_online_run_is_its_single_steps(rule, with_xv, side):
    """The queued form in two calls of 1 and N - 1 pairs: the second call's logits start two floats in, its losses one."""
    k, t, N = (SMALL[kk] for kk in ("k", "t", "N"))
    sizes, margin, _, (idx_d, xv_d), _, want = _small_pairs(rule, with_xv)
    tb, params, eng, opt = _stream_start(rule, sizes, k, t, 2, seed=41)
    logits, losses = torch.full((2 * N,), -7.0, device="cuda"), torch.full((N,), -7.0, device="cuda")
    hyp = _hyper(rule)

    def run(st):
        for o, n in ((0, 1), (1, N - 1)):
            eng.pair_online_run(hyp, rule, idx_d[2 * o:2 * (o + n)], None if xv_d is None else xv_d[2 * o:2 * (o + n)], opt,
                                margin=margin, logits=logits[2 * o:], losses=losses[o:], stream=st)
    with queued_online_form(b"afm_pair_online_persistent"):
        assert eng.pair_online_form(ATTN_RULE[rule])[0] == 0
        issue(side, run)
    got = _everything(tb, params, opt, losses, dict(logits=logits, grad=eng.grad, error=eng.error))
    assert opt.step == 2 + N and tb.step == (N if LAYOUT[rule] == "moments" else 0)
    _assert_same(got, want, f"{rule} queued pair online run")


def test_pair_online_run_of_zero_pairs_touches_nothing():
    rule, F, k, t = "adam", 5, 3, 4
    sizes = _sizes(F, 7)
    tb, params, eng, opt = _stream_start(rule, sizes, k, t, 2, seed=3)
    before = _everything(tb, params, opt, torch.zeros(1), dict(grad=eng.grad))
    idx_d = torch.zeros((2, F), dtype=torch.int32, device="cuda")       # (an empty tensor has no address to pass)
    fmx = _fmx()
    L, hyp = fmx._lib, _hyper(rule)
    rc = eng.lib.fmx_afm_pair_online_run(tb.c_struct(), hyp.ref(), L.RULES[rule], C.byref(eng.c_afm), idx_d.data_ptr(), None, 0, 0.0,
                                         eng.workspace.data_ptr(), eng.workspace.numel() * 4, eng.grad.data_ptr(), opt.ref(), None,
                                         None, eng.error.data_ptr(), None)
    assert rc == L.OK
    after = _everything(tb, params, opt, torch.zeros(1), dict(grad=eng.grad))
    _assert_same(after, before, "N_pairs = 0")
    assert opt.step == 2 and tb.step == 0


# ---- 9. the classes ----
def _afm_adam():
    from models.models_online_deep.afm_adam import AFMAdam
    return AFMAdam


def _class_data(sizes, B, seed, n_neg=1):
    """positives [B, F], their values, the item field and explicit negatives [B, n_neg, 1] (never the positive's own item)"""
    rng = np.random.default_rng(seed)
    F = len(sizes)
    pos = np.stack([rng.integers(0, s, size=B) for s in sizes], axis=1).astype(np.int32)
    pos[::3, :F - 1] = pos[0, :F - 1]
    xv = rng.uniform(0.2, 1.8, size=pos.shape).astype(np.float32)
    neg = (pos[:, F - 1:F, None] + 1 + rng.integers(0, sizes[-1] - 1, size=(B, n_neg, 1))) % sizes[-1]
    return pos, xv, [F - 1], neg.astype(np.int64)


def _models(n, sizes, k, t, rule, fused=True, lr=0.01, seed=5):
    out = []
    for _ in range(n):
        torch.manual_seed(seed)
        out.append(_afm_adam()(sizes, embedding_size=k, attention_size=t, batch_size=64, n=lr, update_rule=rule, fused_optimizer=fused))
    return out


@pytest.mark.parametrize("sampled", [False, True], ids=["explicit_negatives", "sampled_negatives"])
@pytest.mark.parametrize("rule", ["adam", "ftrl"])
def test_class_fit_pairs_is_the_engine_pair_step(rule, sampled):
    import fmx
    sizes, k, t, B, margin = [20, 300, 5, 64, 9, 40], 8, 4, 50, 0.1
    a, b = _models(2, sizes, k, t, rule)
    pos, xv, fields, neg = _class_data(sizes, B, seed=3, n_neg=2)
    for step in range(2):
        if sampled:
            la = a.fit_pairs(pos, xv, fields, n_neg=2, margin=margin, generator=torch.Generator().manual_seed(7 + step),
                             attention=True)
            idx_d, xv_d, _ = b._inputs(pos, xv)
            negs = fmx.pairwise.sample_negatives(idx_d, fields, [sizes[-1]], n_neg=2, generator=torch.Generator().manual_seed(7 + step))
        else:
            la = a.fit_pairs(pos, xv, fields, negatives=neg, margin=margin, attention=True)
            idx_d, xv_d, _ = b._inputs(pos, xv)
            negs = neg
        rows, vals = fmx.pairwise.assemble_pairs(idx_d, xv_d, fields, negs)
        assert rows.shape[0] == 2 * 2 * B
        b._engine.pair_step(b._hyper, rule, rows, vals, margin=margin, opt=b._attn_fused)
        assert torch.equal(la, b._engine.loss_out[0]) and np.isfinite(float(la)) and float(la) != 0
        b._engine.check_error_flag()
    _same_models(a, b)
    assert a._attn_fused.step == 2


@pytest.mark.parametrize("rule", ["adam", "sgd"])
def test_class_fit_pairs_with_and_without_the_fused_optimizer(rule):
    """fused_optimizer=False splits the step as update_embedding does: the same table step (bit for bit), the attention
    parameters' rule on torch.  Both settings' attention parameters are held to float64 on afm_pair_f64's gradient with
    test_afm_stream_gpu.check_attention, the comparison test_afm_class_adaptive_steps_track_f64 / test_class_fused_steps_track_f64
    make of the two settings."""
    sizes, k, t, B, margin = _sizes(14, 14), 8, 8, 128, 0.0
    lr = HYP["lr"] if rule == "sgd" else 0.01
    (fused,), (plain,) = _models(1, sizes, k, t, rule, True, lr), _models(1, sizes, k, t, rule, False, lr)
    pos, xv, fields, neg = _class_data(sizes, B, seed=9)
    F32 = lambda v: float(np.float32(v))
    b1, b2 = fused._betas()
    h = dict(lr=F32(lr), eps=F32(fused._adam["eps"]), beta1=b1, beta2=b2)
    V, w, bias, params = _model_state(fused)
    idx = np.repeat(pos, 2, axis=0)
    idx[1::2, -1] = neg[:, 0, 0]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    ref = afm_pair_f64(V, w, bias, params, k, t, idx.astype(np.int64) + offs[:-1], np.repeat(xv, 2, axis=0), margin=margin)
    before_f = opt_state(fused._attn_flat, fused._attn_fused)
    before_p = (plain._attn_flat.detach().double().cpu().numpy(),) + (_attn_state(plain)[1:] if rule == "adam" else (None, None))
    lf = fused.fit_pairs(pos, xv, fields, negatives=neg, margin=margin, attention=True)
    lp = plain.fit_pairs(pos, xv, fields, negatives=neg, margin=margin, attention=True)
    assert torch.equal(lf, lp)
    assert_within_f64(float(lf), ref["loss"], float(np.sum(ref["floor_loss"])) / B, "mean pair loss")
    sf, sp = fused.state_dict(), plain.state_dict()
    for key in sf:
        if "embeddings" in key or key == "bias":
            assert torch.equal(sf[key], sp[key]), key
    check_attention(rule, h, 1, before_f, opt_state(fused._attn_flat, fused._attn_fused), ref, f"{rule} fused")
    after_p = (plain._attn_flat.detach().double().cpu().numpy(),) + (_attn_state(plain)[1:] if rule == "adam" else (None, None))
    check_attention(rule, h, 1, before_p, after_p, ref, f"{rule} torch")


@pytest.mark.parametrize("rule", ["adam", "ftrl"])
def test_class_pair_experiment_equals_the_loop_and_survives_pickling(rule):
    sizes, k, t, N, margin = [4, 3, 5, 6], 4, 4, 30, 0.1
    a, b = _models(2, sizes, k, t, rule)
    pos, xv, fields, neg = _class_data(sizes, N, seed=21)
    half = N // 2
    ra = a.run_pair_experiment(pos[:half], xv[:half], fields, negatives=neg[:half], margin=margin, attention=True)
    a2 = pickle.loads(pickle.dumps(a))                     # a round trip in the middle of the run
    ra2 = [m.run_pair_experiment(pos[half:], xv[half:], fields, negatives=neg[half:], margin=margin, attention=True) for m in (a, a2)]
    assert ra2[0][1:] == ra2[1][1:]
    _same_models(a, a2)
    # the host loop of one-pair steps on a second model
    pred = []
    for i in range(N):
        b.fit_pairs(pos[i:i + 1], xv[i:i + 1], fields, negatives=neg[i:i + 1], margin=margin, attention=True)
        pred.append(bool(b._engine.logit[0] > b._engine.logit[1]))
    _same_models(a, b)
    assert a._attn_fused.step == N
    pred = np.array(pred)
    for r, p in ((ra, pred[:half]), (ra2[0], pred[half:])):
        n = len(p)
        assert r[3] == {"correct": int(p.sum()), "wrong": int(n - p.sum())}
        assert r[2] == [float(np.cumsum(p)[i] / (i + 1) * 100) for i in sorted({0, n - 1})] and r[1] == r[2][-1]
    # fused_optimizer=False: the same protocol as a host loop; zero pairs
    (c,) = _models(1, sizes, k, t, rule, fused=False)
    rc = c.run_pair_experiment(pos[:5], xv[:5], fields, negatives=neg[:5], margin=margin, attention=True)
    assert sum(rc[3].values()) == 5 and 0 <= rc[1] <= 100
    rz = a.run_pair_experiment(pos[:0], xv[:0], fields, negatives=neg[:0], margin=margin, attention=True)
    assert rz[1:] == (0.0, [], {"correct": 0, "wrong": 0})


# ---- 10. it trains ----
@pytest.mark.parametrize("margin", MARGINS)
@pytest.mark.parametrize("F,k,t", [(4, 4, 4), (12, 10, 4)])
def test_sixty_pair_steps_bring_the_loss_down(F, k, t, margin):
    """Sixty sgd steps (lr 0.05) on one fixed batch of 64 pairs: the kernels' loss falls by at least half of what the float64
    restatement, iterated on the same data from the same state, falls by.  (That restatement falls monotonically on this data: 0.7199 -> 0.6969 and
    0.7359 -> 0.7059 at margin 0, 0.5307 -> 0.5154 and 0.5432 -> 0.5239 at margin 0.1; the kernels' losses print the same digits.)  Then the trained model is evaluated by rank."""
    sizes, Bp, lr, T = _sizes(F, F), 64, 0.05, 60
    rng = np.random.default_rng(F)
    (m,) = _models(1, sizes, k, t, "sgd", True, lr)
    sd = m.state_dict()
    for key, v in sd.items():                              # test_afm_gpu.make's distributions
        if key.startswith("second_order"):
            sd[key] = torch.from_numpy((rng.normal(size=tuple(v.shape)) * 0.4).astype(np.float32))
        elif key.startswith("first_order"):
            sd[key] = torch.from_numpy((rng.normal(size=tuple(v.shape)) * 0.3).astype(np.float32))
        elif key in ("attention_linear.weight", "attention_linear.bias", "H", "P"):
            sd[key] = torch.from_numpy((rng.normal(size=tuple(v.shape)) * 0.5).astype(np.float32))
        elif key == "bias":
            sd[key] = torch.full_like(v, 0.2)
    m.load_state_dict(sd)
    pos, xv, fields, neg = _class_data(sizes, Bp, seed=F + 1)
    V, w, bias, params = (np.asarray(a, np.float64) for a in _model_state(m))
    idx = np.repeat(pos, 2, axis=0)
    idx[1::2, -1] = neg[:, 0, 0]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    rows, x2 = idx.astype(np.int64) + offs[:-1], np.repeat(xv, 2, axis=0)
    want = []
    for _ in range(T):
        r = afm_pair_f64(V, w, float(bias), params, k, t, rows, x2, margin=margin)
        want.append(r["loss"])
        V, w, params = V - lr * r["dV"], w - lr * r["dw"], params - lr * r["dparams"]
    got = [float(m.fit_pairs(pos, xv, fields, negatives=neg, margin=margin, attention=True)) for _ in range(T)]
    print(f"F={F} margin={margin}: float64 {want[0]:.4f} -> {want[-1]:.4f}, kernels {got[0]:.4f} -> {got[-1]:.4f}")
    assert want[0] - want[-1] > 0
    assert got[0] - got[-1] >= 0.5 * (want[0] - want[-1]), (got[0], got[-1], want[0], want[-1])
    metrics = m.evaluate_ranking(pos, xv, fields, pos[:, -1].astype(np.int64))
    assert metrics and all(np.isfinite(float(v)) for v in metrics.values()), metrics
