"""fmx_afm_list_* on the GPU: the list forward's logits against fmx_afm_forward bit for bit and its loss / dlogit against the
float64 restatement in tests/afm_list_f64.py; one list step against float64 across the pair-tile geometries, list sizes and
update rules (from non-zero moments too), the bias words and their state bit-unchanged under every rule; exact cancellation when
the two rows of a G = 2 list coincide; an index outside its field; determinism; guard bands; the stream against its steps and the
online run against one-list steps, bit for bit; AFMAdam.fit_lists / run_list_experiment(attention=True); and sixty steps that
bring the list loss down."""
import ctypes as C
import functools
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from afm_list_f64 import U32, afm_list_f64, live_params  # noqa: E402
from helpers import assert_within_f64  # noqa: E402
from test_adaptive_rules_cpu import rule_apply  # noqa: E402
from test_afm_gpu import (HYP, _attn_state, _check_rule, _model_state, _sizes, _touched, assert_exercised, engine,  # noqa: E402
                          make)
from test_afm_pair_gpu import _assert_same, _class_data, _everything, _models, bits  # noqa: E402
from test_afm_stream_gpu import (LAYOUT, SMALL, SMALL_CASES, SMALL_RULES, _hyper, _same_models, _stream_start, check_attention,  # noqa: E402
                                 issue, opt_state)

pytestmark = pytest.mark.gpu

RULES = ["signadam", "ftrl", "adam", "adagrad", "sgd"]
NAN_WORD = 0x7FC00123          # a quiet NaN with a payload: the guard bands' pattern


def _fmx():
    import fmx
    return fmx


def list_sizes(F, G, seed):
    """_sizes with an item field (the last) of at least G + 1 rows: a list's G items are distinct"""
    sizes = _sizes(F, seed)
    sizes[-1] = max(sizes[-1], G + 1)
    return sizes


def list_batch(sizes, Bl, G, seed=1, xv_kind="ones", hot=False):
    """Bl lists of G rows -> (idx int32 [Bl G, F], xv [Bl G, F] or None, global rows [Bl G, F]).  The item is the last field; a
    list's negatives are its positive with other, distinct indices of that field (the values kept); every third list takes list
    0's whole context, so every context field has runs of G and longer."""
    rng = np.random.default_rng(seed)
    F = len(sizes)
    pos = np.stack([rng.integers(0, s, size=Bl) for s in sizes], axis=1).astype(np.int32)
    if hot:
        pos[:, 0] = rng.integers(0, 2, size=Bl)          # two rows of field 0 take every occurrence: runs cross 64-entry tiles
    pos[::3, :F - 1] = pos[0, :F - 1]
    idx = np.repeat(pos, G, axis=0)
    n_item = sizes[-1]
    for i in range(Bl):
        idx[G * i + 1:G * (i + 1), F - 1] = (pos[i, F - 1] + 1 + rng.permutation(n_item - 1)[:G - 1]) % n_item
    xv = None
    if xv_kind != "ones":
        xp = rng.uniform(0.2, 1.8, size=pos.shape).astype(np.float32)
        if xv_kind == "zeros":
            xp[:, ::3] = 0.0
        xv = np.repeat(xp, G, axis=0)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return idx, xv, idx.astype(np.int64) + offs[:-1][None, :]


def _live(params, st, k, t, rows, xv, valid=None):
    x = np.ones(rows.shape) if xv is None else xv
    fixed = live_params(st["params"], st["V"], k, t, rows, x if valid is None else x * valid)
    params.copy_(torch.from_numpy(fixed))
    st["params"] = fixed


def assert_precheck(ref, F, G, inv_b, what):
    """What every float64-tolerance test asserts of its own data: no list at the loss's flat end (the negatives hold at least 1 %
    of the mass), no dead attention unit, every pair tile carrying gradient."""
    mass = np.abs(ref["dz"][0::G]) / inv_b
    assert (mass >= 0.01).all(), f"{what}: min negatives' mass {mass.min():.3g}"
    assert_exercised(ref, F, what)


# ---- 1. the forward ----
# (F, k -> kp, t, B_lists, G, xv): one field pair / two tiles / criteo width; kp 4, 16, 16; t 1, 4, 16; G 2, 3, 5, 16; 1, 33 and
# 1,025 lists (a workgroup walks two lists)
FORWARD_CASES = [(2, 3, 1, 1, 2, "ones"), (12, 10, 4, 33, 3, "random"), (39, 16, 16, 33, 5, "zeros"), (2, 3, 4, 1025, 16, "random"),
                 (12, 16, 16, 1, 16, "ones")]


@pytest.mark.parametrize("F,k,t,Bl,G,xv_kind", FORWARD_CASES)
def test_list_forward(F, k, t, Bl, G, xv_kind):
    fmx = _fmx()
    B = Bl * G
    sizes = list_sizes(F, G, F + Bl)
    tb, params, st = make(sizes, k, t, seed=F + k)
    idx, xv, rows = list_batch(sizes, Bl, G, seed=Bl, xv_kind=xv_kind)
    _live(params, st, k, t, rows, xv)
    eng = engine(tb, params, t, B + 8)
    idx_d, xv_d, _ = eng.to_device(idx, xv)
    hyp = fmx.Hyper(**HYP)
    eng.forward(hyp, idx_d, xv_d)
    plain = eng.logit[:B].cpu().numpy().copy()
    eng.logit.view(torch.int32).fill_(NAN_WORD)
    eng.loss_b.view(torch.int32).fill_(NAN_WORD)
    dz = torch.full((B + 8,), NAN_WORD, dtype=torch.int32, device="cuda").view(torch.float32)
    inv_b = 0.37 / Bl
    assert eng.list_forward(hyp, idx_d, G, xv_d, inv_b=inv_b, dz=dz) == Bl
    torch.cuda.synchronize()
    logit, loss, dzn = eng.logit[:B].cpu().numpy(), eng.loss_b[:B].cpu().numpy(), dz[:B].cpu().numpy()
    assert int(eng.error.item()) == 0
    for name, buf in (("logit_out", eng.logit), ("loss_out", eng.loss_b), ("dz_out", dz)):       # the guard bands behind the B rows
        assert bool((buf.view(torch.int32)[B:B + 8] == NAN_WORD).all()), f"{name}: written past its {B} rows"
    np.testing.assert_array_equal(bits(logit), bits(plain), err_msg="the list forward's logits are not fmx_afm_forward's")
    for j in range(1, G):
        assert not bits(loss[j::G]).any(), f"loss[G i + {j}] is not +0"
    ref = afm_list_f64(st["V"], st["w"], st["bias"], st["params"], k, t, rows, G, xv, inv_b=inv_b)
    assert_precheck(ref, F, G, inv_b, f"forward F={F} Bl={Bl} G={G}")
    assert_within_f64(logit, ref["logit"], ref["floor_logit"], "logit")
    assert_within_f64(loss, ref["loss_b"], ref["floor_loss"], "list loss")
    assert_within_f64(dzn, ref["dz"], ref["floor_dz"], "dlogit")
    assert (dzn[0::G] < 0).all() and (dzn.reshape(Bl, G)[:, 1:] > 0).all()


def test_list_forward_stays_finite_at_wide_logit_gaps():
    """The item rows' first-order weights are -90, 0 or +90: lists hold logit gaps beyond +-80 in both directions."""
    fmx = _fmx()
    F, k, t, Bl, G = 6, 8, 4, 64, 5
    sizes = list_sizes(F, G, 3)
    tb, params, st = make(sizes, k, t, seed=2)
    first = int(sum(sizes[:-1]))
    item = torch.arange(sizes[-1], device="cuda")
    tb.rows[first:, tb.kp] = 90.0 * ((item % 3) - 1).float()
    idx, xv, rows = list_batch(sizes, Bl, G, seed=5, xv_kind="ones")
    eng = engine(tb, params, t, Bl * G)
    idx_d, xv_d, _ = eng.to_device(idx, xv)
    dz = torch.zeros(Bl * G, device="cuda")
    eng.list_forward(fmx.Hyper(**HYP), idx_d, G, xv_d, inv_b=1.0, dz=dz)
    z = eng.logit[:Bl * G].cpu().numpy().reshape(Bl, G)
    gap = z[:, 1:] - z[:, :1]
    assert gap.max() > 80 and gap.min() < -80, (gap.min(), gap.max())
    loss, dzn = eng.loss_b[:Bl * G].cpu().numpy().reshape(Bl, G), dz.cpu().numpy().reshape(Bl, G)
    assert np.isfinite(z).all() and np.isfinite(loss).all() and np.isfinite(dzn).all()
    assert (loss[:, 0] >= 0).all() and (dzn[:, 0] <= 0).all() and (dzn[:, 1:] >= 0).all() and (np.abs(dzn) <= 1).all()
    assert loss[:, 0].max() > 80 and loss[:, 0].min() < 1e-30          # both ends of the softmax were reached
    assert (np.abs(dzn.astype(np.float64).sum(1)) <= 4 * G * U32).all()


# ---- 2. one step against float64 ----
def _set_moments(tb, k, rule, seed):
    """Non-zero optimizer state for the table's rows and bias (adam: m and v; adagrad: v, m stays 0) -> (mV, vV, mw, vw) float64"""
    rng = np.random.default_rng(seed)
    R, kp, zo = tb.rows.shape[0], tb.kp, tb.z_offset
    mV = (0.01 * rng.standard_normal((R, k))).astype(np.float32) * (rule == "adam")
    vV = (1e-4 * rng.uniform(0.5, 2.0, (R, k))).astype(np.float32)
    mw = (0.01 * rng.standard_normal(R)).astype(np.float32) * (rule == "adam")
    vw = (1e-4 * rng.uniform(0.5, 2.0, R)).astype(np.float32)
    tb.rows[:, zo:zo + k] = torch.from_numpy(mV).cuda()
    tb.rows[:, zo + kp:zo + kp + k] = torch.from_numpy(vV).cuda()
    tb.rows[:, kp + 1] = torch.from_numpy(mw).cuda()
    tb.rows[:, kp + 2] = torch.from_numpy(vw).cuda()
    return tuple(a.astype(np.float64) for a in (mV, vV, mw, vw))


def _check_rule_from(rule, got, before, m, v, g, g_tol, what):
    """test_afm_gpu._check_rule's comparison (the rule's response to the gradient's own bound, the same multipliers) for the
    adaptive rules started from the moments (m, v): test_adaptive_rules_cpu.rule_apply is the rule."""
    h = {kk: float(np.float32(HYP[kk])) for kk in ("lr", "eps", "beta1", "beta2")}
    f = lambda gg: rule_apply(before, m, v, gg, rule, h, 1)[0]
    ref, lo, hi = f(g), f(g - g_tol), f(g + g_tol)
    tol = np.abs(hi - lo) / 2 + 1e-5 * np.abs(ref - before) + 8 * U32 * (np.abs(ref) + np.abs(before))
    err = np.abs(np.asarray(got, np.float64) - ref)
    bad = err > tol
    assert not np.any(bad), f"{what}: {int(np.sum(bad))}/{np.size(bad)} off, worst err/tol {float(np.max(err / np.maximum(tol, 1e-300))):.2f}"


def _list_step_and_check(rule, sizes, k, t, Bl, G, xv_kind="random", hot=False, seed=0, bad=None, moments=False):
    """test_afm_pair_gpu._pair_step_and_check for a list step: the mean loss, the logits, the attention gradient, every touched
    row's V and w under the rule, the untouched rows bit for bit; the bias words and their state bit-unchanged.  bad = (row,
    field): that index is put outside its field.  moments: the adaptive rules start from non-zero moments."""
    fmx = _fmx()
    F, B = len(sizes), Bl * G
    tb, params, st = make(sizes, k, t, layout=LAYOUT[rule], seed=seed)
    mom = _set_moments(tb, k, rule, seed + 1) if moments and LAYOUT[rule] == "moments" else None
    idx, xv, rows = list_batch(sizes, Bl, G, seed=seed + 7, xv_kind=xv_kind, hot=hot)
    valid = None
    if bad is not None:
        valid = np.ones(idx.shape, bool)
        valid[bad] = False
        idx[bad] = sizes[bad[1]] + 3
        rows[bad] = 0
    _live(params, st, k, t, rows, xv, valid)
    if LAYOUT[rule] == "moments":                          # non-zero bias moments: a zero gradient would still move the word along them
        tb.bias[1], tb.bias[2] = 0.01, 1e-4
    eng = engine(tb, params, t, B)
    rows_before = tb.rows.detach().cpu().numpy().copy()
    bias_before = tb.bias.detach().cpu().numpy().copy()
    idx_d, xv_d, _ = eng.to_device(idx, xv)
    eng.list_step(fmx.Hyper(**HYP), rule, idx_d, G, xv_d)
    torch.cuda.synchronize()
    assert int(eng.error.item()) == (0 if bad is None else 1)
    ref = afm_list_f64(st["V"], st["w"], st["bias"], st["params"], k, t, rows, G, xv, valid=valid)
    assert_precheck(ref, F, G, 1.0 / Bl, f"F={F} k={k} t={t} Bl={Bl} G={G}")
    assert_within_f64(float(eng.loss_out.item()), ref["loss"], float(np.sum(ref["floor_loss"])) / Bl, "mean list loss")
    assert_within_f64(eng.logit[:B].cpu().numpy(), ref["logit"], ref["floor_logit"], "logits before the update")
    assert_within_f64(eng.grad.cpu().numpy(), ref["dparams"], ref["fl_dparams"], "attention gradient")
    R = int(sum(sizes))
    u = _touched(rows if valid is None else rows[valid], R)
    rows_after = tb.rows.detach().cpu().numpy()
    np.testing.assert_array_equal(bits(rows_after[~u]), bits(rows_before[~u]), err_msg="untouched rows moved")
    # ---- the bias is not part of a list step: its words and their state keep their bits under every rule ----
    np.testing.assert_array_equal(bits(tb.bias.detach().cpu().numpy()), bits(bias_before), err_msg=f"{rule}: the bias words moved")
    gV, gw = ref["dV"][u], ref["dw"][u]
    tV, tw = 1e-5 * np.abs(gV) + ref["fl_dV"][u], 1e-5 * np.abs(gw) + ref["fl_dw"][u]
    kp = tb.kp
    if rule == "ftrl":   # test_afm_gpu._step_and_check's (z, n) checks; make() starts from n = 0.1
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
    V0, w0 = rows_before[u, :k].astype(np.float64), rows_before[u, kp].astype(np.float64)
    if mom is not None:
        mV, vV, mw, vw = mom
        _check_rule_from(rule, rows_after[u, :k], V0, mV[u], vV[u], gV, tV, f"{rule} V from moments")
        _check_rule_from(rule, rows_after[u, kp], w0, mw[u], vw[u], gw, tw, f"{rule} w from moments")
        return
    _check_rule(rule, rows_after[u, :k], V0, gV, tV, f"{rule} V")
    _check_rule(rule, rows_after[u, kp], w0, gw, tw, f"{rule} w")


# (F, k -> kp, t, B_lists, G, xv)
STEP_GEOMETRY = [
    pytest.param(2, 3, 1, 1, 2, "ones", id="F2-k3-t1-L1-G2-one_field_pair"),
    pytest.param(12, 10, 4, 33, 3, "random", id="F12-k10-t4-L33-G3-two_tiles"),
    pytest.param(39, 16, 16, 33, 5, "zeros", id="F39-k16-t16-L33-G5-criteo_width"),
    pytest.param(12, 16, 16, 1, 16, "ones", id="F12-k16-t16-L1-G16-the_limit"),
    pytest.param(2, 3, 4, 1025, 16, "random", id="F2-k3-t4-L1025-G16-two_lists_a_workgroup"),
    pytest.param(2, 10, 4, 1025, 2, "zeros", id="F2-k10-t4-L1025-G2"),
]


@pytest.mark.parametrize("F,k,t,Bl,G,xv_kind", STEP_GEOMETRY)
def test_list_step_geometry(F, k, t, Bl, G, xv_kind):
    _list_step_and_check("sgd", list_sizes(F, G, F + Bl), k, t, Bl, G, xv_kind=xv_kind, seed=F + t)


# every rule from make()'s state (ftrl: n = 0.1, never zero), and the rules that keep moments from non-zero ones as well
@pytest.mark.parametrize("rule,moments", [(r, False) for r in RULES] + [("adam", True), ("adagrad", True)],
                         ids=RULES + ["adam-nonzero_moments", "adagrad-nonzero_moments"])
def test_list_step_rules_multi_tile(rule, moments):
    # F = 12: 66 pairs in 2 tiles; two hot rows of field 0 take all 165 rows (runs cross 64-entry update tiles)
    _list_step_and_check(rule, list_sizes(12, 5, 20), 10, 4, 33, 5, hot=True, seed=9, moments=moments)


@pytest.mark.parametrize("bad", [(3 * 5, 3), (3 * 7 + 2, 9)], ids=["in_a_positive", "in_a_negative"])
def test_list_step_bad_index(bad):
    _list_step_and_check("sgd", list_sizes(12, 3, 12), 10, 4, 33, 3, seed=4, bad=bad)


# ---- 3. exact cancellation at G = 2 ----
def test_list_step_identical_rows_cancel_exactly():
    fmx = _fmx()
    F, k, t, Bl, G = 12, 10, 4, 33, 2
    sizes = list_sizes(F, G, 12)
    tb, params, st = make(sizes, k, t, seed=6)
    idx, xv, rows = list_batch(sizes, Bl, G, seed=8, xv_kind="random")
    idx[1::2] = idx[0::2]
    eng = engine(tb, params, t, Bl * G)
    rows_before, bias_before = tb.rows.cpu().numpy().copy(), tb.bias.cpu().numpy().copy()
    idx_d, xv_d, _ = eng.to_device(idx, xv)
    dz = torch.zeros(Bl * G, device="cuda")
    inv_b = 1.0 / 32                                       # a power of two: -+ inv_b / 2 is exact
    eng.list_forward(fmx.Hyper(**HYP), idx_d, G, xv_d, inv_b=inv_b, dz=dz)
    dzn = dz.cpu().numpy()
    assert (dzn[0::2] == np.float32(-0.5 * inv_b)).all() and (dzn[1::2] == np.float32(0.5 * inv_b)).all()
    eng.list_step(fmx.Hyper(**HYP), "sgd", idx_d, G, xv_d, inv_b=inv_b)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bits(tb.rows.cpu().numpy()), bits(rows_before), err_msg="a row moved")
    np.testing.assert_array_equal(bits(tb.bias.cpu().numpy()), bits(bias_before), err_msg="the bias moved")
    ln2 = np.float32(np.log(2.0))
    ulp = np.spacing(ln2)
    loss = eng.loss_b[:Bl * G].cpu().numpy()
    assert (np.abs(loss[0::2] - ln2) <= ulp).all() and not bits(loss[1::2]).any()


# ---- 4. determinism ----
@pytest.mark.parametrize("F,k,t,Bl,G", [(39, 16, 16, 33, 5), (2, 3, 4, 1025, 16)])
def test_list_step_is_deterministic(F, k, t, Bl, G):
    fmx = _fmx()
    sizes = list_sizes(F, G, F)
    outs = []
    for _ in range(2):
        tb, params, eng, opt = _stream_start("sgd", sizes, k, t, Bl * G, seed=11)
        idx, xv, rows = list_batch(sizes, Bl, G, seed=12, xv_kind="random", hot=True)
        idx_d, xv_d, _ = eng.to_device(idx, xv)
        eng.list_step(fmx.Hyper(**HYP), "sgd", idx_d, G, xv_d, opt=opt)
        eng.list_step(fmx.Hyper(**HYP), "sgd", idx_d, G, xv_d, opt=opt)
        torch.cuda.synchronize()
        outs.append((tb.rows.cpu().numpy().copy(), tb.bias.cpu().numpy().copy(), params.cpu().numpy().copy(),
                     eng.grad.cpu().numpy().copy(), eng.loss_out.cpu().numpy().copy(), eng.logit[:Bl * G].cpu().numpy().copy()))
    for a, b in zip(*outs):
        np.testing.assert_array_equal(bits(a), bits(b))


# ---- 5. guard bands ----
def test_list_step_writes_nothing_past_its_buffers():
    """NaN patterns behind the workspace (past the 16 scratch bytes) and behind logit_out survive a step."""
    fmx = _fmx()
    L = fmx._lib
    F, k, t, Bl, G, rule = 12, 10, 4, 33, 5, "adam"
    B = Bl * G
    sizes = list_sizes(F, G, 5)
    tb, params, eng, opt = _stream_start(rule, sizes, k, t, B, seed=3)
    idx, xv, rows = list_batch(sizes, Bl, G, seed=4, xv_kind="random")
    idx_d, xv_d, _ = eng.to_device(idx, xv)
    need = int(eng.lib.fmx_afm_list_workspace_bytes(tb.c_struct(), C.byref(eng.c_afm), Bl, G))
    assert need == int(eng.lib.fmx_afm_workspace_bytes(tb.c_struct(), C.byref(eng.c_afm), B)) + 16
    ws = torch.zeros(need // 4 + 64, dtype=torch.int32, device="cuda")
    ws[need // 4:] = NAN_WORD
    logit = torch.full((B + 16,), NAN_WORD, dtype=torch.int32, device="cuda")
    hyp = _hyper(rule)
    opt.c.step = opt.step
    rc = eng.lib.fmx_afm_list_step_opt(tb.c_struct(), hyp.ref(), L.RULES[rule], C.byref(eng.c_afm), idx_d.data_ptr(), xv_d.data_ptr(), Bl, G,
                                       1.0 / Bl, ws.data_ptr(), need, eng.grad.data_ptr(), opt.ref(), logit.data_ptr(),
                                       eng.loss_out.data_ptr(), eng.error.data_ptr(), None)
    L.check(rc)
    torch.cuda.synchronize()
    assert int(eng.error.item()) == 0 and np.isfinite(float(eng.loss_out.item()))
    assert bool((ws[need // 4:] == NAN_WORD).all()), "written past the workspace"
    assert bool((logit[B:] == NAN_WORD).all()), "written past logit_out"
    assert bool(torch.isfinite(logit[:B].view(torch.float32)).all())
    # one byte less is refused before anything is launched
    rc = eng.lib.fmx_afm_list_step_opt(tb.c_struct(), hyp.ref(), L.RULES[rule], C.byref(eng.c_afm), idx_d.data_ptr(), xv_d.data_ptr(), Bl, G,
                                       1.0 / Bl, ws.data_ptr(), need - 1, eng.grad.data_ptr(), opt.ref(), logit.data_ptr(),
                                       eng.loss_out.data_ptr(), eng.error.data_ptr(), None)
    assert rc == L.ERR_SHAPE


# ---- 6. the stream is its steps ----
@pytest.mark.parametrize("F,k,t,Bl,G", [(12, 10, 4, 33, 3), (39, 16, 16, 16, 5)])
@pytest.mark.parametrize("rule", RULES)
def test_list_stream_equals_its_steps_bit_for_bit(rule, F, k, t, Bl, G):
    n_pool, n_steps = 3, 5
    sizes = list_sizes(F, G, 31)
    pool = [list_batch(sizes, Bl, G, seed=300 + j, xv_kind="random", hot=True) for j in range(n_pool)]
    idx_pool = torch.from_numpy(np.stack([p[0] for p in pool])).cuda().contiguous()
    xv_pool = torch.from_numpy(np.stack([p[1] for p in pool])).cuda().contiguous()
    hyp = _hyper(rule)
    moments = LAYOUT[rule] == "moments"

    tb, params, eng, opt = _stream_start(rule, sizes, k, t, Bl * G, seed=41)
    losses = torch.zeros(n_steps, device="cuda")
    for s in range(n_steps):
        eng.list_step(hyp, rule, idx_pool[s % n_pool], G, xv_pool[s % n_pool], opt=opt)
        losses[s] = eng.loss_out[0]
    want = _everything(tb, params, opt, losses)
    assert int(eng.error.item()) == 0 and opt.step == 2 + n_steps and tb.step == (n_steps if moments else 0)
    assert bool(torch.isfinite(want["losses"]).all()) and bool((want["losses"] > 0).all())

    for split in ((n_steps,), (2, 3)):
        tb, params, eng, opt = _stream_start(rule, sizes, k, t, Bl * G, seed=41)
        losses = torch.full((n_steps,), -1.0, device="cuda")
        done = 0
        for n in split:
            # a call starts at batch 0 of the pool it is given: the second call's pool is the first's, rotated by `done`
            order = [(done + j) % n_pool for j in range(n_pool)]
            eng.list_stream(hyp, rule, idx_pool[order].contiguous(), xv_pool[order].contiguous(), Bl, G, n, opt, losses=losses[done:])
            done += n
        got = _everything(tb, params, opt, losses)
        assert int(eng.error.item()) == 0 and opt.step == 2 + n_steps and tb.step == (n_steps if moments else 0)
        _assert_same(got, want, f"{rule} list stream {split}")


# ---- 7. the online run is one-list steps ----
@pytest.mark.parametrize("F,k,t,G", [pytest.param(5, 3, 4, 3, id="kp4-G3"), pytest.param(12, 10, 4, 5, id="kp16-G5")])
@pytest.mark.parametrize("rule", RULES)
def test_list_online_run_equals_one_list_steps_bit_for_bit(rule, F, k, t, G):
    N = 24
    sizes = [int(s) for s in np.random.default_rng(F).integers(2, 6, size=F)]
    sizes[-1] = G + 2
    idx, xv, rows = list_batch(sizes, N, G, seed=500 + F, xv_kind="random")
    hyp = _hyper(rule)
    moments = LAYOUT[rule] == "moments"

    tb, params, eng, opt = _stream_start(rule, sizes, k, t, G, seed=41)
    idx_d, xv_d, _ = eng.to_device(idx, xv)
    logits, losses = torch.zeros(N * G, device="cuda"), torch.zeros(N, device="cuda")
    for i in range(N):
        sl = slice(G * i, G * (i + 1))
        eng.forward(hyp, idx_d[sl], xv_d[sl])                                      # the list's logits before its update
        before = eng.logit[:G].clone()
        eng.list_step(hyp, rule, idx_d[sl], G, xv_d[sl], inv_b=1.0, opt=opt)
        assert torch.equal(eng.logit[:G], before)
        logits[sl] = eng.logit[:G]
        losses[i] = eng.loss_out[0]
    want = _everything(tb, params, opt, losses, dict(logits=logits, grad=eng.grad, error=eng.error))
    assert opt.step == 2 + N and tb.step == (N if moments else 0) and int(want["error"]) == 0
    assert bool(torch.isfinite(want["losses"]).all()) and bool((want["losses"] > 0).all())

    for split in ((N,), (1, 15, 8)):
        tb, params, eng, opt = _stream_start(rule, sizes, k, t, G, seed=41)
        logits, losses = torch.full((N * G,), -7.0, device="cuda"), torch.full((N,), -7.0, device="cuda")
        o = 0
        for n in split:
            eng.list_online_run(hyp, rule, idx_d[G * o:G * (o + n)], G, xv_d[G * o:G * (o + n)], opt, logits=logits[G * o:],
                                losses=losses[o:])
            o += n
        got = _everything(tb, params, opt, losses, dict(logits=logits, grad=eng.grad, error=eng.error))
        assert opt.step == 2 + N and tb.step == (N if moments else 0)
        _assert_same(got, want, f"{rule} list online run {split}")


# ---- the one queue of steps at its smallest (test_afm_stream_gpu's SMALL): 3 lists of G = 3 a step, a pool of 3 walked twice and
#      a step more, 5 lists online (the list run is always queued) -- without xv, and from a stream that is not torch's default ----
@functools.lru_cache(maxsize=None)
def _small_lists(rule, with_xv):
    """(sizes, pool and stream on the device, what the single list steps on the default stream leave): computed once per case"""
    F, k, t, Bl, n_pool, n_steps, N = (SMALL[kk] for kk in ("F", "k", "t", "units", "n_pool", "n_steps", "N"))
    G = Bl
    sizes, kind = list_sizes(F, G, 31), "random" if with_xv else "ones"
    pool = [list_batch(sizes, Bl, G, seed=300 + j, xv_kind=kind) for j in range(n_pool)]
    idx_pool = torch.from_numpy(np.stack([p[0] for p in pool])).cuda().contiguous()
    xv_pool = torch.from_numpy(np.stack([p[1] for p in pool])).cuda().contiguous() if with_xv else None
    hyp = _hyper(rule)
    tb, params, eng, opt = _stream_start(rule, sizes, k, t, Bl * G, seed=41)
    losses = torch.zeros(n_steps, device="cuda")
    for s in range(n_steps):
        j = s % n_pool
        eng.list_step(hyp, rule, idx_pool[j], G, None if xv_pool is None else xv_pool[j], opt=opt)
        losses[s] = eng.loss_out[0]
    want_stream = _everything(tb, params, opt, losses)
    assert int(eng.error.item()) == 0 and opt.step == 2 + n_steps

    idx, xv, _ = list_batch(sizes, N, G, seed=340, xv_kind=kind)
    tb, params, eng, opt = _stream_start(rule, sizes, k, t, G, seed=41)
    idx_d, xv_d, _ = eng.to_device(idx, xv)
    logits, losses = torch.zeros(N * G, device="cuda"), torch.zeros(N, device="cuda")
    for i in range(N):
        sl = slice(G * i, G * (i + 1))
        eng.list_step(hyp, rule, idx_d[sl], G, None if xv_d is None else xv_d[sl], inv_b=1.0, opt=opt)
        logits[sl] = eng.logit[:G]                                 # (the step's own forward: the logits before its update)
        losses[i] = eng.loss_out[0]
    want_online = _everything(tb, params, opt, losses, dict(logits=logits, grad=eng.grad, error=eng.error))
    assert opt.step == 2 + N and int(want_online["error"]) == 0
    for want in (want_stream, want_online):
        assert bool(torch.isfinite(want["losses"]).all()) and bool((want["losses"] > 0).all())
    return sizes, G, (idx_pool, xv_pool), (idx_d, xv_d), want_stream, want_online


@SMALL_CASES
@SMALL_RULES
def test_small_list_stream_is_its_single_steps(rule, with_xv, side):
    k, t, Bl, n_steps = (SMALL[kk] for kk in ("k", "t", "units", "n_steps"))
    sizes, G, (idx_pool, xv_pool), _, want, _ = _small_lists(rule, with_xv)
    tb, params, eng, opt = _stream_start(rule, sizes, k, t, Bl * G, seed=41)
    losses = torch.full((n_steps,), -1.0, device="cuda")
    issue(side, lambda st: eng.list_stream(_hyper(rule), rule, idx_pool, xv_pool, Bl, G, n_steps, opt, losses=losses, stream=st))
    got = _everything(tb, params, opt, losses)
    assert int(eng.error.item()) == 0 and opt.step == 2 + n_steps and tb.step == (n_steps if LAYOUT[rule] == "moments" else 0)
    _assert_same(got, want, f"{rule} list stream")


@SMALL_CASES
@SMALL_RULES
def test_small_list_online_run_is_its_single_steps(rule, with_xv, side):
    """Two calls of 1 and N - 1 lists: the second call's logits start G floats in, its losses one."""
    k, t, N = (SMALL[kk] for kk in ("k", "t", "N"))
    sizes, G, _, (idx_d, xv_d), _, want = _small_lists(rule, with_xv)
    tb, params, eng, opt = _stream_start(rule, sizes, k, t, G, seed=41)
    logits, losses = torch.full((N * G,), -7.0, device="cuda"), torch.full((N,), -7.0, device="cuda")
    hyp = _hyper(rule)

    def run(st):
        for o, n in ((0, 1), (1, N - 1)):
            eng.list_online_run(hyp, rule, idx_d[G * o:G * (o + n)], G, None if xv_d is None else xv_d[G * o:G * (o + n)], opt,
                                logits=logits[G * o:], losses=losses[o:], stream=st)
    issue(side, run)
    got = _everything(tb, params, opt, losses, dict(logits=logits, grad=eng.grad, error=eng.error))
    assert opt.step == 2 + N and tb.step == (N if LAYOUT[rule] == "moments" else 0)
    _assert_same(got, want, f"{rule} list online run")


def test_list_online_run_of_zero_lists_touches_nothing():
    rule, F, k, t, G = "adam", 5, 3, 4, 4
    sizes = list_sizes(F, G, 7)
    tb, params, eng, opt = _stream_start(rule, sizes, k, t, G, seed=3)
    before = _everything(tb, params, opt, torch.zeros(1), dict(grad=eng.grad))
    fmx = _fmx()
    L, hyp = fmx._lib, _hyper(rule)
    rc = eng.lib.fmx_afm_list_online_run(tb.c_struct(), hyp.ref(), L.RULES[rule], C.byref(eng.c_afm), None, None, 0, G, None, 0, None,
                                         opt.ref(), None, None, None, None)
    assert rc == L.OK
    after = _everything(tb, params, opt, torch.zeros(1), dict(grad=eng.grad))
    _assert_same(after, before, "N = 0")
    assert opt.step == 2 and tb.step == 0


# ---- 8. the classes ----
def _list_rows_of(sizes, pos, xv, neg):
    """The global rows [B G, F] and values of the positives and their explicit negatives [B, n_neg, 1], the positive first"""
    G = 1 + neg.shape[1]
    idx = np.repeat(pos, G, axis=0)
    for j in range(1, G):
        idx[j::G, -1] = neg[:, j - 1, 0]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return idx.astype(np.int64) + offs[:-1], np.repeat(xv, G, axis=0), G


@pytest.mark.parametrize("sampled", [False, True], ids=["explicit_negatives", "sampled_negatives"])
@pytest.mark.parametrize("rule", ["adam", "ftrl"])
def test_class_fit_lists_is_the_engine_list_step(rule, sampled):
    import fmx
    sizes, k, t, B, n_neg = [20, 300, 5, 64, 9, 40], 8, 4, 50, 3
    a, b = _models(2, sizes, k, t, rule)
    pos, xv, fields, neg = _class_data(sizes, B, seed=3, n_neg=n_neg)
    for step in range(2):
        if sampled:
            la = a.fit_lists(pos, xv, fields, n_neg=n_neg, generator=torch.Generator().manual_seed(7 + step), attention=True)
            idx_d, xv_d, _ = b._inputs(pos, xv)
            negs = fmx.pairwise.sample_negatives(idx_d, fields, [sizes[-1]], n_neg=n_neg, generator=torch.Generator().manual_seed(7 + step))
        else:
            la = a.fit_lists(pos, xv, fields, negatives=neg, attention=True)
            idx_d, xv_d, _ = b._inputs(pos, xv)
            negs = neg
        rows, vals = fmx.pairwise.assemble_lists(idx_d, xv_d, fields, negs)
        assert rows.shape[0] == (1 + n_neg) * B
        b._engine.list_step(b._hyper, rule, rows, 1 + n_neg, vals, opt=b._attn_fused)
        assert torch.equal(la, b._engine.loss_out[0]) and np.isfinite(float(la)) and float(la) > 0
        b._engine.check_error_flag()
    _same_models(a, b)
    assert a._attn_fused.step == 2
    with pytest.raises(ValueError, match="15"):
        a.fit_lists(pos, xv, fields, n_neg=16, attention=True)
    with pytest.raises(NotImplementedError, match="pure FM logit"):
        a.fit_lists(pos, xv, fields, negatives=neg)


@pytest.mark.parametrize("rule", ["adam", "sgd"])
def test_class_fit_lists_with_and_without_the_fused_optimizer(rule):
    """fused_optimizer=False splits the step as fit_pairs does: the same table step (bit for bit), the attention parameters' rule
    on torch.  Both settings' attention parameters are held to float64 on afm_list_f64's gradient with
    test_afm_stream_gpu.check_attention, as test_class_fit_pairs_with_and_without_the_fused_optimizer holds fit_pairs'."""
    sizes, k, t, B, n_neg = _sizes(14, 14), 8, 8, 64, 2
    lr = HYP["lr"] if rule == "sgd" else 0.01
    (fused,), (plain,) = _models(1, sizes, k, t, rule, True, lr), _models(1, sizes, k, t, rule, False, lr)
    pos, xv, fields, neg = _class_data(sizes, B, seed=9, n_neg=n_neg)
    F32 = lambda v: float(np.float32(v))
    b1, b2 = fused._betas()
    h = dict(lr=F32(lr), eps=F32(fused._adam["eps"]), beta1=b1, beta2=b2)
    V, w, bias, params = _model_state(fused)
    rows, x, G = _list_rows_of(sizes, pos, xv, neg)
    ref = afm_list_f64(V, w, bias, params, k, t, rows, G, x)
    before_f = opt_state(fused._attn_flat, fused._attn_fused)
    before_p = (plain._attn_flat.detach().double().cpu().numpy(),) + (_attn_state(plain)[1:] if rule == "adam" else (None, None))
    lf = fused.fit_lists(pos, xv, fields, negatives=neg, attention=True)
    lp = plain.fit_lists(pos, xv, fields, negatives=neg, attention=True)
    assert torch.equal(lf, lp)
    assert_within_f64(float(lf), ref["loss"], float(np.sum(ref["floor_loss"])) / B, "mean list loss")
    sf, sp = fused.state_dict(), plain.state_dict()
    for key in sf:
        if "embeddings" in key or key == "bias":
            assert torch.equal(sf[key], sp[key]), key
    check_attention(rule, h, 1, before_f, opt_state(fused._attn_flat, fused._attn_fused), ref, f"{rule} fused")
    after_p = (plain._attn_flat.detach().double().cpu().numpy(),) + (_attn_state(plain)[1:] if rule == "adam" else (None, None))
    check_attention(rule, h, 1, before_p, after_p, ref, f"{rule} torch")


@pytest.mark.parametrize("rule", ["adam", "ftrl"])
def test_class_list_experiment_equals_the_loop_and_survives_pickling(rule):
    sizes, k, t, N, n_neg = [4, 3, 5, 7], 4, 4, 30, 3
    G = 1 + n_neg
    a, b = _models(2, sizes, k, t, rule)
    pos, xv, fields, neg = _class_data(sizes, N, seed=21, n_neg=n_neg)
    half = N // 2
    ra = a.run_list_experiment(pos[:half], xv[:half], fields, negatives=neg[:half], attention=True)
    a2 = pickle.loads(pickle.dumps(a))                     # a round trip in the middle of the run
    ra2 = [m.run_list_experiment(pos[half:], xv[half:], fields, negatives=neg[half:], attention=True) for m in (a, a2)]
    assert ra2[0][1:] == ra2[1][1:]
    _same_models(a, a2)
    # the host loop of one-list steps on a second model: correct is rank 0, read from the logits before the update
    pred = []
    for i in range(N):
        b.fit_lists(pos[i:i + 1], xv[i:i + 1], fields, negatives=neg[i:i + 1], attention=True)
        z = b._engine.logit[:G]
        pred.append(not bool((z[1:] >= z[0]).any()))
    _same_models(a, b)
    assert a._attn_fused.step == N
    pred = np.array(pred)
    for r, p in ((ra, pred[:half]), (ra2[0], pred[half:])):
        n = len(p)
        assert r[3] == {"correct": int(p.sum()), "wrong": int(n - p.sum())}
        assert r[2] == [float(np.cumsum(p)[i] / (i + 1) * 100) for i in sorted({0, n - 1})] and r[1] == r[2][-1]
    # fused_optimizer=False: the same protocol as a host loop; zero lists
    (c,) = _models(1, sizes, k, t, rule, fused=False)
    rc = c.run_list_experiment(pos[:5], xv[:5], fields, negatives=neg[:5], attention=True)
    assert sum(rc[3].values()) == 5 and 0 <= rc[1] <= 100
    rz = a.run_list_experiment(pos[:0], xv[:0], fields, negatives=neg[:0], attention=True)
    assert rz[1:] == (0.0, [], {"correct": 0, "wrong": 0})


# ---- 9. it trains ----
@pytest.mark.parametrize("F,k,t", [(4, 4, 4), (12, 10, 4)])
def test_sixty_list_steps_bring_the_loss_down(F, k, t):
    """Sixty sgd steps (lr 0.05) on one fixed batch of 64 lists of 1 + 4: the kernels' loss falls by at least half of what the
    float64 restatement, iterated on the same data from the same state, falls by.  Then the trained model is evaluated by rank."""
    sizes, Bl, lr, T, n_neg = list_sizes(F, 5, F), 64, 0.05, 60, 4
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
    pos, xv, fields, neg = _class_data(sizes, Bl, seed=F + 1, n_neg=n_neg)
    V, w, bias, params = (np.asarray(a, np.float64) for a in _model_state(m))
    rows, x, G = _list_rows_of(sizes, pos, xv, neg)
    want = []
    for _ in range(T):
        r = afm_list_f64(V, w, float(bias), params, k, t, rows, G, x)
        want.append(r["loss"])
        V, w, params = V - lr * r["dV"], w - lr * r["dw"], params - lr * r["dparams"]
    bias_before = m._table.bias.cpu().numpy().copy()
    got = [float(m.fit_lists(pos, xv, fields, negatives=neg, attention=True)) for _ in range(T)]
    print(f"F={F}: float64 {want[0]:.4f} -> {want[-1]:.4f}, kernels {got[0]:.4f} -> {got[-1]:.4f}")
    assert want[0] - want[-1] > 0
    assert got[0] - got[-1] >= 0.5 * (want[0] - want[-1]), (got[0], got[-1], want[0], want[-1])
    np.testing.assert_array_equal(bits(m._table.bias.cpu().numpy()), bits(bias_before), err_msg="sixty list steps moved the bias")
    metrics = m.evaluate_ranking(pos, xv, fields, pos[:, -1].astype(np.int64))
    assert metrics and all(np.isfinite(float(v)) for v in metrics.values()), metrics
