"""The attentional FM kernels (fmx_afm_forward, fmx_afm_step, fmx_fm_update_occ) against the float64 restatement in
tests/afm_f64.py: logits and losses within 1e-5 + the fp32 floor, one step of every update rule, determinism, bad arguments;
the step across the pair-tile geometries, every BWD kp and t = 1 .. 64, the rules at a multi-tile shape, five-step adam /
adagrad trajectories, the FTRL / moments / sigmoid-loss forwards, and AFMAdam's persistent optimizers step by step."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from afm_f64 import U32, afm_f64, live_params, tiles  # noqa: E402
from helpers import assert_within_f64  # noqa: E402
from test_adaptive_rules_cpu import rule_apply  # noqa: E402
from test_adaptive_rules_gpu import HYP as AHYP, _floors, state_of  # noqa: E402

pytestmark = pytest.mark.gpu

HYP = dict(lr=0.05, eps=1e-8, alpha=0.05, beta=1.0, l1=0.001, l2=0.01, beta1=0.9, beta2=0.999)


def _fmx():
    import fmx
    return fmx


def make(sizes, k, t, layout="weights", seed=0, scale=0.4):
    """A table and attention parameters with seeded weights -> (table, params_dev, state); state holds the fp32 weights the
    kernels see (V [R, k], w [R], bias) and the flat params."""
    fmx = _fmx()
    rng = np.random.default_rng(seed)
    R = int(sum(sizes))
    V = (rng.normal(size=(R, k)) * scale).astype(np.float32)
    w = (rng.normal(size=R) * 0.3).astype(np.float32)
    ftrl = {kk: HYP[kk] for kk in ("alpha", "beta", "l1", "l2")}
    tb = fmx.FlatTable(sizes, k, layout=layout, ftrl=ftrl)
    if layout == "ftrl":
        from fmx.table import ftrl_z_for_weight_torch
        zV = ftrl_z_for_weight_torch(torch.from_numpy(V), ftrl)
        zw = ftrl_z_for_weight_torch(torch.from_numpy(w), ftrl)
        tb.load_ftrl_state(zV, torch.full_like(zV, 0.1), zw, torch.full_like(zw, 0.1))
        tb.bias[0], tb.bias[1] = 0.0, 0.1
    else:
        tb.rows[:, :k] = torch.from_numpy(V).cuda()
        tb.rows[:, tb.kp] = torch.from_numpy(w).cuda()
        tb.bias[0] = 0.2
    torch.cuda.synchronize()
    n = t * k + 2 * t + k
    params = (rng.normal(size=n) * 0.5).astype(np.float32)
    st = dict(V=tb.V.detach().cpu().numpy()[:, :k].copy(), w=tb.w.detach().cpu().numpy().copy(),
              bias=float(tb.bias_weight()), params=params)
    return tb, torch.from_numpy(params).cuda(), st


def batch(sizes, B, seed=1, xv_kind="ones", hot=False):
    rng = np.random.default_rng(seed)
    idx = np.stack([rng.integers(0, s, size=B) for s in sizes], axis=1).astype(np.int32)
    if hot:
        idx[:, 0] = rng.integers(0, 2, size=B)          # two rows of field 0 take every occurrence: runs cross 64-entry tiles
    y = (rng.uniform(size=B) < 0.4).astype(np.float32)
    xv = None
    if xv_kind == "random":
        xv = rng.uniform(0.2, 1.8, size=idx.shape).astype(np.float32)
    elif xv_kind == "zeros":
        xv = rng.uniform(0.2, 1.8, size=idx.shape).astype(np.float32)
        xv[:, ::3] = 0.0
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    rows = idx.astype(np.int64) + offs[:-1][None, :]
    return idx, xv, y, rows


def engine(tb, params, t, B):
    from fmx.afm import AFMEngine
    return AFMEngine(tb, params, t, max_batch=B)


FORWARD_CASES = [  # (F, k, t, B, xv)
    (2, 4, 1, 1, "ones"), (3, 10, 4, 63, "random"), (10, 16, 16, 64, "zeros"), (39, 16, 16, 4097, "ones"),
    (64, 64, 64, 63, "random"), (39, 10, 64, 64, "zeros"), (64, 4, 1, 64, "ones"), (10, 64, 4, 1, "random"),
    (3, 16, 64, 4097, "random"),
]


@pytest.mark.parametrize("F,k,t,B,xv_kind", FORWARD_CASES)
def test_afm_forward_matches_f64(F, k, t, B, xv_kind):
    fmx = _fmx()
    sizes = [int(s) for s in np.random.default_rng(F).integers(2, 300, size=F)]
    tb, params, st = make(sizes, k, t, seed=F + k)
    idx, xv, y, rows = batch(sizes, B, seed=B, xv_kind=xv_kind)
    eng = engine(tb, params, t, B)
    idx_d, xv_d, y_d = eng.to_device(idx, xv, y)
    eng.forward(fmx.Hyper(**HYP), idx_d, xv_d, y_d, loss="logits")
    ref = afm_f64(st["V"], st["w"], st["bias"], st["params"], k, t, rows, xv, y)
    assert_within_f64(eng.logit[:B].cpu().numpy(), ref["logit"], ref["floor_logit"], "logit")
    assert_within_f64(eng.loss_b[:B].cpu().numpy(), ref["loss_b"], ref["floor_loss"], "loss")
    assert int(eng.error.item()) == 0


def test_afm_forward_flags_bad_index():
    fmx = _fmx()
    sizes = [5, 7, 9]
    tb, params, st = make(sizes, 8, 4)
    idx, xv, y, rows = batch(sizes, 64)
    idx[3, 1] = 7                                        # outside field 1
    eng = engine(tb, params, 4, 64)
    idx_d, _, _ = eng.to_device(idx)
    eng.forward(fmx.Hyper(**HYP), idx_d)
    valid = np.ones(idx.shape, bool)
    valid[3, 1] = False
    rows[3, 1] = 0
    ref = afm_f64(st["V"], st["w"], st["bias"], st["params"], 8, 4, rows, valid=valid)
    assert_within_f64(eng.logit[:64].cpu().numpy(), ref["logit"], ref["floor_logit"], "logit")
    with pytest.raises(IndexError):
        eng.check_error_flag()


@pytest.mark.parametrize("layout,F,k,t,B", [
    pytest.param("ftrl", 39, 16, 16, 1025, id="ftrl-F39-t16"), pytest.param("moments", 39, 16, 64, 300, id="moments-F39-t64"),
    pytest.param("ftrl", 64, 64, 64, 64, id="ftrl-F64-kp64"), pytest.param("moments", 64, 64, 8, 130, id="moments-F64-kp64")])
def test_afm_forward_layouts_match_f64(layout, F, k, t, B):
    """The FTRL-layout forward (k_afm<KP, true, false>: the bias derived from its (z, n) pair in the kernel) and the
    moments-layout forward (wider rows) against afm_f64 on the derived weights, multi-tile."""
    fmx = _fmx()
    sizes = _sizes(F, F + 1)
    tb, params, st = make(sizes, k, t, layout=layout, seed=F + t)
    if layout == "ftrl":                 # z outside the L1 dead zone: the derived bias (about 0.011) is far from the raw z
        tb.bias[0], tb.bias[1] = -0.3, 0.1
        st["bias"] = float(tb.bias_weight())
        assert abs(st["bias"]) > 0.005 and abs(st["bias"] - float(tb.bias[0])) > 0.1
    idx, xv, y, rows = batch(sizes, B, seed=B + F, xv_kind="random")
    eng = engine(tb, params, t, B)
    idx_d, xv_d, y_d = eng.to_device(idx, xv, y)
    eng.forward(fmx.Hyper(**HYP), idx_d, xv_d, y_d, loss="logits")
    ref = afm_f64(st["V"], st["w"], st["bias"], st["params"], k, t, rows, xv, y, chunk=_chunk(F, k, t))
    assert_within_f64(eng.logit[:B].cpu().numpy(), ref["logit"], ref["floor_logit"], "logit")
    assert_within_f64(eng.loss_b[:B].cpu().numpy(), ref["loss_b"], ref["floor_loss"], "loss")
    assert int(eng.error.item()) == 0


@pytest.mark.parametrize("F,k,t,B", [(3, 4, 4, 63), (39, 16, 16, 1025)])
def test_afm_forward_sigmoid_loss_matches_f64(F, k, t, B):
    """fmx_afm_forward with FMX_LOSS_BCE_SIGMOID: the per-sample BCE with logits of sigmoid(logit)."""
    fmx = _fmx()
    sizes = _sizes(F, F + 2)
    tb, params, st = make(sizes, k, t, seed=F)
    idx, xv, y, rows = batch(sizes, B, seed=B, xv_kind="random")
    eng = engine(tb, params, t, B)
    idx_d, xv_d, y_d = eng.to_device(idx, xv, y)
    eng.forward(fmx.Hyper(**HYP), idx_d, xv_d, y_d, loss="sigmoid")
    ref = afm_f64(st["V"], st["w"], st["bias"], st["params"], k, t, rows, xv, y, loss="sigmoid", chunk=_chunk(F, k, t))
    assert_within_f64(eng.logit[:B].cpu().numpy(), ref["logit"], ref["floor_logit"], "logit")
    assert_within_f64(eng.loss_b[:B].cpu().numpy(), ref["loss_b"], ref["floor_loss"], "sigmoid loss")
    logits = afm_f64(st["V"], st["w"], st["bias"], st["params"], k, t, rows, xv, y, chunk=_chunk(F, k, t))
    assert np.max(np.abs(ref["loss_b"] - logits["loss_b"])) > 0.05        # the two losses are told apart


# ---- one step: the rules in float64 on the f64 gradient; the tolerance is the rule's response to the gradient's own bound ----
def _rule_f64(rule, p, g):
    if rule == "sgd":
        return p - HYP["lr"] * g
    if rule == "signadam":
        return p - HYP["lr"] * g / (np.abs(g) + HYP["eps"])
    if rule == "adagrad":                                 # first step from G = 0 (torch.optim.Adagrad)
        return p - HYP["lr"] * g / (np.sqrt(g * g) + HYP["eps"])
    if rule == "adam":                                    # first step from m = v = 0 (torch.optim.SparseAdam)
        b1, b2 = float(np.float32(HYP["beta1"])), float(np.float32(HYP["beta2"]))
        m, v = (1 - b1) * g, (1 - b2) * g * g
        return p - HYP["lr"] * np.sqrt(1 - b2) / (1 - b1) * m / (np.sqrt(v) + HYP["eps"])
    raise ValueError(rule)


def _check_rule(rule, got, before, g, g_tol, what):
    ref = _rule_f64(rule, before, g)
    lo, hi = _rule_f64(rule, before, g - g_tol), _rule_f64(rule, before, g + g_tol)
    tol = np.abs(hi - lo) / 2 + 1e-5 * np.abs(ref - before) + 8 * U32 * (np.abs(ref) + np.abs(before))
    err = np.abs(np.asarray(got, np.float64) - ref)
    bad = err > tol
    assert not np.any(bad), f"{what}: {int(np.sum(bad))}/{np.size(bad)} off, worst err/tol {float(np.max(err / np.maximum(tol, 1e-300))):.2f}"


def _touched(rows, R):
    m = np.zeros(R, bool)
    m[np.unique(rows)] = True
    return m


def _chunk(F, k, t, elems=1 << 22):
    """Samples per afm_f64 evaluation: [chunk, P, max(k, t)] intermediates of about 4 M doubles."""
    return max(1, elems // (F * (F - 1) // 2 * max(k, t)))


def _live(tb, params, st, k, t, rows, xv):
    """The attention parameters with no dead unit (afm_f64.live_params), on the device and in the state."""
    fixed = live_params(st["params"], st["V"], k, t, rows, xv, chunk=_chunk(rows.shape[1], k, t))
    params.copy_(torch.from_numpy(fixed))
    st["params"] = fixed


def assert_exercised(ref, F, what):
    """The case's float64 gradients reach every attention unit and every pair tile of the kernels."""
    assert ref["unit_live"].all(), f"{what}: dead attention units {np.flatnonzero(~ref['unit_live'])}"
    dead = [i for i, (pb, n) in enumerate(tiles(F)) if not ref["pair_live"][pb:pb + n].any()]
    assert not dead, f"{what}: pair tiles {dead} of {len(tiles(F))} take no gradient"


def _step_and_check(rule, sizes, k, t, B, xv_kind="random", hot=False, seed=0, live=False, bad=None):
    """live: no dead attention unit, and every pair tile asserted to carry gradient; bad = (sample, field): that index is put
    outside its field -- the row is absent, the error word raised, the gradients those of afm_f64(valid=...)."""
    fmx = _fmx()
    layout = {"sgd": "weights", "signadam": "weights", "ftrl": "ftrl", "adam": "moments", "adagrad": "moments"}[rule]
    tb, params, st = make(sizes, k, t, layout=layout, seed=seed)
    idx, xv, y, rows = batch(sizes, B, seed=seed + 7, xv_kind=xv_kind, hot=hot)
    valid = None
    if bad is not None:
        valid = np.ones(idx.shape, bool)
        valid[bad] = False
        idx[bad] = sizes[bad[1]] + 3                     # outside its field
        rows[bad] = 0                                    # (x = 0 there: the f64 statement takes nothing from it)
    chunk = _chunk(len(sizes), k, t)
    if live:
        x = np.ones(idx.shape) if xv is None else xv
        _live(tb, params, st, k, t, rows, x if valid is None else x * valid)
    eng = engine(tb, params, t, B)
    rows_before = tb.rows.detach().cpu().numpy().copy()
    bias_before = tb.bias.detach().cpu().numpy().copy()
    idx_d, xv_d, y_d = eng.to_device(idx, xv, y)
    eng.step(fmx.Hyper(**HYP), rule, idx_d, xv_d, y_d)
    torch.cuda.synchronize()
    assert int(eng.error.item()) == (0 if bad is None else 1)
    ref = afm_f64(st["V"], st["w"], st["bias"], st["params"], k, t, rows, xv, y, valid=valid, chunk=chunk)
    if live:
        assert_exercised(ref, len(sizes), f"F={len(sizes)} k={k} t={t} B={B}")
    assert_within_f64(float(eng.loss_out.item()), ref["loss"], float(np.mean(ref["floor_loss"])), "mean loss")
    assert_within_f64(eng.grad.cpu().numpy(), ref["dparams"], ref["fl_dparams"], "attention gradient")
    R = int(sum(sizes))
    u = _touched(rows if valid is None else rows[valid], R)
    rows_after = tb.rows.detach().cpu().numpy()
    np.testing.assert_array_equal(rows_after[~u], rows_before[~u], err_msg="untouched rows moved")
    gV, gw = ref["dV"][u], ref["dw"][u]
    tV, tw = 1e-5 * np.abs(gV) + ref["fl_dV"][u], 1e-5 * np.abs(gw) + ref["fl_dw"][u]
    kp = tb.kp
    if rule == "ftrl":   # the state (z, n) of the embeddings; n' = n + g^2, z' = z + g - (sqrt(n') - sqrt(n)) / alpha * V
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
    _check_rule(rule, np.float64(tb.bias[0].item()), np.float64(bias_before[0]), ref["dbias"],
                1e-5 * abs(ref["dbias"]) + ref["fl_dbias"], f"{rule} bias")


def test_afm_step_sgd():
    _step_and_check("sgd", [30, 200, 7, 1000, 50, 3, 90, 400, 12, 60], 16, 8, 512)


def test_afm_step_sgd_hot_rows_cross_tiles():
    # field 0: 2 rows hit by all 1,000 samples -- runs of ~500 occurrences cross 64-entry tiles and take the hand-off
    _step_and_check("sgd", [5, 40, 3, 700], 10, 4, 1000, xv_kind="ones", hot=True)


def test_afm_step_sgd_split_large_field():
    # a field of 2^20 + 5 rows at B = 4096: (index, sample) needs 33 bits, so the table cuts the field into sort pieces
    sizes = [(1 << 20) + 5, 3, 50]
    tb, _, _ = make(sizes, 8, 4)
    tb.ensure_sort_split(4096)
    assert tb._sort_split is not None
    del tb
    _step_and_check("sgd", sizes, 8, 4, 4096, xv_kind="random", seed=3)


@pytest.mark.parametrize("rule", ["signadam", "adam", "adagrad", "ftrl"])
def test_afm_step_rules(rule):
    _step_and_check(rule, [40, 9, 300, 17, 2, 80, 5, 120], 16, 16, 256, hot=True, seed=5)


CRITEO_SIZES = [63, 113, 126, 51, 224, 148, 100, 79, 104, 9, 32, 57, 82, 1457, 555, 176373, 129683, 305, 19, 11887,
                632, 3, 41738, 5170, 175446, 3170, 27, 11356, 165602, 10, 4641, 2030, 4, 172761, 18, 15, 57903, 86,
                44549]    # test_kernels_gpu.py's Criteo-39 fields


def _sizes(F, seed):
    return [int(s) for s in np.random.default_rng(seed).integers(2, 300, size=F)]


# (F, k -> kp, t, B, xv): the pair tiles (at most 64 pairs of whole pair rows), every BWD kp, t = 1 .. 64, and the grid's
# sample walk (B > 1024: a workgroup takes two or more samples).  F = 12 is the smallest two-tile set (63 + 3 pairs).
STEP_GEOMETRY = [
    pytest.param(12, 10, 4, 300, "random", id="F12-k10-t4-B300-two_tiles"),
    pytest.param(13, 3, 1, 1, "ones", id="F13-k3-t1-B1-kp4"),
    pytest.param(39, 16, 16, 4096, "random", id="F39-criteo-k16-t16-B4096-bench"),
    pytest.param(39, 16, 4, 1025, "zeros", id="F39-k16-t4-B1025"),
    pytest.param(39, 16, 64, 1025, "zeros", id="F39-k16-t64-B1025"),
    pytest.param(40, 20, 64, 130, "random", id="F40-k20-t64-B130-kp32"),
    pytest.param(64, 64, 64, 64, "random", id="F64-k64-t64-B64-largest_lds"),
    pytest.param(64, 33, 7, 2500, "ones", id="F64-k33-t7-B2500-kp64"),
    pytest.param(2, 1, 64, 4097, "random", id="F2-k1-t64-B4097-one_pair"),
]


@pytest.mark.parametrize("F,k,t,B,xv_kind", STEP_GEOMETRY)
def test_afm_step_geometry(F, k, t, B, xv_kind):
    """One sgd step against float64 at the shapes the kernels take: loss, attention gradient, every touched row, the
    untouched rows bit for bit; no attention unit dead and every pair tile carrying gradient."""
    sizes = CRITEO_SIZES if B == 4096 and F == 39 else _sizes(F, F + B)
    _step_and_check("sgd", sizes, k, t, B, xv_kind=xv_kind, seed=F + t, live=True)


@pytest.mark.parametrize("rule", ["signadam", "ftrl", "adam", "adagrad"])
def test_afm_step_rules_multi_tile(rule):
    # F = 20: 190 pairs in 4 tiles; two hot rows of field 0 take all 1,000 samples (runs cross 64-entry update tiles)
    _step_and_check(rule, _sizes(20, 20), 16, 16, 1000, hot=True, seed=9, live=True)


def test_afm_step_bad_index_multi_tile():
    """An index outside its field in a three-tile step (F = 16: 54 + 63 + 3 pairs; field 9 is in all three): the row is absent from the forward and the update, the
    flag is raised, the gradients are those of afm_f64(valid=...)."""
    sizes = _sizes(16, 16)
    _step_and_check("sgd", sizes, 8, 8, 300, seed=4, live=True, bad=(17, 9))


# ---- several steps of the persistent rules: every step against rule_apply on the GPU's own state before it ----
# The adaptive rules divide by the row's own gradient scale, so a gradient's absolute noise shows where the row's |g| and G
# are small.  dlogit = sigmoid(logit) - y is rounded absolutely: 1 + exp(-z) to half an ulp of 1 (2^-24), the quotient to
# half an ulp below 1 (2^-25) -- under 2^-23 in units of inv_b, which afm_f64(dz_abs=...) carries into the floors.  (AFMAdam's
# reference initialisation gives logits of +-28, where sigmoid - 1 is that rounding and nothing else.)
DZ_ABS = 2.0 ** -23


def _grad_ex(ref, urows):
    """The f64 gradients of the touched rows and their fp32 noise (1e-5 relative plus the floor), as
    test_adaptive_rules_gpu.assert_step takes them."""
    gV, gw, gb = ref["dV"][urows], ref["dw"][urows], ref["dbias"]
    return dict(gV=gV, gw=gw, gb=gb, gnoise_V=1e-5 * np.abs(gV) + ref["fl_dV"][urows],
                gnoise_w=1e-5 * np.abs(gw) + ref["fl_dw"][urows], gnoise_b=1e-5 * abs(gb) + ref["fl_dbias"])


def _rule_rows(before, urows, ex, rule, h, step):
    """rule_apply on the touched rows and the bias of a moments table's state (test_adaptive_rules_gpu.state_of)."""
    new = {kk: np.array(v, dtype=np.float64, copy=True) for kk, v in before.items()}
    for p, m, v, g in (("V", "mV", "vV", ex["gV"]), ("w", "mw", "vw", ex["gw"])):
        new[p][urows], new[m][urows], new[v][urows] = rule_apply(new[p][urows], new[m][urows], new[v][urows], g, rule, h, step)
    new["bias"], new["mb"], new["vb"] = rule_apply(before["bias"], before["mb"], before["vb"], ex["gb"], rule, h, step)
    return new


def _floors_gn(rule, h, t, g, gn, m2, v2):
    """test_adaptive_rules_gpu._floors with the second-order term of v's: (|g| + gn)^2 - g^2 = 2 |g| gn + gn^2.  The
    first-order 2 |g| gn it has is short where gn is not small against |g| -- a unit on its relu kink moves the gradient of
    the rows it touches by a whole term (afm_f64's kink floor)."""
    fp, fm, fv = _floors(rule, h, t, g, gn, m2, v2)
    return fp, fm, fv + (1 - h["beta2"] if rule == "adam" else 1.0) * gn * gn


def _assert_rows(before, after, ref, urows, ex, rule, h, t, what):
    """assert_step on a moments table with _floors_gn: untouched rows bit for bit, the deltas within 1e-5 plus the floors."""
    untouched = np.setdiff1d(np.arange(before["V"].shape[0]), urows)
    for kk in ("V", "w", "mV", "vV", "mw", "vw"):
        np.testing.assert_array_equal(after[kk][untouched], before[kk][untouched], err_msg=f"{what}: untouched rows moved ({kk})")
    for p, m, v, g, gn in (("V", "mV", "vV", ex["gV"], ex["gnoise_V"]), ("w", "mw", "vw", ex["gw"], ex["gnoise_w"]),
                           ("bias", "mb", "vb", np.float64(ex["gb"]), np.float64(ex["gnoise_b"]))):
        sel = (lambda a: a[urows]) if p != "bias" else (lambda a: a)
        floors = _floors_gn(rule, h, t, g, gn + 1e-30, sel(ref[m]), sel(ref[v]))
        for name, f in zip((p, m, v), floors):
            if not (rule == "adagrad" and name == m):
                _assert_delta(sel(after[name]), sel(before[name]), sel(ref[name]), f, f"{what}/{name}")


def _assert_delta(got, before, ref, floor, what):
    """test_adaptive_rules_gpu.assert_step's comparison: the deltas within 1e-5 relative plus the floors."""
    da, dr = np.asarray(got, np.float64) - before, ref - before
    tol = 1e-5 * np.abs(dr) + floor + 2.5e-7 * np.abs(ref) + 1e-12
    bad = np.abs(da - dr) > tol
    assert not np.any(bad), (f"{what}: {int(np.sum(bad))}/{np.size(bad)} off, worst err/tol "
                             f"{float(np.max(np.abs(da - dr) / tol)):.2f}")


@pytest.mark.parametrize("rule", ["adam", "adagrad"])
def test_afm_step_trajectory_adaptive(rule):
    """Five fmx_afm_step calls on one moments table (F = 20: 4 pair tiles; hot rows): every step's table against rule_apply
    at step count t = s on the GPU's state before it and afm_f64's gradients -- the adam rule's bias correction follows the
    table's count (AFMEngine.step)."""
    fmx = _fmx()
    sizes, k, t, B, T = _sizes(20, 21), 16, 16, 1000, 5
    h = AHYP[rule]
    hyp = fmx.Hyper(lr=h["lr"], eps=h["eps"], beta1=h["beta1"], beta2=h["beta2"])
    tb, params, st = make(sizes, k, t, layout="moments", seed=13)
    data = [batch(sizes, B, seed=100 + s, xv_kind="random", hot=True) for s in range(T)]
    _live(tb, params, st, k, t, data[0][3], data[0][1])
    eng = engine(tb, params, t, B)
    for s, (idx, xv, y, rows) in enumerate(data, start=1):
        before = state_of(tb)
        idx_d, xv_d, y_d = eng.to_device(idx, xv, y)
        eng.step(hyp, rule, idx_d, xv_d, y_d)
        torch.cuda.synchronize()
        assert tb.step == s and int(eng.error.item()) == 0
        ref = afm_f64(before["V"], before["w"], before["bias"], st["params"], k, t, rows, xv, y, chunk=_chunk(20, k, t),
                      dz_abs=DZ_ABS)
        if s == 1:
            assert_exercised(ref, 20, f"{rule} trajectory")
        assert_within_f64(eng.grad.cpu().numpy(), ref["dparams"], ref["fl_dparams"], f"step {s} attention gradient")
        urows = np.unique(rows)
        ex = _grad_ex(ref, urows)
        _assert_rows(before, state_of(tb), _rule_rows(before, urows, ex, rule, h, s), urows, ex, rule, h, s,
                     what=f"{rule} step {s}")


def test_afm_step_is_deterministic():
    fmx = _fmx()
    sizes = [3, 9, 1000, 500, 4, 17, 200, 31] * 4
    outs = []
    for _ in range(2):
        tb, params, st = make(sizes, 16, 16, seed=11)
        idx, xv, y, rows = batch(sizes, 4096, seed=12, hot=True)
        eng = engine(tb, params, 16, 4096)
        idx_d, xv_d, y_d = eng.to_device(idx, xv, y)
        eng.step(fmx.Hyper(**HYP), "sgd", idx_d, xv_d, y_d)
        eng.step(fmx.Hyper(**HYP), "sgd", idx_d, xv_d, y_d)
        torch.cuda.synchronize()
        outs.append((tb.rows.cpu().numpy().copy(), tb.bias.cpu().numpy().copy(), eng.grad.cpu().numpy().copy(),
                     eng.loss_out.cpu().numpy().copy()))
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a, b)


def test_afm_bad_arguments():
    fmx = _fmx()
    lib = fmx._lib.load()
    L = fmx._lib
    hyp = fmx.Hyper(**HYP)

    def ws_bytes(tb, afm, B):
        return int(lib.fmx_afm_workspace_bytes(tb.c_struct(), C.byref(afm), B))

    tb65 = fmx.FlatTable([3] * 65, 4)
    p65 = torch.zeros(4 * 4 + 8 + 4, device="cuda")
    assert ws_bytes(tb65, L.Afm(p65.data_ptr(), 4, 4), 8) == L.ERR_UNSUPPORTED           # F = 65
    tb = fmx.FlatTable([3, 4, 5], 4)
    p = torch.zeros(65 * 4 + 130 + 4, device="cuda")
    assert ws_bytes(tb, L.Afm(p.data_ptr(), 4, 65), 8) == L.ERR_UNSUPPORTED              # t = 65
    afm = L.Afm(p.data_ptr(), 4, 4)
    mapped = fmx.FlatTable([3, 4], 4, field_cols=[0, 1], field_base=[0, 0], n_cols=2)
    assert ws_bytes(mapped, afm, 8) == L.ERR_UNSUPPORTED                                 # an owner table
    idx = torch.zeros((8, 3), dtype=torch.int32, device="cuda")
    y = torch.zeros(8, device="cuda")
    grad = torch.zeros(p.numel(), device="cuda")
    need = ws_bytes(tb, afm, 8)
    assert need > 0
    ws = torch.zeros(need // 4 + 64, dtype=torch.int32, device="cuda")

    def step(afm_, idx_p, nbytes):
        return lib.fmx_afm_step(tb.c_struct(), hyp.ref(), L.RULE_SGD, C.byref(afm_), idx_p, None, y.data_ptr(), 8, 0.125,
                                ws.data_ptr(), nbytes, grad.data_ptr(), None, None, None)

    assert step(afm, idx.data_ptr(), need - 16) == L.ERR_SHAPE                           # short workspace
    assert step(afm, None, need) == L.ERR_ARG                                            # null pointers
    assert step(L.Afm(None, 4, 4), idx.data_ptr(), need) == L.ERR_ARG
    assert lib.fmx_afm_forward(None, C.byref(afm), hyp.ref(), idx.data_ptr(), None, None, 8, 0, 0.125, None, None, None,
                               None) == L.ERR_ARG
    assert lib.fmx_fm_update_occ(mapped.c_struct(), hyp.ref(), L.RULE_SGD, ws.data_ptr(), need, None, y.data_ptr(),
                                 grad.data_ptr(), 8, 8, None, 0.125, None, None) == L.ERR_UNSUPPORTED
    assert step(afm, idx.data_ptr(), need) == L.OK
    torch.cuda.synchronize()


# ---- the class ----
def _model_state(m):
    sd = m.state_dict()
    k, t, F = m.embedding_size, m.attention_size, m.field_size
    V = np.concatenate([sd[f"second_order_embeddings.{i}.weight"].numpy() for i in range(F)])
    w = np.concatenate([sd[f"first_order_embeddings.{i}.weight"].numpy().reshape(-1) for i in range(F)])
    params = np.concatenate([sd["attention_linear.weight"].numpy().reshape(-1), sd["attention_linear.bias"].numpy(),
                             sd["H"].numpy(), sd["P"].numpy()])
    return V, w, float(sd["bias"]), params


def test_afm_class_initial_parameters_follow_the_reference_rng_order():
    import torch.nn as nn
    from models.models_online_deep.afm_adam import AFMAdam
    sizes, k, t = [7, 30, 4, 12], 6, 5
    torch.manual_seed(123)
    m = AFMAdam(sizes, embedding_size=k, attention_size=t)
    torch.manual_seed(123)                      # the reference's constructor, restated (afm_adam.py:30-41)
    first = [nn.Embedding(s, 1).weight.data for s in sizes]
    second = [nn.Embedding(s, k).weight.data for s in sizes]
    lin = nn.Linear(k, t)
    H, P = torch.randn(t), torch.randn(k)
    sd = m.state_dict()
    for i in range(len(sizes)):
        assert torch.equal(sd[f"first_order_embeddings.{i}.weight"], first[i])
        assert torch.equal(sd[f"second_order_embeddings.{i}.weight"], second[i])
    assert torch.equal(sd["attention_linear.weight"], lin.weight.data) and torch.equal(sd["attention_linear.bias"], lin.bias.data)
    assert torch.equal(sd["H"], H) and torch.equal(sd["P"], P)
    assert float(sd["bias"]) == np.float32(0.99) and float(sd["n"]) == np.float32(0.003)


def test_afm_class_steps_track_f64():
    from models.models_online_deep.afm_adam import AFMAdam
    sizes, k, t, B = [20, 300, 5, 64, 9, 150], 8, 4, 200
    torch.manual_seed(0)
    m = AFMAdam(sizes, embedding_size=k, attention_size=t, batch_size=B, n=0.05, update_rule="sgd")
    for s in range(3):
        idx, xv, y, rows = batch(sizes, B, seed=40 + s, xv_kind="random")
        V, w, bias, params = _model_state(m)
        ref = afm_f64(V, w, bias, params, k, t, rows, xv, y)
        loss = float(m.update_embedding(idx, xv, y))
        assert_within_f64(loss, ref["loss"], float(np.mean(ref["floor_loss"])), f"step {s} loss")
        V2, w2, bias2, params2 = _model_state(m)
        fl = 0.05 * (1e-5 * np.abs(ref["dparams"]) + ref["fl_dparams"]) + 4 * U32 * np.abs(params)
        assert (np.abs((params2 - params) + 0.05 * ref["dparams"]) <= fl).all(), f"step {s} attention parameters"
        u = _touched(rows, V.shape[0])
        flV = 0.05 * (1e-5 * np.abs(ref["dV"][u]) + ref["fl_dV"][u]) + 4 * U32 * np.abs(V[u])
        assert (np.abs((V2[u] - V[u]) + 0.05 * ref["dV"][u]) <= flV).all(), f"step {s} embeddings"
        np.testing.assert_array_equal(V2[~u], V[~u])
    pred = m.predict_proba(idx, xv)
    assert pred.shape == (B,) and np.all((pred > 0) & (pred < 1))


def test_afm_class_fit_returns_epoch_losses():
    from models.models_online_deep.afm_adam import AFMAdam
    sizes, k, t = [20, 300, 5, 64], 8, 4
    idx, xv, y, rows = batch(sizes, 600, seed=3, xv_kind="random")
    torch.manual_seed(1)
    m = AFMAdam(sizes, embedding_size=k, attention_size=t, n_epochs=3, batch_size=128, n=0.01)
    train, valid = m.fit(idx[:500], xv[:500], y[:500], idx[500:], xv[500:], y[500:])
    assert len(train) == 3 and len(valid) == 3
    assert train[-1] < train[0]
    V, w, bias, params = _model_state(m)
    ref = afm_f64(V, w, bias, params, k, t, rows[500:], xv[500:], y[500:])
    assert abs(valid[-1] - ref["loss"]) <= 1e-5 * ref["loss"] + float(np.mean(ref["floor_loss"]))
    tm, acc, roc, cm = m.run_experiment(idx, xv, y)
    assert sum(cm.values()) == 600 and 0 <= acc <= 100 and set(roc) == {"tpr", "fpr"}


@pytest.mark.parametrize("rule", ["adam", "ftrl", "signadam"])
def test_afm_class_state_dict_and_pickle_resume_bit_for_bit(rule):
    import pickle
    from models.models_online_deep.afm_adam import AFMAdam
    sizes, k, t, B = [20, 300, 5, 64, 9], 8, 4, 128
    torch.manual_seed(2)
    m = AFMAdam(sizes, embedding_size=k, attention_size=t, batch_size=B, update_rule=rule, n=0.01)
    data = [batch(sizes, B, seed=60 + s, xv_kind="random") for s in range(3)]
    for idx, xv, y, _ in data[:2]:
        m.update_embedding(idx, xv, y)
    if rule != "ftrl":     # (ftrl: the reference's keys hold the derived weights only; its (z, n) state travels in the pickle)
        m2 = AFMAdam(sizes, embedding_size=k, attention_size=t, batch_size=B, update_rule=rule, n=0.01)
        m2.load_state_dict(m.state_dict())
        for a, b in zip(m.state_dict().values(), m2.state_dict().values()):
            assert torch.equal(a, b)
    m3 = pickle.loads(pickle.dumps(m))
    idx, xv, y, _ = data[2]
    l1, l3 = m.update_embedding(idx, xv, y), m3.update_embedding(idx, xv, y)
    assert torch.equal(l1, l3)
    for key, a in m.state_dict().items():
        assert torch.equal(a, m3.state_dict()[key]), key
    if rule == "adam":
        o1, o3 = m.optimizer_state_dict(), m3.optimizer_state_dict()
        for kk in ("mV", "vV", "mw", "vw", "bias_mv"):
            assert torch.equal(o1["table"][kk], o3["table"][kk])
        assert o1["table"]["step"] == o3["table"]["step"] == 3


def _attn_state(m):
    """The attention optimizer's state before a step, flat in [W | b | H | P] order, float64: (step, m, v) -- adam:
    exp_avg / exp_avg_sq; adagrad: m = 0, v = sum."""
    st, step, mm, vv = m._attn_opt.state, 0, [], []
    for prm in m._attn_params():
        s = st.get(prm, {})
        step = int(float(s["step"])) if "step" in s else 0
        n = prm.numel()
        if m.update_rule == "adam":
            mm.append(s["exp_avg"].double().cpu().reshape(-1) if s else torch.zeros(n, dtype=torch.float64))
            vv.append(s["exp_avg_sq"].double().cpu().reshape(-1) if s else torch.zeros(n, dtype=torch.float64))
        else:
            mm.append(torch.zeros(n, dtype=torch.float64))
            vv.append(s["sum"].double().cpu().reshape(-1))
    return step, torch.cat(mm).numpy(), torch.cat(vv).numpy()


@pytest.mark.parametrize("rule", ["adam", "adagrad"])
def test_afm_class_adaptive_steps_track_f64(rule):
    """AFMAdam's persistent rules over 4 update_embedding calls (F = 14: 2 pair tiles): the tables against rule_apply on the
    touched rows at the table's step count; the attention parameters against torch.optim.Adam / Adagrad restated in float64
    from the optimizer's own state before the step, both on afm_f64's gradients."""
    from models.models_online_deep.afm_adam import AFMAdam
    sizes, k, t, B, n = _sizes(14, 14), 8, 8, 256, 0.01
    torch.manual_seed(5)
    m = AFMAdam(sizes, embedding_size=k, attention_size=t, batch_size=B, n=n, update_rule=rule)
    F32 = lambda v: float(np.float32(v))
    b1, b2 = m._betas()
    eps = m._adam["eps"] if rule == "adam" else m._adagrad["eps"]
    h = dict(lr=F32(n), eps=F32(eps), beta1=b1, beta2=b2)            # the table's hyper-parameters, as the kernels see them
    for s in range(1, 5):
        idx, xv, y, rows = batch(sizes, B, seed=80 + s, xv_kind="random")
        before = state_of(m._table)
        params = m._attn_flat.detach().double().cpu().numpy()
        ostep, om, ov = _attn_state(m)
        ref = afm_f64(before["V"], before["w"], before["bias"], params, k, t, rows, xv, y, dz_abs=DZ_ABS)
        loss = float(m.update_embedding(idx, xv, y))
        torch.cuda.synchronize()
        assert m._table.step == s and ostep == s - 1
        assert_within_f64(loss, ref["loss"], float(np.mean(ref["floor_loss"])), f"step {s} loss")
        urows = np.unique(rows)
        ex = _grad_ex(ref, urows)
        _assert_rows(before, state_of(m._table), _rule_rows(before, urows, ex, rule, h, s), urows, ex, rule, h, s,
                     what=f"{rule} step {s} tables")
        # torch.optim.Adam: p -= lr / bc1 * m' / (sqrt(v') / sqrt(bc2) + eps) -- rule_apply's form with eps sqrt(bc2)
        g, gn = ref["dparams"], 1e-5 * np.abs(ref["dparams"]) + ref["fl_dparams"] + 1e-30
        ha = dict(h, lr=m._attn_opt.param_groups[0]["lr"], eps=eps * (np.sqrt(1 - b2 ** s) if rule == "adam" else 1.0))
        p2, m2, v2 = rule_apply(params, om, ov, g, rule, ha, s)
        fp, fm, fv = _floors_gn(rule, ha, s, g, gn, m2, v2)
        _assert_delta(m._attn_flat.detach().cpu().numpy(), params, p2, fp, f"{rule} step {s} attention parameters")
        ostep2, om2, ov2 = _attn_state(m)
        assert ostep2 == s
        _assert_delta(ov2, ov, v2, fv, f"{rule} step {s} attention second moments")
        if rule == "adam":
            _assert_delta(om2, om, m2, fm, f"{rule} step {s} attention first moments")


def test_afm_class_ftrl_predict_proba_matches_f64():
    """AFMAdam(update_rule='ftrl').predict_proba -- the FTRL forward, bias derived in the kernel -- against afm_f64 on the
    model's derived weights, after two steps, at F = 14 (2 pair tiles)."""
    from models.models_online_deep.afm_adam import AFMAdam
    sizes, k, t, B = _sizes(14, 15), 8, 4, 300
    torch.manual_seed(6)
    m = AFMAdam(sizes, embedding_size=k, attention_size=t, batch_size=B, n=0.05, update_rule="ftrl")
    for s in range(2):
        idx, xv, y, _ = batch(sizes, B, seed=90 + s, xv_kind="random")
        m.update_embedding(idx, xv, y)
    torch.cuda.synchronize()
    z = float(m._table.bias[0])
    idx, xv, y, rows = batch(sizes, B, seed=99, xv_kind="random")
    V, w, bias, params = _model_state(m)
    assert abs(bias - z) > 0.1                                       # the raw z would not pass for the bias
    ref = afm_f64(V, w, bias, params, k, t, rows, xv)
    pred = m.predict_proba(idx, xv)
    sig = 1.0 / (1.0 + np.exp(-ref["logit"]))
    tol = 0.25 * (1e-5 * np.abs(ref["logit"]) + ref["floor_logit"]) + 4 * U32
    assert (np.abs(pred - sig) <= tol).all(), f"predict_proba: max err {np.max(np.abs(pred - sig)):.3e}"
