"""Pairwise-ranking (BPR) training of the attentional FM without a GPU: the five fmx_afm_pair_* symbols and their argument counts,
every refusal that is decided on the host (pointers that are never dereferenced), the class surface (the `attention` keyword), and
tests/afm_pair_f64.py against plain float64 autograd and against the FM pair loss it reduces to.  No device is touched."""
import ctypes as C
import importlib
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from test_adaptive_rules_cpu import _fake_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = {"fmx_afm_pair_forward": 13, "fmx_afm_pair_step": 16, "fmx_afm_pair_step_opt": 17, "fmx_afm_pair_stream": 18,
          "fmx_afm_pair_online_run": 16}
STEPS = [w for w in COUNTS if w != "fmx_afm_pair_forward"]
WITH_OPT = ("fmx_afm_pair_step_opt", "fmx_afm_pair_stream", "fmx_afm_pair_online_run")


def _lib():
    import fmx
    L = fmx._lib
    return fmx, L, L.load()


def _afm(L, params=0x80000, k=16, t=4):
    return L.Afm(params, k, t)


def _opt(L, rule=None, m=0xA0000, v=0xB0000, step=0, beta1=0.9):
    return L.MlpOpt(m, v, 0.01, 1e-8, beta1, 0.999, L.RULE_ADAM if rule is None else rule, step)


_DEFAULT = object()


def _call(who, lib, L, t, h, afm=_DEFAULT, rule=None, idx=0x60000, n=4, margin=0.0, ws=0x50000, ws_bytes=1 << 40, grad=0x70000,
          opt=_DEFAULT, n_pool=1, n_steps=0):
    """The call with fake pointers: only ever sent where a host check refuses it, or where it launches nothing (the stream with
    n_steps = 0, the online run with N_pairs = 0)."""
    tp = None if t is None else C.byref(t)
    hp = None if h is None else h.ref()
    afm = _afm(L) if afm is _DEFAULT else afm
    ap = None if afm is None else C.byref(afm)
    opt = _opt(L) if opt is _DEFAULT else opt
    op = None if opt is None else C.byref(opt)
    rule = L.RULE_SIGNADAM if rule is None else rule
    if who == "fmx_afm_pair_forward":
        return lib.fmx_afm_pair_forward(tp, ap, hp, idx, None, n, margin, 1.0, None, None, None, None, None)
    if who == "fmx_afm_pair_step":
        return lib.fmx_afm_pair_step(tp, hp, rule, ap, idx, None, n, margin, 1.0, ws, ws_bytes, grad, None, None, None, None)
    if who == "fmx_afm_pair_step_opt":
        return lib.fmx_afm_pair_step_opt(tp, hp, rule, ap, idx, None, n, margin, 1.0, ws, ws_bytes, grad, op, None, None, None, None)
    if who == "fmx_afm_pair_stream":
        return lib.fmx_afm_pair_stream(tp, hp, rule, ap, idx, None, n_pool, n, margin, 1.0, n_steps, ws, ws_bytes, grad, op, None,
                                       None, None)
    return lib.fmx_afm_pair_online_run(tp, hp, rule, ap, idx, None, n, margin, ws, ws_bytes, grad, op, None, None, None, None)


def test_symbols_and_argument_counts():
    fmx, L, lib = _lib()
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    defined = set(re.findall(r"\bT\s+(fmx_\w+)", out))
    header = open(os.path.join(ROOT, "include", "fmx.h")).read()
    for name, n in COUNTS.items():
        assert name in defined, name
        assert name in L.EXPORTS and len(getattr(lib, name).argtypes) == n, name
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert decl and len(decl.group(1).split(",")) == n, name
        comment = header[:decl.start()].rsplit("/*", 1)[1]
        assert "meta_fm.py:145-169" in comment, name       # each declaration's comment cites the reference's pair objective
    assert lib.fmx_version() == 104


@pytest.mark.parametrize("who", list(COUNTS))
def test_host_decided_refusals(who):
    fmx, L, lib = _lib()
    A, SH, UN, AL = L.ERR_ARG, L.ERR_SHAPE, L.ERR_UNSUPPORTED, L.ERR_ALIGN
    h = fmx.Hyper(lr=0.01)
    t = _fake_table(L.LAYOUT_WEIGHTS)
    online = who == "fmx_afm_pair_online_run"
    count = "N_pairs" if online else "B_pairs"
    mapped = _fake_table(L.LAYOUT_WEIGHTS)
    mapped.field_cols, mapped.n_cols = 0x90000, 2
    one_field = _fake_table(L.LAYOUT_WEIGHTS)
    one_field.n_fields = 1
    cases = [
        ("table", dict(t=None), A, "table"),
        ("hyper", dict(h=None), A, "hyper"),
        ("idx", dict(idx=None), A, "idx"),
        ("afm", dict(afm=None), A, "attention parameters"),
        ("afm->params", dict(afm=_afm(L, params=None)), A, "attention parameters"),
        ("count -3", dict(n=-3), A, count),
        ("2 * count beyond int32", dict(n=2 ** 30), A, count),
        ("margin < 0", dict(margin=-0.1), A, "margin"),
        ("margin nan", dict(margin=float("nan")), A, "margin"),
        ("margin inf", dict(margin=float("inf")), A, "margin"),
        ("field_cols", dict(t=mapped), UN, "field_cols"),
        # what check_afm refuses
        ("one field", dict(t=one_field), UN, "fields"),
        ("afm->k", dict(afm=_afm(L, k=8)), SH, "afm->k"),
        ("t = 0", dict(afm=_afm(L, t=0)), UN, "attention size"),
        ("t = 65", dict(afm=_afm(L, t=65)), UN, "attention size"),
    ]
    if not online:
        cases += [("count 0", dict(n=0), A, count)]
    if who != "fmx_afm_pair_forward":
        need = lib.fmx_afm_workspace_bytes(C.byref(t), C.byref(_afm(L)), 2 if online else 8)
        assert need > 0
        tm = _fake_table(L.LAYOUT_MOMENTS)
        cases += [
            ("workspace null", dict(ws=None), A, "null argument"),
            ("attn_grad_out null", dict(grad=None), A, "null argument"),
            ("workspace short", dict(ws_bytes=need - 1), SH, "workspace"),
            ("workspace misaligned", dict(ws=0x50008), AL, "workspace"),
            # check_rule
            ("ftrl rule on a weights table", dict(rule=L.RULE_FTRL), A, "FMX_RULE_FTRL"),
            ("adam rule on a weights table", dict(rule=L.RULE_ADAM), A, "FMX_RULE_ADAM"),
            ("sgd on a moments table", dict(t=tm, rule=L.RULE_SGD), A, "rule"),
            ("unknown rule", dict(rule=9), A, "rule"),
            # check_adam
            ("adam beta1", dict(t=tm, rule=L.RULE_ADAM, h=fmx.Hyper(beta1=1.0)), A, who),
            ("adam step", dict(t=tm, rule=L.RULE_ADAM, h=fmx.Hyper(step=-1)), A, who),
        ]
    if who in WITH_OPT:
        cases += [
            ("opt null", dict(opt=None), A, "opt"),
            # check_afm_opt
            ("attention rule ftrl", dict(opt=_opt(L, rule=L.RULE_FTRL)), A, "attention rule"),
            ("adam without m", dict(opt=_opt(L, m=None)), A, "opt->m"),
            ("adagrad without v", dict(opt=_opt(L, rule=L.RULE_ADAGRAD, v=None)), A, "opt->v"),
            ("opt beta1", dict(opt=_opt(L, beta1=1.0)), A, "beta1"),
            ("opt step < 0", dict(opt=_opt(L, step=-1)), A, "opt->step"),
            ("opt->m misaligned", dict(opt=_opt(L, m=0xA0004)), AL, "16-byte"),
            ("afm->params misaligned", dict(afm=_afm(L, params=0x80004)), AL, "16-byte"),
        ]
    if who == "fmx_afm_pair_stream":
        cases += [("n_pool 0", dict(n_pool=0), A, "n_pool"), ("n_steps -1", dict(n_steps=-1), A, "n_steps"),
                  ("opt step + n_steps beyond int32", dict(opt=_opt(L, step=2 ** 31 - 5), n_steps=8), A, "opt->step")]
    if online:
        cases += [("opt step + N beyond int32", dict(opt=_opt(L, step=2 ** 31 - 3)), A, "opt->step")]
    for what, kw, want, word in cases:
        kw = dict(dict(t=t, h=h), **kw)
        rc = _call(who, lib, L, kw.pop("t"), kw.pop("h"), **kw)
        msg = lib.fmx_last_error_string().decode()
        assert rc == want, (who, what, rc, msg)
        assert msg and who in msg and word in msg, (who, what, msg)
    if who != "fmx_afm_pair_forward":
        # 2 * B_pairs rows beyond what the sort accepts: check_sort_geometry's refusal for that batch, before any launch
        if not online:
            rc = _call(who, lib, L, t, h, n=16385)
            assert rc == UN and who in lib.fmx_last_error_string().decode(), lib.fmx_last_error_string()
    # exactly fmx_afm_workspace_bytes(table, afm, 2 * B_pairs) bytes are enough: the calls that launch nothing return 0
    if who == "fmx_afm_pair_stream":
        assert _call(who, lib, L, t, h, ws_bytes=need, n_steps=0) == L.OK
    if online:
        assert _call(who, lib, L, t, h, ws_bytes=need, n=0) == L.OK
        assert _call(who, lib, L, t, h, ws_bytes=need - 1, n=0) == SH


# ---- the class surface: the keyword is `attention`, the default keeps refusing ----
def test_afm_class_surface():
    from models.models_online_deep.afm_adam import AFMAdam
    obj = object.__new__(AFMAdam)             # (no GPU: the constructor raises; the refusal needs no state)
    for name in ("fit_pairs", "run_pair_experiment"):
        params = inspect.signature(getattr(AFMAdam, name)).parameters
        assert list(params)[1:] == ["Xi", "Xv", "item_fields", "negatives", "n_neg", "margin", "candidates", "generator", "attention"]
        assert params["attention"].default is False and "full" not in params
        with pytest.raises(NotImplementedError, match="pure FM logit") as err:
            getattr(AFMAdam, name)(obj, [[0, 0]], [[1.0, 1.0]], [1], negatives=[[1]])
        assert "attention=True" in str(err.value)
        with pytest.raises(TypeError):
            getattr(AFMAdam, name)(obj, [[0, 0]], [[1.0, 1.0]], [1], negatives=[[1]], full=True)


@pytest.mark.parametrize("cls,extra", [("FMAdam", []), ("DeepFMAdam", ["full"]), ("NFMAdam", ["full"]), ("DeepFMOnn", []), ("NFMOnn", [])])
def test_other_classes_signatures_unchanged(cls, extra):
    mod = {"FMAdam": "fm_adam", "DeepFMAdam": "deepfm_adam", "NFMAdam": "nfm_adam", "DeepFMOnn": "deepfm_onn", "NFMOnn": "nfm_onn"}[cls]
    klass = getattr(importlib.import_module("models.models_online_deep." + mod), cls)
    for name in ("fit_pairs", "run_pair_experiment"):
        params = list(inspect.signature(getattr(klass, name)).parameters)[1:]
        assert params == ["Xi", "Xv", "item_fields", "negatives", "n_neg", "margin", "candidates", "generator"] + extra, (cls, name)
        assert "attention" not in params


# ---- tests/afm_pair_f64.py ----
def _data(F, k, t, Bp, seed):
    rng = np.random.default_rng(seed)
    sizes = rng.integers(3, 12, F)
    off = np.concatenate([[0], np.cumsum(sizes)])
    R = int(off[-1])
    V = (0.4 * rng.standard_normal((R, k))).astype(np.float32)
    w = (0.3 * rng.standard_normal(R)).astype(np.float32)
    params = (0.5 * rng.standard_normal(t * k + 2 * t + k)).astype(np.float32)
    local = np.stack([rng.integers(0, s, 2 * Bp) for s in sizes], axis=1)
    local[1::2, :-1] = local[0::2, :-1]                                       # a pair shares its context: the item is the last field
    local[1::2, -1] = (local[0::2, -1] + 1 + rng.integers(0, sizes[-1] - 1, Bp)) % sizes[-1]
    rows = local + off[:-1]
    x = rng.uniform(0.5, 1.5, (2 * Bp, F)).astype(np.float32)
    return V, w, np.float32(0.2), params, rows, x


@pytest.mark.parametrize("margin", [0.0, 0.1])
@pytest.mark.parametrize("shape", [(2, 4, 1, 1), (5, 3, 4, 6), (13, 8, 16, 7)])
def test_afm_pair_f64_is_plain_autograd(shape, margin):
    from afm_pair_f64 import afm_pair_f64
    F, k, t, Bp = shape
    V, w, bias, params, rows, x = _data(F, k, t, Bp, 7 * F + Bp)
    r = afm_pair_f64(V, w, bias, params, k, t, rows, x, margin=margin)

    Vt = torch.tensor(V, dtype=torch.float64, requires_grad=True)
    wt = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    bt = torch.tensor(float(bias), dtype=torch.float64, requires_grad=True)
    pt = torch.tensor(params, dtype=torch.float64, requires_grad=True)
    W, bW, hh, pp = pt[:t * k].reshape(t, k), pt[t * k:t * k + t], pt[t * k + t:t * k + 2 * t], pt[t * k + 2 * t:]
    rt, xt = torch.tensor(rows), torch.tensor(x, dtype=torch.float64)
    z = []
    for b in range(2 * Bp):                                # sample by sample, pair by pair: nothing shared with the helper's batching
        e = Vt[rt[b]] * xt[b][:, None]
        qs, ss = [], []
        for i in range(F - 1):
            for j in range(i + 1, F):
                q = e[i] * e[j]
                qs.append(q)
                ss.append((hh * torch.relu(W @ q + bW)).sum())
        a = torch.softmax(torch.stack(ss), 0)
        z.append(bt + (wt[rt[b]] * xt[b]).sum() + sum(a[n] * (pp * qs[n]).sum() for n in range(len(qs))))
    z = torch.stack(z)
    dd = z[0::2] - z[1::2]
    li = -torch.log(torch.sigmoid(dd) + margin)
    loss = li.sum() / Bp
    loss.backward()

    def close(got, want, what):
        want = np.asarray(want)
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12 * max(np.abs(want).max(), 1e-300), err_msg=what)

    close(r["logit"], z.detach().numpy(), "logit")
    close(r["loss_b"][0::2], li.detach().numpy(), "loss_b")
    assert not r["loss_b"][1::2].any()
    close(r["loss"], float(loss.detach()), "loss")
    close(r["dV"], Vt.grad.numpy(), "dV")
    close(r["dw"], wt.grad.numpy(), "dw")
    close(r["dparams"], pt.grad.numpy(), "dparams")
    assert r["dbias"] == 0.0 and abs(float(bt.grad)) <= 1e-15
    assert np.array_equal(r["dz"][1::2], -r["dz"][0::2])
    close(r["dz"][0::2] * Bp, r["g"], "g")
    for name in ("floor_logit", "floor_loss", "floor_dz", "fl_dV", "fl_dw", "fl_dparams"):
        assert np.isfinite(r[name]).all() and (r[name] >= 0).all(), name


@pytest.mark.parametrize("margin", [0.0, 0.1])
def test_afm_pair_f64_reduces_to_the_fm_pair_loss(margin):
    """h = 0 makes every score 0 and the softmax uniform; p = P (1, ..., 1) then gives p . sum a q = sum_ij <e_i, e_j>: the FM."""
    from afm_pair_f64 import afm_pair_f64
    from pair_f64 import pair_step_f64
    F, k, t, Bp = 5, 3, 4, 6
    V, w, bias, params, rows, x = _data(F, k, t, Bp, 3)
    P = F * (F - 1) // 2
    params[t * k + t:t * k + 2 * t] = 0
    params[t * k + 2 * t:] = P
    r = afm_pair_f64(V, w, bias, params, k, t, rows, x, margin=margin)
    fm = pair_step_f64(dict(V=V, w=w, bias=bias), rows, x, margin, "sgd", dict(lr=0.05), 1.0 / Bp)
    np.testing.assert_allclose(r["logit"], fm["logit"], rtol=1e-12)
    assert abs(r["loss"] - fm["loss"]) <= 1e-12 * abs(fm["loss"])
    np.testing.assert_allclose(r["dz"], fm["dz"], rtol=1e-11, atol=1e-15)
    u = fm["urows"]
    np.testing.assert_allclose(r["dV"][u], fm["dV"], rtol=1e-11, atol=1e-12 * np.abs(fm["dV"]).max())
    np.testing.assert_allclose(r["dw"][u], fm["dw"], rtol=1e-11, atol=1e-12 * np.abs(fm["dw"]).max())
