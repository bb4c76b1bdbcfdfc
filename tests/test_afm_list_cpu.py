"""Listwise (sampled-softmax) training of the attentional FM without a GPU: the six fmx_afm_list_* symbols and their argument
counts, every refusal that is decided on the host (pointers that are never dereferenced), the workspace size, the class surface
(the `attention` keyword), and tests/afm_list_f64.py against plain float64 autograd and against the pair helper it equals at
G = 2.  No device is touched."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from test_adaptive_rules_cpu import _fake_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = {"fmx_afm_list_workspace_bytes": 4, "fmx_afm_list_forward": 13, "fmx_afm_list_step": 16, "fmx_afm_list_step_opt": 17,
          "fmx_afm_list_stream": 18, "fmx_afm_list_online_run": 16}
CALLS = [w for w in COUNTS if w != "fmx_afm_list_workspace_bytes"]
WITH_OPT = ("fmx_afm_list_step_opt", "fmx_afm_list_stream", "fmx_afm_list_online_run")


def _lib():
    import fmx
    L = fmx._lib
    return fmx, L, L.load()


def _afm(L, params=0x80000, k=16, t=4):
    return L.Afm(params, k, t)


def _opt(L, rule=None, m=0xA0000, v=0xB0000, step=0, beta1=0.9):
    return L.MlpOpt(m, v, 0.01, 1e-8, beta1, 0.999, L.RULE_ADAM if rule is None else rule, step)


_DEFAULT = object()


def _call(who, lib, L, t, h, afm=_DEFAULT, rule=None, idx=0x60000, n=4, G=4, ws=0x50000, ws_bytes=1 << 40, grad=0x70000,
          opt=_DEFAULT, n_pool=1, n_steps=0):
    """The call with fake pointers: only ever sent where a host check refuses it, or where it launches nothing (the stream with
    n_steps = 0, the online run with N = 0)."""
    tp = None if t is None else C.byref(t)
    hp = None if h is None else h.ref()
    afm = _afm(L) if afm is _DEFAULT else afm
    ap = None if afm is None else C.byref(afm)
    opt = _opt(L) if opt is _DEFAULT else opt
    op = None if opt is None else C.byref(opt)
    rule = L.RULE_SIGNADAM if rule is None else rule
    if who == "fmx_afm_list_forward":
        return lib.fmx_afm_list_forward(tp, ap, hp, idx, None, n, G, 1.0, None, None, None, None, None)
    if who == "fmx_afm_list_step":
        return lib.fmx_afm_list_step(tp, hp, rule, ap, idx, None, n, G, 1.0, ws, ws_bytes, grad, None, None, None, None)
    if who == "fmx_afm_list_step_opt":
        return lib.fmx_afm_list_step_opt(tp, hp, rule, ap, idx, None, n, G, 1.0, ws, ws_bytes, grad, op, None, None, None, None)
    if who == "fmx_afm_list_stream":
        return lib.fmx_afm_list_stream(tp, hp, rule, ap, idx, None, n_pool, n, G, 1.0, n_steps, ws, ws_bytes, grad, op, None, None, None)
    return lib.fmx_afm_list_online_run(tp, hp, rule, ap, idx, None, n, G, ws, ws_bytes, grad, op, None, None, None, None)


def test_symbols_and_argument_counts():
    fmx, L, lib = _lib()
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    defined = set(re.findall(r"\bT\s+(fmx_\w+)", out))
    header = open(os.path.join(ROOT, "include", "fmx.h")).read()
    for name, n in COUNTS.items():
        assert name in defined, name
        assert name in L.EXPORTS and len(getattr(lib, name).argtypes) == n, name
        decl = re.search(r"\bint(?:64_t)? " + name + r"\(([^;]*)\);", header)
        assert decl and len(decl.group(1).split(",")) == n, name
        comment = header[:decl.start()].rsplit("/*", 1)[1]
        assert "meta_fm.py:145-169" in comment, name       # each declaration's comment cites the reference's nearest counterpart
    assert "fmx_afm_list_workspace_bytes" in L.I64_RETURNS and lib.fmx_afm_list_workspace_bytes.restype is C.c_int64


def test_workspace_bytes_is_the_afm_steps_plus_the_scratch():
    fmx, L, lib = _lib()
    t, afm = _fake_table(L.LAYOUT_WEIGHTS), _afm(L)
    for B, G in ((1, 2), (1, 16), (7, 5), (33, 3), (2048, 16)):
        want = lib.fmx_afm_workspace_bytes(C.byref(t), C.byref(afm), B * G)
        assert want > 0 and lib.fmx_afm_list_workspace_bytes(C.byref(t), C.byref(afm), B, G) == want + 16, (B, G)
    who = "fmx_afm_list_workspace_bytes"
    for B, G, code in ((0, 4, L.ERR_ARG), (4, 1, L.ERR_ARG), (4, 17, L.ERR_ARG), (2 ** 30, 4, L.ERR_ARG)):
        assert lib.fmx_afm_list_workspace_bytes(C.byref(t), C.byref(afm), B, G) == code, (B, G)
        assert who in lib.fmx_last_error_string().decode()
    assert lib.fmx_afm_list_workspace_bytes(None, C.byref(afm), 4, 4) < 0
    assert lib.fmx_afm_list_workspace_bytes(C.byref(t), None, 4, 4) < 0
    assert lib.fmx_afm_list_workspace_bytes(C.byref(t), C.byref(_afm(L, t=65)), 4, 4) == L.ERR_UNSUPPORTED


@pytest.mark.parametrize("who", CALLS)
def test_host_decided_refusals(who):
    fmx, L, lib = _lib()
    A, SH, UN, AL = L.ERR_ARG, L.ERR_SHAPE, L.ERR_UNSUPPORTED, L.ERR_ALIGN
    h = fmx.Hyper(lr=0.01)
    t = _fake_table(L.LAYOUT_WEIGHTS)
    online = who == "fmx_afm_list_online_run"
    mapped = _fake_table(L.LAYOUT_WEIGHTS)
    mapped.field_cols, mapped.n_cols = 0x90000, 2
    one_field = _fake_table(L.LAYOUT_WEIGHTS)
    one_field.n_fields = 1
    cases = [
        # the list refusals of check_list_args
        ("table", dict(t=None), A, "table"),
        ("hyper", dict(h=None), A, "hyper"),
        ("idx", dict(idx=None), A, "idx"),
        ("count -3", dict(n=-3), A, "N" if online else "B_lists"),
        ("G = 1", dict(G=1), A, "G = 1"),
        ("G = 0", dict(G=0), A, "G = 0"),
        ("G = 17", dict(G=17), UN, "G = 17"),
        ("count * G beyond int32", dict(n=2 ** 29, G=8), A, "int32"),
        ("field_cols", dict(t=mapped), UN, "index columns"),
        # what check_afm refuses
        ("afm", dict(afm=None), A, "attention parameters"),
        ("afm->params", dict(afm=_afm(L, params=None)), A, "attention parameters"),
        ("one field", dict(t=one_field), UN, "fields"),
        ("afm->k", dict(afm=_afm(L, k=8)), SH, "afm->k"),
        ("t = 0", dict(afm=_afm(L, t=0)), UN, "attention size"),
        ("t = 65", dict(afm=_afm(L, t=65)), UN, "attention size"),
    ]
    if not online:
        cases += [("count 0", dict(n=0), A, "B_lists")]
    need = lib.fmx_afm_list_workspace_bytes(C.byref(t), C.byref(_afm(L)), 1 if online else 4, 4)
    assert need > 0
    if who != "fmx_afm_list_forward":
        tm = _fake_table(L.LAYOUT_MOMENTS)
        cases += [
            ("workspace null", dict(ws=None), A, "null argument"),
            ("attn_grad_out null", dict(grad=None), A, "null argument"),
            ("workspace short", dict(ws_bytes=need - 1), SH, "workspace"),
            ("workspace without the scratch", dict(ws_bytes=need - 16), SH, "fmx_afm_list_workspace_bytes"),
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
    if who == "fmx_afm_list_stream":
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
    if who != "fmx_afm_list_forward" and not online:
        # B_lists * G rows beyond what the sort accepts: check_sort_geometry's refusal for that batch, before any launch
        rc = _call(who, lib, L, t, h, n=4097, G=8)
        assert rc == UN and who in lib.fmx_last_error_string().decode(), lib.fmx_last_error_string()
    # exactly fmx_afm_list_workspace_bytes bytes are enough: the calls that launch nothing return 0
    if who == "fmx_afm_list_stream":
        assert _call(who, lib, L, t, h, ws_bytes=need, n_steps=0) == L.OK
    if online:
        assert _call(who, lib, L, t, h, ws_bytes=need, n=0) == L.OK
        # an empty stream launches nothing, and its buffers may be null
        assert lib.fmx_afm_list_online_run(C.byref(t), None, L.RULE_SIGNADAM, C.byref(_afm(L)), None, None, 0, 4, None, 0, None, None,
                                           None, None, None, None) == L.OK


# ---- the class surface: FMAdam's parameters plus a trailing attention=False; the default keeps refusing ----
def test_afm_class_surface():
    from models.models_online_deep.afm_adam import AFMAdam
    from models.models_online_deep.fm_adam import FMAdam
    obj = object.__new__(AFMAdam)             # (no GPU: the constructor raises; the refusals below need no state)
    for name in ("fit_lists", "run_list_experiment"):
        params = inspect.signature(getattr(AFMAdam, name)).parameters
        assert list(params) == list(inspect.signature(getattr(FMAdam, name)).parameters) + ["attention"], name
        assert params["attention"].default is False and params["n_neg"].default == 4 and params["negatives"].default is None
        # without attention: the pure FM's refusal, before the hard negatives', the limit and any state; it names the keyword
        for negatives, n_neg in (([[1]], 4), (None, 4), ("hard", 4), (None, 99), ("hard", 0)):
            with pytest.raises(NotImplementedError, match="pure FM logit") as err:
                getattr(AFMAdam, name)(obj, [[0, 0]], [[1.0, 1.0]], [1], negatives=negatives, n_neg=n_neg)
            msg = str(err.value)
            assert "attention=True" in msg and "AFMAdam" in msg and name in msg and "list loss" in msg, msg
        # with attention: the limit of negatives first (it names 15), then the mined negatives' refusal
        for negatives in (None, "hard"):
            for n_neg in (16, 100, 0):
                with pytest.raises(ValueError, match="15") as err:
                    getattr(AFMAdam, name)(obj, [[0, 0]], [[1.0, 1.0]], [1], negatives=negatives, n_neg=n_neg, attention=True)
                assert name in str(err.value)
        with pytest.raises(NotImplementedError, match="negatives='hard'") as err:
            getattr(AFMAdam, name)(obj, [[0, 0]], [[1.0, 1.0]], [1], negatives="hard", attention=True)
        assert name in str(err.value) and "pure FM logit" not in str(err.value)
    # the pair methods' refusal keeps naming its own loss
    with pytest.raises(NotImplementedError, match="pair loss of the attentional FM's logit"):
        AFMAdam.fit_pairs(obj, [[0, 0]], [[1.0, 1.0]], [1], negatives=[[1]])


# ---- tests/afm_list_f64.py ----
def _data(F, k, t, Bl, G, seed):
    rng = np.random.default_rng(seed)
    sizes = rng.integers(G + 1, G + 9, F)
    off = np.concatenate([[0], np.cumsum(sizes)])
    R = int(off[-1])
    V = (0.4 * rng.standard_normal((R, k))).astype(np.float32)
    w = (0.3 * rng.standard_normal(R)).astype(np.float32)
    params = (0.5 * rng.standard_normal(t * k + 2 * t + k)).astype(np.float32)
    local = np.repeat(np.stack([rng.integers(0, s, Bl) for s in sizes], axis=1), G, axis=0)   # a list shares its context
    for j in range(1, G):                                                          # the item is the last field: G distinct ones
        local[j::G, -1] = (local[0::G, -1] + j) % sizes[-1]
    rows = local + off[:-1]
    x = rng.uniform(0.5, 1.5, (Bl * G, F)).astype(np.float32)
    return V, w, np.float32(0.2), params, rows, x


@pytest.mark.parametrize("shape", [(2, 4, 1, 1, 2), (5, 3, 4, 6, 3), (7, 8, 16, 4, 5), (3, 4, 2, 2, 16)])
def test_afm_list_f64_is_plain_autograd(shape):
    from afm_list_f64 import afm_list_f64
    F, k, t, Bl, G = shape
    V, w, bias, params, rows, x = _data(F, k, t, Bl, G, 7 * F + Bl + G)
    inv_b = 0.37
    r = afm_list_f64(V, w, bias, params, k, t, rows, G, x, inv_b=inv_b)

    Vt = torch.tensor(V, dtype=torch.float64, requires_grad=True)
    wt = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    bt = torch.tensor(float(bias), dtype=torch.float64, requires_grad=True)
    pt = torch.tensor(params, dtype=torch.float64, requires_grad=True)
    W, bW, hh, pp = pt[:t * k].reshape(t, k), pt[t * k:t * k + t], pt[t * k + t:t * k + 2 * t], pt[t * k + 2 * t:]
    rt, xt = torch.tensor(rows), torch.tensor(x, dtype=torch.float64)
    z = []
    for b in range(Bl * G):                                # sample by sample, pair by pair: nothing shared with the helper's batching
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
    zl = z.reshape(Bl, G)
    li = torch.logsumexp(zl, dim=1) - zl[:, 0]
    loss = inv_b * li.sum()
    dz = torch.autograd.grad(loss, z, retain_graph=True)[0]
    loss.backward()

    def close(got, want, what):
        want = np.asarray(want)
        np.testing.assert_allclose(got, want, rtol=1e-11, atol=1e-11 * max(np.abs(want).max(), 1e-300), err_msg=what)

    close(r["logit"], z.detach().numpy(), "logit")
    close(r["loss_b"][0::G], li.detach().numpy(), "loss_b")
    for j in range(1, G):
        assert not r["loss_b"][j::G].any()
    close(r["loss"], float(loss.detach()), "loss")
    close(r["dz"], dz.numpy(), "dz")
    close(r["dV"], Vt.grad.numpy(), "dV")
    close(r["dw"], wt.grad.numpy(), "dw")
    close(r["dparams"], pt.grad.numpy(), "dparams")
    assert r["dbias"] == 0.0 and r["fl_dbias"] == 0.0 and abs(float(bt.grad)) <= 1e-15 * inv_b * Bl * G
    for name in ("floor_logit", "floor_loss", "floor_dz", "fl_dV", "fl_dw", "fl_dparams"):
        assert np.isfinite(r[name]).all() and (r[name] >= 0).all(), name
    # the list block's floors are list_f64's two lines over the list's logit floors
    u, f_z = 2.0 ** -24, r["floor_logit"].reshape(Bl, G).sum(1)
    np.testing.assert_allclose(r["floor_dz"], np.repeat((0.25 * f_z + (1.5 * G + 10) * u) * inv_b, G), rtol=1e-14)
    np.testing.assert_allclose(r["floor_loss"][0::G], f_z + u * (1.5 * G + 4 + 6 * np.abs(r["loss_b"][0::G])), rtol=1e-14)


def test_afm_list_f64_at_two_rows_is_the_pair_helper():
    from afm_list_f64 import afm_list_f64
    from afm_pair_f64 import afm_pair_f64
    F, k, t, Bp = 5, 3, 4, 6
    V, w, bias, params, rows, x = _data(F, k, t, Bp, 2, 3)
    lst = afm_list_f64(V, w, bias, params, k, t, rows, 2, x)
    pair = afm_pair_f64(V, w, bias, params, k, t, rows, x, margin=0.0)
    for name in ("logit", "loss_b", "dz", "dV", "dw", "dparams"):
        np.testing.assert_allclose(lst[name], pair[name], rtol=1e-12, atol=1e-12 * np.abs(pair[name]).max(), err_msg=name)
    assert abs(lst["loss"] - pair["loss"]) <= 1e-12 * abs(pair["loss"])
    assert lst["dbias"] == pair["dbias"] == 0.0
    assert np.array_equal(lst["unit_live"], pair["unit_live"]) and np.array_equal(lst["pair_live"], pair["pair_live"])


def test_afm_list_f64_is_finite_at_wide_logit_gaps():
    """Logit gaps of +-80 inside a list: p_0 -> 1 and p_0 -> 0; the negatives' mass keeps its digits."""
    from afm_list_f64 import list_dz_t
    z = torch.tensor([[80.0, 0.0, -3.0], [-80.0, 0.0, 1.0], [0.0, 0.0, 0.0]], dtype=torch.float64)
    g = list_dz_t(z).numpy()
    assert np.isfinite(g).all() and (g[:, 0] < 0).all() and (g[:, 1:] > 0).all()
    np.testing.assert_allclose(g.sum(1), 0.0, atol=1e-16)
    np.testing.assert_allclose(g[0, 0], -(np.exp(-80.0) + np.exp(-83.0)), rtol=1e-12)
    np.testing.assert_allclose(g[2], [-2 / 3, 1 / 3, 1 / 3], rtol=1e-15)
