"""Listwise (sampled-softmax) training of the FM without a GPU: the four fmx_fm_list_* symbols and their argument counts, what the
header promises, every refusal that is decided on the host (pointers that are never dereferenced), assemble_lists on CPU tensors,
the classes that refuse the list loss, and tests/list_f64.py against torch's float64 autograd and against pair_f64 at G = 2.  No
device is touched."""
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
COUNTS = {"fmx_fm_list_workspace_bytes": 3, "fmx_fm_list_forward": 9, "fmx_fm_list_step": 13, "fmx_fm_list_stream": 14}
CALLS = ["fmx_fm_list_forward", "fmx_fm_list_step", "fmx_fm_list_stream"]


def _lib():
    import fmx
    L = fmx._lib
    return fmx, L, L.load()


def _out(L, S=0x40000, loss=0x41000, dz=0x42000):
    o = L.FwdOut()
    o.S, o.loss, o.dz = S, loss, dz
    return o


def _call(who, lib, L, t, h, rule=None, idx=0x60000, n=4, G=4, ws=0x50000, ws_bytes=1 << 40, out=None, n_pool=1, n_steps=0):
    """The call with fake pointers: only ever sent where a host check refuses it (the stream also with n_steps = 0, which
    checks everything and launches nothing)."""
    tp = None if t is None else C.byref(t)
    hp = None if h is None else h.ref()
    op = None if out is None else C.byref(out)
    rule = L.RULE_SIGNADAM if rule is None else rule
    if who == "fmx_fm_list_forward":
        return lib.fmx_fm_list_forward(tp, hp, idx, None, n, G, 1.0, op, None)
    if who == "fmx_fm_list_step":
        return lib.fmx_fm_list_step(tp, hp, rule, idx, None, n, G, 1.0, ws, ws_bytes, op, None, None)
    return lib.fmx_fm_list_stream(tp, hp, rule, idx, n_pool, n, G, 1.0, n_steps, ws, ws_bytes, op, None, None)


def test_symbols_and_argument_counts():
    fmx, L, lib = _lib()
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    defined = set(re.findall(r"\bT\s+(fmx_\w+)", out))
    header = open(os.path.join(ROOT, "include", "fmx.h")).read()
    for name, n in COUNTS.items():
        assert re.fullmatch(r"fmx_[a-z_]+", name)
        assert name in defined, name
        assert name in L.EXPORTS and len(getattr(lib, name).argtypes) == n, name
        decl = re.search(r"\bint(?:64_t)? " + name + r"\(([^;]*)\);", header)
        assert decl and len(decl.group(1).split(",")) == n, name
        # each declaration's comment says what it replaces: nothing -- the nearest counterpart is the reference's pair objective
        comment = header[:decl.start()].rsplit("/*", 1)[1]
        assert "Replaces:" in comment and "meta_fm.py:145-169" in comment and "no listwise loss" in comment, name
    assert "fmx_fm_list_workspace_bytes" in L.I64_RETURNS and lib.fmx_fm_list_workspace_bytes.restype is C.c_int64
    assert lib.fmx_version() == 104


def test_header_states_the_objective():
    header = open(os.path.join(ROOT, "include", "fmx.h")).read()
    start = header.index("listwise (sampled-softmax) training of the pure FM")
    text = " ".join(header[start:header.index("int64_t fmx_fm_list_workspace_bytes")].split())
    for phrase in ("2 <= G <= 16", "m = max_j z_j", "e_j = exp(z_j - m)", "s = e_0 + e_1 + ... + e_{G-1} (added in that order)",
                   "loss_i = log(s) - (z_0 - m)", "dz_j = (e_j / s) inv_b", "dz_0 = -((e_1 + ... + e_{G-1}) / s) inv_b",
                   "not 1 - p_0", "finite for every finite set of logits", "BIT-UNCHANGED", "16 scratch bytes",
                   "the forward reads the real bias", "rounding-level gradients", "FMX_RULE_SIGNADAM normalises",
                   "G > 16", "FMX_ERR_UNSUPPORTED", "the reference has no listwise loss", "meta_fm.py:145-169"):
        assert phrase in text, phrase


def test_workspace_bytes_is_the_step_workspace_and_the_scratch():
    fmx, L, lib = _lib()
    t = _fake_table(L.LAYOUT_WEIGHTS)
    for B, G in ((1, 2), (3, 4), (5, 16), (2048, 8)):
        assert lib.fmx_fm_list_workspace_bytes(C.byref(t), B, G) == lib.fmx_workspace_bytes(C.byref(t), B * G) + 16
    for B, G in ((0, 4), (4, 1), (4, 17), (2 ** 30, 4)):
        assert lib.fmx_fm_list_workspace_bytes(C.byref(t), B, G) < 0, (B, G)
    assert lib.fmx_fm_list_workspace_bytes(None, 4, 4) < 0


@pytest.mark.parametrize("who", CALLS)
def test_host_decided_refusals(who):
    fmx, L, lib = _lib()
    A, SH, UN = L.ERR_ARG, L.ERR_SHAPE, L.ERR_UNSUPPORTED
    h = fmx.Hyper(lr=0.01)
    t = _fake_table(L.LAYOUT_WEIGHTS)
    mapped = _fake_table(L.LAYOUT_WEIGHTS)
    mapped.field_cols, mapped.n_cols = 0x90000, 2
    based = _fake_table(L.LAYOUT_WEIGHTS)
    based.field_base = 0x90000
    cases = [
        ("table", dict(t=None), A, "table"),
        ("hyper", dict(h=None), A, "hyper"),
        ("idx", dict(idx=None), A, "idx"),
        ("count 0", dict(n=0), A, "B_lists"),
        ("count -3", dict(n=-3), A, "B_lists"),
        ("G 1", dict(G=1), A, "G = 1"),
        ("G 0", dict(G=0), A, "G = 0"),
        ("G -2", dict(G=-2), A, "G = -2"),
        ("G 17", dict(G=17), UN, "G = 17"),
        ("G 64", dict(G=64), UN, "G = 64"),
        ("rows beyond int32", dict(n=2 ** 28, G=8), A, "int32"),
        ("rows beyond int32 by far", dict(n=2 ** 31 - 1, G=16), A, "int32"),
        ("field_cols", dict(t=mapped), UN, "field_cols"),
        ("field_base", dict(t=based), UN, "field_base"),
    ]
    if who != "fmx_fm_list_forward":
        need = lib.fmx_fm_list_workspace_bytes(C.byref(t), 4, 4)
        assert need == lib.fmx_workspace_bytes(C.byref(t), 16) + 16
        cases += [("ftrl rule on a weights table", dict(rule=L.RULE_FTRL), A, "FMX_RULE_FTRL"),
                  ("adam rule on a weights table", dict(rule=L.RULE_ADAM), A, "FMX_RULE_ADAM"),
                  ("sgd on a moments table", dict(t=_fake_table(L.LAYOUT_MOMENTS), rule=L.RULE_SGD), A, "rule"),
                  ("unknown rule", dict(rule=9), A, "rule"),
                  ("adam betas", dict(t=_fake_table(L.LAYOUT_MOMENTS), h=fmx.Hyper(beta1=1.0), rule=L.RULE_ADAM), A, "beta1"),
                  ("fwd", dict(out=None), A, "fwd"),
                  ("fwd->S", dict(out=_out(L, S=None)), A, "fwd->S"),
                  ("fwd->loss", dict(out=_out(L, loss=None)), A, "fwd->loss"),
                  ("fwd->dz", dict(out=_out(L, dz=None)), A, "fwd->dz"),
                  ("fwd->dz unaligned", dict(out=_out(L, dz=0x42004)), L.ERR_ALIGN, "fwd->dz"),
                  ("workspace null", dict(ws=None), A, "workspace"),
                  ("workspace unaligned", dict(ws=0x50008), L.ERR_ALIGN, "workspace"),
                  ("workspace short", dict(ws_bytes=need - 17), SH, "workspace"),
                  ("workspace without the scratch", dict(ws_bytes=need - 16), SH, "fmx_fm_list_workspace_bytes"),
                  ("workspace one byte short", dict(ws_bytes=need - 1), SH, "fmx_fm_list_workspace_bytes")]
    else:
        cases += [("out", dict(out=None), A, "out"),
                  ("out->S unaligned", dict(out=_out(L, S=0x40004)), L.ERR_ALIGN, "out->S")]
    for what, kw, want, word in cases:
        kw = dict(dict(t=t, h=h, out=_out(L)), **kw)
        rc = _call(who, lib, L, kw.pop("t"), kw.pop("h"), **kw)
        msg = lib.fmx_last_error_string().decode()
        assert rc == want, (who, what, rc, msg)
        assert msg and who in msg and word in msg, (who, what, msg)
    if who == "fmx_fm_list_forward":
        return
    # B_lists * G beyond what the sort accepts: whatever fmx_sort_occurrences reports for that batch, unchanged
    for n_lists, G in ((16385, 2), (2049, 16), (2 ** 26, 16)):
        want = lib.fmx_sort_occurrences(C.byref(t), 0x60000, n_lists * G, 0x50000, 1 << 40, None, None)
        want_msg = lib.fmx_last_error_string().decode()
        assert want == UN
        rc = _call(who, lib, L, t, h, n=n_lists, G=G, out=_out(L))
        assert rc == want and lib.fmx_last_error_string().decode() == want_msg, (rc, lib.fmx_last_error_string())
    if who == "fmx_fm_list_stream":
        # a workspace of exactly fmx_fm_list_workspace_bytes is enough (n_steps = 0 checks everything and launches nothing)
        assert _call(who, lib, L, t, h, out=_out(L), ws_bytes=need) == L.OK
        for kw in (dict(n_pool=0), dict(n_steps=-1)):
            rc = _call(who, lib, L, t, h, out=_out(L), **kw)
            assert rc == A and who in lib.fmx_last_error_string().decode()
        # adam: step + n_steps within int32
        tm = _fake_table(L.LAYOUT_MOMENTS)
        rc = _call(who, lib, L, tm, fmx.Hyper(step=2 ** 31 - 5), rule=L.RULE_ADAM, out=_out(L), n_steps=8)
        assert rc == A and who in lib.fmx_last_error_string().decode()


# ---- fmx/pairwise.py on CPU tensors ----
@pytest.mark.parametrize("n_neg", [1, 3])
@pytest.mark.parametrize("item_fields", [[2], [1, 3]])
def test_assemble_lists(n_neg, item_fields):
    from fmx.pairwise import assemble_lists, assemble_pairs
    g = torch.Generator().manual_seed(5)
    sizes = [7, 5, 11, 3]
    B, F, m, G = 6, 4, len(item_fields), 1 + n_neg
    pos = torch.stack([torch.randint(s, (B,), generator=g) for s in sizes], dim=1).to(torch.int32)
    xv = torch.rand((B, F), generator=g)
    neg = torch.stack([(pos[:, f].long().reshape(B, 1) + 1 + torch.arange(n_neg).reshape(1, n_neg)) % sizes[f] for f in item_fields], dim=2)
    other = [f for f in range(F) if f not in item_fields]
    for values in (None, xv):
        rows, vals = assemble_lists(pos, values, item_fields, neg if n_neg > 1 else neg[:, 0])
        assert rows.dtype == torch.int32 and rows.shape == (B * G, F) and rows.is_contiguous()
        assert torch.equal(rows[0::G], pos)                                          # a positive appears once, at the head of its list
        for b in range(B):
            for j in range(n_neg):
                r = rows[G * b + 1 + j]
                assert torch.equal(r[other], pos[b, other])                          # differs in the item columns only
                assert torch.equal(r[item_fields].long(), neg[b, j])
        if values is None:
            assert vals is None
        else:
            assert vals.dtype == torch.float32 and torch.equal(vals, xv.repeat_interleave(G, dim=0))
        # the same positives and negatives as assemble_pairs lays them out
        prow, _ = assemble_pairs(pos, values, item_fields, neg)
        assert torch.equal(prow[1::2].reshape(B, n_neg, F), rows.reshape(B, G, F)[:, 1:])
    nv = torch.full((B, n_neg, m), 0.5)
    _, vals = assemble_lists(pos, None, item_fields, neg, neg_xv=nv)
    vals = vals.reshape(B, G, F)
    assert (vals[:, 1:][:, :, item_fields] == 0.5).all() and (vals[:, 0] == 1).all() and (vals[:, 1:][:, :, other] == 1).all()
    if m == 1:
        rows1, _ = assemble_lists(pos, None, item_fields[0], neg[:, 0, 0])           # [B]: one negative each, one item field
        assert rows1.shape == (2 * B, F)
    # assemble_pairs' errors
    for bad in (dict(pos_idx=pos[0]), dict(item_fields=[]), dict(item_fields=[1, 1]), dict(item_fields=[F]), dict(neg_items=neg[:-1]),
                dict(pos_xv=xv[:, :-1])):
        kw = dict(dict(pos_idx=pos, pos_xv=xv, item_fields=item_fields, neg_items=neg), **bad)
        with pytest.raises(ValueError):
            assemble_lists(**kw)
        with pytest.raises(ValueError):
            assemble_pairs(**kw)


@pytest.mark.parametrize("cls", ["DeepFMAdam", "NFMAdam", "DeepFMOnn", "NFMOnn", "AFMAdam"])
def test_classes_that_refuse_the_list_loss(cls):
    mod = {"DeepFMAdam": "deepfm_adam", "NFMAdam": "nfm_adam", "DeepFMOnn": "deepfm_onn", "NFMOnn": "nfm_onn", "AFMAdam": "afm_adam"}[cls]
    klass = getattr(importlib.import_module("models.models_online_deep." + mod), cls)
    obj = object.__new__(klass)             # (no GPU: the constructors raise; the refusal needs no state)
    for negatives in ([[1]], None, "hard"):
        with pytest.raises(NotImplementedError, match="pure FM logit") as ei:
            klass.fit_lists(obj, [[0, 0]], [[1.0, 1.0]], [1], negatives=negatives)
        assert cls in str(ei.value) and "fit_lists" in str(ei.value)


def test_fit_lists_signature_and_the_limit_of_negatives():
    from models.models_online_deep.fm_adam import FMAdam
    params = inspect.signature(FMAdam.fit_lists).parameters
    assert list(params)[1:] == ["Xi", "Xv", "item_fields", "negatives", "n_neg", "candidates", "generator"]
    assert params["n_neg"].default == 4 and params["negatives"].default is None
    obj = object.__new__(FMAdam)            # (the limit is checked before the model is looked at)
    for negatives in (None, "hard"):
        for n_neg in (16, 100, 0):
            with pytest.raises(ValueError, match="15"):
                FMAdam.fit_lists(obj, [[0, 0]], [[1.0, 1.0]], [1], negatives=negatives, n_neg=n_neg)
    import fmx
    assert fmx._lib.LIST_MAX_G == 16


# ---- tests/list_f64.py against torch's float64 autograd of inv_b * sum_i CE ----
def _problem(G, B, seed=17):
    rng = np.random.default_rng(seed)
    sizes, k = [7, 5, 11, 3], 4
    off = np.concatenate([[0], np.cumsum(sizes)])
    R, F = int(off[-1]), len(sizes)
    state = dict(V=rng.normal(0, 0.3, (R, k)).astype(np.float32), w=rng.normal(0, 0.3, R).astype(np.float32), bias=np.float32(0.2))
    local = np.stack([rng.integers(0, s, B * G) for s in sizes], axis=1).reshape(B, G, F)
    local[:, :, :2] = local[:, :1, :2]                    # the lists share their context columns
    local = local.reshape(B * G, F)
    x = rng.uniform(0.5, 1.5, (B, G, F)).astype(np.float32)
    x[:, :, :2] = x[:, :1, :2]                            # ... and those columns' values
    return state, local, off, x.reshape(B * G, F), R, F


def test_list_f64_is_the_autograd_step():
    from list_f64 import list_step_f64
    G, B = 4, 6
    state, local, off, x, R, F = _problem(G, B)
    local[G * 2 + 3, 2:] = local[G * 2, 2:]               # one negative is its positive (item columns and all)
    x[G * 2 + 3] = x[G * 2]
    rows = local + off[:-1]
    inv_b = 1.0 / B
    r = list_step_f64(state, rows, x, G, "sgd", dict(lr=0.05), inv_b)

    V = torch.tensor(state["V"], dtype=torch.float64, requires_grad=True)
    w = torch.tensor(state["w"], dtype=torch.float64, requires_grad=True)
    b = torch.tensor(float(state["bias"]), dtype=torch.float64, requires_grad=True)
    rt, xt = torch.tensor(rows), torch.tensor(x, dtype=torch.float64)
    e = V[rt] * xt[:, :, None]
    z = (w[rt] * xt).sum(1) + 0.5 * (e.sum(1) ** 2 - (e * e).sum(1)).sum(1) + b
    z.retain_grad()
    ce = torch.nn.functional.cross_entropy(z.reshape(B, G), torch.zeros(B, dtype=torch.long), reduction="none")
    loss = ce.sum() * inv_b
    loss.backward()
    assert abs(r["loss"] - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
    np.testing.assert_allclose(r["logit"], z.detach().numpy(), rtol=1e-12)
    np.testing.assert_allclose(r["loss_b"][0::G], ce.detach().numpy(), rtol=1e-12)
    assert not r["loss_b"].reshape(B, G)[:, 1:].any()
    np.testing.assert_allclose(r["dz"], z.grad.numpy(), rtol=1e-12, atol=1e-15)
    zz = r["logit"].reshape(B, G)
    assert zz[2, 3] == zz[2, 0] and r["dz"][G * 2 + 3] > 0 > r["dz"][G * 2]          # the negative that equals its positive
    u = r["urows"]
    scale_V, scale_w = np.abs(V.grad.numpy()).max(), np.abs(w.grad.numpy()).max()
    np.testing.assert_allclose(r["dV"], V.grad.numpy()[u], rtol=1e-12, atol=1e-12 * scale_V)
    np.testing.assert_allclose(r["dw"], w.grad.numpy()[u], rtol=1e-12, atol=1e-12 * scale_w)
    mask = np.ones(R, bool)
    mask[u] = False
    assert not V.grad.numpy()[mask].any() and not w.grad.numpy()[mask].any()
    # the bias: no gradient (autograd's is the sum of a list's dz, zero up to float64 rounding); the helper defines 0 and keeps it
    assert r["db"] == 0.0 and abs(float(b.grad)) <= 1e-15
    assert r["new"]["bias"] == np.float64(state["bias"]) and r["floor"]["bias"] == 0.0
    # the shared context columns' first-order weights: a gradient that is zero in exact arithmetic
    ctx = np.isin(u, np.unique(rows[:, :2]))
    assert ctx.any() and np.abs(r["dw"][ctx]).max() <= 1e-15 < np.abs(r["dw"][~ctx]).max()
    # ... and the step is the SGD step of those gradients
    np.testing.assert_allclose(r["new"]["V"][u], state["V"][u].astype(np.float64) - 0.05 * V.grad.numpy()[u], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(r["new"]["w"][u], state["w"][u].astype(np.float64) - 0.05 * w.grad.numpy()[u], rtol=1e-12, atol=1e-15)
    # the floors are positive where something is computed
    assert (r["floor"]["dz"] > 0).all() and (r["floor"]["loss_b"][0::G] > 0).all() and r["floor"]["loss"] > 0


@pytest.mark.parametrize("rule", ["sgd", "ftrl"])
def test_list_f64_at_two_rows_is_pair_f64_without_a_margin(rule):
    from list_f64 import list_step_f64
    from pair_f64 import pair_step_f64
    from oracle.fm_oracle import ftrl_z_for_weight
    B = 9
    state, local, off, x, R, F = _problem(2, B, seed=23)
    rows = local + off[:-1]
    hyper = dict(lr=0.05)
    if rule == "ftrl":
        hyper = dict(alpha=0.05, beta=1.0, l1=0.001, l2=0.01)
        state = dict(zV=ftrl_z_for_weight(state["V"], **hyper), nV=np.full_like(state["V"], 0.1), zw=ftrl_z_for_weight(state["w"], **hyper),
                     nw=np.full_like(state["w"], 0.1), zb=np.float32(0.3), nb=np.float32(0.1))
    a = list_step_f64(state, rows, x, 2, rule, hyper, 1.0 / B)
    p = pair_step_f64(state, rows, x, 0.0, rule, hyper, 1.0 / B)

    def close(x_, y_, what):
        x_, y_ = np.asarray(x_, np.float64), np.asarray(y_, np.float64)
        assert np.all(np.abs(x_ - y_) <= 1e-12 * np.maximum(np.abs(y_), np.abs(y_).max() * 1e-3)), what
    close(a["loss"], p["loss"], "loss")
    close(a["logit"], p["logit"], "logit")
    close(a["dz"], p["dz"], "dz")
    close(a["dV"], p["dV"], "dV")
    close(a["dw"][np.abs(p["dw"]) > 1e-12], p["dw"][np.abs(p["dw"]) > 1e-12], "dw")
    assert np.array_equal(a["urows"], p["urows"])
    keys = ("zV", "nV", "zw", "nw") if rule == "ftrl" else ("V", "w")
    for kk in keys:
        close(a["new"][kk], p["new"][kk], kk)
    # the bias: the pair helper applies a gradient that is zero up to rounding, the list helper none
    for kk in (("zb", "nb") if rule == "ftrl" else ("bias",)):
        assert a["new"][kk] == np.float64(state[kk]) and abs(p["new"][kk] - a["new"][kk]) <= p["floor"][kk]
