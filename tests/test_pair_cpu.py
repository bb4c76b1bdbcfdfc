"""Pairwise-ranking (BPR) training of the FM without a GPU: the four fmx_fm_pair_* symbols and their argument counts, every
refusal that is decided on the host (pointers that are never dereferenced), the torch plumbing of fmx/pairwise.py on CPU
tensors, the classes that refuse the pair loss, and tests/pair_f64.py against torch's float64 autograd.  No device is touched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from test_adaptive_rules_cpu import _fake_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = {"fmx_fm_pair_forward": 9, "fmx_fm_pair_step": 13, "fmx_fm_pair_stream": 14, "fmx_fm_pair_online_run": 12}


def _lib():
    import fmx
    L = fmx._lib
    return fmx, L, L.load()


def _out(L, S=0x40000, loss=0x41000, dz=0x42000):
    o = L.FwdOut()
    o.S, o.loss, o.dz = S, loss, dz
    return o


def _call(who, lib, L, t, h, rule=None, idx=0x60000, n=4, margin=0.0, ws=0x50000, ws_bytes=1 << 40, out=None, n_pool=1, n_steps=0):
    """The call with fake pointers: only ever sent where a host check refuses it (the stream also with n_steps = 0, which
    checks everything and launches nothing)."""
    tp = None if t is None else C.byref(t)
    hp = None if h is None else h.ref()
    op = None if out is None else C.byref(out)
    rule = L.RULE_SIGNADAM if rule is None else rule
    if who == "fmx_fm_pair_forward":
        return lib.fmx_fm_pair_forward(tp, hp, idx, None, n, margin, 1.0, op, None)
    if who == "fmx_fm_pair_step":
        return lib.fmx_fm_pair_step(tp, hp, rule, idx, None, n, margin, 1.0, ws, ws_bytes, op, None, None)
    if who == "fmx_fm_pair_stream":
        return lib.fmx_fm_pair_stream(tp, hp, rule, idx, n_pool, n, margin, 1.0, n_steps, ws, ws_bytes, op, None, None)
    return lib.fmx_fm_pair_online_run(tp, hp, rule, idx, None, n, margin, 0x70000, None, None, None, None)


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
        # each declaration's comment cites the reference's pair objective
        comment = header[:decl.start()].rsplit("/*", 1)[1]
        assert "meta_fm.py:145-169" in comment, name
    assert lib.fmx_version() == 104


@pytest.mark.parametrize("who", list(COUNTS))
def test_host_decided_refusals(who):
    fmx, L, lib = _lib()
    A, SH, UN = L.ERR_ARG, L.ERR_SHAPE, L.ERR_UNSUPPORTED
    h = fmx.Hyper(lr=0.01)
    t = _fake_table(L.LAYOUT_WEIGHTS)
    step_like = who in ("fmx_fm_pair_step", "fmx_fm_pair_stream")
    mapped = _fake_table(L.LAYOUT_WEIGHTS)
    mapped.field_cols, mapped.n_cols = 0x90000, 2
    based = _fake_table(L.LAYOUT_WEIGHTS)
    based.field_base = 0x90000
    cases = [
        ("table", dict(t=None), A, "table"),
        ("hyper", dict(h=None), A, "hyper"),
        ("idx", dict(idx=None), A, "idx"),
        ("count 0", dict(n=0), A, "N" if who.endswith("online_run") else "B_pairs"),
        ("count -3", dict(n=-3), A, "N" if who.endswith("online_run") else "B_pairs"),
        ("margin < 0", dict(margin=-0.1), A, "margin"),
        ("margin nan", dict(margin=float("nan")), A, "margin"),
        ("margin inf", dict(margin=float("inf")), A, "margin"),
        ("field_cols", dict(t=mapped), UN, "field_cols"),
        ("field_base", dict(t=based), UN, "field_base"),
    ]
    if who != "fmx_fm_pair_forward":
        cases += [("ftrl rule on a weights table", dict(rule=L.RULE_FTRL), A, "FMX_RULE_FTRL"),
                  ("adam rule on a weights table", dict(rule=L.RULE_ADAM), A, "FMX_RULE_ADAM"),
                  ("sgd on a moments table", dict(t=_fake_table(L.LAYOUT_MOMENTS), rule=L.RULE_SGD), A, "rule"),
                  ("unknown rule", dict(rule=9), A, "rule")]
    if step_like:
        need = lib.fmx_workspace_bytes(C.byref(t), 8)
        assert need > 0
        cases += [("fwd", dict(out=None), A, "fwd"),
                  ("fwd->S", dict(out=_out(L, S=None)), A, "fwd->S"),
                  ("fwd->loss", dict(out=_out(L, loss=None)), A, "fwd->loss"),
                  ("fwd->dz", dict(out=_out(L, dz=None)), A, "fwd->dz"),
                  ("workspace null", dict(ws=None), A, "workspace"),
                  ("workspace short", dict(ws_bytes=need - 1), SH, "workspace")]
    for what, kw, want, word in cases:
        kw = dict(dict(t=t, h=h, out=_out(L)), **kw)
        rc = _call(who, lib, L, kw.pop("t"), kw.pop("h"), **kw)
        msg = lib.fmx_last_error_string().decode()
        assert rc == want, (who, what, rc, msg)
        assert msg and who in msg and word in msg, (who, what, msg)
    if step_like:
        # 2 * B_pairs beyond what the sort accepts: whatever fmx_sort_occurrences reports for that batch, unchanged
        for n_pairs in (16385, 2 ** 30 + 5):
            want = lib.fmx_sort_occurrences(C.byref(t), 0x60000, min(2 * n_pairs, 2 ** 31 - 1), 0x50000, 1 << 40, None, None)
            want_msg = lib.fmx_last_error_string().decode()
            assert want == UN
            rc = _call(who, lib, L, t, h, n=n_pairs, out=_out(L))
            assert rc == want and lib.fmx_last_error_string().decode() == want_msg, (rc, lib.fmx_last_error_string())
        # the workspace of exactly fmx_workspace_bytes(table, 2 * B_pairs) is enough (the stream: n_steps = 0 launches nothing)
        if who == "fmx_fm_pair_stream":
            assert _call(who, lib, L, t, h, out=_out(L), ws_bytes=need) == L.OK
            for kw in (dict(n_pool=0), dict(n_steps=-1)):
                rc = _call(who, lib, L, t, h, out=_out(L), **kw)
                assert rc == A and who in lib.fmx_last_error_string().decode()
            # adam: step + n_steps within int32
            tm = _fake_table(L.LAYOUT_MOMENTS)
            rc = _call(who, lib, L, tm, fmx.Hyper(step=2 ** 31 - 5), rule=L.RULE_ADAM, out=_out(L), n_steps=8)
            assert rc == A and who in lib.fmx_last_error_string().decode()
    if who == "fmx_fm_pair_online_run":
        wide = _fake_table(L.LAYOUT_WEIGHTS)
        wide.n_fields = 65                                # kp = 16: 4 passes of 16 lane groups hold 64 fields
        rc = _call(who, lib, L, wide, h)
        assert rc == UN and who in lib.fmx_last_error_string().decode()
        rc = lib.fmx_fm_pair_online_run(C.byref(t), h.ref(), L.RULE_SIGNADAM, 0x60000, None, 4, 0.0, None, None, None, None, None)
        assert rc == A and "pred_out" in lib.fmx_last_error_string().decode()


# ---- fmx/pairwise.py on CPU tensors ----
@pytest.mark.parametrize("n_neg", [1, 3])
@pytest.mark.parametrize("item_fields", [[2], [1, 3]])
def test_assemble_pairs(n_neg, item_fields):
    from fmx.pairwise import assemble_pairs
    g = torch.Generator().manual_seed(5)
    sizes = [7, 5, 11, 3]
    B, F, m = 6, 4, len(item_fields)
    pos = torch.stack([torch.randint(s, (B,), generator=g) for s in sizes], dim=1).to(torch.int32)
    xv = torch.rand((B, F), generator=g)
    neg = torch.stack([(pos[:, f].long().reshape(B, 1) + 1 + torch.arange(n_neg).reshape(1, n_neg)) % sizes[f] for f in item_fields], dim=2)
    for values in (None, xv):
        rows, vals = assemble_pairs(pos, values, item_fields, neg if n_neg > 1 else neg[:, 0])
        assert rows.dtype == torch.int32 and rows.shape == (2 * B * n_neg, F)
        other = [f for f in range(F) if f not in item_fields]
        for b in range(B):
            for j in range(n_neg):
                p = b * n_neg + j
                assert torch.equal(rows[2 * p], pos[b])                              # a positive is repeated once per negative
                assert torch.equal(rows[2 * p + 1, other], pos[b, other])            # differs in the item columns only
                assert torch.equal(rows[2 * p + 1, item_fields].long(), neg[b, j])
                assert (rows[2 * p + 1, item_fields] != pos[b, item_fields]).any()
        if values is None:
            assert vals is None
        else:
            assert torch.equal(vals[0::2], xv.repeat_interleave(n_neg, dim=0)) and torch.equal(vals[1::2], vals[0::2])
    # the negatives' own values
    nv = torch.full((B, n_neg, m), 0.5)
    _, vals = assemble_pairs(pos, None, item_fields, neg, neg_xv=nv)
    assert (vals[1::2][:, item_fields] == 0.5).all() and (vals[0::2] == 1).all()


def test_sample_negatives_never_the_positive_and_seeded():
    from fmx.pairwise import sample_negatives
    sizes = [7, 5, 11]
    n = 10000
    pos = torch.stack([torch.arange(n) % s for s in sizes], dim=1).to(torch.int32)
    a = sample_negatives(pos, [1], [5], generator=torch.Generator().manual_seed(11))
    assert a.shape == (n, 1, 1) and int(a.min()) >= 0 and int(a.max()) < 5
    assert not (a[:, 0, 0] == pos[:, 1]).any()
    for own in range(5):                                  # every other item appears for every positive
        seen = set(a[pos[:, 1] == own, 0, 0].tolist())
        assert seen == set(range(5)) - {own}, (own, seen)
    b = sample_negatives(pos, [1], [5], generator=torch.Generator().manual_seed(11))
    c = sample_negatives(pos, [1], [5], generator=torch.Generator().manual_seed(12))
    assert torch.equal(a, b) and not torch.equal(a, c)
    # several negatives, two item fields: a negative may share one of the two item rows with the positive, never both
    d = sample_negatives(pos[:500], [0, 2], [7, 11], n_neg=3, generator=torch.Generator().manual_seed(1))
    assert d.shape == (500, 3, 2)
    same = d == pos[:500, [0, 2]].long().reshape(500, 1, 2)
    assert not same.all(dim=2).any() and same.any()
    # a candidate list instead of sizes
    cand = torch.tensor([0, 2, 4])
    e = sample_negatives(pos, 1, cand, generator=torch.Generator().manual_seed(3))
    assert set(e.reshape(-1).tolist()) == {0, 2, 4} and not (e[:, 0, 0] == pos[:, 1]).any()
    with pytest.raises(ValueError):
        sample_negatives(pos, [1], [1])


@pytest.mark.parametrize("cls", ["DeepFMAdam", "NFMAdam", "DeepFMOnn", "NFMOnn", "AFMAdam"])
def test_classes_that_refuse_the_pair_loss(cls):
    import importlib
    mod = {"DeepFMAdam": "deepfm_adam", "NFMAdam": "nfm_adam", "DeepFMOnn": "deepfm_onn", "NFMOnn": "nfm_onn", "AFMAdam": "afm_adam"}[cls]
    klass = getattr(importlib.import_module("models.models_online_deep." + mod), cls)
    obj = object.__new__(klass)             # (no GPU: the constructors raise; the refusal needs no state)
    for name in ("fit_pairs", "run_pair_experiment"):
        with pytest.raises(NotImplementedError, match="pure FM logit"):
            getattr(klass, name)(obj, [[0, 0]], [[1.0, 1.0]], [1], negatives=[[1]])
    from models.models_online_deep.fm_adam import FMAdam
    import inspect
    assert list(inspect.signature(FMAdam.fit_pairs).parameters)[1:] == ["Xi", "Xv", "item_fields", "negatives", "n_neg", "margin",
                                                                         "candidates", "generator"]


# ---- tests/pair_f64.py against torch's float64 autograd of inv_b * sum_i loss_i ----
@pytest.mark.parametrize("margin", [0.0, 0.1])
def test_pair_f64_is_the_autograd_step(margin):
    from pair_f64 import pair_step_f64
    rng = np.random.default_rng(17)
    sizes, k, B = [7, 5, 11, 3], 4, 6
    off = np.concatenate([[0], np.cumsum(sizes)])
    R, F = int(off[-1]), len(sizes)
    state = dict(V=rng.normal(0, 0.3, (R, k)).astype(np.float32), w=rng.normal(0, 0.3, R).astype(np.float32), bias=np.float32(0.2))
    local = np.stack([rng.integers(0, s, 2 * B) for s in sizes], axis=1)
    local[1::2, :2] = local[0::2, :2]                     # the pairs share their context columns
    local[3, 3] = local[2, 3]                             # ... and one pair one of its two item rows
    rows = local + off[:-1]
    x = rng.uniform(0.5, 1.5, (2 * B, F)).astype(np.float32)
    inv_b = 1.0 / B
    r = pair_step_f64(state, rows, x, margin, "sgd", dict(lr=0.05), inv_b)

    V = torch.tensor(state["V"], dtype=torch.float64, requires_grad=True)
    w = torch.tensor(state["w"], dtype=torch.float64, requires_grad=True)
    b = torch.tensor(float(state["bias"]), dtype=torch.float64, requires_grad=True)
    rt, xt = torch.tensor(rows), torch.tensor(x, dtype=torch.float64)
    e = V[rt] * xt[:, :, None]
    z = (w[rt] * xt).sum(1) + 0.5 * (e.sum(1) ** 2 - (e * e).sum(1)).sum(1) + b
    dd = z[0::2] - z[1::2]
    loss = (-torch.log(torch.sigmoid(dd) + margin)).sum() * inv_b
    loss.backward()
    assert abs(r["loss"] - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
    np.testing.assert_allclose(r["logit"], z.detach().numpy(), rtol=1e-12)
    u = r["urows"]
    scale_V, scale_w = np.abs(V.grad.numpy()).max(), np.abs(w.grad.numpy()).max()
    np.testing.assert_allclose(r["dV"], V.grad.numpy()[u], rtol=1e-12, atol=1e-12 * scale_V)
    np.testing.assert_allclose(r["dw"], w.grad.numpy()[u], rtol=1e-12, atol=1e-12 * scale_w)
    mask = np.ones(R, bool)
    mask[u] = False
    assert not V.grad.numpy()[mask].any() and not w.grad.numpy()[mask].any()
    # the bias gradient is 0 within f_db: the sum of +g and -g over the pairs, in the helper and in autograd
    assert abs(r["db"]) <= r["floor"]["db"] and abs(float(b.grad)) <= r["floor"]["db"]
    # ... and the step is the SGD step of those gradients
    np.testing.assert_allclose(r["new"]["V"][u], state["V"][u].astype(np.float64) - 0.05 * V.grad.numpy()[u], rtol=1e-12, atol=1e-15)
    assert abs(r["new"]["bias"] - float(state["bias"])) <= r["floor"]["bias"]
