"""Pairwise-ranking (BPR) training of DeepFM / NFM without a GPU: fmx_mlp_pair_section and fmx_deepfm_pair_stream in the
library, the binding and the header; every refusal that is decided on the host (pointers that are never dereferenced; the
stream also with n_steps = 0, which checks everything and launches nothing); the classes' full keyword; and
tests/pair_mlp_f64.py against a direct float64 autograd of an interleaved batch.  No device is touched."""
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
COUNTS = {"fmx_mlp_pair_section": 18, "fmx_deepfm_pair_stream": 23}
P = 0x100000  # fake 16-byte aligned device pointers


def _lib():
    import fmx
    L = fmx._lib
    return fmx, L, L.load()


def test_symbols_argument_counts_and_citations():
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
        for cite in ("meta_fm.py:145-169", "deepfm_adam.py:", "nfm_adam.py:"):
            assert cite in comment, (name, cite)
    assert lib.fmx_version() == 104


def _mlp(L, params=P, layers=2, k=16, hidden=40):
    return L.Mlp(params, layers, k, hidden, 0)


def _opt(L, rule=None, m=P + 0x1000, v=P + 0x2000, beta1=0.9, beta2=0.999, step=0):
    return L.MlpOpt(m, v, 0.01, 1e-8, beta1, beta2, L.RULE_ADAM if rule is None else rule, step)


def _section(lib, L, mlp, bi=P, ld_bi=16, base=P, n=4, margin=0.0, ws=P, ws_bytes=1 << 40, dz=P, gbi=P, ld_gbi=16, grads=P, opt=None):
    return lib.fmx_mlp_pair_section(None if mlp is None else C.byref(mlp), bi, ld_bi, base, n, margin, 0.25, ws, ws_bytes, None, dz, gbi,
                                    ld_gbi, grads, 0.0, None if opt is None else C.byref(opt), None, None)


def test_section_refusals():
    fmx, L, lib = _lib()
    A, SH, AL, UN = L.ERR_ARG, L.ERR_SHAPE, L.ERR_ALIGN, L.ERR_UNSUPPORTED
    who = "fmx_mlp_pair_section"
    m = _mlp(L)
    need = lib.fmx_mlp_section_workspace_bytes(C.byref(m), 8)
    assert need > 0
    cases = [
        ("B_pairs 0", dict(n=0), A, "B_pairs"), ("B_pairs -3", dict(n=-3), A, "B_pairs"), ("B_pairs 2^30", dict(n=2 ** 30), A, "B_pairs"),
        ("margin < 0", dict(margin=-0.1), A, "margin"), ("margin nan", dict(margin=float("nan")), A, "margin"),
        ("margin inf", dict(margin=float("inf")), A, "margin"),
        # fmx_mlp_section's refusals
        ("mlp", dict(mlp=None), A, "null"), ("params", dict(mlp=_mlp(L, params=None)), A, "null"), ("workspace", dict(ws=None), A, "null"),
        ("bi", dict(bi=None), A, "null"), ("base", dict(base=None), A, "null"), ("dz_out", dict(dz=None), A, "null"),
        ("gbi_out", dict(gbi=None), A, "null"), ("grads", dict(grads=None), A, "null"),
        ("9 layers", dict(mlp=_mlp(L, layers=9)), UN, "layers"), ("hidden 0", dict(mlp=_mlp(L, hidden=0)), UN, "hidden"),
        ("workspace alignment", dict(ws=P + 4), AL, "aligned"),
        ("ld_bi < k", dict(ld_bi=12), SH, "ld_bi"), ("ld_gbi < k", dict(ld_gbi=12), SH, "ld_gbi"),
        ("workspace short", dict(ws_bytes=need - 1), SH, "workspace"),
        # fmx_mlp_section_opt's, with opt
        ("opt: unknown rule", dict(opt=_opt(L, rule=L.RULE_FTRL)), A, "rule"), ("opt: v null", dict(opt=_opt(L, v=None)), A, "opt->v"),
        ("opt: m null under adam", dict(opt=_opt(L, m=None)), A, "opt->m"), ("opt: beta1 = 1", dict(opt=_opt(L, beta1=1.0)), A, "beta1"),
        ("opt: step < 0", dict(opt=_opt(L, step=-1)), A, "step"), ("opt: step + 1 > int32", dict(opt=_opt(L, step=2 ** 31 - 1)), A, "step"),
        ("opt: m alignment", dict(opt=_opt(L, m=P + 4)), AL, "aligned"), ("opt: grads alignment", dict(opt=_opt(L), grads=P + 4), AL, "aligned"),
        ("opt: workspace short", dict(opt=_opt(L), ws_bytes=need - 1), SH, "workspace"),
    ]
    for what, kw, want, word in cases:
        kw = dict(dict(mlp=m), **kw)
        rc = _section(lib, L, kw.pop("mlp"), **kw)
        msg = lib.fmx_last_error_string().decode()
        assert rc == want, (what, rc, msg)
        assert word in msg and (who in msg or want == AL), (what, msg)


def _out(L, S=P, bi=P, logit=P, sfirst=P):
    o = L.FwdOut()
    o.S, o.bi, o.logit, o.sfirst = S, bi, logit, sfirst
    return o


def _stream(lib, L, t, h, mlp, rule=None, fm_term=1, idx=P, n_pool=1, n=4, margin=0.0, n_steps=0, ws=P, ws_bytes=1 << 40, mws=P,
            mws_bytes=1 << 40, out=None, dz=P, gbi=P, grads=P, opt=None):
    return lib.fmx_deepfm_pair_stream(None if t is None else C.byref(t), None if h is None else h.ref(), L.RULE_SIGNADAM if rule is None else rule,
                                      None if mlp is None else C.byref(mlp), fm_term, idx, n_pool, n, margin, 0.25, n_steps, ws, ws_bytes,
                                      mws, mws_bytes, None if out is None else C.byref(out), dz, gbi, grads, 0.01,
                                      None if opt is None else C.byref(opt), None, None)


def test_stream_refusals():
    fmx, L, lib = _lib()
    A, SH, AL, UN = L.ERR_ARG, L.ERR_SHAPE, L.ERR_ALIGN, L.ERR_UNSUPPORTED
    who = "fmx_deepfm_pair_stream"
    h, m = fmx.Hyper(lr=0.01), _mlp(L)
    t, tm, tf = _fake_table(L.LAYOUT_WEIGHTS), _fake_table(L.LAYOUT_MOMENTS), _fake_table(L.LAYOUT_FTRL)
    mapped = _fake_table(L.LAYOUT_WEIGHTS)
    mapped.field_cols, mapped.n_cols = 0x90000, 2
    based = _fake_table(L.LAYOUT_WEIGHTS)
    based.field_base = 0x90000
    need, mneed = lib.fmx_workspace_bytes(C.byref(t), 8), lib.fmx_mlp_section_workspace_bytes(C.byref(m), 8)
    assert need > 0 and mneed > 0
    cases = [
        # the fmx_fm_pair_* family's
        ("table", dict(t=None), A, "table"), ("hyper", dict(h=None), A, "hyper"), ("idx_pool", dict(idx=None), A, "idx"),
        ("B_pairs 0", dict(n=0), A, "B_pairs"), ("B_pairs -3", dict(n=-3), A, "B_pairs"),
        ("margin < 0", dict(margin=-0.1), A, "margin"), ("margin nan", dict(margin=float("nan")), A, "margin"),
        ("margin inf", dict(margin=float("inf")), A, "margin"),
        ("field_cols", dict(t=mapped), UN, "field_cols"), ("field_base", dict(t=based), UN, "field_base"),
        ("n_pool 0", dict(n_pool=0), A, "n_pool"), ("n_steps -1", dict(n_steps=-1), A, "n_steps"),
        # fmx_deepfm_stream's (opt null)
        ("adaptive rule without opt", dict(t=tm, rule=L.RULE_ADAM), UN, "FMX_RULE_ADAM"),
        ("ftrl rule on a weights table", dict(rule=L.RULE_FTRL), A, "FMX_RULE_FTRL"), ("unknown rule", dict(rule=9), A, "rule"),
        ("mlp", dict(mlp=None), A, "null"), ("workspace", dict(ws=None), A, "null"), ("mlp_workspace", dict(mws=None), A, "null"),
        ("fwd", dict(out=None), A, "null"), ("fwd->bi", dict(out=_out(L, bi=None)), A, "bi"), ("fwd->logit", dict(out=_out(L, logit=None)), A, "logit"),
        ("dz", dict(dz=None), A, "null"), ("gbi", dict(gbi=None), A, "null"), ("grads", dict(grads=None), A, "null"),
        ("NFM without sfirst", dict(fm_term=0, out=_out(L, sfirst=None)), UN, "sfirst"),
        ("NFM on an FTRL table", dict(fm_term=0, t=tf, rule=L.RULE_FTRL), UN, "fm_term"),
        ("k > kp", dict(mlp=_mlp(L, k=32)), SH, "kp"), ("dz alignment", dict(dz=P + 4), AL, "aligned"),
        ("workspace short", dict(ws_bytes=need - 1), SH, "workspace"), ("mlp workspace short", dict(mws_bytes=mneed - 1), SH, "MLP workspace"),
        # fmx_deepfm_stream_opt's (opt given)
        ("opt: v null", dict(opt=_opt(L, v=None)), A, "opt->v"), ("opt: unknown rule", dict(opt=_opt(L, rule=L.RULE_SIGNADAM)), A, "rule"),
        ("opt: step + n_steps > int32", dict(opt=_opt(L, step=2 ** 31 - 5), n_steps=8), A, "step"),
        ("opt: mlp workspace short", dict(opt=_opt(L), mws_bytes=mneed - 1), SH, "MLP workspace"),
        ("opt: NFM on an FTRL table", dict(opt=_opt(L), fm_term=0, t=tf, rule=L.RULE_FTRL), UN, "fm_term"),
        ("opt: adam tables, step + n_steps > int32", dict(opt=_opt(L), t=tm, rule=L.RULE_ADAM, h=fmx.Hyper(step=2 ** 31 - 5), n_steps=8), A, "step"),
    ]
    for what, kw, want, word in cases:
        kw = dict(dict(t=t, h=h, mlp=m, out=_out(L)), **kw)
        rc = _stream(lib, L, kw.pop("t"), kw.pop("h"), kw.pop("mlp"), **kw)
        msg = lib.fmx_last_error_string().decode()
        assert rc == want, (what, rc, msg)
        assert who in msg and word in msg, (what, msg)
    # 2 * B_pairs beyond what the sort accepts: whatever fmx_sort_occurrences reports for that batch, unchanged
    for n_pairs in (16385, 2 ** 30 + 5):
        want = lib.fmx_sort_occurrences(C.byref(t), P, min(2 * n_pairs, 2 ** 31 - 1), P, 1 << 40, None, None)
        want_msg = lib.fmx_last_error_string().decode()
        assert want == UN
        rc = _stream(lib, L, t, h, m, n=n_pairs, out=_out(L))
        assert rc == want and lib.fmx_last_error_string().decode() == want_msg, (rc, lib.fmx_last_error_string())
    # exactly the two workspace sizes of 2 * B_pairs rows are enough, under either rule and for both classes
    for kw in (dict(), dict(fm_term=0), dict(opt=_opt(L)), dict(opt=_opt(L), t=tm, rule=L.RULE_ADAM), dict(opt=_opt(L), t=tm, rule=L.RULE_ADAGRAD, fm_term=0),
               dict(t=tf, rule=L.RULE_FTRL)):
        kw = dict(dict(t=t), **kw)
        assert _stream(lib, L, kw.pop("t"), h, m, out=_out(L), ws_bytes=need, mws_bytes=mneed, **kw) == L.OK, (kw, lib.fmx_last_error_string())


# ---- the classes ----
def _klass(cls):
    mod = {"DeepFMAdam": "deepfm_adam", "NFMAdam": "nfm_adam", "DeepFMOnn": "deepfm_onn", "NFMOnn": "nfm_onn", "AFMAdam": "afm_adam"}[cls]
    return getattr(importlib.import_module("models.models_online_deep." + mod), cls)


@pytest.mark.parametrize("cls", ["DeepFMAdam", "NFMAdam"])
def test_full_false_is_the_refusal_and_adam_needs_the_fused_optimizer(cls):
    klass = _klass(cls)
    obj = object.__new__(klass)             # (no GPU: the constructors raise; neither refusal needs more state than set here)
    for name in ("fit_pairs", "run_pair_experiment"):
        sig = inspect.signature(getattr(klass, name)).parameters
        assert list(sig)[-1] == "full" and sig["full"].default is False
        for kw in (dict(), dict(full=False)):
            with pytest.raises(NotImplementedError, match="pure FM logit") as ei:
                getattr(klass, name)(obj, [[0, 0]], [[1.0, 1.0]], [1], negatives=[[1]], **kw)
            assert "full=True" in str(ei.value)
    for rule in ("adam", "adagrad"):
        object.__setattr__(obj, "update_rule", rule)
        object.__setattr__(obj, "_mlp_fused", None)
        with pytest.raises(ValueError, match="fused_optimizer"):
            klass.fit_pairs(obj, [[0, 0]], [[1.0, 1.0]], [1], negatives=[[1]], full=True)


def test_the_other_classes_and_signatures_are_unchanged():
    from models.models_online_deep.fm_adam import FMAdam
    from models.models_online_deep._base import OnlineFMBase
    want = ["Xi", "Xv", "item_fields", "negatives", "n_neg", "margin", "candidates", "generator"]
    for name in ("fit_pairs", "run_pair_experiment"):
        assert getattr(FMAdam, name) is getattr(OnlineFMBase, name)
        assert list(inspect.signature(getattr(FMAdam, name)).parameters)[1:] == want
    for cls in ("DeepFMOnn", "NFMOnn", "AFMAdam"):
        klass = _klass(cls)
        obj = object.__new__(klass)
        for name in ("fit_pairs", "run_pair_experiment"):
            assert "full" not in inspect.signature(getattr(klass, name)).parameters, (cls, name)
            with pytest.raises(NotImplementedError, match="pure FM logit"):
                getattr(klass, name)(obj, [[0, 0]], [[1.0, 1.0]], [1], negatives=[[1]])
            with pytest.raises(TypeError):
                getattr(klass, name)(obj, [[0, 0]], [[1.0, 1.0]], [1], negatives=[[1]], full=True)


# ---- tests/pair_mlp_f64.py against a direct float64 autograd of an interleaved batch ----
@pytest.mark.parametrize("margin", [0.0, 0.1])
def test_pair_mlp_f64_is_the_autograd(margin):
    from pair_mlp_f64 import pair_mlp_f64
    rng = np.random.default_rng(23)
    k, H, L, Pn = 5, 7, 3, 6
    n_par = sum(H * (k if l == 0 else H) + H for l in range(L))
    params = rng.normal(0, 0.5, n_par).astype(np.float32)
    bi = rng.normal(0, 0.7, (2 * Pn, k)).astype(np.float32)
    base = rng.normal(0, 0.5, 2 * Pn).astype(np.float32)
    inv_b = 1.0 / Pn
    r = pair_mlp_f64(params, k, H, L, bi, base, margin, inv_b)

    p = torch.tensor(params, dtype=torch.float64, requires_grad=True)
    x0 = torch.tensor(bi, dtype=torch.float64, requires_grad=True)
    b0 = torch.tensor(base, dtype=torch.float64, requires_grad=True)
    x, off = x0, 0
    for l in range(L):
        i = k if l == 0 else H
        W, b = p[off:off + H * i].view(H, i), p[off + H * i:off + H * i + H]
        x = torch.relu(x @ W.t() + b)
        off += H * i + H
    z = b0 + x.sum(1)
    pos, neg = z.view(Pn, 2)[:, 0], z.view(Pn, 2)[:, 1]                   # the interleaving, stated another way
    loss = (-torch.log(torch.sigmoid(pos - neg) + margin)).sum() * inv_b
    loss.backward()
    tight = dict(rtol=1e-12, atol=0.0)
    assert abs(r["loss"] - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
    np.testing.assert_allclose(r["out"], z.detach().numpy(), **tight)
    np.testing.assert_allclose(r["dz"], b0.grad.numpy(), rtol=1e-12, atol=1e-12 * np.abs(b0.grad.numpy()).max())
    np.testing.assert_allclose(r["gbi"], x0.grad.numpy(), rtol=1e-12, atol=1e-12 * np.abs(x0.grad.numpy()).max())
    np.testing.assert_allclose(r["flat"], p.grad.numpy(), rtol=1e-12, atol=1e-12 * np.abs(p.grad.numpy()).max())
    np.testing.assert_array_equal(r["dz"][1::2], -r["dz"][0::2])
    assert np.any(p.grad.numpy()) and np.any(x0.grad.numpy())
    off = 0
    for l in range(L):                                                     # the per-layer views are the flat layout
        i = k if l == 0 else H
        np.testing.assert_array_equal(r["grads"][l][0].reshape(-1), r["flat"][off:off + H * i])
        np.testing.assert_array_equal(r["grads"][l][1], r["flat"][off + H * i:off + H * i + H])
        assert r["gnoise"][l][0].shape == (H, i) and (r["gnoise"][l][0] >= 0).all() and np.isfinite(r["gnoise"][l][0]).all()
        off += H * i + H
