"""The one-workgroup pair step and the online pair loop of DeepFM / NFM without a GPU: fmx_mlp_pair_fit and
fmx_online_run_mlp_pair in the library, the binding and the header; every refusal that is decided on the host (pointers that
are never dereferenced; the loop also with N = 0, which checks everything and launches nothing); and the classes' switch
pair_loop_on_device.  No device is touched."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

from test_adaptive_rules_cpu import _fake_table
from test_pair_mlp_cpu import P, _klass, _mlp, _opt, _out

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = {"fmx_mlp_pair_fit": 15, "fmx_online_run_mlp_pair": 18}


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


def _fit(lib, L, mlp, h="default", rule=None, bi=P, kp=16, base=P, n=2, margin=0.0, logit=None, dz=P, gbi=P, loss=None, opt=None):
    import fmx
    h = fmx.Hyper(lr=0.01) if h == "default" else h
    return lib.fmx_mlp_pair_fit(None if mlp is None else C.byref(mlp), None if h is None else h.ref(), L.RULE_SIGNADAM if rule is None else rule,
                                bi, kp, base, n, margin, 0.5, logit, dz, gbi, loss, None if opt is None else C.byref(opt), None)


def test_pair_fit_refusals():
    fmx, L, lib = _lib()
    A, AL, UN = L.ERR_ARG, L.ERR_ALIGN, L.ERR_UNSUPPORTED
    who = "fmx_mlp_pair_fit"
    cases = [
        ("B_pairs 0", dict(n=0), A, "B_pairs"), ("B_pairs -3", dict(n=-3), A, "B_pairs"),
        ("margin < 0", dict(margin=-0.1), A, "margin"), ("margin nan", dict(margin=float("nan")), A, "margin"),
        ("margin inf", dict(margin=float("inf")), A, "margin"),
        # fmx_mlp_fit's
        ("mlp", dict(mlp=None), A, "null"), ("params", dict(mlp=_mlp(L, params=None)), A, "null"), ("hyper", dict(h=None), A, "null"),
        ("bi", dict(bi=None), A, "null"), ("base", dict(base=None), A, "null"), ("dz_out", dict(dz=None), A, "null"),
        ("gbi_out", dict(gbi=None), A, "null"),
        ("rule ftrl", dict(rule=L.RULE_FTRL), A, "rule"), ("rule 9", dict(rule=9), A, "rule"),
        ("rule adam without opt", dict(rule=L.RULE_ADAM), UN, "FMX_RULE_ADAM"), ("rule adagrad without opt", dict(rule=L.RULE_ADAGRAD), UN, "FMX_RULE_ADAGRAD"),
        ("B_pairs 9", dict(n=9), UN, "B_pairs"), ("k 64", dict(mlp=_mlp(L, k=64), kp=64), UN, "k <="),
        ("hidden 65", dict(mlp=_mlp(L, hidden=65)), UN, "hidden"), ("hidden 0", dict(mlp=_mlp(L, hidden=0)), UN, "hidden"),
        ("9 layers", dict(mlp=_mlp(L, layers=9)), UN, "layers"), ("kp < k", dict(kp=12), UN, "k="),
        # fmx_mlp_fit_opt's, with opt
        ("opt: unknown rule", dict(opt=_opt(L, rule=L.RULE_FTRL)), A, "rule"), ("opt: signadam", dict(opt=_opt(L, rule=L.RULE_SIGNADAM)), A, "rule"),
        ("opt: v null", dict(opt=_opt(L, v=None)), A, "opt->v"), ("opt: m null under adam", dict(opt=_opt(L, m=None)), A, "opt->m"),
        ("opt: beta1 = 1", dict(opt=_opt(L, beta1=1.0)), A, "beta1"), ("opt: beta2 < 0", dict(opt=_opt(L, beta2=-0.1)), A, "beta2"),
        ("opt: step < 0", dict(opt=_opt(L, step=-1)), A, "step"), ("opt: step + 1 > int32", dict(opt=_opt(L, step=2 ** 31 - 1)), A, "step"),
        ("opt: m alignment", dict(opt=_opt(L, m=P + 4)), AL, "aligned"), ("opt: v alignment", dict(opt=_opt(L, v=P + 4)), AL, "aligned"),
        ("opt: params alignment", dict(opt=_opt(L), mlp=_mlp(L, params=P + 4)), AL, "aligned"),
        ("opt: B_pairs 9", dict(opt=_opt(L), n=9), UN, "B_pairs"), ("opt: k 64", dict(opt=_opt(L), mlp=_mlp(L, k=64), kp=64), UN, "k <="),
    ]
    m = _mlp(L)
    for what, kw, want, word in cases:
        kw = dict(dict(mlp=m), **kw)
        rc = _fit(lib, L, kw.pop("mlp"), **kw)
        msg = lib.fmx_last_error_string().decode()
        assert rc == want, (what, rc, msg)
        assert who in msg and word in msg, (what, msg)


def _run(lib, L, t, h, mlp, rule=None, fm_term=1, idx=P, xv=None, n=0, margin=0.0, ws=P, ws_bytes=1 << 40, out=None, scratch=P,
         pred=P, logit=None, loss=None, opt=None):
    return lib.fmx_online_run_mlp_pair(None if t is None else C.byref(t), None if h is None else h.ref(), L.RULE_SIGNADAM if rule is None else rule,
                                       None if mlp is None else C.byref(mlp), fm_term, idx, xv, n, margin, ws, ws_bytes,
                                       None if out is None else C.byref(out), scratch, pred, logit, loss,
                                       None if opt is None else C.byref(opt), None)


def test_online_run_refusals():
    fmx, L, lib = _lib()
    A, SH, AL, UN = L.ERR_ARG, L.ERR_SHAPE, L.ERR_ALIGN, L.ERR_UNSUPPORTED
    who = "fmx_online_run_mlp_pair"
    h, m = fmx.Hyper(lr=0.01), _mlp(L)
    t, tm, tf = _fake_table(L.LAYOUT_WEIGHTS), _fake_table(L.LAYOUT_MOMENTS), _fake_table(L.LAYOUT_FTRL)
    mapped = _fake_table(L.LAYOUT_WEIGHTS)
    mapped.field_cols, mapped.n_cols = 0x90000, 2
    based = _fake_table(L.LAYOUT_WEIGHTS)
    based.field_base = 0x90000
    need = lib.fmx_workspace_bytes(C.byref(t), 2)
    assert need > 0
    cases = [
        # the pair family's
        ("table", dict(t=None), A, "table"), ("hyper", dict(h=None), A, "hyper"), ("idx", dict(idx=None, n=3), A, "idx"),
        ("N -1", dict(n=-1), A, "N"), ("2N > int32", dict(n=2 ** 30), A, "int32"), ("pred_out", dict(pred=None, n=3), A, "pred_out"),
        ("margin < 0", dict(margin=-0.1), A, "margin"), ("margin nan", dict(margin=float("nan")), A, "margin"),
        ("margin inf", dict(margin=float("inf")), A, "margin"),
        ("field_cols", dict(t=mapped), UN, "field_cols"), ("field_base", dict(t=based), UN, "field_base"),
        # fmx_online_run_mlp's (opt null)
        ("mlp", dict(mlp=None), A, "null"), ("params", dict(mlp=_mlp(L, params=None)), A, "null"), ("workspace", dict(ws=None), A, "null"),
        ("fwd", dict(out=None), A, "null"), ("scratch", dict(scratch=None), A, "null"),
        ("fwd->S", dict(out=_out(L, S=None)), A, "fwd"), ("fwd->bi", dict(out=_out(L, bi=None)), A, "fwd"),
        ("fwd->logit", dict(out=_out(L, logit=None)), A, "fwd"), ("fwd->sfirst", dict(out=_out(L, sfirst=None)), A, "fwd"),
        ("scratch alignment", dict(scratch=P + 4), AL, "aligned"), ("workspace alignment", dict(ws=P + 4), AL, "aligned"),
        ("adam tables without opt", dict(t=tm, rule=L.RULE_ADAM), UN, "FMX_RULE_ADAM"),
        ("adagrad tables without opt", dict(t=tm, rule=L.RULE_ADAGRAD), UN, "FMX_RULE_ADAGRAD"),
        ("ftrl without opt", dict(t=tf, rule=L.RULE_FTRL), A, "rule"), ("unknown rule", dict(rule=9), A, "rule"),
        ("signadam on a moments table", dict(t=tm), A, "FMX_LAYOUT_WEIGHTS"),
        ("k 64", dict(mlp=_mlp(L, k=64)), UN, "k <="), ("hidden 65", dict(mlp=_mlp(L, hidden=65)), UN, "hidden"),
        ("9 layers", dict(mlp=_mlp(L, layers=9)), UN, "layers"), ("k > kp", dict(mlp=_mlp(L, k=32)), UN, "k="),
        ("workspace short", dict(ws_bytes=need - 1), SH, "workspace"),
        # fmx_online_run_mlp_opt's (opt given)
        ("opt: unknown rule", dict(opt=_opt(L, rule=L.RULE_FTRL)), A, "rule"), ("opt: v null", dict(opt=_opt(L, v=None)), A, "opt->v"),
        ("opt: m null under adam", dict(opt=_opt(L, m=None)), A, "opt->m"), ("opt: beta1 = 1", dict(opt=_opt(L, beta1=1.0)), A, "beta1"),
        ("opt: step < 0", dict(opt=_opt(L, step=-1)), A, "step"), ("opt: step + N > int32", dict(opt=_opt(L, step=2 ** 31 - 5), n=8), A, "step"),
        ("opt: m alignment", dict(opt=_opt(L, m=P + 4)), AL, "aligned"),
        ("opt: rule / layout", dict(opt=_opt(L), t=tm, rule=L.RULE_SGD), A, "FMX_LAYOUT_WEIGHTS"),
        ("opt: adam tables, beta1", dict(opt=_opt(L), t=tm, rule=L.RULE_ADAM, h=fmx.Hyper(beta1=1.0)), A, "beta1"),
        ("opt: adam tables, step + N > int32", dict(opt=_opt(L), t=tm, rule=L.RULE_ADAM, h=fmx.Hyper(step=2 ** 31 - 5), n=8), A, "step"),
        ("opt: NFM on an FTRL table", dict(opt=_opt(L), fm_term=0, t=tf, rule=L.RULE_FTRL), UN, "fm_term"),
        ("opt: workspace short", dict(opt=_opt(L), ws_bytes=need - 1), SH, "workspace"),
    ]
    for what, kw, want, word in cases:
        kw = dict(dict(t=t, h=h, mlp=m, out=_out(L)), **kw)
        rc = _run(lib, L, kw.pop("t"), kw.pop("h"), kw.pop("mlp"), **kw)
        msg = lib.fmx_last_error_string().decode()
        assert rc == want, (what, rc, msg)
        assert word in msg and (who in msg or want == AL), (what, msg)
    # N = 0: everything is checked, nothing is launched, and the stream's own buffers may be null; exactly
    # fmx_workspace_bytes(table, 2) is enough, under either family and for both classes
    for kw in (dict(), dict(fm_term=0), dict(opt=_opt(L)), dict(opt=_opt(L), t=tm, rule=L.RULE_ADAM), dict(opt=_opt(L), t=tm, rule=L.RULE_ADAGRAD, fm_term=0),
               dict(opt=_opt(L), t=tf, rule=L.RULE_FTRL), dict(rule=L.RULE_SGD)):
        kw = dict(dict(t=t), **kw)
        assert _run(lib, L, kw.pop("t"), h, m, out=_out(L), ws_bytes=need, idx=None, pred=None, **kw) == L.OK, (kw, lib.fmx_last_error_string())


# ---- the classes ----
@pytest.mark.parametrize("cls", ["DeepFMAdam", "NFMAdam"])
def test_pair_loop_on_device_defaults_to_false(cls):
    klass = _klass(cls)
    assert klass.pair_loop_on_device is False
    obj = object.__new__(klass)             # (no GPU: the constructors raise)
    assert obj.pair_loop_on_device is False
    object.__setattr__(obj, "pair_loop_on_device", True)
    assert obj.pair_loop_on_device is True and klass.pair_loop_on_device is False
    for name in ("fit_pairs", "run_pair_experiment"):
        sig = inspect.signature(getattr(klass, name)).parameters
        assert list(sig)[-1] == "full" and sig["full"].default is False
    # the switch does not open the refusal of full=False
    with pytest.raises(NotImplementedError, match="pure FM logit"):
        klass.run_pair_experiment(obj, [[0, 0]], [[1.0, 1.0]], [1], negatives=[[1]])


def test_the_other_classes_do_not_have_the_switch():
    from models.models_online_deep.fm_adam import FMAdam
    for klass in [FMAdam] + [_klass(c) for c in ("DeepFMOnn", "NFMOnn", "AFMAdam")]:
        assert not hasattr(klass, "pair_loop_on_device"), klass
        for name in ("fit_pairs", "run_pair_experiment"):
            assert "full" not in inspect.signature(getattr(klass, name)).parameters, (klass, name)
