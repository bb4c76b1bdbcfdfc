"""The one-workgroup list step and the online list loop of DeepFM / NFM without a GPU: fmx_mlp_list_fit and
fmx_online_run_mlp_list in the library, the binding and the header; every refusal that is decided on the host (fake pointers
that are never dereferenced; the loop also with N = 0, which checks everything and launches nothing); the classes' switch
list_loop_on_device and _list_device_loop_ok() for each rule and network size; and the unchanged signatures.  No device is
touched."""
import ctypes as C
import inspect
import os
import re
import subprocess
import types

import pytest

from test_adaptive_rules_cpu import _fake_table
from test_list_mlp_abi_cpu import _klass
from test_pair_mlp_cpu import P, _mlp, _opt, _out

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIT, RUN = "fmx_mlp_list_fit", "fmx_online_run_mlp_list"
COUNTS = {FIT: 17, RUN: 19}


def _lib():
    import fmx
    L = fmx._lib
    return fmx, L, L.load()


@pytest.mark.parametrize("who", [FIT, RUN])
def test_symbol_is_declared_listed_and_exported(who):
    fmx, L, lib = _lib()
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert who in set(re.findall(r"\bT\s+(fmx_\w+)", out))
    assert who in L.EXPORTS and len(getattr(lib, who).argtypes) == COUNTS[who]
    header = open(os.path.join(ROOT, "include", "fmx.h")).read()
    decl = re.search(r"\bint " + who + r"\(([^;]*)\);", header)
    assert decl and len(decl.group(1).split(",")) == COUNTS[who]
    assert header.index("int fmx_online_run_mlp_pair(") < decl.start()          # declared behind the pair forms they mirror
    text = " ".join(header[:decl.start()].rsplit("/*", 1)[1].split())
    for word in ("Replaces:", "Restates:", "deepfm_adam.py:", "nfm_adam.py:"):
        assert word in text, (who, word)
    assert lib.fmx_version() == 104


def _fit(lib, L, mlp, h="default", rule=None, bi=P, kp=16, base=P, corr=None, B=2, G=4, logit=None, dz=P, gbi=P, loss=None, rank=None,
         opt=None):
    import fmx
    h = fmx.Hyper(lr=0.01) if h == "default" else h
    return lib.fmx_mlp_list_fit(None if mlp is None else C.byref(mlp), None if h is None else h.ref(), L.RULE_SIGNADAM if rule is None else rule,
                                bi, kp, base, corr, B, G, 0.5, logit, dz, gbi, loss, rank, None if opt is None else C.byref(opt), None)


def test_list_fit_refusals():
    fmx, L, lib = _lib()
    A, AL, UN = L.ERR_ARG, L.ERR_ALIGN, L.ERR_UNSUPPORTED
    cases = [
        # the list's shape, as fmx_mlp_list_section refuses it
        ("B_lists 0", dict(B=0), A, "B_lists = 0"), ("B_lists -2", dict(B=-2), A, "B_lists = -2"), ("G 1", dict(G=1), A, "G = 1"),
        ("G 0", dict(G=0), A, "G = 0"), ("G 17", dict(B=1, G=17), UN, "G = 17"), ("rows beyond int32", dict(B=2 ** 28, G=8), A, "int32"),
        # the one-workgroup step's limits on B_lists * G rows
        ("18 rows", dict(B=2, G=9), UN, "B_lists * G"), ("5 x 4", dict(B=5, G=4), UN, "B_lists * G"),
        # fmx_mlp_pair_fit's
        ("mlp", dict(mlp=None), A, "null"), ("params", dict(mlp=_mlp(L, params=None)), A, "null"), ("hyper", dict(h=None), A, "null"),
        ("bi", dict(bi=None), A, "null"), ("base", dict(base=None), A, "null"), ("dz_out", dict(dz=None), A, "null"),
        ("gbi_out", dict(gbi=None), A, "null"),
        ("rule ftrl", dict(rule=L.RULE_FTRL), A, "rule"), ("rule 9", dict(rule=9), A, "rule"),
        ("rule adam without opt", dict(rule=L.RULE_ADAM), UN, "FMX_RULE_ADAM"), ("rule adagrad without opt", dict(rule=L.RULE_ADAGRAD), UN, "FMX_RULE_ADAGRAD"),
        ("k 64", dict(mlp=_mlp(L, k=64), kp=64), UN, "k <="), ("hidden 65", dict(mlp=_mlp(L, hidden=65)), UN, "hidden"),
        ("hidden 0", dict(mlp=_mlp(L, hidden=0)), UN, "hidden"), ("9 layers", dict(mlp=_mlp(L, layers=9)), UN, "layers"),
        ("kp < k", dict(kp=12), UN, "k="),
        # with opt
        ("opt: G 17", dict(opt=_opt(L), B=1, G=17), UN, "G = 17"),
        ("opt: unknown rule", dict(opt=_opt(L, rule=L.RULE_FTRL)), A, "rule"), ("opt: signadam", dict(opt=_opt(L, rule=L.RULE_SIGNADAM)), A, "rule"),
        ("opt: v null", dict(opt=_opt(L, v=None)), A, "opt->v"), ("opt: m null under adam", dict(opt=_opt(L, m=None)), A, "opt->m"),
        ("opt: beta1 = 1", dict(opt=_opt(L, beta1=1.0)), A, "beta1"), ("opt: beta2 < 0", dict(opt=_opt(L, beta2=-0.1)), A, "beta2"),
        ("opt: step < 0", dict(opt=_opt(L, step=-1)), A, "step"), ("opt: step + 1 > int32", dict(opt=_opt(L, step=2 ** 31 - 1)), A, "step"),
        ("opt: m alignment", dict(opt=_opt(L, m=P + 4)), AL, "aligned"), ("opt: v alignment", dict(opt=_opt(L, v=P + 4)), AL, "aligned"),
        ("opt: params alignment", dict(opt=_opt(L), mlp=_mlp(L, params=P + 4)), AL, "aligned"),
        ("opt: 18 rows", dict(opt=_opt(L), B=2, G=9), UN, "B_lists * G"), ("opt: k 64", dict(opt=_opt(L), mlp=_mlp(L, k=64), kp=64), UN, "k <="),
    ]
    m = _mlp(L)
    for what, kw, want, word in cases:
        kw = dict(dict(mlp=m), **kw)
        rc = _fit(lib, L, kw.pop("mlp"), **kw)
        msg = lib.fmx_last_error_string().decode()
        assert rc == want, (what, rc, msg)
        assert FIT in msg and word in msg, (what, msg)


def _run(lib, L, t, h, mlp, rule=None, fm_term=1, idx=P, xv=None, corr=None, n=0, G=4, ws=P, ws_bytes=1 << 40, out=None, scratch=P,
         rank=P, logit=None, loss=None, opt=None):
    return lib.fmx_online_run_mlp_list(None if t is None else C.byref(t), None if h is None else h.ref(), L.RULE_SIGNADAM if rule is None else rule,
                                       None if mlp is None else C.byref(mlp), fm_term, idx, xv, corr, n, G, ws, ws_bytes,
                                       None if out is None else C.byref(out), scratch, rank, logit, loss,
                                       None if opt is None else C.byref(opt), None)


def test_online_run_refusals_and_the_empty_stream():
    fmx, L, lib = _lib()
    A, SH, AL, UN = L.ERR_ARG, L.ERR_SHAPE, L.ERR_ALIGN, L.ERR_UNSUPPORTED
    h, m = fmx.Hyper(lr=0.01), _mlp(L)
    t, tm, tf = _fake_table(L.LAYOUT_WEIGHTS), _fake_table(L.LAYOUT_MOMENTS), _fake_table(L.LAYOUT_FTRL)
    mapped = _fake_table(L.LAYOUT_WEIGHTS)
    mapped.field_cols, mapped.n_cols = 0x90000, 2
    based = _fake_table(L.LAYOUT_WEIGHTS)
    based.field_base = 0x90000
    split = _fake_table(L.LAYOUT_WEIGHTS)
    split.n_sort_fields, split.sort_offsets, split.sort_cols, split.max_sort_field_rows = 3, 0x91000, 0x92000, 25
    big = _fake_table(L.LAYOUT_WEIGHTS)                      # a field too large for a 32-bit (index, sample) composite at 4 rows
    big.n_rows, big.max_field_rows = 2 ** 31, 2 ** 30
    need = int(lib.fmx_fm_list_workspace_bytes(C.byref(t), 1, 4))
    assert need == int(lib.fmx_workspace_bytes(C.byref(t), 4)) + 16
    cases = [
        # the list shape and check_list_args's table checks
        ("table", dict(t=None), A, "table"), ("hyper", dict(h=None), A, "hyper"), ("idx", dict(idx=None, n=3), A, "idx"),
        ("N -1", dict(n=-1), A, "N"), ("G 1", dict(G=1), A, "G = 1"), ("G 0", dict(G=0), A, "G = 0"), ("G 17", dict(G=17), UN, "G = 17"),
        ("N G > int32", dict(n=2 ** 29, G=8), A, "int32"), ("rank_out", dict(rank=None, n=3), A, "rank_out"),
        ("field_cols", dict(t=mapped), UN, "field_cols"), ("field_base", dict(t=based), UN, "field_base"),
        ("sort split", dict(t=split), UN, "sort split"),
        # fmx_online_run_mlp_pair's
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
        ("a field beyond the composite", dict(t=big), UN, "composite"),
        ("workspace one byte short", dict(ws_bytes=need - 1), SH, "fmx_fm_list_workspace_bytes"),
        ("workspace without the bias scratch", dict(ws_bytes=need - 16), SH, "16 bytes behind"),
        ("workspace short of the step's", dict(ws_bytes=need - 17), SH, "workspace"),
        # with opt
        ("opt: unknown rule", dict(opt=_opt(L, rule=L.RULE_FTRL)), A, "rule"), ("opt: v null", dict(opt=_opt(L, v=None)), A, "opt->v"),
        ("opt: m null under adam", dict(opt=_opt(L, m=None)), A, "opt->m"), ("opt: beta1 = 1", dict(opt=_opt(L, beta1=1.0)), A, "beta1"),
        ("opt: step < 0", dict(opt=_opt(L, step=-1)), A, "step"), ("opt: step + N > int32", dict(opt=_opt(L, step=2 ** 31 - 5), n=8), A, "step"),
        ("opt: m alignment", dict(opt=_opt(L, m=P + 4)), AL, "aligned"),
        ("opt: rule / layout", dict(opt=_opt(L), t=tm, rule=L.RULE_SGD), A, "FMX_LAYOUT_WEIGHTS"),
        ("opt: adam tables, beta1", dict(opt=_opt(L), t=tm, rule=L.RULE_ADAM, h=fmx.Hyper(beta1=1.0)), A, "beta1"),
        ("opt: adam tables, step + N > int32", dict(opt=_opt(L), t=tm, rule=L.RULE_ADAM, h=fmx.Hyper(step=2 ** 31 - 5), n=8), A, "step"),
        ("opt: NFM on an FTRL table", dict(opt=_opt(L), fm_term=0, t=tf, rule=L.RULE_FTRL), UN, "fm_term"),
        ("opt: workspace one byte short", dict(opt=_opt(L), ws_bytes=need - 1), SH, "workspace"),
    ]
    for what, kw, want, word in cases:
        kw = dict(dict(t=t, h=h, mlp=m, out=_out(L)), **kw)
        rc = _run(lib, L, kw.pop("t"), kw.pop("h"), kw.pop("mlp"), **kw)
        msg = lib.fmx_last_error_string().decode()
        assert rc == want, (what, rc, msg)
        assert word in msg and (RUN in msg or want == AL), (what, msg)
    # N = 0: everything is checked, nothing is launched, and the stream's own buffers may be null; exactly
    # fmx_fm_list_workspace_bytes(table, 1, G) is enough, under either family, for both classes, at every G
    for kw in (dict(), dict(fm_term=0), dict(opt=_opt(L)), dict(opt=_opt(L), t=tm, rule=L.RULE_ADAM), dict(opt=_opt(L), t=tm, rule=L.RULE_ADAGRAD, fm_term=0),
               dict(opt=_opt(L), t=tf, rule=L.RULE_FTRL), dict(rule=L.RULE_SGD), dict(G=2), dict(G=16), dict(corr=P)):
        kw = dict(dict(t=t, G=4), **kw)
        tt = kw.pop("t")
        exact = int(lib.fmx_fm_list_workspace_bytes(C.byref(tt), 1, kw["G"]))
        assert _run(lib, L, tt, h, m, out=_out(L), ws_bytes=exact, idx=None, rank=None, **kw) == L.OK, (kw, lib.fmx_last_error_string())


# ---- the classes ----
@pytest.mark.parametrize("cls", ["DeepFMAdam", "NFMAdam"])
def test_list_loop_on_device_defaults_to_false_and_the_signatures_stand(cls):
    from models.models_online_deep.fm_adam import FMAdam
    klass = _klass(cls)
    assert klass.list_loop_on_device is False
    obj = object.__new__(klass)             # (no GPU: the constructors raise)
    assert obj.list_loop_on_device is False
    object.__setattr__(obj, "list_loop_on_device", True)
    assert obj.list_loop_on_device is True and klass.list_loop_on_device is False
    for name in ("fit_lists", "run_list_experiment"):
        params = inspect.signature(getattr(klass, name)).parameters
        assert list(params) == list(inspect.signature(getattr(FMAdam, name)).parameters) + ["full"]
        assert params["full"].default is False and params["n_neg"].default == 4 and params["negatives"].default is None
    # the switch does not open the refusal of full=False
    with pytest.raises(NotImplementedError, match="pure FM logit"):
        klass.run_list_experiment(obj, [[0, 0]], [[1.0, 1.0]], [1], negatives=[[1]])
    doc = " ".join(klass.run_list_experiment.__doc__.split())
    for word in ("list_loop_on_device", "fmx_online_run_mlp_list", "up front", "not bit for bit"):
        assert word in doc, word


class _Table:
    def __init__(self, kp, mapped=False, split=None):
        self.kp, self.mapped, self._sort_split = kp, mapped, split


def _model(cls, rule, fused, k=10, hidden=10, layers=5, F=10, kp=16, **table):
    """The state _list_device_loop_ok() reads, on an object that never saw a device"""
    import fmx
    obj = object.__new__(_klass(cls))
    e = object.__new__(fmx.FMEngine)
    e.table = _Table(kp, **table)
    for name, value in dict(update_rule=rule, _mlp_fused=object() if fused else None, _engine=e, _table=e.table, embedding_size=k,
                            neuron_per_hidden_layer=hidden, num_hidden_layers=layers, field_size=F).items():
        object.__setattr__(obj, name, value)
    return obj


@pytest.mark.parametrize("cls", ["DeepFMAdam", "NFMAdam"])
def test_list_device_loop_ok(cls):
    ok = lambda *a, **kw: _model(cls, *a, **kw)._list_device_loop_ok()
    # the rules: signadam / sgd, and adam / adagrad with the fused optimizer alone; ftrl never
    assert ok("signadam", False) and ok("sgd", False) and ok("signadam", True)
    assert ok("adam", True) and ok("adagrad", True)
    assert not ok("adam", False) and not ok("adagrad", False) and not ok("ftrl", False) and not ok("ftrl", True)
    # the one-workgroup step's limits (fit mode: k <= 63, hidden <= 64, 1 .. 8 layers), at the longest list
    assert ok("signadam", False, k=63, kp=64) and not ok("signadam", False, k=64, kp=64)
    assert ok("sgd", False, hidden=64) and not ok("sgd", False, hidden=65)
    assert ok("adam", True, layers=8) and not ok("adam", True, layers=9) and not ok("adam", True, layers=0)
    # a network above the LDS cap still runs on the device: the call queues its launches (k = 63, 64 x 8: 33,280 parameters)
    assert ok("adam", True, k=63, kp=64, hidden=64, layers=8)
    # the table: list_online_run_fits -- the fields one wavefront's passes hold, plain fields, no sort split
    assert ok("signadam", False, F=64, kp=16) and not ok("signadam", False, F=65, kp=16)
    assert ok("signadam", False, F=16, kp=64) and not ok("signadam", False, F=17, kp=64)
    assert not ok("signadam", False, mapped=True) and not ok("signadam", False, split=(1, 2))
    # G is a parameter of the check, every list length the step takes
    m = _model(cls, "signadam", False)
    assert all(m._list_device_loop_ok(G) for G in (2, 3, 8, 9, 16))
