"""The list loss of DeepFM / NFM without a GPU: the symbols fmx_mlp_list_section and fmx_deepfm_list_stream, every refusal they
decide on the host (fake pointers that are never dereferenced), both workspace checks one byte short, the empty stream, and the
classes' fit_lists / run_list_experiment(full=...) signatures and refusals.  No device is touched."""
import ctypes as C
import importlib
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from test_adaptive_rules_cpu import _fake_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SECTION, STREAM = "fmx_mlp_list_section", "fmx_deepfm_list_stream"
N_ARGS = {SECTION: 19, STREAM: 24}


def _lib():
    import fmx
    L = fmx._lib
    return fmx, L, L.load()


@pytest.mark.parametrize("who", [SECTION, STREAM])
def test_symbol_is_declared_listed_and_exported(who):
    fmx, L, lib = _lib()
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert who in set(re.findall(r"\bT\s+(fmx_\w+)", out))
    assert who in L.EXPORTS and len(getattr(lib, who).argtypes) == N_ARGS[who]
    header = open(os.path.join(ROOT, "include", "fmx.h")).read()
    decl = re.search(r"\bint " + who + r"\(([^;]*)\);", header)
    assert decl and len(decl.group(1).split(",")) == N_ARGS[who]
    # declared behind the pair forms they mirror
    assert header.index("int fmx_deepfm_pair_stream(") < decl.start()
    text = " ".join(header[:decl.start()].rsplit("/*", 1)[1].split())
    assert "Replaces:" in text and who in text


def _mlp(L, k=16, hidden=64, layers=2, params=0x40000):
    return L.Mlp(params, layers, k, hidden, 0)


def _opt(L, rule=None, m=0x50000, v=0x51000, step=0, beta1=0.9):
    return L.MlpOpt(m, v, 0.01, 1e-8, beta1, 0.999, L.RULES["adam"] if rule is None else rule, step)


def _section(lib, L, mlp, bi=0x60000, ld_bi=16, base=0x61000, corr=None, B=4, G=4, ws=0x80000, ws_bytes=None, logit=None, dz=0x62000,
             gbi=0x63000, ld_gbi=16, grads=0x64000, opt=None):
    """fmx_mlp_list_section with fake pointers: only ever sent where a host check answers it."""
    if ws_bytes is None:
        ws_bytes = 0 if mlp is None else max(int(lib.fmx_mlp_section_workspace_bytes(C.byref(mlp), max(B * G, 1))), 0)
    return lib.fmx_mlp_list_section(None if mlp is None else C.byref(mlp), bi, ld_bi, base, corr, B, G, 0.25, ws, ws_bytes, logit, dz, gbi,
                                    ld_gbi, grads, 0.0, None if opt is None else C.byref(opt), None, None)


def test_section_refusals():
    fmx, L, lib = _lib()
    A, UN, SH, AL = L.ERR_ARG, L.ERR_UNSUPPORTED, L.ERR_SHAPE, L.ERR_ALIGN
    m = _mlp(L)
    need = int(lib.fmx_mlp_section_workspace_bytes(C.byref(m), 16))
    assert need > 0
    cases = [
        ("B_lists 0", dict(B=0), A, "B_lists = 0"),
        ("B_lists -2", dict(B=-2), A, "B_lists = -2"),
        ("G 1", dict(G=1), A, "G = 1"),
        ("G 0", dict(G=0), A, "G = 0"),
        ("G 17", dict(G=17), UN, "G = 17"),
        ("rows beyond int32", dict(B=2 ** 28, G=8, ws_bytes=1 << 40), A, "int32"),
        ("mlp", dict(mlp=None), A, "null"),
        ("params", dict(mlp=_mlp(L, params=None), ws_bytes=need), A, "null"),
        ("workspace", dict(ws=None), A, "null"),
        ("workspace alignment", dict(ws=0x80004), AL, "aligned"),
        ("no layers", dict(mlp=_mlp(L, layers=0), ws_bytes=need), UN, "layers"),
        ("workspace one byte short", dict(ws_bytes=need - 1), SH, "fmx_mlp_section_workspace_bytes"),
        ("bi", dict(bi=None), A, "null"),
        ("base", dict(base=None), A, "null"),
        ("dz_out", dict(dz=None), A, "null"),
        ("gbi_out", dict(gbi=None), A, "null"),
        ("grads", dict(grads=None), A, "null"),
        ("ld_bi", dict(ld_bi=15), SH, "ld_bi"),
        ("ld_gbi", dict(ld_gbi=12), SH, "ld_gbi"),
        # with opt: the shape first, then what fmx_mlp_section_opt refuses
        ("opt: G 17", dict(G=17, opt=_opt(L)), UN, "G = 17"),
        ("opt: unknown rule", dict(opt=_opt(L, rule=L.RULES["signadam"])), A, "rule"),
        ("opt: v", dict(opt=_opt(L, v=None)), A, "opt->v"),
        ("opt: m under adam", dict(opt=_opt(L, m=None)), A, "opt->m"),
        ("opt: beta1", dict(opt=_opt(L, beta1=1.0)), A, "beta1"),
        ("opt: step", dict(opt=_opt(L, step=2 ** 31 - 1)), A, "step"),
        ("opt: alignment", dict(opt=_opt(L, v=0x51004)), AL, "aligned"),
        ("opt: workspace one byte short", dict(opt=_opt(L), ws_bytes=need - 1), SH, "fmx_mlp_section_workspace_bytes"),
    ]
    for what, kw, want, word in cases:
        kw = dict(dict(mlp=m), **kw)
        rc = _section(lib, L, kw.pop("mlp"), **kw)
        msg = lib.fmx_last_error_string().decode()
        assert rc == want, (what, rc, msg)
        assert msg and word in msg, (what, msg)
        assert SECTION in msg or want == AL and "workspace must be" in msg, (what, msg)      # (mlp_big_check's alignment message is shared)


def _fwd(L, S=0x70000, bi=0x71000, logit=0x72000, sfirst=0x73000, sample_ld=0):
    o = L.FwdOut()
    o.S, o.bi, o.logit, o.sfirst, o.sample_ld = S, bi, logit, sfirst, sample_ld
    return o


def _stream(lib, L, t, h, rule=None, mlp="default", fm_term=1, idx=0x60000, n_pool=2, B=4, G=4, corr=None, n_steps=0, ws=0x80000,
            ws_bytes=None, mws=0x90000, mws_bytes=None, fwd="default", dz=0x62000, gbi=0x63000, grads=0x64000, opt=None):
    """fmx_deepfm_list_stream with fake pointers and n_steps = 0 by default: nothing is ever launched."""
    mlp = _mlp(L) if mlp == "default" else mlp
    fwd = _fwd(L) if fwd == "default" else fwd
    rows = max(B * G, 1) if 0 < B * G < 2 ** 31 else 1
    if ws_bytes is None:
        ws_bytes = 0 if t is None or not 2 <= G <= 16 or B < 1 or B * G >= 2 ** 31 else max(int(lib.fmx_fm_list_workspace_bytes(C.byref(t), B, G)), 0)
    if mws_bytes is None:
        mws_bytes = 0 if mlp is None else max(int(lib.fmx_mlp_section_workspace_bytes(C.byref(mlp), rows)), 0)
    rule = L.RULE_SIGNADAM if rule is None else rule
    return lib.fmx_deepfm_list_stream(None if t is None else C.byref(t), None if h is None else h.ref(), rule,
                                      None if mlp is None else C.byref(mlp), fm_term, idx, n_pool, B, G, corr, 0.25, n_steps, ws, ws_bytes,
                                      mws, mws_bytes, None if fwd is None else C.byref(fwd), dz, gbi, grads, 0.05,
                                      None if opt is None else C.byref(opt), None, None)


def test_stream_refusals_workspaces_and_the_empty_stream():
    fmx, L, lib = _lib()
    A, UN, SH, AL = L.ERR_ARG, L.ERR_UNSUPPORTED, L.ERR_SHAPE, L.ERR_ALIGN
    h = fmx.Hyper(lr=0.01)
    t = _fake_table(L.LAYOUT_WEIGHTS)
    mom = _fake_table(L.LAYOUT_MOMENTS)
    ftrl = _fake_table(L.LAYOUT_FTRL)
    mapped = _fake_table(L.LAYOUT_WEIGHTS)
    mapped.field_cols, mapped.n_cols = 0x90000, 2
    big = _fake_table(L.LAYOUT_WEIGHTS)                      # a field too large for a 32-bit (index, sample) composite at 16 rows
    big.n_rows, big.max_field_rows = 2 ** 31, 2 ** 30
    need = int(lib.fmx_fm_list_workspace_bytes(C.byref(t), 4, 4))
    assert need == int(lib.fmx_workspace_bytes(C.byref(t), 16)) + 16
    mneed = int(lib.fmx_mlp_section_workspace_bytes(C.byref(_mlp(L)), 16))
    cases = [
        # check_list_args
        ("table", dict(t=None), A, "table"),
        ("hyper", dict(h=None), A, "hyper"),
        ("idx_pool", dict(idx=None), A, "idx"),
        ("B_lists 0", dict(B=0), A, "B_lists = 0"),
        ("G 1", dict(G=1), A, "G = 1"),
        ("G 17", dict(G=17), UN, "G = 17"),
        ("rows beyond int32", dict(B=2 ** 28, G=8), A, "int32"),
        ("field_cols", dict(t=mapped), UN, "field_cols"),
        # check_sort_geometry on B_lists G rows
        ("beyond the sort's width", dict(B=4096, G=16), UN, "sort width"),
        ("a field beyond the composite", dict(t=big), UN, "composite"),
        # check_pool_steps
        ("n_pool 0", dict(n_pool=0), A, "n_pool = 0"),
        ("n_steps -1", dict(n_steps=-1), A, "n_steps = -1"),
        # the network and opt, as fmx_deepfm_stream / fmx_deepfm_stream_opt check them
        ("adam tables without opt", dict(t=mom, rule=L.RULE_ADAM), UN, "FMX_RULE_ADAM"),
        ("ftrl rule on a weights table", dict(rule=L.RULE_FTRL), A, "FMX_RULE_FTRL"),
        ("mlp", dict(mlp=None), A, "null"),
        ("workspace", dict(ws=None), A, "null"),
        ("mlp_workspace", dict(mws=None), A, "null"),
        ("fwd", dict(fwd=None), A, "null"),
        ("fwd->bi", dict(fwd=_fwd(L, bi=None)), A, "bi"),
        ("fwd->logit", dict(fwd=_fwd(L, logit=None)), A, "logit"),
        ("dz", dict(dz=None), A, "null"),
        ("gbi", dict(gbi=None), A, "null"),
        ("grads", dict(grads=None), A, "null"),
        ("sample_ld", dict(fwd=_fwd(L, sample_ld=32)), A, "sample_ld"),
        ("NFM without sfirst", dict(fm_term=0, fwd=_fwd(L, sfirst=None)), UN, "fm_term = 0"),
        ("NFM on an FTRL table", dict(fm_term=0, t=ftrl, rule=L.RULE_FTRL), UN, "fm_term = 0"),
        ("NFM on a moments table without opt", dict(fm_term=0, t=mom, rule=L.RULE_ADAM), UN, "FMX_RULE_ADAM"),
        ("no layers", dict(mlp=_mlp(L, layers=0), mws_bytes=mneed), UN, "layers"),
        ("k beyond kp", dict(mlp=_mlp(L, k=20)), SH, "k=20"),
        ("dz alignment", dict(dz=0x62004), AL, "aligned"),
        ("opt: adam betas of the tables", dict(t=mom, rule=L.RULE_ADAM, h=fmx.Hyper(beta1=1.0), opt=_opt(L)), A, "beta1"),
        ("opt: v", dict(opt=_opt(L, v=None)), A, "opt->v"),
        ("opt: steps beyond int32", dict(opt=_opt(L, step=2 ** 31 - 3), n_steps=8), A, "step"),
        # both workspaces, one byte short, under either rule of the network
        ("MLP workspace one byte short", dict(mws_bytes=mneed - 1), SH, "fmx_mlp_section_workspace_bytes"),
        ("MLP workspace one byte short (opt)", dict(mws_bytes=mneed - 1, opt=_opt(L)), SH, "fmx_mlp_section_workspace_bytes"),
        ("workspace one byte short", dict(ws_bytes=need - 1), SH, "fmx_fm_list_workspace_bytes"),
        ("workspace without the bias scratch", dict(ws_bytes=need - 16), SH, "16 bytes behind"),
        ("workspace short of the step's", dict(ws_bytes=need - 17), SH, "workspace"),
    ]
    for what, kw, want, word in cases:
        kw = dict(dict(t=t, h=h), **kw)
        rc = _stream(lib, L, kw.pop("t"), kw.pop("h"), **kw)
        msg = lib.fmx_last_error_string().decode()
        assert rc == want, (what, rc, msg)
        assert msg and STREAM in msg and word in msg, (what, msg)
    # the empty stream: FMX_OK under either rule of the network, DeepFM and NFM, with and without corr_pool
    assert _stream(lib, L, t, h) == L.OK
    assert _stream(lib, L, t, h, fm_term=0, corr=0xA0000) == L.OK
    assert _stream(lib, L, mom, fmx.Hyper(lr=0.01), rule=L.RULE_ADAM, opt=_opt(L)) == L.OK
    assert _stream(lib, L, ftrl, h, rule=L.RULE_FTRL, ws_bytes=int(lib.fmx_fm_list_workspace_bytes(C.byref(ftrl), 4, 4))) == L.OK


def _klass(cls):
    mod = {"DeepFMAdam": "deepfm_adam", "NFMAdam": "nfm_adam", "DeepFMOnn": "deepfm_onn", "NFMOnn": "nfm_onn"}[cls]
    return getattr(importlib.import_module("models.models_online_deep." + mod), cls)


@pytest.mark.parametrize("cls", ["DeepFMAdam", "NFMAdam"])
def test_signatures_and_refusals_of_the_network_classes(cls):
    from fmx.pairwise import HardNegatives, PopularityNegatives
    from models.models_online_deep.fm_adam import FMAdam
    klass = _klass(cls)
    obj = object.__new__(klass)             # (no GPU: the constructors raise; these refusals need no state)
    for method in ("fit_lists", "run_list_experiment"):
        params = inspect.signature(getattr(klass, method)).parameters
        assert list(params) == list(inspect.signature(getattr(FMAdam, method)).parameters) + ["full"]
        assert params["full"].default is False and params["n_neg"].default == 4 and params["negatives"].default is None
        call = lambda **kw: getattr(klass, method)(obj, [[0, 0]], [[1.0, 1.0]], [1], **kw)
        # full=False: today's refusal, whatever the negatives
        for negatives in ([[1]], None, "hard", PopularityNegatives(np.ones(5))):
            with pytest.raises(NotImplementedError, match="pure FM logit") as ei:
                call(negatives=negatives)
            assert cls in str(ei.value) and method in str(ei.value)
        # full=True: mined negatives are refused by name, as fit_pairs(full=True) refuses them
        for negatives in ("hard", HardNegatives(8)):
            with pytest.raises(NotImplementedError, match="negatives='hard'") as ei:
                call(negatives=negatives, full=True)
            assert cls in str(ei.value) and method in str(ei.value)
        # ... and a count of drawn negatives outside 1 .. 15 before the model is looked at
        for negatives in (None, PopularityNegatives(np.ones(5))):
            for n_neg in (0, 16):
                with pytest.raises(ValueError, match="15") as ei:
                    call(negatives=negatives, n_neg=n_neg, full=True)
                assert cls in str(ei.value) and method in str(ei.value)


@pytest.mark.parametrize("cls", ["DeepFMOnn", "NFMOnn"])
def test_the_onn_classes_refuse_under_full_as_well(cls):
    klass = _klass(cls)
    obj = object.__new__(klass)
    for method in ("fit_lists", "run_list_experiment"):
        assert list(inspect.signature(getattr(klass, method)).parameters)[-1] == "full"
        for full in (False, True):
            with pytest.raises(NotImplementedError, match="pure FM logit") as ei:
                getattr(klass, method)(obj, [[0, 0]], [[1.0, 1.0]], [1], negatives=[[1]], full=full)
            assert cls in str(ei.value) and method in str(ei.value)
