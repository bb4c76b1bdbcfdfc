"""fmx_afm_online_run (the attentional FM's online predict-then-fit loop in one call) without a GPU: the symbol and its argument
count, and every refusal that is decided on the host -- each with pointers that are never dereferenced, each naming the entry
point in fmx_last_error_string().  No device is touched."""
import ctypes as C
import os
import re
import subprocess

from test_adaptive_rules_cpu import _fake_table
from test_afm_stream_cpu import _afm, _opt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHO = "fmx_afm_online_run"
N_ARGS = 16


def _lib():
    import fmx
    L = fmx._lib
    return fmx, L, L.load()


def _call(lib, t, h, rule, afm, o, N=8, idx=0x60000, y=0x70000, ws=0x50000, ws_bytes=1 << 40, grad=0xC0000):
    """The call with fake pointers: only ever sent where a host check refuses it, or with N = 0 (everything is checked, nothing
    is launched)."""
    return lib.fmx_afm_online_run(None if t is None else C.byref(t), None if h is None else h.ref(), rule,
                                  None if afm is None else C.byref(afm), idx, None, y, N, ws, ws_bytes, grad,
                                  None if o is None else C.byref(o), None, None, None, None)


def _refused(lib, rc, want, what):
    msg = lib.fmx_last_error_string().decode()
    assert rc == want, (what, rc, msg)
    assert WHO in msg, (what, msg)


def test_symbol_is_declared_listed_and_exported():
    fmx, L, lib = _lib()
    assert WHO in L.EXPORTS
    assert len(lib.fmx_afm_online_run.argtypes) == N_ARGS
    text = open(os.path.join(ROOT, "include", "fmx.h")).read()
    decl = re.search(r"\bint " + WHO + r"\(([^;]*)\);", text)
    assert decl and len(decl.group(1).split(",")) == N_ARGS
    args = [a.strip() for a in decl.group(1).split(",")]
    assert args[7] == "int32_t N" and args[11] == "const fmx_mlp_opt_t *opt" and args[12] == "float *logit_out"
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT " + WHO + r"$", out, re.M)
    assert lib.fmx_version() == 104          # the symbol is what a caller probes for


def test_null_arguments():
    fmx, L, lib = _lib()
    t, h, o = _fake_table(L.LAYOUT_MOMENTS), fmx.Hyper(lr=0.01), _opt(L, L.RULE_ADAM)
    _refused(lib, _call(lib, None, h, L.RULE_ADAM, _afm(L), o), L.ERR_ARG, "null table")
    _refused(lib, _call(lib, t, h, L.RULE_ADAM, None, o), L.ERR_ARG, "null afm")
    _refused(lib, _call(lib, t, h, L.RULE_ADAM, _afm(L), None), L.ERR_ARG, "null opt")
    _refused(lib, _call(lib, t, h, L.RULE_ADAM, _afm(L), o, idx=None), L.ERR_ARG, "null idx")
    _refused(lib, _call(lib, t, h, L.RULE_ADAM, _afm(L), o, y=None), L.ERR_ARG, "null y")
    _refused(lib, _call(lib, t, None, L.RULE_ADAM, _afm(L), o), L.ERR_ARG, "null hyper")
    _refused(lib, _call(lib, t, h, L.RULE_ADAM, _afm(L), o, grad=None), L.ERR_ARG, "null attn_grad_out")
    _refused(lib, _call(lib, t, h, L.RULE_ADAM, _afm(L), o, ws=None), L.ERR_ARG, "null workspace")


def test_stream_length_and_rules():
    fmx, L, lib = _lib()
    t, h, o = _fake_table(L.LAYOUT_MOMENTS), fmx.Hyper(lr=0.01), _opt(L, L.RULE_ADAM)
    _refused(lib, _call(lib, t, h, L.RULE_ADAM, _afm(L), o, N=-1), L.ERR_ARG, "N < 0")
    for rule in (7, -1, L.RULE_SGD, L.RULE_FTRL):            # unknown, or not the moments layout's
        _refused(lib, _call(lib, t, h, rule, _afm(L), o), L.ERR_ARG, f"table rule {rule}")
    for rule in (7, -1, L.RULE_FTRL):
        _refused(lib, _call(lib, t, h, L.RULE_ADAM, _afm(L), _opt(L, rule)), L.ERR_ARG, f"attention rule {rule}")
    # N = 0 with everything in order: nothing to launch, under every pairing of the rules
    for layout, trule in ((L.LAYOUT_WEIGHTS, L.RULE_SIGNADAM), (L.LAYOUT_WEIGHTS, L.RULE_SGD), (L.LAYOUT_FTRL, L.RULE_FTRL),
                          (L.LAYOUT_MOMENTS, L.RULE_ADAGRAD), (L.LAYOUT_MOMENTS, L.RULE_ADAM)):
        for arule, kw in ((L.RULE_SIGNADAM, dict(m=None, v=None)), (L.RULE_SGD, dict(m=None, v=None)),
                          (L.RULE_ADAGRAD, dict(m=None)), (L.RULE_ADAM, {})):
            rc = _call(lib, _fake_table(layout), h, trule, _afm(L), _opt(L, arule, **kw), N=0)
            assert rc == L.OK, (layout, trule, arule, lib.fmx_last_error_string())


def test_optimizer_state():
    fmx, L, lib = _lib()
    t, h = _fake_table(L.LAYOUT_MOMENTS), fmx.Hyper(lr=0.01)
    A, AL = L.ERR_ARG, L.ERR_ALIGN
    for what, okw, akw, want in [
            ("v null under adagrad", dict(rule=L.RULE_ADAGRAD, v=None), {}, A),
            ("v null under adam", dict(rule=L.RULE_ADAM, v=None), {}, A),
            ("m null under adam", dict(rule=L.RULE_ADAM, m=None), {}, A),
            ("beta1 = 1", dict(rule=L.RULE_ADAM, beta1=1.0), {}, A),
            ("beta1 < 0", dict(rule=L.RULE_ADAM, beta1=-0.5), {}, A),
            ("beta2 = 1", dict(rule=L.RULE_ADAM, beta2=1.0), {}, A),
            ("beta2 < 0", dict(rule=L.RULE_ADAM, beta2=-0.1), {}, A),
            ("step < 0", dict(rule=L.RULE_SGD, step=-1), {}, A),
            ("m misaligned", dict(rule=L.RULE_ADAM, m=0xD0004), {}, AL),
            ("v misaligned", dict(rule=L.RULE_ADAGRAD, v=0xE0008), {}, AL),
            ("params misaligned", dict(rule=L.RULE_ADAM), dict(params=0x80004), AL)]:
        _refused(lib, _call(lib, t, h, L.RULE_ADAM, _afm(L, **akw), _opt(L, **okw)), want, what)


def test_step_counts_stay_within_int32():
    fmx, L, lib = _lib()
    t, h = _fake_table(L.LAYOUT_MOMENTS), fmx.Hyper(lr=0.01)
    # the attention parameters' count
    assert _call(lib, t, h, L.RULE_ADAM, _afm(L), _opt(L, L.RULE_ADAM, step=2 ** 31 - 1), N=0) == L.OK
    _refused(lib, _call(lib, t, h, L.RULE_ADAM, _afm(L), _opt(L, L.RULE_ADAM, step=2 ** 31 - 8), N=8), L.ERR_ARG, "opt->step + N")
    _refused(lib, _call(lib, t, h, L.RULE_ADAGRAD, _afm(L), _opt(L, L.RULE_SGD, step=2 ** 31 - 8), N=8), L.ERR_ARG, "opt->step + N, sgd")
    # the tables' count, read under their ADAM alone
    o = _opt(L, L.RULE_ADAM)
    assert _call(lib, t, fmx.Hyper(step=2 ** 31 - 9), L.RULE_ADAM, _afm(L), o, N=0) == L.OK
    _refused(lib, _call(lib, t, fmx.Hyper(step=2 ** 31 - 5), L.RULE_ADAM, _afm(L), o, N=8), L.ERR_ARG, "hyper->step + N")
    _refused(lib, _call(lib, t, fmx.Hyper(step=-1), L.RULE_ADAM, _afm(L), o, N=1), L.ERR_ARG, "hyper->step < 0")
    _refused(lib, _call(lib, t, fmx.Hyper(beta1=1.0), L.RULE_ADAM, _afm(L), o, N=1), L.ERR_ARG, "hyper->beta1")
    assert _call(lib, t, fmx.Hyper(step=2 ** 31 - 5), L.RULE_ADAGRAD, _afm(L), o, N=0) == L.OK      # adagrad reads no count


def test_workspace_and_table():
    fmx, L, lib = _lib()
    t, h, o = _fake_table(L.LAYOUT_MOMENTS), fmx.Hyper(lr=0.01), _opt(L, L.RULE_ADAM)
    need = lib.fmx_afm_workspace_bytes(C.byref(t), C.byref(_afm(L)), 1)
    assert need > 0
    assert _call(lib, t, h, L.RULE_ADAM, _afm(L), o, N=0, ws_bytes=need) == L.OK
    _refused(lib, _call(lib, t, h, L.RULE_ADAM, _afm(L), o, ws_bytes=need - 1), L.ERR_SHAPE, "workspace short")
    _refused(lib, _call(lib, t, h, L.RULE_ADAM, _afm(L), o, ws=0x50004), L.ERR_ALIGN, "workspace misaligned")
    _refused(lib, _call(lib, t, h, L.RULE_ADAM, _afm(L, k=8), o), L.ERR_SHAPE, "afm->k")
    _refused(lib, _call(lib, t, h, L.RULE_ADAM, _afm(L, t=65), o), L.ERR_UNSUPPORTED, "t = 65")
    mapped = _fake_table(L.LAYOUT_MOMENTS)
    mapped.field_cols, mapped.n_cols = 0x40000, 2
    _refused(lib, _call(lib, mapped, h, L.RULE_ADAM, _afm(L), o), L.ERR_UNSUPPORTED, "mapped table")
    mapped = _fake_table(L.LAYOUT_MOMENTS)
    mapped.field_base = 0x40000
    _refused(lib, _call(lib, mapped, h, L.RULE_ADAM, _afm(L), o), L.ERR_UNSUPPORTED, "mapped table (field_base)")


def test_option_returns_the_previous_value():
    fmx, L, lib = _lib()
    try:
        assert lib.fmx_set_option(b"afm_online_persistent", 0) == 1          # the default
        assert lib.fmx_set_option(b"afm_online_persistent", 1) == 0
    finally:
        lib.fmx_set_option(b"afm_online_persistent", 1)
    assert lib.fmx_set_option(b"afm_online_persistent", 1) == 1


def test_python_surface():
    import inspect
    import fmx
    assert list(inspect.signature(fmx.AFMEngine.online_run).parameters)[1:] == ["hyper", "rule", "idx_d", "xv_d", "y_d", "opt",
                                                                                "logits", "losses", "stream"]
    from models.models_online_deep.afm_adam import AFMAdam
    assert list(inspect.signature(AFMAdam.run_online_experiment).parameters) == ["self", "data_Xi", "data_Xv", "data_Y"]
    assert callable(AFMAdam.run_experiment)
