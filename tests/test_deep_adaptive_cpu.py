"""fmx_mlp_section_opt / fmx_deepfm_stream_opt (DeepFM / NFM with the network under a persistent rule of its own) without a
GPU: the symbols and their argument counts, the C layout of fmx_mlp_opt_t, and every refusal that is decided on the host --
each with pointers that are never dereferenced, each naming its entry point in fmx_last_error_string().  No device is touched."""
import ctypes as C
import os
import subprocess

import pytest

from test_adaptive_rules_cpu import _fake_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    import fmx
    L = fmx._lib
    return fmx, L, L.load()


def _opt(L, rule, m=0xD0000, v=0xE0000, lr=0.01, eps=1e-8, beta1=0.9, beta2=0.999, step=0):
    return L.MlpOpt(m, v, lr, eps, beta1, beta2, rule, step)


def _mlp(L, params=0x80000, n_layers=2, k=16, hidden=32):
    return L.Mlp(params, n_layers, k, hidden, 0)


def _section(lib, L, m, o, B=64, ws=0x90000, ws_bytes=1 << 40, grads=0xC0000, bi=0x40000):
    return lib.fmx_mlp_section_opt(C.byref(m), L.LOSS_BCE_LOGITS, bi, 16, 0x41000, 0x70000, B, 1.0 / B, ws, ws_bytes, None,
                                   0xA0000, 0xB0000, 16, grads, None if o is None else C.byref(o), None, None)


def _stream(lib, L, t, h, rule, m, o, fm_term=1, B=64, n_steps=1, ws_bytes=1 << 40, mlp_ws=0x90000, mlp_ws_bytes=1 << 40,
            grads=0xC0000, sfirst=True):
    out = L.FwdOut()
    out.S = out.bi = out.logit = out.dz = out.loss = 0x40000
    out.sfirst = 0x40000 if sfirst else None
    return lib.fmx_deepfm_stream_opt(C.byref(t), h.ref(), rule, C.byref(m), L.LOSS_BCE_LOGITS, fm_term, 0x60000, 0x70000, 1, B,
                                     1.0 / B, n_steps, 0x50000, ws_bytes, mlp_ws, mlp_ws_bytes, C.byref(out), 0xA0000, 0xB0000,
                                     grads, None if o is None else C.byref(o), None, None)


def test_symbols_and_argument_counts():
    fmx, L, lib = _lib()
    assert "fmx_mlp_section_opt" in L.EXPORTS and "fmx_deepfm_stream_opt" in L.EXPORTS
    # fmx_mlp_section's 17 arguments with lr_apply replaced by opt, plus the workspace's size
    assert len(lib.fmx_mlp_section_opt.argtypes) == len(lib.fmx_mlp_section.argtypes) + 1 == 18
    # fmx_deepfm_stream's 22 with lr_mlp replaced by opt, plus the MLP workspace's size
    assert len(lib.fmx_deepfm_stream_opt.argtypes) == len(lib.fmx_deepfm_stream.argtypes) + 1 == 23
    assert lib.fmx_version() == 104          # the new symbols are what a caller probes for


def test_header_declares_the_calls_with_those_counts():
    import re
    text = open(os.path.join(ROOT, "include", "fmx.h")).read()
    for name, n in (("fmx_mlp_section_opt", 18), ("fmx_deepfm_stream_opt", 23)):
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", text)
        assert decl, name
        assert len(decl.group(1).split(",")) == n, name


def test_mlp_opt_struct_matches_the_header(tmp_path):
    fmx, L, lib = _lib()
    S = L.MlpOpt
    names = [f[0] for f in S._fields_]
    assert names == ["m", "v", "lr", "eps", "beta1", "beta2", "rule", "step"]
    src = tmp_path / "opt.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fmx.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(fmx_mlp_opt_t));\n'
                   + "".join(f'  printf(" %zu", offsetof(fmx_mlp_opt_t, {n}));\n' for n in names) + "  return 0;\n}\n")
    exe = tmp_path / "opt"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(S)] + [getattr(S, n).offset for n in names]
    assert C.sizeof(S) == 40


def _refusals(L):
    """(what, keyword arguments of _opt / of the call, expected status): the host-decided refusals the two calls share."""
    A, AL, SH = L.ERR_ARG, L.ERR_ALIGN, L.ERR_SHAPE
    return [
        ("opt null", dict(opt=None), {}, A),
        ("unknown rule", dict(opt=dict(rule=L.RULE_FTRL)), {}, A),
        ("signadam is not a network rule", dict(opt=dict(rule=L.RULE_SIGNADAM)), {}, A),
        ("rule 7", dict(opt=dict(rule=7)), {}, A),
        ("v null", dict(opt=dict(rule=L.RULE_ADAGRAD, v=None)), {}, A),
        ("v null under sgd", dict(opt=dict(rule=L.RULE_SGD, v=None)), {}, A),
        ("m null under adam", dict(opt=dict(rule=L.RULE_ADAM, m=None)), {}, A),
        ("beta1 = 1", dict(opt=dict(rule=L.RULE_ADAM, beta1=1.0)), {}, A),
        ("beta2 < 0", dict(opt=dict(rule=L.RULE_ADAM, beta2=-0.1)), {}, A),
        ("step < 0", dict(opt=dict(rule=L.RULE_ADAM, step=-1)), {}, A),
        ("step overflows", dict(opt=dict(rule=L.RULE_ADAM, step=2 ** 31 - 1)), {}, A),
        ("m misaligned", dict(opt=dict(rule=L.RULE_ADAM, m=0xD0004)), {}, AL),
        ("v misaligned", dict(opt=dict(rule=L.RULE_ADAGRAD, v=0xE0008)), {}, AL),
        ("grads misaligned", dict(opt=dict(rule=L.RULE_ADAM)), dict(grads=0xC0004), AL),
        ("params misaligned", dict(opt=dict(rule=L.RULE_ADAM), params=0x80004), {}, AL),
    ]


@pytest.mark.parametrize("who", ["fmx_mlp_section_opt", "fmx_deepfm_stream_opt"])
def test_host_decided_refusals_name_the_entry_point(who):
    fmx, L, lib = _lib()
    t = _fake_table(L.LAYOUT_MOMENTS)
    h = fmx.Hyper(lr=0.01)
    for what, kw, call_kw, want in _refusals(L):
        o = None if kw.get("opt", {}) is None else _opt(L, **kw["opt"])
        m = _mlp(L, params=kw.get("params", 0x80000))
        rc = _section(lib, L, m, o, **call_kw) if who == "fmx_mlp_section_opt" else _stream(lib, L, t, h, L.RULE_ADAM, m, o, **call_kw)
        msg = lib.fmx_last_error_string().decode()
        assert rc == want, (who, what, rc, msg)
        assert who in msg, (what, msg)
    # m may be null under adagrad and sgd: the call gets past the optimizer's checks to the workspace size
    for rule in (L.RULE_ADAGRAD, L.RULE_SGD):
        o, m = _opt(L, rule, m=None), _mlp(L)
        rc = _section(lib, L, m, o, ws_bytes=16) if who == "fmx_mlp_section_opt" else _stream(lib, L, t, h, L.RULE_ADAM, m, o, mlp_ws_bytes=16)
        assert rc == L.ERR_SHAPE, (who, rule, lib.fmx_last_error_string())


@pytest.mark.parametrize("who", ["fmx_mlp_section_opt", "fmx_deepfm_stream_opt"])
def test_the_mlp_workspace_size_is_checked(who):
    fmx, L, lib = _lib()
    t = _fake_table(L.LAYOUT_MOMENTS)
    h = fmx.Hyper(lr=0.01)
    m, o = _mlp(L), _opt(L, L.RULE_ADAM)
    need = lib.fmx_mlp_section_workspace_bytes(C.byref(m), 64)
    assert need > 0
    call = ((lambda n: _section(lib, L, m, o, ws_bytes=n)) if who == "fmx_mlp_section_opt"
            else (lambda n: _stream(lib, L, t, h, L.RULE_ADAM, m, o, mlp_ws_bytes=n)))
    for n in (0, need - 1):
        rc = call(n)
        msg = lib.fmx_last_error_string().decode()
        assert rc == L.ERR_SHAPE and who in msg and "fmx_mlp_section_workspace_bytes" in msg, (n, rc, msg)


def test_stream_opt_pairs_table_rules_and_layouts():
    """ADAM on a MOMENTS table gets past the rule checks (the next refusal is the MLP workspace's size, FMX_ERR_SHAPE); ADAM on a
    WEIGHTS table is FMX_ERR_ARG, as everywhere; the weights rules are still taken on a weights table."""
    fmx, L, lib = _lib()
    h = fmx.Hyper(lr=0.01)
    m, o = _mlp(L), _opt(L, L.RULE_ADAM)
    for layout, rule, want in [(L.LAYOUT_MOMENTS, L.RULE_ADAM, L.ERR_SHAPE), (L.LAYOUT_MOMENTS, L.RULE_ADAGRAD, L.ERR_SHAPE),
                               (L.LAYOUT_WEIGHTS, L.RULE_SIGNADAM, L.ERR_SHAPE), (L.LAYOUT_FTRL, L.RULE_FTRL, L.ERR_SHAPE),
                               (L.LAYOUT_WEIGHTS, L.RULE_ADAM, L.ERR_ARG), (L.LAYOUT_WEIGHTS, L.RULE_ADAGRAD, L.ERR_ARG),
                               (L.LAYOUT_MOMENTS, L.RULE_SIGNADAM, L.ERR_ARG), (L.LAYOUT_FTRL, L.RULE_ADAM, L.ERR_ARG)]:
        rc = _stream(lib, L, _fake_table(layout), h, rule, m, o, mlp_ws_bytes=16)
        msg = lib.fmx_last_error_string().decode()
        assert rc == want, (layout, rule, rc, msg)
        if want == L.ERR_SHAPE:
            assert "fmx_deepfm_stream_opt" in msg and "fmx_mlp_section_workspace_bytes" in msg, msg
    # the tables' own adam hyper-parameters are checked as fmx_fm_stream checks them
    for bad in (fmx.Hyper(beta1=1.0), fmx.Hyper(step=-1), fmx.Hyper(step=2 ** 31 - 1)):
        assert _stream(lib, L, _fake_table(L.LAYOUT_MOMENTS), bad, L.RULE_ADAM, m, o) == L.ERR_ARG
    # the call's steps count against the network's step too
    assert _stream(lib, L, _fake_table(L.LAYOUT_MOMENTS), h, L.RULE_ADAM, m, _opt(L, L.RULE_ADAM, step=2 ** 31 - 5), n_steps=8) == L.ERR_ARG


def test_stream_opt_nfm_layouts():
    """fm_term = 0 (NFM): weights and moments tables pass (to the next check), FTRL tables and a missing sfirst are refused."""
    fmx, L, lib = _lib()
    h = fmx.Hyper(lr=0.01)
    m, o = _mlp(L), _opt(L, L.RULE_ADAM)
    for layout, rule, want in [(L.LAYOUT_MOMENTS, L.RULE_ADAM, L.ERR_SHAPE), (L.LAYOUT_WEIGHTS, L.RULE_SGD, L.ERR_SHAPE),
                               (L.LAYOUT_FTRL, L.RULE_FTRL, L.ERR_UNSUPPORTED)]:
        rc = _stream(lib, L, _fake_table(layout), h, rule, m, o, fm_term=0, mlp_ws_bytes=16)
        assert rc == want, (layout, rc, lib.fmx_last_error_string())
    rc = _stream(lib, L, _fake_table(L.LAYOUT_MOMENTS), h, L.RULE_ADAM, m, o, fm_term=0, sfirst=False)
    assert rc == L.ERR_UNSUPPORTED and b"fmx_deepfm_stream_opt" in lib.fmx_last_error_string()


def test_python_surface():
    import inspect
    import fmx
    assert "mlp_opt" in inspect.signature(fmx.FMEngine.mlp_section).parameters
    assert "mlp_opt" in inspect.signature(fmx.FMEngine.prepare_deepfm_stream).parameters
    assert issubclass(fmx.HipDeepOptBackend, fmx.HipDeepBackend)
    be = fmx.HipDeepOptBackend(None, fmx.Hyper(), "adam", object())     # the adaptive rules are taken; HipDeepBackend's refusal stays
    assert be.rule == "adam"
    with pytest.raises(ValueError):
        fmx.HipDeepBackend(None, fmx.Hyper(), "adam")
    with pytest.raises(ValueError):
        fmx.MlpOpt(8, "signadam", device="cpu")
    o = fmx.MlpOpt(8, "adagrad", device="cpu")
    assert o.c.rule == fmx._lib.RULE_ADAGRAD and abs(o.c.eps - 1e-10) < 1e-16 and o.m.numel() == o.v.numel() == 8
    o.step = 5
    o.ref()
    assert o.c.step == 5 and set(o.state_dict()) == {"m", "v", "step"}
