"""fmx_mlp_fit_opt / fmx_online_run_mlp_opt (the online predict-then-fit loop of DeepFM / NFM with the network under a persistent
rule of its own and the tables under any rule) without a GPU: the symbols and their argument counts, every refusal that is
decided on the host -- each with pointers that are never dereferenced, each naming its entry point in
fmx_last_error_string() --, the old entry points' unchanged answers, and the Python surface.  No device is touched: every call
below returns from its host-side checks (the ones that pass them all are stopped by N = 0 or by the workspace's size)."""
import ctypes as C
import inspect
import os
import re

import pytest

from test_adaptive_rules_cpu import _fake_table
from test_deep_adaptive_cpu import _mlp, _opt, _refusals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIT, RUN = "fmx_mlp_fit_opt", "fmx_online_run_mlp_opt"


def _lib():
    import fmx
    L = fmx._lib
    return fmx, L, L.load()


def _fwd(L, sfirst=True):
    out = L.FwdOut()
    out.S = out.bi = out.logit = out.dz = out.loss = 0x40000
    out.sfirst = 0x40000 if sfirst else None
    return out


def _fit(lib, L, m, o, h=None, B=1, loss=None):
    return lib.fmx_mlp_fit_opt(C.byref(m), None if h is None else h.ref(), L.LOSS_BCE_SIGMOID if loss is None else loss, 0x40000, 16,
                               0x41000, 0x70000, B, 1.0 / B, 0xA0000, 0xB0000, None, None if o is None else C.byref(o), None)


def _run(lib, L, t, h, rule, m, o, fm_term=1, N=0, ws_bytes=1 << 40, loss=None, ws=0x50000, scratch=0xD0000):
    out = _fwd(L)
    return lib.fmx_online_run_mlp_opt(C.byref(t), h.ref(), rule, L.LOSS_BCE_SIGMOID if loss is None else loss, C.byref(m), fm_term,
                                      0x60000, None, 0x70000, N, ws, ws_bytes, C.byref(out), scratch, 0xE0000,
                                      None if o is None else C.byref(o), None)


def test_symbols_and_argument_counts():
    fmx, L, lib = _lib()
    assert FIT in L.EXPORTS and RUN in L.EXPORTS
    # fmx_mlp_fit's 14 arguments with `rule` replaced by opt
    assert len(lib.fmx_mlp_fit_opt.argtypes) == len(lib.fmx_mlp_fit.argtypes) == 14
    # fmx_online_run_mlp's 20 without hedge, hedge_b, hedge_s, alpha, plus opt
    assert len(lib.fmx_online_run_mlp_opt.argtypes) == len(lib.fmx_online_run_mlp.argtypes) - 4 + 1 == 17
    assert lib.fmx_version() == 104          # the new symbols are what a caller probes for


def test_header_declares_the_calls_with_those_counts():
    text = open(os.path.join(ROOT, "include", "fmx.h")).read()
    for name, n in ((FIT, 14), (RUN, 17)):
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", text)
        assert decl, name
        assert len(decl.group(1).split(",")) == n, name
    assert "#define FMX_VERSION 104" in text


@pytest.mark.parametrize("who", [FIT, RUN])
def test_optimizer_refusals_name_the_entry_point(who):
    """mlp_opt_check's checks of opt, unchanged: the list the mini-batch _opt calls are held to (grads is not an argument here)."""
    fmx, L, lib = _lib()
    t = _fake_table(L.LAYOUT_MOMENTS)
    h = fmx.Hyper(lr=0.01)
    n = 0
    for what, kw, call_kw, want in _refusals(L):
        if call_kw:
            continue
        o = None if kw.get("opt", {}) is None else _opt(L, **kw["opt"])
        m = _mlp(L, params=kw.get("params", 0x80000))
        rc = _fit(lib, L, m, o, h) if who == FIT else _run(lib, L, t, h, L.RULE_ADAM, m, o, N=1)
        msg = lib.fmx_last_error_string().decode()
        assert rc == want, (who, what, rc, msg)
        assert who in msg, (what, msg)
        n += 1
    assert n == 14
    # m may be null under adagrad and sgd: the stream call gets past the optimizer's checks to the workspace's size
    for rule in (L.RULE_ADAGRAD, L.RULE_SGD):
        rc = _run(lib, L, t, h, L.RULE_ADAM, _mlp(L), _opt(L, rule, m=None), ws_bytes=16)
        assert rc == L.ERR_SHAPE and RUN in lib.fmx_last_error_string().decode(), (rule, rc, lib.fmx_last_error_string())


def test_step_counts_of_the_whole_call_stay_in_int32():
    fmx, L, lib = _lib()
    t = _fake_table(L.LAYOUT_MOMENTS)
    m = _mlp(L)
    top = 2 ** 31 - 1
    # the network's count, under every rule of the network
    for rule in (L.RULE_ADAM, L.RULE_ADAGRAD, L.RULE_SGD):
        assert _run(lib, L, t, fmx.Hyper(), L.RULE_ADAGRAD, m, _opt(L, rule, step=top - 7), N=8) == L.ERR_ARG
        assert RUN in lib.fmx_last_error_string().decode()
        assert _run(lib, L, t, fmx.Hyper(), L.RULE_ADAGRAD, m, _opt(L, rule, step=top - 7), N=0, ws_bytes=16) == L.ERR_SHAPE
    assert _fit(lib, L, m, _opt(L, L.RULE_ADAM, step=top)) == L.ERR_ARG
    # the tables' count under FMX_RULE_ADAM (and its betas), as fmx_fm_online_run checks them
    o = _opt(L, L.RULE_ADAM)
    for bad in (fmx.Hyper(step=top - 7), fmx.Hyper(step=-1), fmx.Hyper(beta1=1.0), fmx.Hyper(beta2=-0.5)):
        assert _run(lib, L, t, bad, L.RULE_ADAM, m, o, N=8) == L.ERR_ARG
        assert RUN in lib.fmx_last_error_string().decode()
    assert _run(lib, L, t, fmx.Hyper(step=top - 7), L.RULE_ADAGRAD, m, o, N=0, ws_bytes=16) == L.ERR_SHAPE     # adagrad does not count


def test_table_rules_and_layouts_are_paired_as_in_fm_online_run():
    fmx, L, lib = _lib()
    h = fmx.Hyper(lr=0.01)
    m, o = _mlp(L), _opt(L, L.RULE_ADAM)
    for layout, rule, want in [(L.LAYOUT_MOMENTS, L.RULE_ADAM, L.ERR_SHAPE), (L.LAYOUT_MOMENTS, L.RULE_ADAGRAD, L.ERR_SHAPE),
                               (L.LAYOUT_WEIGHTS, L.RULE_SIGNADAM, L.ERR_SHAPE), (L.LAYOUT_WEIGHTS, L.RULE_SGD, L.ERR_SHAPE),
                               (L.LAYOUT_FTRL, L.RULE_FTRL, L.ERR_SHAPE),
                               (L.LAYOUT_WEIGHTS, L.RULE_ADAM, L.ERR_ARG), (L.LAYOUT_WEIGHTS, L.RULE_ADAGRAD, L.ERR_ARG),
                               (L.LAYOUT_MOMENTS, L.RULE_SIGNADAM, L.ERR_ARG), (L.LAYOUT_FTRL, L.RULE_ADAM, L.ERR_ARG),
                               (L.LAYOUT_MOMENTS, L.RULE_FTRL, L.ERR_ARG), (L.LAYOUT_MOMENTS, 9, L.ERR_ARG)]:
        rc = _run(lib, L, _fake_table(layout), h, rule, m, o, ws_bytes=16)      # ERR_SHAPE: past every check, at the workspace's size
        msg = lib.fmx_last_error_string().decode()
        assert rc == want and RUN in msg, (layout, rule, rc, msg)
    # NFM reads bias[0] as the bias weight: weights and moments tables, not FTRL ones (as in fmx_deepfm_stream_opt)
    rc = _run(lib, L, _fake_table(L.LAYOUT_FTRL), h, L.RULE_FTRL, m, o, fm_term=0)
    assert rc == L.ERR_UNSUPPORTED and RUN in lib.fmx_last_error_string().decode()
    for layout, rule in ((L.LAYOUT_MOMENTS, L.RULE_ADAM), (L.LAYOUT_WEIGHTS, L.RULE_SIGNADAM)):
        assert _run(lib, L, _fake_table(layout), h, rule, m, o, fm_term=0, ws_bytes=16) == L.ERR_SHAPE


def test_the_old_calls_checks_are_run_first_and_n_zero_is_a_checked_no_op():
    fmx, L, lib = _lib()
    t, h = _fake_table(L.LAYOUT_MOMENTS), fmx.Hyper(lr=0.01)
    m, o = _mlp(L), _opt(L, L.RULE_ADAM)
    assert _run(lib, L, t, h, L.RULE_ADAM, m, o, N=0) == L.OK                     # nothing to launch
    assert _run(lib, L, t, h, L.RULE_ADAM, m, o, N=-1) == L.ERR_ARG
    assert _run(lib, L, t, h, L.RULE_ADAM, m, None, N=0) == L.ERR_ARG            # ... but every argument is still checked
    assert _run(lib, L, t, h, L.RULE_ADAM, m, o, N=0, loss=L.LOSS_NONE) == L.ERR_ARG
    assert _run(lib, L, t, h, L.RULE_ADAM, m, o, N=0, ws=0x50004) == L.ERR_ALIGN
    assert _run(lib, L, t, h, L.RULE_ADAM, m, o, N=0, scratch=0xD0008) == L.ERR_ALIGN
    assert _run(lib, L, t, h, L.RULE_ADAM, _mlp(L, k=64, hidden=64), o, N=0) == L.ERR_UNSUPPORTED     # fit: k <= 63
    for rc in (lib.fmx_online_run_mlp_opt(None, h.ref(), L.RULE_ADAM, L.LOSS_BCE_LOGITS, C.byref(m), 1, 0x60000, None, 0x70000, 0,
                                          0x50000, 1 << 40, C.byref(_fwd(L)), 0xD0000, 0xE0000, C.byref(o), None),
               lib.fmx_online_run_mlp_opt(C.byref(t), h.ref(), L.RULE_ADAM, L.LOSS_BCE_LOGITS, C.byref(m), 1, None, None, 0x70000, 0,
                                          0x50000, 1 << 40, C.byref(_fwd(L)), 0xD0000, 0xE0000, C.byref(o), None),
               lib.fmx_online_run_mlp_opt(C.byref(t), h.ref(), L.RULE_ADAM, L.LOSS_BCE_LOGITS, C.byref(m), 1, 0x60000, None, 0x70000, 0,
                                          0x50000, 1 << 40, C.byref(_fwd(L, sfirst=False)), 0xD0000, 0xE0000, C.byref(o), None)):
        assert rc == L.ERR_ARG and RUN in lib.fmx_last_error_string().decode(), lib.fmx_last_error_string()
    bad = _fake_table(L.LAYOUT_MOMENTS)
    bad.kp = 12
    assert _run(lib, L, bad, h, L.RULE_ADAM, m, o) == L.ERR_SHAPE and RUN in lib.fmx_last_error_string().decode()
    # fmx_mlp_fit_opt: fmx_mlp_fit's own checks (hyper may be null: the learning rate is opt's)
    assert _fit(lib, L, m, o, loss=L.LOSS_NONE) == L.ERR_ARG and FIT in lib.fmx_last_error_string().decode()
    assert _fit(lib, L, _mlp(L, k=64, hidden=64), o) == L.ERR_UNSUPPORTED and FIT in lib.fmx_last_error_string().decode()
    assert _fit(lib, L, m, o, B=17) == L.ERR_UNSUPPORTED and FIT in lib.fmx_last_error_string().decode()       # one workgroup: B <= 16


def test_the_old_entry_points_still_refuse_the_adaptive_rules():
    fmx, L, lib = _lib()
    h, m = fmx.Hyper(lr=0.01), _mlp(L)
    for rule, name in ((L.RULE_ADAGRAD, "FMX_RULE_ADAGRAD"), (L.RULE_ADAM, "FMX_RULE_ADAM")):
        t = _fake_table(L.LAYOUT_MOMENTS)
        rc = lib.fmx_online_run_mlp(C.byref(t), h.ref(), rule, L.LOSS_BCE_SIGMOID, C.byref(m), 0, 1, 0.0, 0.0, None, 0x60000, None,
                                    0x70000, 4, 0x50000, 1 << 40, C.byref(_fwd(L)), 0xD0000, 0xE0000, None)
        msg = lib.fmx_last_error_string().decode()
        assert rc == L.ERR_UNSUPPORTED and name in msg and "fmx_online_run_mlp" in msg and RUN not in msg, (rc, msg)
        rc = lib.fmx_mlp_fit(C.byref(m), h.ref(), rule, L.LOSS_BCE_SIGMOID, 0x40000, 16, 0x40000, 0x70000, 1, 1.0, 0xA0000, 0xB0000,
                             None, None)
        msg = lib.fmx_last_error_string().decode()
        assert rc == L.ERR_UNSUPPORTED and name in msg and "fmx_mlp_fit" in msg and FIT not in msg, (rc, msg)
    # ... and their other answers: FTRL in fit mode, a layout / rule mismatch
    rc = lib.fmx_online_run_mlp(C.byref(_fake_table(L.LAYOUT_FTRL)), h.ref(), L.RULE_FTRL, L.LOSS_BCE_SIGMOID, C.byref(m), 0, 1, 0.0,
                                0.0, None, 0x60000, None, 0x70000, 4, 0x50000, 1 << 40, C.byref(_fwd(L)), 0xD0000, 0xE0000, None)
    assert rc == L.ERR_ARG
    rc = lib.fmx_online_run_mlp(C.byref(_fake_table(L.LAYOUT_MOMENTS)), h.ref(), L.RULE_SIGNADAM, L.LOSS_BCE_SIGMOID, C.byref(m), 0, 1,
                                0.0, 0.0, None, 0x60000, None, 0x70000, 4, 0x50000, 1 << 40, C.byref(_fwd(L)), 0xD0000, 0xE0000, None)
    assert rc == L.ERR_ARG
    assert lib.fmx_mlp_fit(C.byref(m), h.ref(), L.RULE_FTRL, L.LOSS_BCE_SIGMOID, 0x40000, 16, 0x40000, 0x70000, 1, 1.0, 0xA0000,
                           0xB0000, None, None) == L.ERR_ARG


def test_python_surface():
    import fmx
    assert "mlp_opt" in inspect.signature(fmx.FMEngine.mlp_fit).parameters
    assert "mlp_opt" in inspect.signature(fmx.FMEngine.online_run_mlp).parameters
    assert inspect.signature(fmx.FMEngine.mlp_fit).parameters["mlp_opt"].default is None
    assert inspect.signature(fmx.FMEngine.online_run_mlp).parameters["mlp_opt"].default is None
    from models.models_online_deep.deepfm_adam import DeepFMAdam
    from models.models_online_deep.nfm_adam import NFMAdam
    import torch
    if not torch.cuda.is_available():       # there is no CPU path: construction says so
        for M in (DeepFMAdam, NFMAdam):
            with pytest.raises(RuntimeError):
                M([3, 4], embedding_size=4, num_hidden_layers=2, neuron_per_hidden_layer=8, update_rule="adam", fused_optimizer=True)
    for M in (DeepFMAdam, NFMAdam):
        assert "fused_optimizer" in (M._device_loop_ok.__doc__ or "") and "fmx_mlp_fit_opt" in M._device_loop_ok.__doc__
