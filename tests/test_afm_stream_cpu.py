"""fmx_afm_step_opt / fmx_afm_stream (the attentional FM with its attention parameters under a rule of their own, and many steps
in one call) without a GPU: the symbols and their argument counts, and every refusal that is decided on the host -- each with
pointers that are never dereferenced, each naming its entry point in fmx_last_error_string().  No device is touched."""
import ctypes as C
import os
import re

import pytest

from test_adaptive_rules_cpu import _fake_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHO = ["fmx_afm_step_opt", "fmx_afm_stream"]


def _lib():
    import fmx
    L = fmx._lib
    return fmx, L, L.load()


def _opt(L, rule, m=0xD0000, v=0xE0000, lr=0.01, eps=1e-8, beta1=0.9, beta2=0.999, step=0):
    return L.MlpOpt(m, v, lr, eps, beta1, beta2, rule, step)


def _afm(L, params=0x80000, k=16, t=4):
    return L.Afm(params, k, t)


def _call(who, lib, L, t, h, rule, afm, o, B=64, idx=0x60000, y=0x70000, ws=0x50000, ws_bytes=1 << 40, grad=0xC0000, n_pool=1,
          n_steps=0):
    """The call with fake pointers.  The step is only ever sent where a host check refuses it; the stream defaults to n_steps = 0,
    which checks everything and launches nothing."""
    op = None if o is None else C.byref(o)
    ap = None if afm is None else C.byref(afm)
    hp = None if h is None else h.ref()
    inv_b = 1.0 / max(B, 1)
    if who == "fmx_afm_step_opt":
        return lib.fmx_afm_step_opt(C.byref(t), hp, rule, ap, idx, None, y, B, inv_b, ws, ws_bytes, grad, op, None, None, None)
    return lib.fmx_afm_stream(C.byref(t), hp, rule, ap, idx, None, y, n_pool, B, inv_b, n_steps, ws, ws_bytes, grad, op, None,
                              None, None)


def test_symbols_and_argument_counts():
    fmx, L, lib = _lib()
    assert "fmx_afm_step_opt" in L.EXPORTS and "fmx_afm_stream" in L.EXPORTS
    assert len(lib.fmx_afm_step_opt.argtypes) == len(lib.fmx_afm_step.argtypes) + 1 == 16      # fmx_afm_step's, plus opt
    assert len(lib.fmx_afm_stream.argtypes) == 18
    assert lib.fmx_version() == 104          # the new symbols are what a caller probes for
    assert issubclass(fmx.AfmOpt, fmx.MlpOpt) and "signadam" in fmx.AfmOpt.RULES and "signadam" not in fmx.MlpOpt.RULES


def test_header_declares_the_calls_with_those_counts():
    text = open(os.path.join(ROOT, "include", "fmx.h")).read()
    for name, n in (("fmx_afm_step", 15), ("fmx_afm_step_opt", 16), ("fmx_afm_stream", 18)):
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", text)
        assert decl, name
        assert len(decl.group(1).split(",")) == n, name
    # opt stands right after attn_grad_out
    args = [a.strip() for a in re.search(r"\bint fmx_afm_step_opt\(([^;]*)\);", text).group(1).split(",")]
    i = [j for j, a in enumerate(args) if a.endswith("attn_grad_out")][0]
    assert args[i + 1] == "const fmx_mlp_opt_t *opt"


def _opt_refusals(L):
    """(what, keyword arguments of _opt or None, keyword arguments of the attention struct, expected status)"""
    A, AL = L.ERR_ARG, L.ERR_ALIGN
    return [
        ("opt null", None, {}, A),
        ("ftrl is not an attention rule", dict(rule=L.RULE_FTRL), {}, A),
        ("rule 7", dict(rule=7), {}, A),
        ("rule -1", dict(rule=-1), {}, A),
        ("v null under adagrad", dict(rule=L.RULE_ADAGRAD, v=None), {}, A),
        ("v null under adam", dict(rule=L.RULE_ADAM, v=None), {}, A),
        ("m null under adam", dict(rule=L.RULE_ADAM, m=None), {}, A),
        ("beta1 = 1", dict(rule=L.RULE_ADAM, beta1=1.0), {}, A),
        ("beta1 < 0", dict(rule=L.RULE_ADAM, beta1=-0.5), {}, A),
        ("beta2 = 1", dict(rule=L.RULE_ADAM, beta2=1.0), {}, A),
        ("beta2 < 0", dict(rule=L.RULE_ADAM, beta2=-0.1), {}, A),
        ("step < 0", dict(rule=L.RULE_ADAM, step=-1), {}, A),
        ("step < 0 under sgd", dict(rule=L.RULE_SGD, step=-1), {}, A),
        ("m misaligned", dict(rule=L.RULE_ADAM, m=0xD0004), {}, AL),
        ("v misaligned", dict(rule=L.RULE_ADAGRAD, v=0xE0008), {}, AL),
        ("params misaligned", dict(rule=L.RULE_ADAM), dict(params=0x80004), AL),
    ]


@pytest.mark.parametrize("who", WHO)
def test_host_decided_refusals_of_the_optimizer_state(who):
    fmx, L, lib = _lib()
    t = _fake_table(L.LAYOUT_MOMENTS)
    h = fmx.Hyper(lr=0.01)
    for what, okw, akw, want in _opt_refusals(L):
        o = None if okw is None else _opt(L, **okw)
        rc = _call(who, lib, L, t, h, L.RULE_ADAM, _afm(L, **akw), o)
        msg = lib.fmx_last_error_string().decode()
        assert rc == want, (who, what, rc, msg)
        assert who in msg, (what, msg)
    # step + the call's steps beyond int32
    if who == "fmx_afm_step_opt":
        rc = _call(who, lib, L, t, h, L.RULE_ADAM, _afm(L), _opt(L, L.RULE_ADAM, step=2 ** 31 - 1))
    else:
        assert _call(who, lib, L, t, h, L.RULE_ADAM, _afm(L), _opt(L, L.RULE_ADAM, step=2 ** 31 - 1), n_steps=0) == L.OK
        rc = _call(who, lib, L, t, h, L.RULE_ADAM, _afm(L), _opt(L, L.RULE_ADAM, step=2 ** 31 - 8), n_steps=8)
    msg = lib.fmx_last_error_string().decode()
    assert rc == L.ERR_ARG and who in msg, (rc, msg)


def test_moments_may_be_null_where_the_rule_keeps_none():
    """signadam and sgd take m = v = null, adagrad m = null, whatever the tables' rule: the stream gets through every check
    (n_steps = 0: OK, nothing launched)."""
    fmx, L, lib = _lib()
    h = fmx.Hyper(lr=0.01)
    for rule, kw in ((L.RULE_SIGNADAM, dict(m=None, v=None)), (L.RULE_SGD, dict(m=None, v=None)), (L.RULE_ADAGRAD, dict(m=None)),
                     (L.RULE_ADAM, {})):
        o = _opt(L, rule, **kw)
        for layout, trule in ((L.LAYOUT_WEIGHTS, L.RULE_SIGNADAM), (L.LAYOUT_FTRL, L.RULE_FTRL), (L.LAYOUT_MOMENTS, L.RULE_ADAGRAD)):
            t = _fake_table(layout)
            rc = _call("fmx_afm_stream", lib, L, t, h, trule, _afm(L), o)
            assert rc == L.OK, (rule, layout, lib.fmx_last_error_string())


@pytest.mark.parametrize("who", WHO)
def test_the_steps_own_checks_come_first_and_name_the_entry_point(who):
    fmx, L, lib = _lib()
    h = fmx.Hyper(lr=0.01)
    t = _fake_table(L.LAYOUT_MOMENTS)
    o = _opt(L, L.RULE_ADAM)
    A, SH, AL, UN = L.ERR_ARG, L.ERR_SHAPE, L.ERR_ALIGN, L.ERR_UNSUPPORTED
    need = lib.fmx_afm_workspace_bytes(C.byref(t), C.byref(_afm(L)), 64)
    assert need > 0
    cases = [
        ("null attention struct", dict(afm=None), A),
        ("null attention parameters", dict(afm=_afm(L, params=None)), A),
        ("afm->k differs from the table's", dict(afm=_afm(L, k=8)), SH),
        ("t = 65", dict(afm=_afm(L, t=65)), UN),
        ("null hyper", dict(h=None), A),
        ("null idx", dict(idx=None), A),
        ("null y", dict(y=None), A),
        ("null workspace", dict(ws=None), A),
        ("null attn_grad_out", dict(grad=None), A),
        ("B = 0", dict(B=0), A),
        ("rule / layout", dict(rule=L.RULE_SGD), A),
        ("workspace misaligned", dict(ws=0x50004), AL),
        ("workspace short", dict(ws_bytes=need - 1), SH),
    ]
    for what, kw, want in cases:
        kw = dict(dict(h=h, rule=L.RULE_ADAM, afm=_afm(L)), **kw)
        rc = _call(who, lib, L, t, kw.pop("h"), kw.pop("rule"), kw.pop("afm"), o, **kw)
        msg = lib.fmx_last_error_string().decode()
        assert rc == want, (who, what, rc, msg)
        assert who in msg, (what, msg)
    # the tables' own adam hyper-parameters, before anything is launched
    for bad in (fmx.Hyper(beta1=1.0), fmx.Hyper(beta2=-0.1), fmx.Hyper(step=-1), fmx.Hyper(step=2 ** 31 - 1)):
        rc = _call(who, lib, L, t, bad, L.RULE_ADAM, _afm(L), o, n_steps=1 if who == "fmx_afm_stream" else 0)
        msg = lib.fmx_last_error_string().decode()
        assert rc == A and who in msg, (rc, msg)
    # the sort's geometry: a field too large for a 32-bit (index, sample) composite at this batch size
    big = _fake_table(L.LAYOUT_MOMENTS)
    big.n_rows, big.max_field_rows = 1 << 40, 1 << 31
    rc = _call(who, lib, L, big, h, L.RULE_ADAM, _afm(L), o, B=4096)
    msg = lib.fmx_last_error_string().decode()
    assert rc == UN and who in msg, (rc, msg)


def test_stream_pool_and_step_counts():
    fmx, L, lib = _lib()
    h = fmx.Hyper(lr=0.01)
    t = _fake_table(L.LAYOUT_MOMENTS)
    o = _opt(L, L.RULE_ADAM)
    for kw in (dict(n_pool=0), dict(n_pool=-1), dict(n_steps=-1)):
        rc = _call("fmx_afm_stream", lib, L, t, h, L.RULE_ADAM, _afm(L), o, **kw)
        msg = lib.fmx_last_error_string().decode()
        assert rc == L.ERR_ARG and "fmx_afm_stream" in msg, (kw, rc, msg)
    # the table's count too: step + n_steps within int32
    assert _call("fmx_afm_stream", lib, L, t, fmx.Hyper(step=2 ** 31 - 9), L.RULE_ADAM, _afm(L), o) == L.OK
    rc = _call("fmx_afm_stream", lib, L, t, fmx.Hyper(step=2 ** 31 - 5), L.RULE_ADAM, _afm(L), o, n_steps=8)
    assert rc == L.ERR_ARG and b"fmx_afm_stream" in lib.fmx_last_error_string()
    # n_steps = 0 with every argument in order: nothing to launch
    assert _call("fmx_afm_stream", lib, L, t, h, L.RULE_ADAM, _afm(L), o, n_steps=0, n_pool=3) == L.OK


def test_signadam_is_still_refused_by_the_mlp_calls():
    from test_deep_adaptive_cpu import _mlp, _section
    fmx, L, lib = _lib()
    rc = _section(lib, L, _mlp(L), _opt(L, L.RULE_SIGNADAM))
    assert rc == L.ERR_ARG and b"fmx_mlp_section_opt" in lib.fmx_last_error_string()
    with pytest.raises(ValueError):
        fmx.MlpOpt(8, "signadam", device="cpu")
    o = fmx.AfmOpt(8, "signadam", device="cpu")
    assert o.c.rule == L.RULE_SIGNADAM and abs(o.c.eps - 1e-8) < 1e-14


def test_python_surface():
    import inspect
    import fmx
    assert "opt" in inspect.signature(fmx.AFMEngine.step).parameters
    assert list(inspect.signature(fmx.AFMEngine.stream).parameters)[1:9] == ["hyper", "rule", "idx_pool", "xv_pool", "y_pool", "B",
                                                                             "n_steps", "opt"]
    from models.models_online_deep.afm_adam import AFMAdam
    assert inspect.signature(AFMAdam.__init__).parameters["fused_optimizer"].default is False


# ---- the float64 reference of the attention parameters' persistent rules: torch's own optimizers, one step from a given state ----
def torch_dense_step(rule, h, s, p, m, v, g):
    """Step s (1-based) of torch.optim.Adam / torch.optim.Adagrad in float64 on the flat parameters p with gradient g, from the
    state (m, v) left by s - 1 steps (adagrad: the sum of squares in v).  -> (p, m, v) after it.  h: lr, eps (, beta1, beta2)."""
    import numpy as np
    import torch
    prm = torch.nn.Parameter(torch.tensor(np.asarray(p, dtype=np.float64)))
    if rule == "adam":
        opt = torch.optim.Adam([prm], lr=float(h["lr"]), betas=(float(h["beta1"]), float(h["beta2"])), eps=float(h["eps"]))
        state = {"step": torch.tensor(float(s - 1)), "exp_avg": torch.tensor(np.asarray(m, dtype=np.float64)),
                 "exp_avg_sq": torch.tensor(np.asarray(v, dtype=np.float64))}
    else:
        opt = torch.optim.Adagrad([prm], lr=float(h["lr"]), eps=float(h["eps"]))
        state = {"step": torch.tensor(float(s - 1)), "sum": torch.tensor(np.asarray(v, dtype=np.float64))}
    opt.load_state_dict({"state": {0: state}, "param_groups": opt.state_dict()["param_groups"]})
    prm.grad = torch.tensor(np.asarray(g, dtype=np.float64))
    opt.step()
    st = opt.state[prm]
    if rule == "adam":
        return prm.detach().numpy().copy(), st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy()
    return prm.detach().numpy().copy(), np.zeros_like(np.asarray(p, dtype=np.float64)), st["sum"].numpy().copy()


@pytest.mark.parametrize("rule", ["adam", "adagrad"])
def test_the_dense_rule_as_the_header_states_it_is_torchs(rule):
    """fmx_mlp_opt_t's rearranged ADAM -- step_size = lr sqrt(1 - beta2^t) / (1 - beta1^t) over sqrt(v) + eps sqrt(1 - beta2^t) -- is
    torch.optim.Adam, a zero gradient included (the moments decay and the parameter still moves); ADAGRAD is torch.optim.Adagrad."""
    import numpy as np
    from test_adaptive_rules_cpu import rule_apply
    rng = np.random.default_rng(3)
    h = dict(lr=0.01, eps=1e-8 if rule == "adam" else 1e-10, beta1=float(np.float32(0.9)), beta2=float(np.float32(0.999)))
    n = 40
    p, m, v = rng.normal(size=n), np.zeros(n), np.zeros(n)
    for s in range(1, 6):
        g = rng.normal(size=n) * 1e-3
        g[:5] = 0.0 if s > 1 else g[:5]             # coordinates whose gradient vanishes after the first step
        p2, m2, v2 = torch_dense_step(rule, h, s, p, m, v, g)
        ha = dict(h, eps=h["eps"] * (np.sqrt(1 - h["beta2"] ** s) if rule == "adam" else 1.0))
        p3, m3, v3 = rule_apply(p, m, v, g, rule, ha, s)
        np.testing.assert_allclose(p2, p3, rtol=1e-12, atol=0)
        np.testing.assert_allclose(v2, v3, rtol=1e-12, atol=0)
        if rule == "adam":
            np.testing.assert_allclose(m2, m3, rtol=1e-12, atol=1e-300)
            if s > 1:
                assert (p2[:5] != p[:5]).all() and (np.abs(m2[:5]) < np.abs(m[:5])).all()
        p, m, v = p2, m2, v2
