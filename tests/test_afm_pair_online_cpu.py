"""The one-workgroup form of fmx_afm_pair_online_run without a GPU: fmx_afm_pair_online_form (which form a shape takes: the tile
buffers of k_afm_pair_online, or 0 for the queued pair steps) on hand-built structs whose pointers are never dereferenced, the
option "afm_pair_online_persistent" that switches the form off, and the query's own refusals.  No device is touched."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHO = "fmx_afm_pair_online_form"
OPTION = b"afm_pair_online_persistent"
N_ARGS = 4

# (F, k, t) whose attention moments (2 r4(G) floats) would cost the one-workgroup form a tile buffer: 8 buffers fit without them,
# so they stay in global memory (afm_online_buffers).  tests/test_afm_pair_online_gpu.py runs this shape under adam / adam.
MOMENTS_IN_GLOBAL = (56, 16, 16)


def _lib():
    import fmx
    L = fmx._lib
    return fmx, L, L.load()


def fake_table(L, F, k, layout=None):
    """A table struct of F fields and width k whose pointers are never dereferenced."""
    kp = next(p for p in (4, 8, 16, 32, 64) if p >= k)
    t = L.Table()
    t.rows, t.field_offsets, t.bias = 0x10000, 0x20000, 0x30000
    t.n_rows, t.n_fields, t.k, t.kp = 100 * F, F, k, kp
    t.layout = L.LAYOUT_MOMENTS if layout is None else layout
    t.z_offset, t.row_stride = 2 * kp, 5 * kp + 4
    t.max_field_rows = 100
    return t


def form(lib, L, F, k, t, rule=None, want_mom=True):
    tb, afm, mom = fake_table(L, F, k), L.Afm(0x80000, k, t), C.c_int32(-1)
    rc = lib.fmx_afm_pair_online_form(C.byref(tb), C.byref(afm), L.RULE_ADAM if rule is None else rule, C.byref(mom) if want_mom else None)
    return rc, mom.value


def test_symbol_is_declared_listed_and_exported():
    fmx, L, lib = _lib()
    assert WHO in L.EXPORTS
    assert len(lib.fmx_afm_pair_online_form.argtypes) == N_ARGS
    text = open(os.path.join(ROOT, "include", "fmx.h")).read()
    decl = re.search(r"\bint " + WHO + r"\(([^;]*)\);", text)
    assert decl
    args = [a.strip() for a in decl.group(1).split(",")]
    assert args == ["const fmx_table_t *table", "const fmx_afm_t *afm", "int32_t attn_rule", "int32_t *moments_in_lds"]
    comment = text[:decl.start()].rsplit("/*", 1)[1]
    assert "Replaces:" in comment and "Restates:" in comment
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT " + WHO + r"$", out, re.M)


def test_option_returns_the_previous_value():
    fmx, L, lib = _lib()
    try:
        assert lib.fmx_set_option(OPTION, 0) == 1          # the default
        assert lib.fmx_set_option(OPTION, 1) == 0
    finally:
        lib.fmx_set_option(OPTION, 1)
    assert lib.fmx_set_option(OPTION, 1) == 1


ONE_WORKGROUP = [(3, 4, 4), (12, 10, 4), (39, 16, 16), (64, 33, 7), (40, 20, 64)]


@pytest.mark.parametrize("F,k,t", ONE_WORKGROUP)
def test_shapes_that_take_the_one_workgroup_form(F, k, t):
    fmx, L, lib = _lib()
    for rule in (L.RULE_SIGNADAM, L.RULE_SGD, L.RULE_ADAGRAD, L.RULE_ADAM):
        nb, mom = form(lib, L, F, k, t, rule)
        assert 0 < nb <= 8, (rule, nb, lib.fmx_last_error_string())
        assert mom in (0, 1) and (mom == 0 or rule in (L.RULE_ADAGRAD, L.RULE_ADAM))     # a rule without moments keeps none in LDS
    assert form(lib, L, F, k, t, want_mom=False)[0] == form(lib, L, F, k, t)[0]          # moments_in_lds may be null


def test_tile_buffers_and_moments():
    fmx, L, lib = _lib()
    assert form(lib, L, 39, 16, 16) == (8, 1)              # 16 tiles: 8 buffers, two rounds; the moments beside them
    assert form(lib, L, 3, 4, 4) == (1, 1)                 # one tile
    assert form(lib, L, 12, 10, 4) == (2, 1)               # two tiles
    assert form(lib, L, 2, 1, 1) == (1, 1)                 # one field pair
    assert form(lib, L, 64, 64, 64) == (0, 0)              # not even two tile buffers beside the sample: the queued form
    nb, mom = form(lib, L, *MOMENTS_IN_GLOBAL)
    assert nb == 8 and mom == 0                            # the moments would cost a buffer: they stay in global memory
    assert form(lib, L, *MOMENTS_IN_GLOBAL, rule=L.RULE_SGD) == (8, 0)


def test_the_option_switches_the_form_off_everywhere():
    fmx, L, lib = _lib()
    try:
        assert lib.fmx_set_option(OPTION, 0) == 1
        for F, k, t in ONE_WORKGROUP + [(64, 64, 64), MOMENTS_IN_GLOBAL, (2, 1, 1)]:
            assert form(lib, L, F, k, t) == (0, 0), (F, k, t)
    finally:
        lib.fmx_set_option(OPTION, 1)
    assert form(lib, L, 39, 16, 16) == (8, 1)


def test_null_and_refused_arguments():
    fmx, L, lib = _lib()
    tb, afm = fake_table(L, 12, 10), L.Afm(0x80000, 10, 4)

    def refused(rc, want, what):
        msg = lib.fmx_last_error_string().decode()
        assert rc == want and WHO in msg, (what, rc, msg)

    refused(lib.fmx_afm_pair_online_form(None, C.byref(afm), L.RULE_ADAM, None), L.ERR_ARG, "null table")
    refused(lib.fmx_afm_pair_online_form(C.byref(tb), None, L.RULE_ADAM, None), L.ERR_ARG, "null afm")
    refused(lib.fmx_afm_pair_online_form(C.byref(tb), C.byref(L.Afm(None, 10, 4)), L.RULE_ADAM, None), L.ERR_ARG, "null params")
    for rule in (L.RULE_FTRL, 7, -1):
        refused(lib.fmx_afm_pair_online_form(C.byref(tb), C.byref(afm), rule, None), L.ERR_ARG, f"attention rule {rule}")
    refused(lib.fmx_afm_pair_online_form(C.byref(tb), C.byref(L.Afm(0x80000, 8, 4)), L.RULE_ADAM, None), L.ERR_SHAPE, "afm->k")
    refused(lib.fmx_afm_pair_online_form(C.byref(tb), C.byref(L.Afm(0x80000, 10, 65)), L.RULE_ADAM, None), L.ERR_UNSUPPORTED, "t = 65")
    refused(lib.fmx_afm_pair_online_form(C.byref(tb), C.byref(L.Afm(0x80000, 10, 0)), L.RULE_ADAM, None), L.ERR_UNSUPPORTED, "t = 0")
    one = fake_table(L, 1, 10)
    refused(lib.fmx_afm_pair_online_form(C.byref(one), C.byref(afm), L.RULE_ADAM, None), L.ERR_UNSUPPORTED, "one field")
    mapped = fake_table(L, 12, 10)
    mapped.field_cols, mapped.n_cols = 0x40000, 2
    refused(lib.fmx_afm_pair_online_form(C.byref(mapped), C.byref(afm), L.RULE_ADAM, None), L.ERR_UNSUPPORTED, "mapped table")
    mom = C.c_int32(-1)                                    # a refusal leaves the caller's word alone
    assert lib.fmx_afm_pair_online_form(None, C.byref(afm), L.RULE_ADAM, C.byref(mom)) == L.ERR_ARG and mom.value == -1


def test_python_surface():
    import fmx
    assert list(inspect.signature(fmx.AFMEngine.pair_online_form).parameters) == ["self", "attn_rule"]
    from models.models_online_deep.afm_adam import AFMAdam
    assert "attention" in inspect.signature(AFMAdam.run_pair_experiment).parameters
