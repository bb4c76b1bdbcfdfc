"""The FM's online list loop without a GPU: the symbol fmx_fm_list_online_run and its argument count, what its header comment
promises, every refusal that is decided on the host (pointers that are never dereferenced), the empty stream, the classes that
refuse run_list_experiment, and FMAdam.run_list_experiment's signature and limit of negatives.  No device is touched."""
import ctypes as C
import importlib
import inspect
import os
import re
import subprocess

import pytest

from test_adaptive_rules_cpu import _fake_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHO = "fmx_fm_list_online_run"
N_ARGS = 12


def _lib():
    import fmx
    L = fmx._lib
    return fmx, L, L.load()


def _call(lib, L, t, h, rule=None, idx=0x60000, N=4, G=4, rank=0x70000, logit=None, loss=None):
    """The call with fake pointers: only ever sent where a host check answers it."""
    tp = None if t is None else C.byref(t)
    hp = None if h is None else h.ref()
    rule = L.RULE_SIGNADAM if rule is None else rule
    return lib.fmx_fm_list_online_run(tp, hp, rule, idx, None, N, G, rank, logit, loss, None, None)


def test_symbol_and_argument_count():
    fmx, L, lib = _lib()
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert WHO in set(re.findall(r"\bT\s+(fmx_\w+)", out))
    assert WHO in L.EXPORTS and len(getattr(lib, WHO).argtypes) == N_ARGS
    header = open(os.path.join(ROOT, "include", "fmx.h")).read()
    decl = re.search(r"\bint " + WHO + r"\(([^;]*)\);", header)
    assert decl and len(decl.group(1).split(",")) == N_ARGS
    # declared behind the batched list calls, in front of the MLP section
    assert header.index("int fmx_fm_list_stream(") < decl.start() < header.index("typedef struct fmx_mlp {")
    assert lib.fmx_version() == 104


def test_header_states_the_contract():
    header = open(os.path.join(ROOT, "include", "fmx.h")).read()
    decl = header.index("int " + WHO + "(")
    text = " ".join(header[:decl].rsplit("/*", 1)[1].split())
    for phrase in ("idx [N G, F]", "rank_out[i]", "(required)", "0: the positive is first", "fmx_fm_pair_online_run's pred_out[i]",
                   "logit_out[G i + j] (or null)", "loss_out[i] (or null)", "BEFORE the list's update",
                   "bit-identical to N calls of fmx_fm_list_step with B_lists = 1", "inv_b = 1",
                   "in the order the table update adds them", "hyper->step + i + 1",
                   "The bias is read once and never written", "bit-unchanged",
                   "n_fields > 4 * (64 / (kp / 4))", "sort split", "n_sort_fields > 0", "FMX_ERR_UNSUPPORTED", "rank_out null",
                   "N == 0 is FMX_OK", "sets *error to 1",
                   "Replaces: nothing -- the reference has no listwise loss", "meta_fm.py:145-169", "fm_adam.py:90-119"):
        assert phrase in text, phrase


def test_host_decided_refusals():
    fmx, L, lib = _lib()
    A, UN = L.ERR_ARG, L.ERR_UNSUPPORTED
    h = fmx.Hyper(lr=0.01)
    t = _fake_table(L.LAYOUT_WEIGHTS)
    mapped = _fake_table(L.LAYOUT_WEIGHTS)
    mapped.field_cols, mapped.n_cols = 0x90000, 2
    based = _fake_table(L.LAYOUT_WEIGHTS)
    based.field_base = 0x90000
    split = _fake_table(L.LAYOUT_WEIGHTS)
    split.sort_offsets, split.sort_cols, split.n_sort_fields, split.max_sort_field_rows = 0x90000, 0x91000, 3, 25
    wide = _fake_table(L.LAYOUT_WEIGHTS)                 # kp = 16: 16 lane groups, 4 passes: 64 fields fit, 65 do not
    wide.n_fields, wide.n_rows, wide.max_field_rows = 65, 6500, 100
    fits = _fake_table(L.LAYOUT_WEIGHTS)
    fits.n_fields, fits.n_rows, fits.max_field_rows = 64, 6400, 100
    cases = [
        ("table", dict(t=None), A, "table"),
        ("hyper", dict(h=None), A, "hyper"),
        ("idx", dict(idx=None), A, "idx"),
        ("N -3", dict(N=-3), A, "N = -3"),
        ("G 1", dict(G=1), A, "G = 1"),
        ("G 0", dict(G=0), A, "G = 0"),
        ("G 17", dict(G=17), UN, "G = 17"),
        ("rows beyond int32", dict(N=2 ** 28, G=8), A, "int32"),
        ("rank_out", dict(rank=None), A, "rank_out"),
        ("field_cols", dict(t=mapped), UN, "field_cols"),
        ("field_base", dict(t=based), UN, "field_base"),
        ("sort split", dict(t=split), UN, "sort split"),
        ("too many fields", dict(t=wide), UN, "65 fields"),
        ("ftrl rule on a weights table", dict(rule=L.RULE_FTRL), A, "FMX_RULE_FTRL"),
        ("adam rule on a weights table", dict(rule=L.RULE_ADAM), A, "FMX_RULE_ADAM"),
        ("sgd on a moments table", dict(t=_fake_table(L.LAYOUT_MOMENTS), rule=L.RULE_SGD), A, "rule"),
        ("unknown rule", dict(rule=9), A, "rule"),
        ("adam betas", dict(t=_fake_table(L.LAYOUT_MOMENTS), h=fmx.Hyper(beta1=1.0), rule=L.RULE_ADAM), A, "beta1"),
        ("adam steps beyond int32", dict(t=_fake_table(L.LAYOUT_MOMENTS), h=fmx.Hyper(step=2 ** 31 - 5), rule=L.RULE_ADAM, N=8), A, "step"),
    ]
    for what, kw, want, word in cases:
        kw = dict(dict(t=t, h=h), **kw)
        rc = _call(lib, L, kw.pop("t"), kw.pop("h"), **kw)
        msg = lib.fmx_last_error_string().decode()
        assert rc == want, (what, rc, msg)
        assert msg and WHO in msg and word in msg, (what, msg)
    # the refusals do not depend on the optional outputs
    assert _call(lib, L, split, h, logit=0x71000, loss=0x72000) == UN
    # an empty stream: FMX_OK, nothing launched, the buffers may be null -- on the largest table the call takes as well
    for tt in (t, fits, _fake_table(L.LAYOUT_FTRL)):
        rule = L.RULE_FTRL if tt.layout == L.LAYOUT_FTRL else None
        assert _call(lib, L, tt, h, rule=rule, N=0) == L.OK
        assert _call(lib, L, tt, None, rule=rule, idx=None, N=0, rank=None) == L.OK
    # ... but not on a table or under a rule that is wrong anyway
    assert _call(lib, L, None, h, N=0) == A
    assert _call(lib, L, t, h, rule=L.RULE_FTRL, N=0) == A


@pytest.mark.parametrize("cls", ["DeepFMAdam", "NFMAdam", "DeepFMOnn", "NFMOnn", "AFMAdam"])
def test_classes_that_refuse_the_list_experiment(cls):
    mod = {"DeepFMAdam": "deepfm_adam", "NFMAdam": "nfm_adam", "DeepFMOnn": "deepfm_onn", "NFMOnn": "nfm_onn", "AFMAdam": "afm_adam"}[cls]
    klass = getattr(importlib.import_module("models.models_online_deep." + mod), cls)
    obj = object.__new__(klass)             # (no GPU: the constructors raise; the refusal needs no state)
    for negatives in ([[1]], None, "hard"):
        with pytest.raises(NotImplementedError, match="pure FM logit") as ei:
            klass.run_list_experiment(obj, [[0, 0]], [[1.0, 1.0]], [1], negatives=negatives)
        assert cls in str(ei.value) and "run_list_experiment" in str(ei.value)


def test_run_list_experiment_signature_and_the_limit_of_negatives():
    from models.models_online_deep.fm_adam import FMAdam
    params = inspect.signature(FMAdam.run_list_experiment).parameters
    assert list(params)[1:] == ["Xi", "Xv", "item_fields", "negatives", "n_neg", "candidates", "generator"]
    assert params["n_neg"].default == 4 and params["negatives"].default is None
    assert list(params) == list(inspect.signature(FMAdam.fit_lists).parameters)
    obj = object.__new__(FMAdam)            # (the limit is checked before the model is looked at)
    for negatives in (None, "hard"):
        for n_neg in (16, 100, 0):
            with pytest.raises(ValueError, match="15") as ei:
                FMAdam.run_list_experiment(obj, [[0, 0]], [[1.0, 1.0]], [1], negatives=negatives, n_neg=n_neg)
            assert "run_list_experiment" in str(ei.value)


def test_the_block_loop_is_shared_with_the_pair_form():
    from models.models_online_deep._ranking import RankingTraining
    pair = inspect.getsource(RankingTraining.run_pair_experiment)
    lists = inspect.getsource(RankingTraining.run_list_experiment)
    assert "_walk_mined_blocks" in pair and "_walk_mined_blocks" in lists
    assert "remine_every" in inspect.getsource(RankingTraining._walk_mined_blocks)
    assert "for b0 in range" not in pair and "for b0 in range" not in lists
