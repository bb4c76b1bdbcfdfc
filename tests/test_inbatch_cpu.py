"""In-batch sampled-softmax training of the FM without a GPU: the fmx_fm_inbatch_* symbols and their argument counts, what the
header promises, every refusal that is decided on the host (pointers that are never dereferenced), tests/inbatch_f64.py against
torch's float64 autograd on the explicit B B assembled rows and against list_f64 / listq_f64 on those rows as B lists of G = B,
in_batch_keys on CPU tensors, fit_in_batch's signature and the classes that refuse it.  No device is touched."""
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
COUNTS = {"fmx_fm_inbatch_splits": 2, "fmx_fm_inbatch_lse_bytes": 2, "fmx_fm_inbatch_forward": 16, "fmx_fm_inbatch_backward": 17,
          "fmx_fm_inbatch_occ_grad": 14, "fmx_fm_inbatch_workspace_bytes": 3, "fmx_fm_inbatch_step": 16, "fmx_fm_inbatch_stream": 17}
SIDES = ["fmx_fm_inbatch_forward", "fmx_fm_inbatch_backward"]
TABLE_CALLS = ["fmx_fm_inbatch_occ_grad", "fmx_fm_inbatch_step", "fmx_fm_inbatch_stream"]


def _lib():
    import fmx
    L = fmx._lib
    return fmx, L, L.load()


def test_symbols_and_argument_counts():
    fmx, L, lib = _lib()
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    defined = set(re.findall(r"\bT\s+(fmx_\w+)", out))
    header = open(os.path.join(ROOT, "include", "fmx.h")).read()
    for name, n in COUNTS.items():
        assert name in defined, name
        assert name in L.EXPORTS and len(getattr(lib, name).argtypes) == n, name
        decl = re.search(r"\bint(?:32_t|64_t)? " + name + r"\(([^;]*)\);", header)
        assert decl and len(decl.group(1).split(",")) == n, name
        comment = header[:decl.start()].rsplit("/*", 1)[1]
        assert "Replaces:" in comment and "torch.log_softmax(S_u S_c^T" in comment and "log_q)" in comment, name
    for name in ("fmx_fm_inbatch_lse_bytes", "fmx_fm_inbatch_workspace_bytes"):
        assert name in L.I64_RETURNS and getattr(lib, name).restype is C.c_int64
    assert lib.fmx_version() == 104


def test_header_states_the_objective():
    header = open(os.path.join(ROOT, "include", "fmx.h")).read()
    start = header.index("in-batch sampled-softmax training of the pure FM")
    text = " ".join(header[start:header.index("int32_t fmx_fm_inbatch_splits")].split())
    for phrase in ("Yi et al. 2019", "side_sums(want_bias=True / False)", "score(i, j) = (a_u[i] + a_c[j]) + dot", "fmx_fm_topk's top_score",
                   "E_i = {i} + {j != i : key[j] != key[i]}", "c_ij = score(i, j) - corr[j]", "bit-identical to the null-corr call",
                   "e_ij = exp(c_ij - m_i)", "loss_i = log(s_i) - (c_ii - m_i)", "g_ii = -(n_i / s_i) inv_b", "g_ij = 0 for ineligible j",
                   "gSu[i, :] = sum_j g_ij S_c[j, :]", "gac[j] = sum_i g_ij", "s_i >= 1", "No float atomics",
                   "splits = min(32, ceil(B / 64))", "E = x * fma(gac[j], S_c[j] - x * v, gSc[j])", "E = x * gSu[i]", "there is no gau term",
                   "BIT-UNCHANGED", "zero-gradient step of a touched row", "B = 1 is legal", "FMX_VERSION stays 104"):
        assert phrase in text, phrase


def test_geometry_is_the_documented_formula():
    fmx, L, lib = _lib()
    from inbatch_f64 import first_split_threshold, geometry
    for B in (1, 2, 63, 64, 65, 128, 129, 1000, 2048, 2049, 4096, 32768):
        for kp in (4, 16, 64):
            assert lib.fmx_fm_inbatch_splits(B, kp) == geometry(B)[0], (B, kp)
    B1 = first_split_threshold()
    assert lib.fmx_fm_inbatch_splits(B1, 16) == 1 and lib.fmx_fm_inbatch_splits(B1 + 1, 16) == 2
    assert lib.fmx_fm_inbatch_splits(0, 16) == L.ERR_ARG and lib.fmx_fm_inbatch_splits(4, 12) == L.ERR_UNSUPPORTED
    assert lib.fmx_fm_inbatch_lse_bytes(0, 16) == L.ERR_ARG and lib.fmx_fm_inbatch_lse_bytes(4, 5) == L.ERR_UNSUPPORTED
    # the lse block: three padded rows of per-row state, four [splits, B] arrays and two [splits, B, kp] ones
    up = lambda n: (n + 255) // 256 * 256  # noqa: E731
    for B, kp in ((1, 4), (65, 16), (1000, 64)):
        s = geometry(B)[0]
        assert lib.fmx_fm_inbatch_lse_bytes(B, kp) == 3 * up(4 * B) + 4 * up(4 * s * B) + 2 * up(4 * s * B * kp)


def _sides(who, lib, L, Su=0x40000, au=0x41000, Sc=0x42000, ac=0x43000, B=4, kp=16, ld=16, lse=0x50000, lse_bytes=1 << 40, out=0x60000):
    if who == "fmx_fm_inbatch_forward":
        return lib.fmx_fm_inbatch_forward(Su, ld, au, Sc, ld, ac, B, kp, None, None, 1.0, lse, lse_bytes, out, None, None)
    return lib.fmx_fm_inbatch_backward(Su, ld, au, Sc, ld, ac, B, kp, None, None, 1.0, lse, lse_bytes, out, 0x61000 if out else None,
                                       0x62000, None)


@pytest.mark.parametrize("who", SIDES)
def test_side_calls_refuse_on_the_host(who):
    fmx, L, lib = _lib()
    A, SH, UN, AL = L.ERR_ARG, L.ERR_SHAPE, L.ERR_UNSUPPORTED, L.ERR_ALIGN
    need = lib.fmx_fm_inbatch_lse_bytes(4, 16)
    cases = [("Su", dict(Su=None), A, "Su"), ("ac", dict(ac=None), A, "ac"), ("B 0", dict(B=0), A, "B = 0"), ("B -2", dict(B=-2), A, "B = -2"),
             ("kp 12", dict(kp=12), UN, "kp = 12"), ("kp 128", dict(kp=128), UN, "kp = 128"), ("kp 0", dict(kp=0), UN, "kp = 0"),
             ("ld short", dict(ld=12), SH, "ld_u"), ("ld odd", dict(ld=18), SH, "ld_u"), ("Su unaligned", dict(Su=0x40004), AL, "Su"),
             ("workspace null", dict(lse=None), A, "workspace"), ("workspace unaligned", dict(lse=0x50008), AL, "workspace"),
             ("workspace short", dict(lse_bytes=need - 1), SH, "fmx_fm_inbatch_lse_bytes"), ("outputs", dict(out=None), A, "null")]
    for what, kw, want, word in cases:
        rc = _sides(who, lib, L, **kw)
        msg = lib.fmx_last_error_string().decode()
        assert rc == want, (who, what, rc, msg)
        assert who in msg and (word in msg or "required" in msg), (who, what, msg)


def _table_call(who, lib, L, t, h, rule=None, idx=0x60000, B=4, fields=(1,), n_fields=None, ws=0x50000, ws_bytes=1 << 40, n_pool=1,
                n_steps=0, fwd=None):
    """The call with fake pointers: only ever sent where a host check refuses it (the stream also with n_steps = 0, which checks
    everything and launches nothing)."""
    tp = None if t is None else C.byref(t)
    hp = None if h is None else h.ref()
    rule = L.RULE_SIGNADAM if rule is None else rule
    arr = None if fields is None else (C.c_int32 * max(len(fields), 1))(*fields)
    n = (0 if fields is None else len(fields)) if n_fields is None else n_fields
    fp = None if fwd is None else C.byref(fwd)
    if who == "fmx_fm_inbatch_occ_grad":
        return lib.fmx_fm_inbatch_occ_grad(tp, idx, None, arr, n, 0x70000, 0x71000, 0x72000, 0x73000, 16, B, 0x74000, 32, None)
    if who == "fmx_fm_inbatch_step":
        return lib.fmx_fm_inbatch_step(tp, hp, rule, idx, None, arr, n, None, None, B, 1.0, ws, ws_bytes, fp, None, None)
    return lib.fmx_fm_inbatch_stream(tp, hp, rule, idx, arr, n, None, None, n_pool, B, 1.0, n_steps, ws, ws_bytes, fp, None, None)


@pytest.mark.parametrize("who", TABLE_CALLS)
def test_table_calls_refuse_on_the_host(who):
    fmx, L, lib = _lib()
    A, SH, UN, AL = L.ERR_ARG, L.ERR_SHAPE, L.ERR_UNSUPPORTED, L.ERR_ALIGN
    h = fmx.Hyper(lr=0.01)
    t = _fake_table(L.LAYOUT_WEIGHTS)
    mapped = _fake_table(L.LAYOUT_WEIGHTS)
    mapped.field_cols, mapped.n_cols = 0x90000, 2
    based = _fake_table(L.LAYOUT_WEIGHTS)
    based.field_base = 0x90000
    kp12 = _fake_table(L.LAYOUT_WEIGHTS)
    kp12.kp, kp12.k = 12, 10
    cases = [("table", dict(t=None), A, "table"), ("idx", dict(idx=None), A, "idx"), ("B 0", dict(B=0), A, "B = 0"),
             ("B -3", dict(B=-3), A, "B = -3"), ("no item field", dict(fields=()), A, "n_item_fields = 0"),
             ("three item fields of two", dict(fields=(0, 1, 1)), A, "n_item_fields = 3"), ("negative count", dict(n_fields=-1), A, "n_item_fields"),
             ("null item_fields", dict(fields=None, n_fields=1), A, "item_fields"), ("field 2 of two", dict(fields=(2,)), A, "item field 2"),
             ("field -1", dict(fields=(-1,)), A, "item field -1"), ("repeated", dict(fields=(1, 1)), A, "repeated"),
             ("kp 12", dict(t=kp12), UN, "kp = 12"), ("field_cols", dict(t=mapped), UN, "field_cols"), ("field_base", dict(t=based), UN, "field_base")]
    if who != "fmx_fm_inbatch_occ_grad":
        need = lib.fmx_fm_inbatch_workspace_bytes(C.byref(t), 4, 1)
        assert need > lib.fmx_workspace_bytes(C.byref(t), 4) + 16
        bad_loss = L.FwdOut()
        bad_loss.loss = 0x41004
        cases += [("hyper", dict(h=None), A, "hyper"),
                  ("ftrl rule on a weights table", dict(rule=L.RULE_FTRL), A, "FMX_RULE_FTRL"),
                  ("adam rule on a weights table", dict(rule=L.RULE_ADAM), A, "FMX_RULE_ADAM"),
                  ("sgd on a moments table", dict(t=_fake_table(L.LAYOUT_MOMENTS), rule=L.RULE_SGD), A, "rule"),
                  ("unknown rule", dict(rule=9), A, "rule"),
                  ("adam betas", dict(t=_fake_table(L.LAYOUT_MOMENTS), h=fmx.Hyper(beta1=1.0), rule=L.RULE_ADAM), A, "beta1"),
                  ("workspace null", dict(ws=None), A, "workspace"), ("workspace unaligned", dict(ws=0x50008), AL, "workspace"),
                  ("workspace of a plain step", dict(ws_bytes=lib.fmx_workspace_bytes(C.byref(t), 4) + 16), SH, "fmx_fm_inbatch_workspace_bytes"),
                  ("workspace one byte short", dict(ws_bytes=need - 1), SH, "fmx_fm_inbatch_workspace_bytes"),
                  ("fwd->loss unaligned", dict(fwd=bad_loss), AL, "fwd->loss")]
    for what, kw, want, word in cases:
        kw = dict(dict(t=t, h=h), **kw)
        rc = _table_call(who, lib, L, kw.pop("t"), kw.pop("h"), **kw)
        msg = lib.fmx_last_error_string().decode()
        assert rc == want, (who, what, rc, msg)
        assert msg and who in msg and word in msg, (who, what, msg)
    if who == "fmx_fm_inbatch_occ_grad":
        return
    # B beyond what the sort accepts: refused with fmx_sort_occurrences' code and words, under this entry point's name
    for B in (32769, 2 ** 26):
        want = lib.fmx_sort_occurrences(C.byref(t), 0x60000, B, 0x50000, 1 << 50, None, None)
        want_msg = lib.fmx_last_error_string().decode()
        assert want == UN
        rc = _table_call(who, lib, L, t, h, B=B, ws_bytes=1 << 50)
        msg = lib.fmx_last_error_string().decode()
        assert rc == want and who in msg and want_msg in msg, (rc, msg)
    if who == "fmx_fm_inbatch_stream":
        assert _table_call(who, lib, L, t, h, ws_bytes=need) == L.OK      # n_steps = 0: everything checked, nothing launched
        assert _table_call(who, lib, L, t, h, ws_bytes=need, fwd=L.FwdOut()) == L.OK
        for kw in (dict(n_pool=0), dict(n_steps=-1)):
            rc = _table_call(who, lib, L, t, h, **kw)
            assert rc == A and who in lib.fmx_last_error_string().decode()
        tm = _fake_table(L.LAYOUT_MOMENTS)
        rc = _table_call(who, lib, L, tm, fmx.Hyper(step=2 ** 31 - 5), rule=L.RULE_ADAM, n_steps=8)
        assert rc == A and who in lib.fmx_last_error_string().decode()


def test_workspace_bytes():
    fmx, L, lib = _lib()
    t = _fake_table(L.LAYOUT_WEIGHTS)
    a, b = lib.fmx_fm_inbatch_workspace_bytes(C.byref(t), 64, 1), lib.fmx_fm_inbatch_workspace_bytes(C.byref(t), 65, 1)
    assert lib.fmx_workspace_bytes(C.byref(t), 64) + 16 + lib.fmx_fm_inbatch_lse_bytes(64, 16) < a < b and a % 16 == 0
    assert lib.fmx_fm_inbatch_workspace_bytes(C.byref(t), 64, 2) == a
    for B, n in ((0, 1), (4, 0), (4, 3)):
        assert lib.fmx_fm_inbatch_workspace_bytes(C.byref(t), B, n) == L.ERR_ARG, (B, n)
        assert "fmx_fm_inbatch_workspace_bytes" in lib.fmx_last_error_string().decode()
    assert lib.fmx_fm_inbatch_workspace_bytes(None, 4, 1) == L.ERR_ARG


# ---- fmx/pairwise.py and the classes, on CPU ----
def test_in_batch_keys():
    from fmx.pairwise import in_batch_keys
    idx = torch.tensor([[0, 5, 2, 1], [1, 5, 2, 0], [2, 4, 2, 1], [3, 5, 3, 1], [4, 5, 2, 1]], dtype=torch.int32)
    k1 = in_batch_keys(idx, [2])
    assert k1.dtype == torch.int32 and k1.shape == (5,) and k1.is_contiguous()
    same = k1[:, None] == k1[None, :]
    assert torch.equal(same, idx[:, 2][:, None] == idx[:, 2][None, :])
    k2 = in_batch_keys(idx, [2, 3])
    want = (idx[:, None, 2:] == idx[None, :, 2:]).all(dim=2)
    assert torch.equal(k2[:, None] == k2[None, :], want) and int(k2.max()) == 2 and int(k2.min()) == 0      # dense: 0 .. n_unique - 1
    assert torch.equal(in_batch_keys(idx, 2), k1) and torch.equal(in_batch_keys(idx.numpy(), [3, 2]) == k2[0], k2 == k2[0])
    assert in_batch_keys(idx[:1], [2]).tolist() == [0]
    for bad in (dict(idx=idx[0], item_fields=[2]), dict(idx=idx, item_fields=[]), dict(idx=idx, item_fields=[1, 1]), dict(idx=idx, item_fields=[4])):
        with pytest.raises(ValueError):
            in_batch_keys(**bad)


@pytest.mark.parametrize("cls", ["DeepFMAdam", "NFMAdam", "DeepFMOnn", "NFMOnn", "AFMAdam"])
def test_classes_that_refuse_in_batch_training(cls):
    mod = {"DeepFMAdam": "deepfm_adam", "NFMAdam": "nfm_adam", "DeepFMOnn": "deepfm_onn", "NFMOnn": "nfm_onn", "AFMAdam": "afm_adam"}[cls]
    klass = getattr(importlib.import_module("models.models_online_deep." + mod), cls)
    obj = object.__new__(klass)             # (no GPU: the constructors raise; the refusal needs no state)
    for kw in (dict(), dict(log_q=[0.0]), dict(mask_duplicates=False)):
        with pytest.raises(NotImplementedError, match="pure FM logit") as ei:
            klass.fit_in_batch(obj, [[0, 0]], [[1.0, 1.0]], [1], **kw)
        assert cls in str(ei.value) and "fit_in_batch" in str(ei.value)


def test_fit_in_batch_signature():
    from models.models_online_deep.fm_adam import FMAdam
    params = inspect.signature(FMAdam.fit_in_batch).parameters
    assert list(params)[1:] == ["Xi", "Xv", "item_fields", "log_q", "mask_duplicates", "candidates"]
    assert params["log_q"].default is None and params["mask_duplicates"].default is True and params["candidates"].default is None
    import fmx
    for name in ("inbatch_step", "inbatch_stream"):
        assert callable(getattr(fmx.FMEngine, name))
    assert list(inspect.signature(fmx.FMEngine.inbatch_step).parameters)[1:] == ["hyper", "rule", "idx_d", "item_fields", "xv_d", "corr", "key",
                                                                               "inv_b"]


# ---- tests/inbatch_f64.py against independent arithmetic ----
SIZES, K, ITEM = [7, 5, 11, 3, 6], 4, [2, 4]


def _problem(B, seed=23):
    rng = np.random.default_rng(seed + B)
    off = np.concatenate([[0], np.cumsum(SIZES)])
    R, F = int(off[-1]), len(SIZES)
    state = dict(V=rng.normal(0, 0.3, (R, K)).astype(np.float32), w=rng.normal(0, 0.3, R).astype(np.float32), bias=np.float32(0.2))
    local = np.stack([rng.integers(0, s, B) for s in SIZES], axis=1)
    for i in range(B):                                     # every row its own item: keys that mask nothing
        local[i, 2], local[i, 4] = i % SIZES[2], (i // SIZES[2]) % SIZES[4]
    if B >= 5:
        local[3, [0, 1, 3]] = local[1, [0, 1, 3]]          # a repeated context
    x = rng.uniform(0.5, 1.5, (B, F)).astype(np.float32)
    corr = rng.uniform(-8.0, 0.0, B).astype(np.float32)
    return state, local + off[:-1], x, corr, R, F


def _torch_assembled(state, lrows, lx, lcorr, B, inv_b):
    V = torch.tensor(state["V"], dtype=torch.float64, requires_grad=True)
    w = torch.tensor(state["w"], dtype=torch.float64, requires_grad=True)
    b = torch.tensor(float(state["bias"]), dtype=torch.float64, requires_grad=True)
    rt, xt = torch.tensor(lrows), torch.tensor(lx, dtype=torch.float64)
    e = V[rt] * xt[:, :, None]
    z = (w[rt] * xt).sum(1) + 0.5 * (e.sum(1) ** 2 - (e * e).sum(1)).sum(1) + b
    c = z if lcorr is None else z - torch.tensor(lcorr, dtype=torch.float64)
    ce = -torch.log_softmax(c.reshape(B, B), dim=1)[:, 0]
    loss = ce.sum() * inv_b
    loss.backward()
    return z.detach().numpy(), ce.detach().numpy(), float(loss.detach()), V.grad.numpy(), w.grad.numpy(), float(b.grad)


@pytest.mark.parametrize("with_corr", [False, True])
@pytest.mark.parametrize("B", [2, 5, 16])
def test_inbatch_f64_is_the_assembled_list_step(B, with_corr):
    from inbatch_f64 import assembled_lists, inbatch_step_f64
    from list_f64 import list_step_f64
    from listq_f64 import listq_step_f64
    state, rows, x, corr, R, F = _problem(B)
    corr = corr if with_corr else None
    inv_b = 1.0 / B
    key = np.unique(rows[:, ITEM], axis=0, return_inverse=True)[1].reshape(-1)
    assert len(set(key.tolist())) == B                                          # keys that mask nothing
    lrows, lx, lcorr, order = assembled_lists(rows, x, ITEM, corr)
    ctx_rows = np.unique(rows[:, [0, 1, 3]])
    for k_arg in (None, key):
        r = inbatch_step_f64(state, rows, x, ITEM, "sgd", dict(lr=0.05), corr=corr, key=k_arg, inv_b=inv_b)
        # (a) torch float64 autograd on the explicit B B rows
        z, ce, loss, gV, gw, gb = _torch_assembled(state, lrows, lx, lcorr, B, inv_b)
        score_l = np.take_along_axis(r["score"], order, axis=1)
        np.testing.assert_allclose(score_l.reshape(-1), z, rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(r["loss_b"], ce, rtol=1e-11, atol=1e-13)
        assert abs(r["loss"] - loss) <= 1e-11 * abs(loss)
        u = r["urows"]
        sV, sw = np.abs(gV).max(), np.abs(gw).max()
        np.testing.assert_allclose(r["dV"], gV[u], rtol=1e-10, atol=1e-12 * sV)
        mask = np.ones(R, bool)
        mask[u] = False
        assert not gV[mask].any() and not gw[mask].any()
        item_u = ~np.isin(u, ctx_rows)
        np.testing.assert_allclose(r["dw"][item_u], gw[u][item_u], rtol=1e-10, atol=1e-12 * sw)
        # (b) list_f64 / listq_f64 on the same rows as B lists of G = B, the positive first
        if corr is None:
            ls = list_step_f64(state, lrows, lx, B, "sgd", dict(lr=0.05), inv_b)
        else:
            ls = listq_step_f64(state, lrows, lx, B, lcorr, "sgd", dict(lr=0.05), inv_b)
        assert np.array_equal(ls["urows"], u)
        g_l = np.take_along_axis(r["g"], order, axis=1).reshape(-1)
        np.testing.assert_allclose(g_l, ls["dz"], rtol=1e-11, atol=1e-15)
        np.testing.assert_allclose(r["loss_b"], ls["loss_b"][0::B], rtol=1e-11, atol=1e-13)
        np.testing.assert_allclose(r["dV"], ls["dV"], rtol=1e-10, atol=1e-12 * sV)
        np.testing.assert_allclose(r["new"]["V"], ls["new"]["V"], rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(r["new"]["w"][u][item_u], ls["new"]["w"][u][item_u], rtol=1e-12, atol=1e-14)
        # (c) the difference by definition: the in-batch step DROPS the bias and the context fields' first-order terms, whose
        # gradient is the row sum of g -- zero in exact arithmetic.  The assembled references carry them: autograd's are zero up to
        # float64 rounding, and both lie below the fp32 floor the assembled-list reference itself gives those quantities
        ctx_u = ~item_u
        assert ctx_u.any() and item_u.any()
        assert r["db"] == 0.0 and not r["dw"][ctx_u].any() and not r["floor"]["dw"][ctx_u].any()
        assert abs(gb) <= 1e-14 and np.abs(gw[u][ctx_u]).max() <= 1e-14 < np.abs(gw[u][item_u]).max()
        assert (np.abs(ls["dw"][ctx_u] - r["dw"][ctx_u]) < ls["floor"]["dw"][ctx_u]).all()
        assert (np.abs(ls["new"]["w"][u][ctx_u] - r["new"]["w"][u][ctx_u]) < ls["floor"]["w"][ctx_u]).all()
        assert r["new"]["bias"] == ls["new"]["bias"] == np.float64(state["bias"])
        # the row sums of g that the definition takes as zero
        assert np.abs(r["g"].sum(axis=1)).max() <= 1e-15
        # the floors are positive where something is computed
        fl = r["floor"]
        assert (fl["loss_b"] > 0).all() and (fl["g"][r["eligible"]] > 0).all() and (fl["gSu"] > 0).all() and (fl["occ"] > 0).all()
        assert fl["loss"] > 0 and (fl["dV"] > 0).all()
    # ftrl: the same gradients through the rule block both helpers share
    from oracle.fm_oracle import ftrl_z_for_weight
    # (fp32-representable hyper-parameters: inbatch_f64 reads them as the fp32 values the device gets, list_f64 as given)
    h = {n_: float(np.float32(v)) for n_, v in dict(alpha=0.05, beta=1.0, l1=0.001, l2=0.01).items()}
    rng = np.random.default_rng(3)
    st = dict(zV=ftrl_z_for_weight(state["V"], **h), nV=rng.uniform(0, 0.5, state["V"].shape).astype(np.float32),
              zw=ftrl_z_for_weight(state["w"], **h), nw=rng.uniform(0, 0.5, state["w"].shape).astype(np.float32),
              zb=np.float32(-0.4), nb=np.float32(0.2))
    r = inbatch_step_f64(st, rows, x, ITEM, "ftrl", h, corr=corr, key=key, inv_b=inv_b)
    ls = (list_step_f64(st, lrows, lx, B, "ftrl", h, inv_b) if corr is None else listq_step_f64(st, lrows, lx, B, lcorr, "ftrl", h, inv_b))
    for kk in ("zV", "nV"):
        np.testing.assert_allclose(r["new"][kk], ls["new"][kk], rtol=1e-11, atol=1e-13)
    u, item_u = r["urows"], ~np.isin(r["urows"], ctx_rows)
    for kk in ("zw", "nw"):
        np.testing.assert_allclose(r["new"][kk][u][item_u], ls["new"][kk][u][item_u], rtol=1e-11, atol=1e-13)
        assert (np.abs(r["new"][kk][u][~item_u] - ls["new"][kk][u][~item_u]) < ls["floor"][kk][~item_u]).all()
        assert np.array_equal(r["new"][kk][u][~item_u], np.asarray(st[kk], np.float64)[u][~item_u])     # +0 gradient: unchanged
    assert r["new"]["zb"] == np.float64(st["zb"]) and r["new"]["nb"] == np.float64(st["nb"])


def test_inbatch_f64_masks_accidental_hits():
    from inbatch_f64 import inbatch_step_f64
    B = 6
    state, rows, x, corr, R, F = _problem(B)
    rows[4, ITEM] = rows[1, ITEM]                                               # rows 1 and 4 hold the same item
    key = np.unique(rows[:, ITEM], axis=0, return_inverse=True)[1].reshape(-1)
    r = inbatch_step_f64(state, rows, x, ITEM, "sgd", dict(lr=0.05), corr=corr, key=key)
    el = r["eligible"]
    assert not el[1, 4] and not el[4, 1] and el.sum() == B * B - 2 and el.diagonal().all()
    assert r["g"][1, 4] == 0.0 and r["g"][4, 1] == 0.0 and r["floor"]["g"][1, 4] == 0.0
    free = inbatch_step_f64(state, rows, x, ITEM, "sgd", dict(lr=0.05), corr=corr, key=None)
    assert free["g"][1, 4] > 0 and free["loss_b"][1] > r["loss_b"][1]
    # all keys equal: only the diagonal is eligible -- every loss 0, every gradient 0
    one = inbatch_step_f64(state, rows, x, ITEM, "sgd", dict(lr=0.05), corr=corr, key=np.zeros(B, np.int32))
    assert not one["loss_b"].any() and not one["g"].any() and not one["dV"].any() and one["loss"] == 0.0
    # B = 1
    solo = inbatch_step_f64(state, rows[:1], x[:1], ITEM, "sgd", dict(lr=0.05))
    assert solo["loss"] == 0.0 and not solo["dV"].any() and np.array_equal(solo["new"]["V"], state["V"].astype(np.float64))
