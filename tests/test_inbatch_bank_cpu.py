"""The cross-batch item bank of the in-batch loss without a GPU (fmx_fm_inbatch_bank_*, include/fmx.h): tests/inbatch_bank_f64.py
against torch's float64 autograd on the concatenated logits with the bank detached, and against inbatch_f64 with an empty bank;
the geometry function; a numpy model of the ring over push sequences that fill it exactly, wrap mid-push and repeat; the refusals of
ItemBank, of the C calls (decided on the host: pointers that are never dereferenced) and of the classes; the header's symbols."""
import ctypes as C
import importlib
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from inbatch_bank_f64 import bank_geometry, inbatch_bank_step_f64, ring_push
from inbatch_f64 import geometry, inbatch_step_f64
from test_adaptive_rules_cpu import _fake_table
from test_inbatch_cpu import ITEM, K, _problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = {"fmx_fm_inbatch_bank_splits": 2, "fmx_fm_inbatch_bank_lse_bytes": 3, "fmx_fm_inbatch_bank_forward": 18,
          "fmx_fm_inbatch_bank_backward": 18, "fmx_fm_inbatch_bank_push": 9, "fmx_fm_inbatch_bank_workspace_bytes": 4,
          "fmx_fm_inbatch_bank_step": 17, "fmx_fm_inbatch_bank_stream": 18}


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
        assert "Replaces:" in comment and "torch.log_softmax(cat(" in comment, name
    for name in ("fmx_fm_inbatch_bank_lse_bytes", "fmx_fm_inbatch_bank_workspace_bytes"):
        assert name in L.I64_RETURNS and getattr(lib, name).restype is C.c_int64
    assert lib.fmx_version() == 104
    fields = dict(L.ItemBank._fields_)
    assert list(fields) == ["S", "a", "corr", "key", "state", "capacity", "kp"]
    struct = header[header.index("typedef struct fmx_item_bank"):header.index("} fmx_item_bank_t;")]
    assert [m for m in re.findall(r"\*?(\w+);", struct)] == list(fields)
    assert int(re.search(r"#define FMX_ITEM_BANK_MAX (\d+)", header).group(1)) == L.ITEM_BANK_MAX >= 65536


def test_header_states_the_bank():
    header = open(os.path.join(ROOT, "include", "fmx.h")).read()
    start = header.index("a cross-batch item bank for the in-batch loss")
    lines = [ln.strip().lstrip("*").strip() for ln in header[start:header.index("int32_t fmx_fm_inbatch_bank_splits")].splitlines()]
    text = " ".join(" ".join(lines).split())                                # (a phrase may run over a line break of the comment)
    for phrase in ("Wang et al. 2021", "state[0] (head) is the next slot to write", "a zeroed state is an empty bank",
                   "Q_i = every slot q < count with key[i] != bank.key[q]", "c_iq = score(i, q) - bank.corr[q]",
                   "score(i, q) = (a_u[i] + bank.a[q]) + dot", "every bank item is a negative", "g_iq = (e_iq / s_i) inv_b",
                   "gSu[i] = sum_j g_ij S_c[j] + sum_q g_iq bank.S[q]", "there is still no gau term",
                   "splits_q = min(32, ceil(M / 64))", "a function of M alone, not of count", "No float atomics",
                   "With count = 0 every output of a bank call is bit-identical to the plain call's",
                   "head <- (head + B) mod M, count <- min(M, count + B)", "BEFORE the update",
                   "The push is a launch of its own behind the last reader of the bank"):
        assert phrase in text, phrase


def test_geometry_is_the_documented_formula():
    fmx, L, lib = _lib()
    for M in (1, 63, 64, 65, 130, 2048, 2049, 2113, 4096, 65536, L.ITEM_BANK_MAX):
        want = min(32, -(-M // 64))
        per = -(-M // want)
        assert bank_geometry(M) == (-(-M // per), per) == geometry(M)
        for kp in (4, 16, 64):
            assert lib.fmx_fm_inbatch_bank_splits(M, kp) == bank_geometry(M)[0], (M, kp)
    assert bank_geometry(130) == (3, 44) and bank_geometry(2113) == (32, 67) and bank_geometry(64) == (1, 64)
    assert lib.fmx_fm_inbatch_bank_splits(0, 16) == L.ERR_ARG and lib.fmx_fm_inbatch_bank_splits(4, 12) == L.ERR_UNSUPPORTED
    assert lib.fmx_fm_inbatch_bank_splits(L.ITEM_BANK_MAX + 1, 16) == L.ERR_UNSUPPORTED
    # the lse block: three rows of per-row state, pm / ps / pn over the ranges of both kinds, gac's over the batch's, gSu's over both
    # kinds and gSc's over the batch's, each padded to 256 bytes
    up = lambda n: (n + 255) // 256 * 256  # noqa: E731
    for B, M, kp in ((1, 1, 4), (65, 130, 16), (257, 2113, 64)):
        sb, sq = geometry(B)[0], bank_geometry(M)[0]
        want = 3 * up(4 * B) + 3 * up(4 * (sb + sq) * B) + up(4 * sb * B) + up(4 * (sb + sq) * B * kp) + up(4 * sb * B * kp)
        assert lib.fmx_fm_inbatch_bank_lse_bytes(B, M, kp) == want
        plain = lib.fmx_fm_inbatch_lse_bytes(B, kp)
        assert want > plain if B > 1 else want == plain                     # (B = 1: one more range fits the padding)
    for bad, code in (((0, 4, 16), L.ERR_ARG), ((4, 0, 16), L.ERR_ARG), ((4, 4, 12), L.ERR_UNSUPPORTED), ((4, L.ITEM_BANK_MAX + 1, 16), L.ERR_UNSUPPORTED)):
        assert lib.fmx_fm_inbatch_bank_lse_bytes(*bad) == code
        assert "fmx_fm_inbatch_bank_lse_bytes" in lib.fmx_last_error_string().decode()
    t = _fake_table(L.LAYOUT_WEIGHTS)
    plain = lib.fmx_fm_inbatch_workspace_bytes(C.byref(t), 65, 1)
    with_bank = lib.fmx_fm_inbatch_bank_workspace_bytes(C.byref(t), 65, 130, 1)
    assert with_bank - plain == lib.fmx_fm_inbatch_bank_lse_bytes(65, 130, 16) - lib.fmx_fm_inbatch_lse_bytes(65, 16)
    for bad in ((0, 4, 1), (4, 0, 1), (4, 4, 0)):
        assert lib.fmx_fm_inbatch_bank_workspace_bytes(C.byref(t), *bad) == L.ERR_ARG


# ---- the ring ----
@pytest.mark.parametrize("M,Bs", [(8, [4, 4, 4, 4, 4]), (150, [65, 65, 65, 65, 65, 65]), (7, [3, 3, 3, 3, 3, 3, 3, 3]), (5, [5, 5, 5]),
                                  (1, [1, 1, 1]), (10, [3, 7, 10, 1, 9])])
def test_ring_model(M, Bs):
    """Pushes that fill the ring exactly, wrap mid-push and repeat: the valid slots are always the prefix [0, count), a push
    never writes a slot twice, the ring holds the newest min(M, pushed) items, and head is where the oldest one sits once full"""
    ring = dict(M=M, head=0, count=0)
    held = [None] * M
    pushed = []
    for step, B in enumerate(Bs):
        slots = ring_push(ring, B)
        assert len(set(slots)) == B and all(0 <= q < M for q in slots)
        for j, q in enumerate(slots):
            held[q] = (step, j)
            pushed.append((step, j))
        total = len(pushed)
        assert ring["count"] == min(M, total) and ring["head"] == total % M
        valid = held[:ring["count"]]
        assert None not in valid and all(h is None for h in held[ring["count"]:])
        assert sorted(valid) == sorted(pushed[-min(M, total):])
        if total >= M:
            assert held[ring["head"]] == pushed[-M]


# ---- the reference against independent arithmetic ----
def _bank(B, Q, M, keyed, seed=5):
    rng = np.random.default_rng(seed + Q)
    return dict(S=rng.normal(0, 0.4, (Q, K)).astype(np.float32), a=rng.normal(0, 0.3, Q).astype(np.float32),
                corr=rng.uniform(-8.0, 0.0, Q).astype(np.float32), key=rng.integers(0, B + 3, Q).astype(np.int32) if keyed else None, M=M)


@pytest.mark.parametrize("keyed", [False, True])
@pytest.mark.parametrize("B,Q,M", [(1, 5, 8), (6, 1, 1), (9, 70, 130), (70, 40, 64)])
def test_reference_is_torch_autograd_with_the_bank_detached(B, Q, M, keyed):
    state, rows, x, corr, R, F = _problem(B)
    key = (np.arange(B) % (B // 2 + 1)).astype(np.int32) if keyed else None
    bank = _bank(B, Q, M, keyed)
    inv_b = 1.0 / B
    ref = inbatch_bank_step_f64(state, rows, x, ITEM, "sgd", dict(lr=0.05), bank, corr=corr, key=key, inv_b=inv_b, kp=K)
    V = torch.tensor(state["V"], dtype=torch.float64, requires_grad=True)
    w = torch.tensor(state["w"], dtype=torch.float64, requires_grad=True)
    b = torch.tensor(float(state["bias"]), dtype=torch.float64, requires_grad=True)
    item = np.zeros(F, bool)
    item[ITEM] = True
    rt, xt = torch.tensor(rows), torch.tensor(x, dtype=torch.float64)

    def side(mask, bias):
        e = V[rt[:, mask]] * xt[:, mask, None]
        S = e.sum(1)
        return S, (w[rt[:, mask]] * xt[:, mask]).sum(1) + 0.5 * (S * S - (e * e).sum(1)).sum(1) + bias
    Su, au = side(~item, b)
    Sc, ac = side(item, 0.0)
    bS, ba = torch.tensor(bank["S"], dtype=torch.float64), torch.tensor(bank["a"], dtype=torch.float64)        # detached: plain data
    logits = torch.cat([Su @ Sc.T + au[:, None] + ac[None, :], Su @ bS.T + au[:, None] + ba[None, :]], dim=1)
    logits = logits - torch.cat([torch.tensor(corr, dtype=torch.float64), torch.tensor(bank["corr"], dtype=torch.float64)])[None, :]
    el = torch.ones((B, B + Q), dtype=torch.bool)
    if keyed:
        allk = np.concatenate([key, bank["key"]])
        el = torch.tensor(key[:, None] != allk[None, :])
        el[torch.arange(B), torch.arange(B)] = True
    lsm = torch.log_softmax(torch.where(el, logits, torch.tensor(-np.inf, dtype=torch.float64)), dim=1)
    ce = -lsm[torch.arange(B), torch.arange(B)]
    (ce.sum() * inv_b).backward()
    np.testing.assert_allclose(ref["loss_b"], ce.detach().numpy(), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(ref["bank_score"], (Su @ bS.T + au[:, None] + ba[None, :]).detach().numpy(), rtol=1e-12, atol=1e-13)
    assert np.array_equal(ref["eligible"], el.numpy())
    u = ref["urows"]
    np.testing.assert_allclose(ref["dV"], V.grad.numpy()[u], rtol=1e-10, atol=1e-13)
    # first-order weights: the reference DEFINES the row sum of g as zero (no gau term): autograd's context rows and bias hold the
    # rounding of a sum that is zero in exact arithmetic
    np.testing.assert_allclose(ref["dw"], w.grad.numpy()[u], rtol=1e-10, atol=1e-13)
    assert abs(float(b.grad)) < 1e-13 and ref["db"] == 0.0
    mask = np.ones(R, bool)
    mask[u] = False
    assert not V.grad.numpy()[mask].any() and not w.grad.numpy()[mask].any()
    # every floor is positive where its quantity is read, and the depth of gSu's sum is the documented one
    for name in ("loss_b", "gSu", "gSc", "gac", "bank_score"):
        assert (ref["floor"][name] >= 0).all() and np.isfinite(ref["floor"][name]).all(), name
    if Q:
        assert (ref["n"] > inbatch_step_f64(state, rows, x, ITEM, "sgd", dict(lr=0.05), corr=corr, key=key, inv_b=inv_b, kp=K)["n"] - 1e-300).all()


@pytest.mark.parametrize("rule", ["sgd", "ftrl"])
@pytest.mark.parametrize("B", [1, 5, 66])
def test_reference_with_an_empty_bank_is_inbatch_f64(B, rule):
    state, rows, x, corr, R, F = _problem(B)
    hyper = dict(lr=0.05)
    if rule == "ftrl":
        rng = np.random.default_rng(B)
        hyper = dict(alpha=0.05, beta=1.0, l1=0.001, l2=0.01)
        state = dict(zV=rng.normal(0, 0.3, (R, K)).astype(np.float32), nV=rng.uniform(0.05, 0.2, (R, K)).astype(np.float32),
                     zw=rng.normal(0, 0.3, R).astype(np.float32), nw=rng.uniform(0.05, 0.2, R).astype(np.float32), zb=np.float32(0.1), nb=np.float32(0.1))
    key = (np.arange(B) % (B // 2 + 1)).astype(np.int32)
    empty = dict(S=np.zeros((0, K), np.float32), a=np.zeros(0, np.float32), corr=np.zeros(0, np.float32), key=np.zeros(0, np.int32), M=130)
    got = inbatch_bank_step_f64(state, rows, x, ITEM, rule, hyper, empty, corr=corr, key=key, kp=K)
    want = inbatch_step_f64(state, rows, x, ITEM, rule, hyper, corr=corr, key=key, kp=K)
    for name in ("loss", "loss_b", "m", "s", "n", "g", "gSu", "gSc", "gac", "occ", "dV", "dw", "urows"):
        np.testing.assert_array_equal(got[name], want[name], err_msg=name)
    for name in want["new"]:
        np.testing.assert_array_equal(got["new"][name], want["new"][name], err_msg=name)
    for name in ("loss", "loss_b", "gSc", "gac"):                    # the same floors; gSu's sum is deeper by the bank's empty ranges
        np.testing.assert_array_equal(got["floor"][name], want["floor"][name], err_msg=name)
    assert (got["floor"]["gSu"] >= want["floor"]["gSu"]).all()


# ---- refusals decided on the host ----
def _bank_struct(L, S=0x80000, a=0x81000, corr=None, key=None, state=0x82000, capacity=64, kp=16):
    b = L.ItemBank()
    b.S, b.a, b.corr, b.key, b.state, b.capacity, b.kp = S, a, corr, key, state, capacity, kp
    return b


BANK_CASES = [("S", dict(S=None), "ARG", "bank->S"), ("a", dict(a=None), "ARG", "bank->a"), ("state", dict(state=None), "ARG", "bank->state"),
              ("capacity 0", dict(capacity=0), "ARG", "capacity = 0"), ("capacity -1", dict(capacity=-1), "ARG", "capacity = -1"),
              ("kp", dict(kp=8), "SHAPE", "bank->kp = 8"), ("S unaligned", dict(S=0x80004), "ALIGN", "bank->S"),
              ("bank corr alone", dict(corr=0x83000), "ARG", "corr"), ("bank key alone", dict(key=0x84000), "ARG", "key"),
              ("capacity too large", dict(capacity=(1 << 20) + 1), "UNSUPPORTED", "at most 1048576")]


@pytest.mark.parametrize("who", ["fmx_fm_inbatch_bank_forward", "fmx_fm_inbatch_bank_backward"])
def test_side_calls_refuse_on_the_host(who):
    fmx, L, lib = _lib()
    codes = dict(ARG=L.ERR_ARG, SHAPE=L.ERR_SHAPE, ALIGN=L.ERR_ALIGN, UNSUPPORTED=L.ERR_UNSUPPORTED)

    def call(bank, B=4, kp=16, corr=None, key=None, lse_bytes=1 << 40, Su=0x40000):
        bp = None if bank is None else C.byref(bank)
        if who.endswith("forward"):
            return lib.fmx_fm_inbatch_bank_forward(Su, 16, 0x41000, 0x42000, 16, 0x43000, B, kp, corr, key, bp, 1.0, 0x50000, lse_bytes, 0x60000,
                                                   None, None, None)
        return lib.fmx_fm_inbatch_bank_backward(Su, 16, 0x41000, 0x42000, 16, 0x43000, B, kp, corr, key, bp, 1.0, 0x50000, lse_bytes, 0x60000,
                                                0x61000, 0x62000, None)
    cases = [(what, dict(bank=_bank_struct(L, **kw)), code, word) for what, kw, code, word in BANK_CASES]
    cases += [("null bank", dict(bank=None), "ARG", "bank is null"),
              ("call corr alone", dict(bank=_bank_struct(L), corr=0x70000), "ARG", "corr"),
              ("call key alone", dict(bank=_bank_struct(L), key=0x70000), "ARG", "key"),
              ("what the plain call refuses: Su", dict(bank=_bank_struct(L), Su=None), "ARG", "Su"),
              ("what the plain call refuses: B", dict(bank=_bank_struct(L), B=0), "ARG", "B = 0"),
              ("the plain call's lse block is too small", dict(bank=_bank_struct(L), lse_bytes=lib.fmx_fm_inbatch_lse_bytes(4, 16)), "SHAPE",
               "fmx_fm_inbatch_bank_lse_bytes"),
              ("one byte short", dict(bank=_bank_struct(L), lse_bytes=lib.fmx_fm_inbatch_bank_lse_bytes(4, 64, 16) - 1), "SHAPE",
               "fmx_fm_inbatch_bank_lse_bytes")]
    for what, kw, code, word in cases:
        rc = call(**kw)
        msg = lib.fmx_last_error_string().decode()
        assert rc == codes[code], (who, what, rc, msg)
        assert who in msg and word in msg, (who, what, msg)


@pytest.mark.parametrize("who", ["fmx_fm_inbatch_bank_push", "fmx_fm_inbatch_bank_step", "fmx_fm_inbatch_bank_stream"])
def test_pushing_calls_refuse_on_the_host(who):
    fmx, L, lib = _lib()
    codes = dict(ARG=L.ERR_ARG, SHAPE=L.ERR_SHAPE, ALIGN=L.ERR_ALIGN, UNSUPPORTED=L.ERR_UNSUPPORTED)
    t, h = _fake_table(L.LAYOUT_WEIGHTS), fmx.Hyper(lr=0.01)
    fields = (C.c_int32 * 1)(1)

    def call(bank, B=4, corr=None, key=None, ws_bytes=1 << 40, table=t, n_steps=0):
        bp = None if bank is None else C.byref(bank)
        if who.endswith("push"):
            return lib.fmx_fm_inbatch_bank_push(bp, 0x42000, 16, 0x43000, None, corr, key, B, None)
        tp = None if table is None else C.byref(table)
        if who.endswith("step"):
            return lib.fmx_fm_inbatch_bank_step(tp, h.ref(), L.RULE_SIGNADAM, 0x60000, None, fields, 1, corr, key, bp, B, 1.0, 0x50000, ws_bytes,
                                                None, None, None)
        return lib.fmx_fm_inbatch_bank_stream(tp, h.ref(), L.RULE_SIGNADAM, 0x60000, fields, 1, corr, key, bp, 1, B, 1.0, n_steps, 0x50000,
                                              ws_bytes, None, None, None)
    cases = [(what, dict(bank=_bank_struct(L, **kw)), code, word) for what, kw, code, word in BANK_CASES
             if not (who.endswith("push") and what == "kp")]              # (the push has no kp but the bank's)
    cases += [("null bank", dict(bank=None), "ARG", "bank is null"),
              ("call corr alone", dict(bank=_bank_struct(L), corr=0x70000), "ARG", "corr"),
              ("a step keyed against an unkeyed bank", dict(bank=_bank_struct(L), key=0x70000), "ARG", "key"),
              ("B > capacity", dict(bank=_bank_struct(L, capacity=3)), "UNSUPPORTED", "B = 4 rows do not fit a bank of 3 slots"),
              ("what the plain call refuses: B", dict(bank=_bank_struct(L), B=0), "ARG", "B = 0")]
    if not who.endswith("push"):
        need = lib.fmx_fm_inbatch_bank_workspace_bytes(C.byref(t), 4, 64, 1)
        cases += [("null table", dict(bank=_bank_struct(L), table=None), "ARG", "table"),
                  ("the plain step's workspace is too small", dict(bank=_bank_struct(L), ws_bytes=lib.fmx_fm_inbatch_workspace_bytes(C.byref(t), 4, 1)),
                   "SHAPE", "fmx_fm_inbatch_bank_workspace_bytes"),
                  ("one byte short", dict(bank=_bank_struct(L), ws_bytes=need - 1), "SHAPE", "fmx_fm_inbatch_bank_workspace_bytes")]
    for what, kw, code, word in cases:
        rc = call(**kw)
        msg = lib.fmx_last_error_string().decode()
        assert rc == codes[code], (who, what, rc, msg)
        assert who in msg and word in msg, (who, what, msg)
    if who.endswith("stream"):                                             # n_steps = 0: everything checked, nothing launched
        assert call(_bank_struct(L), ws_bytes=need) == L.OK
        assert call(_bank_struct(L, capacity=4), ws_bytes=lib.fmx_fm_inbatch_bank_workspace_bytes(C.byref(t), 4, 4, 1)) == L.OK


# ---- fmx/pairwise.py and the classes, on CPU ----
def test_item_bank_and_item_keys():
    from fmx.pairwise import ItemBank, item_keys
    fmx, L, lib = _lib()
    bank = ItemBank(130, 16, "cpu")
    assert bank.keyed and bank.corrected and bank.capacity == 130 and bank.kp == 16
    assert bank.S.shape == (130, 16) and bank.a.shape == (130,) and bank.corr.shape == (130,) and bank.key.dtype == torch.int32
    assert bank.state.dtype == torch.int32 and bank.state.tolist() == [0, 0] and bank.count() == 0 and bank.head() == 0
    c = bank.c_struct()._obj
    assert (c.S, c.a, c.corr, c.key, c.state) == tuple(t.data_ptr() for t in (bank.S, bank.a, bank.corr, bank.key, bank.state))
    assert (c.capacity, c.kp) == (130, 16)
    bank.state.copy_(torch.tensor([7, 9], dtype=torch.int32))
    assert bank.count() == 9 and bank.head() == 7
    bank.clear()
    assert bank.state.tolist() == [0, 0]
    free = ItemBank(1, 4, "cpu", keyed=False, corrected=False)
    assert not free.keyed and not free.corrected and free.c_struct()._obj.corr is None and free.c_struct()._obj.key is None
    for bad in (dict(capacity=0, kp=16), dict(capacity=-4, kp=16), dict(capacity=L.ITEM_BANK_MAX + 1, kp=16), dict(capacity=8, kp=12),
                dict(capacity=8, kp=3)):
        with pytest.raises(ValueError, match="capacity" if bad["kp"] == 16 else "kp"):
            ItemBank(device="cpu", **bad)
    # keys that hold across batches: the same item has the same key in another batch, other items another
    sizes = [7, 5, 11, 3]
    a = torch.tensor([[0, 4, 2, 1], [1, 4, 2, 0], [2, 3, 10, 2]], dtype=torch.int32)
    b = torch.tensor([[6, 0, 10, 2], [5, 1, 2, 1]], dtype=torch.int32)
    ka, kb = item_keys(a, [2, 3], sizes), item_keys(b, [2, 3], sizes)
    assert ka.dtype == torch.int32 and ka.tolist() == [2 * 3 + 1, 2 * 3 + 0, 10 * 3 + 2] and kb.tolist() == [32, 7]
    assert item_keys(a, 2, sizes).tolist() == [2, 2, 10]
    with pytest.raises(ValueError, match="int32"):
        item_keys(a, [2, 3], [7, 5, 1 << 20, 1 << 20])
    with pytest.raises(ValueError):
        item_keys(a, [4], sizes)


@pytest.mark.parametrize("cls", ["DeepFMAdam", "NFMAdam", "DeepFMOnn", "NFMOnn", "AFMAdam"])
def test_classes_that_refuse_the_bank(cls):
    from fmx.pairwise import ItemBank
    mod = {"DeepFMAdam": "deepfm_adam", "NFMAdam": "nfm_adam", "DeepFMOnn": "deepfm_onn", "NFMOnn": "nfm_onn", "AFMAdam": "afm_adam"}[cls]
    klass = getattr(importlib.import_module("models.models_online_deep." + mod), cls)
    obj = object.__new__(klass)             # (no GPU: the constructors raise; the refusal needs no state)
    for kw in (dict(), dict(bank=ItemBank(8, 4, "cpu", corrected=False))):
        with pytest.raises(NotImplementedError, match="pure FM logit") as ei:
            klass.fit_in_batch_bank(obj, [[0, 0]], [[1.0, 1.0]], [1], **kw)
        assert cls in str(ei.value) and "fit_in_batch_bank" in str(ei.value)


def test_fit_in_batch_bank_refusals_and_signature():
    from fmx.pairwise import ItemBank
    from models.models_online_deep.fm_adam import FMAdam
    params = inspect.signature(FMAdam.fit_in_batch_bank).parameters
    assert list(params)[1:] == ["Xi", "Xv", "item_fields", "log_q", "mask_duplicates", "candidates", "bank"]
    assert params["bank"].default is None and params["mask_duplicates"].default is True and params["log_q"].default is None
    import fmx
    assert list(inspect.signature(fmx.FMEngine.inbatch_bank_step).parameters)[1:] == ["hyper", "rule", "idx_d", "item_fields", "bank", "xv_d",
                                                                                    "corr", "key", "inv_b"]
    assert callable(fmx.FMEngine.inbatch_bank_stream)

    class Stub(FMAdam):                     # the checks on the bank come before anything touches a device
        _name, _logit_family = "FMAdam", "fm"

        def __init__(self):
            self._table = type("T", (), dict(kp=16))()

        def train(self):
            return self
    m = Stub()
    rows, x = [[0, 0]], [[1.0, 1.0]]
    with pytest.raises(ValueError, match="mask_duplicates"):
        m.fit_in_batch_bank(rows, x, [1], bank=ItemBank(8, 16, "cpu", keyed=False, corrected=False))
    with pytest.raises(ValueError, match="mask_duplicates"):
        m.fit_in_batch_bank(rows, x, [1], mask_duplicates=False, bank=ItemBank(8, 16, "cpu", keyed=True, corrected=False))
    with pytest.raises(ValueError, match="log_q"):
        m.fit_in_batch_bank(rows, x, [1], bank=ItemBank(8, 16, "cpu", keyed=True, corrected=True))
    with pytest.raises(ValueError, match="log_q"):
        m.fit_in_batch_bank(rows, x, [1], log_q=[0.0], bank=ItemBank(8, 16, "cpu", keyed=True, corrected=False))
    with pytest.raises(ValueError, match="kp"):
        m.fit_in_batch_bank(rows, x, [1], bank=ItemBank(8, 4, "cpu", keyed=True, corrected=False))
    with pytest.raises(ValueError, match="ItemBank"):
        m.fit_in_batch_bank(rows, x, [1], bank=object())
