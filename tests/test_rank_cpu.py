"""CPU-only tests of the rank calls' host side (include/fmx.h, fmx_fm_rank / fmx_mlp_rank / fmx_afm_rank): the symbols, the
workspace sizes, the argument checks -- refused before any launch, so the pointers below are never dereferenced --, and the
pure-Python parts of fmx.recommend (targets_matrix, ranking_metrics)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import fmx
from fmx import recommend as rec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 1 << 20   # a 16-byte-aligned stand-in address
L = fmx._lib
NAMES = ["fmx_fm_rank", "fmx_mlp_rank", "fmx_afm_rank"]


def lib():
    return L.load()


def mlp(k=10, hidden=16, layers=3, params=A):
    return L.Mlp(params, layers, k, hidden, 0)


def afm(k=8, t=4, params=A):
    return L.Afm(params, k, t)


def test_symbols_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "fmx.h")).read()
    for name in NAMES:
        for n in (name, name + "_workspace_bytes"):
            assert re.search(r"\b%s\s*\(" % n, header), f"{n} is not declared in include/fmx.h"
            assert n in L.EXPORTS and getattr(lib(), n) is not None
        assert name + "_workspace_bytes" in L.I64_RETURNS
        assert getattr(lib(), name + "_workspace_bytes").restype is C.c_int64


def ws_fns():
    m, a = mlp(), afm()
    return [lambda U, N, T: int(lib().fmx_fm_rank_workspace_bytes(U, N, T)),
            lambda U, N, T: int(lib().fmx_mlp_rank_workspace_bytes(C.byref(m), U, N, T)),
            lambda U, N, T: int(lib().fmx_afm_rank_workspace_bytes(C.byref(a), 3, 1, U, N, T))]


def test_workspace_bytes_is_monotone_and_rejects_bad_sizes():
    Us = [1, 2, 7, 16, 17, 255, 256, 1000, 2048, 4097, 100000]
    Ns = [1, 63, 65, 255, 257, 2048, 2049, 176373, 1 << 20, 1 << 24]
    Ts = [1, 2, 15, 16]
    for f in ws_fns():
        for N in Ns:
            for T in Ts:
                row = [f(U, N, T) for U in Us]
                assert all(b > 0 for b in row) and row == sorted(row), (N, T, row)
        for U in Us:
            for T in Ts:
                col = [f(U, N, T) for N in Ns]
                assert col == sorted(col), (U, T, col)
            for N in Ns:
                ts = [f(U, N, T) for T in Ts]
                assert ts == sorted(ts), (U, N, ts)
        assert f(1 << 20, 1 << 30, 16) > 0
        assert f(-1, 10, 1) == L.ERR_ARG and f(0, 10, 1) == L.ERR_ARG
        assert f(10, -1, 1) == L.ERR_ARG and f(10, 0, 1) == L.ERR_ARG
        assert f(10, 10, 0) == L.ERR_ARG and f(10, 10, -2) == L.ERR_ARG
        assert f(10, 10, 17) == L.ERR_UNSUPPORTED


def fm_call(U=4, N=100, T=2, kp=16, ld_u=16, ld_c=16, Su=A, Sc=A, ws=A, ws_bytes=None, au=A, ac=A, off=None, pos=None, tg=A,
            ro=A, so=A, no=A, filtered=0):
    if ws_bytes is None:
        ws_bytes = max(int(lib().fmx_fm_rank_workspace_bytes(U, N, T)), 0)
    return lib().fmx_fm_rank(Su, ld_u, au, U, Sc, ld_c, ac, N, kp, off, pos, tg, T, filtered, ws, ws_bytes, ro, so, no, None)


def mlp_call(m=None, fm_term=1, U=4, N=100, T=2, kp=16, ld_u=16, ld_c=16, Su=A, Bu=A, Sc=A, Bc=A, ws=A, ws_bytes=None, au=A,
             ac=A, off=None, pos=None, tg=A, ro=A, so=A, no=A, filtered=0):
    m = mlp() if m is None else m
    if ws_bytes is None:
        ws_bytes = max(int(lib().fmx_mlp_rank_workspace_bytes(C.byref(m), U, N, T)), 0)
    return lib().fmx_mlp_rank(C.byref(m), fm_term, Su, Bu, ld_u, au, U, Sc, Bc, ld_c, ac, N, kp, off, pos, tg, T, filtered, ws,
                              ws_bytes, ro, so, no, None)


def afm_call(a=None, n_ctx=3, n_item=1, U=4, N=100, T=2, kp=8, Eu=A, su=A, Ec=A, sc=A, ws=A, ws_bytes=None, off=None, pos=None,
             tg=A, ro=A, so=A, no=A, filtered=0):
    a = afm() if a is None else a
    if ws_bytes is None:
        ws_bytes = max(int(lib().fmx_afm_rank_workspace_bytes(C.byref(a), n_ctx, n_item, U, N, T)), 0)
    return lib().fmx_afm_rank(C.byref(a), Eu, su, n_ctx, U, Ec, sc, n_item, N, kp, off, pos, tg, T, filtered, ws, ws_bytes, ro, so,
                              no, None)


BIG = 1 << 30
# the mistakes the top-K calls refuse, with the top-K calls' codes (tests/test_recommend_cpu.py, test_recommend_mlp_cpu.py)
COMMON = [
    (dict(T=0), L.ERR_ARG),
    (dict(T=17, ws_bytes=BIG), L.ERR_UNSUPPORTED),
    (dict(U=0, ws_bytes=BIG), L.ERR_ARG),
    (dict(N=0, ws_bytes=BIG), L.ERR_ARG),
    (dict(ws=A + 12), L.ERR_ALIGN),
    (dict(ws=None), L.ERR_ARG),
    (dict(tg=None), L.ERR_ARG),
    (dict(ro=None), L.ERR_ARG),
    (dict(off=A), L.ERR_ARG),
    (dict(pos=A), L.ERR_ARG),
    (dict(filtered=2), L.ERR_ARG),
]
SIDES = [
    (dict(ld_u=8), L.ERR_SHAPE),
    (dict(ld_c=18), L.ERR_SHAPE),
    (dict(Su=A + 4), L.ERR_ALIGN),
    (dict(Sc=A + 8), L.ERR_ALIGN),
    (dict(Su=None), L.ERR_ARG),
    (dict(ac=None), L.ERR_ARG),
]


@pytest.mark.parametrize("kw, code", COMMON + SIDES + [
    (dict(kp=12, ld_u=12, ld_c=12), L.ERR_SHAPE),
    (dict(kp=128, ld_u=128, ld_c=128), L.ERR_SHAPE),
])
def test_fm_rank_argument_checks(kw, code):
    assert fm_call(**kw) == code
    assert lib().fmx_last_error_string().decode().startswith("fmx_fm_rank")


@pytest.mark.parametrize("kw, code", COMMON + SIDES + [
    (dict(kp=12, ld_u=12, ld_c=12), L.ERR_UNSUPPORTED),
    (dict(Bu=None), L.ERR_ARG),
    (dict(Bc=A + 4), L.ERR_ALIGN),
    (dict(fm_term=2), L.ERR_ARG),
    (dict(m=mlp(hidden=257), ws_bytes=BIG), L.ERR_UNSUPPORTED),
    (dict(m=mlp(layers=9), ws_bytes=BIG), L.ERR_UNSUPPORTED),
    (dict(m=mlp(k=20), ws_bytes=BIG), L.ERR_UNSUPPORTED),          # k > kp
    (dict(m=mlp(params=None), ws_bytes=BIG), L.ERR_ARG),
])
def test_mlp_rank_argument_checks(kw, code):
    assert mlp_call(**kw) == code
    assert lib().fmx_last_error_string().decode().startswith("fmx_mlp_rank")


@pytest.mark.parametrize("kw, code", COMMON + [
    (dict(kp=12), L.ERR_SHAPE),
    (dict(kp=4), L.ERR_SHAPE),                                     # kp < k
    (dict(Eu=A + 4), L.ERR_ALIGN),
    (dict(sc=None), L.ERR_ARG),
    (dict(n_item=0, ws_bytes=BIG), L.ERR_SHAPE),
    (dict(n_ctx=60, n_item=5, ws_bytes=BIG), L.ERR_UNSUPPORTED),
    (dict(a=afm(t=65), ws_bytes=BIG), L.ERR_UNSUPPORTED),
])
def test_afm_rank_argument_checks(kw, code):
    assert afm_call(**kw) == code
    assert lib().fmx_last_error_string().decode().startswith("fmx_afm_rank")


def test_short_workspace_is_a_shape_error():
    m, a = mlp(), afm()
    for U, N, T in ((1, 1, 1), (7, 1000, 2), (300, 176373, 16), (4096, 1 << 20, 1)):
        for call, need in ((fm_call, lib().fmx_fm_rank_workspace_bytes(U, N, T)),
                           (mlp_call, lib().fmx_mlp_rank_workspace_bytes(C.byref(m), U, N, T)),
                           (afm_call, lib().fmx_afm_rank_workspace_bytes(C.byref(a), 3, 1, U, N, T))):
            assert call(U=U, N=N, T=T, ws_bytes=int(need) - 1) == L.ERR_SHAPE
            assert call(U=U, N=N, T=T, ws_bytes=0) == L.ERR_SHAPE


def test_targets_matrix_pads_chunks_and_checks_u():
    full, chunks = rec.targets_matrix([[3, 4], [], [7]], 3, "cpu")
    assert full.dtype == torch.int32 and full.tolist() == [[3, 4], [-1, -1], [7, -1]]
    assert len(chunks) == 1 and chunks[0].is_contiguous()
    full, chunks = rec.targets_matrix(np.arange(5), 5, "cpu")
    assert full.shape == (5, 1) and full[:, 0].tolist() == [0, 1, 2, 3, 4]
    full, chunks = rec.targets_matrix(torch.arange(2 * 35).reshape(2, 35), 2, "cpu")
    assert [c.shape[1] for c in chunks] == [16, 16, 3] and all(c.is_contiguous() for c in chunks)
    assert torch.equal(torch.cat(chunks, 1), full)
    for bad in ([[1], [2]], np.zeros((4, 2)), np.zeros((3, 2, 2))):
        with pytest.raises(ValueError):
            rec.targets_matrix(bad, 3, "cpu")


def test_ranking_metrics_by_hand():
    m = rec.ranking_metrics(torch.tensor([[0, 1, 9, 10, -1]]), torch.tensor([100]), ks=(1, 10))
    assert m["n"] == 4 and isinstance(m["n"], int) and all(isinstance(v, float) for k, v in m.items() if k != "n")
    assert m["hr@10"] == pytest.approx(3 / 4, abs=1e-12) and m["hr@1"] == pytest.approx(1 / 4, abs=1e-12)
    assert m["ndcg@10"] == pytest.approx((1 + 1 / math.log2(3) + 1 / math.log2(11)) / 4, abs=1e-12)
    assert m["mrr"] == pytest.approx((1 + 1 / 2 + 1 / 10 + 1 / 11) / 4, abs=1e-12)
    assert m["auc"] == pytest.approx((1 + (1 - 1 / 99) + (1 - 9 / 99) + (1 - 10 / 99)) / 4, abs=1e-12)


def test_ranking_metrics_auc_skips_single_candidate_users_and_survives_nothing_valid():
    m = rec.ranking_metrics(torch.tensor([[0], [3], [0]]), torch.tensor([1, 11, 0]))
    assert m["n"] == 3 and m["auc"] == pytest.approx(1 - 3 / 10, abs=1e-12)
    m = rec.ranking_metrics(torch.tensor([[-1, -1]]), torch.tensor([5]))
    assert m["n"] == 0 and all(math.isnan(v) for k, v in m.items() if k != "n")
    m = rec.ranking_metrics(np.array([2, 0]), np.array([10, 10]), ks=(1,))      # [U] ranks, numpy in
    assert m["hr@1"] == 0.5 and m["n"] == 2
