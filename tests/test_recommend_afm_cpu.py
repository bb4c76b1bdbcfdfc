"""CPU-only tests of the AFM recommendation's host side (include/fmx.h, fmx_afm_side / fmx_afm_topk): the symbols, the
workspace size, and the argument checks, which return before any HIP call (the pointers below are never dereferenced)."""
import ctypes as C
import os
import re
import subprocess

import pytest

import fmx

A = 1 << 20   # a 16-byte-aligned stand-in address
E = fmx._lib
NEW = ("fmx_afm_side", "fmx_afm_topk_workspace_bytes", "fmx_afm_topk")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lib():
    return fmx._lib.load()


def afm(k=16, t=16, params=A):
    return fmx._lib.Afm(params, k, t)


def ws_bytes(a, n_ctx, n_item, U, N, K):
    return int(lib().fmx_afm_topk_workspace_bytes(C.byref(a), n_ctx, n_item, U, N, K))


def call(a=None, n_ctx=38, n_item=1, U=4, N=100, K=10, kp=16, Eu=A, su=A, Ec=A, sc=A, ws=A, ws_n=None, off=None, pos=None, tp=A,
         ts=A):
    a = afm() if a is None else a
    if ws_n is None:
        ws_n = max(ws_bytes(a, n_ctx, n_item, U, N, K), 0)
    return lib().fmx_afm_topk(C.byref(a), Eu, su, n_ctx, U, Ec, sc, n_item, N, kp, off, pos, K, ws, ws_n, tp, ts, None)


def test_symbols_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "fmx.h")).read()
    for name in NEW:
        assert re.fullmatch(r"fmx_[a-z_]+", name)
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in fmx._lib.EXPORTS
    out = subprocess.run(["nm", "-D", "--defined-only", fmx._lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NEW:
        assert name in exported, name
    assert lib().fmx_afm_topk_workspace_bytes.restype is C.c_int64
    assert "fmx_afm_topk_workspace_bytes" in fmx._lib.I64_RETURNS
    assert lib().fmx_version() == 104


def test_workspace_bytes_refuses_bad_arguments():
    assert ws_bytes(afm(t=65), 38, 1, 10, 10, 10) == E.ERR_UNSUPPORTED
    assert ws_bytes(afm(t=0), 38, 1, 10, 10, 10) == E.ERR_UNSUPPORTED
    assert ws_bytes(afm(k=65), 38, 1, 10, 10, 10) == E.ERR_UNSUPPORTED
    assert ws_bytes(afm(), 38, 1, 10, 10, 0) == E.ERR_ARG
    assert ws_bytes(afm(), 38, 1, 10, 10, 257) == E.ERR_UNSUPPORTED
    assert ws_bytes(afm(), 40, 25, 10, 10, 10) == E.ERR_UNSUPPORTED        # n_ctx + n_item > 64
    assert ws_bytes(afm(), 0, 1, 10, 10, 10) == E.ERR_SHAPE
    assert ws_bytes(afm(), 1, 0, 10, 10, 10) == E.ERR_SHAPE
    assert ws_bytes(afm(), 38, 1, 0, 10, 10) == E.ERR_ARG
    assert ws_bytes(afm(), 38, 1, 10, 0, 10) == E.ERR_ARG
    assert lib().fmx_afm_topk_workspace_bytes(None, 38, 1, 10, 10, 10) == E.ERR_ARG
    for a, nc, ni in ((afm(64, 64), 63, 1), (afm(1, 1), 1, 1), (afm(10, 4), 30, 34)):
        assert ws_bytes(a, nc, ni, 10, 10, 256) > 0


def test_workspace_bytes_is_monotone():
    assert ws_bytes(afm(16, 64), 1, 1, 1 << 20, 1 << 30, 256) > 2 ** 31
    Us = [1, 2, 7, 63, 64, 65, 255, 256, 300, 1024, 2047, 2048, 2049, 4096, 100000]
    Ns = [1, 63, 255, 256, 257, 1000, 2049, 4097, 176373, 1 << 20, 1 << 24]
    Ks = [1, 2, 10, 64, 100, 128, 129, 256]
    for a, nc, ni in ((afm(16, 16), 38, 1), (afm(4, 1), 1, 1), (afm(64, 64), 32, 32), (afm(10, 4), 11, 2)):
        for N in Ns:
            for K in Ks:
                row = [ws_bytes(a, nc, ni, U, N, K) for U in Us]
                assert all(b > 0 for b in row) and row == sorted(row), (N, K, row)
        for U in Us:
            for K in Ks:
                col = [ws_bytes(a, nc, ni, U, N, K) for N in Ns]
                assert col == sorted(col), (U, K, col)
            for N in Ns:
                ks = [ws_bytes(a, nc, ni, U, N, K) for K in Ks]
                assert ks == sorted(ks), (U, N, ks)


@pytest.mark.parametrize("kw, code", [
    (dict(K=0), E.ERR_ARG),
    (dict(K=257, ws_n=1 << 30), E.ERR_UNSUPPORTED),
    (dict(U=0, ws_n=1 << 30), E.ERR_ARG),
    (dict(N=0, ws_n=1 << 30), E.ERR_ARG),
    (dict(kp=12), E.ERR_SHAPE),
    (dict(kp=128), E.ERR_SHAPE),
    (dict(kp=8), E.ERR_SHAPE),                     # kp < k = 16
    (dict(a=afm(t=65), ws_n=1 << 30), E.ERR_UNSUPPORTED),
    (dict(a=afm(t=0), ws_n=1 << 30), E.ERR_UNSUPPORTED),
    (dict(n_ctx=0, ws_n=1 << 30), E.ERR_SHAPE),
    (dict(n_item=0, ws_n=1 << 30), E.ERR_SHAPE),
    (dict(n_ctx=60, n_item=5, ws_n=1 << 30), E.ERR_UNSUPPORTED),
    (dict(Eu=A + 4), E.ERR_ALIGN),
    (dict(su=A + 8), E.ERR_ALIGN),
    (dict(Ec=A + 12), E.ERR_ALIGN),
    (dict(sc=A + 4), E.ERR_ALIGN),
    (dict(ws=A + 8), E.ERR_ALIGN),
    (dict(a=afm(params=None)), E.ERR_ARG),
    (dict(Eu=None), E.ERR_ARG),
    (dict(su=None), E.ERR_ARG),
    (dict(Ec=None), E.ERR_ARG),
    (dict(sc=None), E.ERR_ARG),
    (dict(ws=None), E.ERR_ARG),
    (dict(tp=None), E.ERR_ARG),
    (dict(ts=None), E.ERR_ARG),
    (dict(off=A), E.ERR_ARG),
    (dict(pos=A), E.ERR_ARG),
])
def test_argument_checks_return_their_codes(kw, code):
    assert call(**kw) == code
    assert lib().fmx_last_error_string().decode().startswith("fmx_afm_topk")


def test_short_workspace_is_a_shape_error():
    for a, nc, ni in ((afm(16, 16), 38, 1), (afm(64, 64), 2, 3)):
        for U, N, K in ((1, 1, 1), (7, 1000, 10), (300, 176373, 256), (4096, 1 << 20, 100)):
            need = ws_bytes(a, nc, ni, U, N, K)
            assert call(a=a, n_ctx=nc, n_item=ni, U=U, N=N, K=K, kp=64 if a.k > 16 else 16, ws_n=need - 1) == E.ERR_SHAPE
            assert call(a=a, n_ctx=nc, n_item=ni, U=U, N=N, K=K, kp=64 if a.k > 16 else 16, ws_n=0) == E.ERR_SHAPE


def test_null_afm_is_an_argument_error():
    assert lib().fmx_afm_topk(None, A, A, 38, 4, A, A, 1, 100, 16, None, None, 10, A, 1 << 30, A, A, None) == E.ERR_ARG


def test_side_checks_its_arguments_before_any_launch():
    L = lib()
    table = fmx._lib.Table()          # a null table: refused first
    fields = (C.c_int32 * 2)(0, 1)
    h = fmx.Hyper(lr=0.01)
    assert L.fmx_afm_side(C.byref(table), C.byref(afm()), h.ref(), A, None, 4, fields, 2, 1, A, A, None, None) == E.ERR_ARG
    assert L.fmx_afm_side(None, C.byref(afm()), h.ref(), A, None, 4, fields, 2, 1, A, A, None, None) == E.ERR_ARG
