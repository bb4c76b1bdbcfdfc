"""CPU-only tests of fmx_fm_topk's host side: the workspace size and the argument checks, which return their codes before
any HIP call (no GPU needed: the pointers below are never dereferenced)."""
import ctypes as C

import pytest

import fmx

A = 1 << 20   # a 16-byte-aligned stand-in address


def lib():
    return fmx._lib.load()


def call(U=4, N=100, K=10, kp=16, ld_u=16, ld_c=16, Su=A, Sc=A, ws=A, ws_bytes=None, au=A, ac=A, off=None, pos=None,
         tp=A, ts=A):
    L = lib()
    if ws_bytes is None:
        ws_bytes = max(int(L.fmx_fm_topk_workspace_bytes(U, N, K)), 0)
    return L.fmx_fm_topk(Su, ld_u, au, U, Sc, ld_c, ac, N, kp, off, pos, K, ws, ws_bytes, tp, ts, None)


def test_workspace_bytes_is_int64_and_monotone():
    L = lib()
    assert L.fmx_fm_topk_workspace_bytes.restype is C.c_int64
    assert "fmx_fm_topk_workspace_bytes" in fmx._lib.I64_RETURNS
    big = int(L.fmx_fm_topk_workspace_bytes(1 << 20, 1 << 30, 256))
    assert big > 2 ** 31                      # would truncate in a 32-bit return
    Us = [1, 2, 7, 16, 17, 63, 64, 65, 255, 256, 300, 1000, 1024, 1025, 2048, 4096, 4097, 20000, 100000]
    Ns = [1, 9, 10, 255, 256, 1000, 2048, 2049, 4097, 176373, 262144, 1 << 20, 1 << 24]
    Ks = [1, 2, 10, 99, 100, 128, 129, 255, 256]
    for N in Ns:
        for K in Ks:
            row = [int(L.fmx_fm_topk_workspace_bytes(U, N, K)) for U in Us]
            assert all(b > 0 for b in row) and row == sorted(row), (N, K, row)
    for U in Us:
        for K in Ks:
            col = [int(L.fmx_fm_topk_workspace_bytes(U, N, K)) for N in Ns]
            assert col == sorted(col), (U, K, col)
        for N in Ns:
            ks = [int(L.fmx_fm_topk_workspace_bytes(U, N, K)) for K in Ks]
            assert ks == sorted(ks), (U, N, ks)


def test_workspace_bytes_rejects_bad_sizes():
    L = lib()
    assert L.fmx_fm_topk_workspace_bytes(0, 10, 10) == fmx._lib.ERR_ARG
    assert L.fmx_fm_topk_workspace_bytes(10, 0, 10) == fmx._lib.ERR_ARG
    assert L.fmx_fm_topk_workspace_bytes(10, 10, 0) == fmx._lib.ERR_ARG
    assert L.fmx_fm_topk_workspace_bytes(10, 10, 257) == fmx._lib.ERR_UNSUPPORTED


@pytest.mark.parametrize("kw, code", [
    (dict(K=0), fmx._lib.ERR_ARG),
    (dict(K=-3), fmx._lib.ERR_ARG),
    (dict(K=257, ws_bytes=1 << 30), fmx._lib.ERR_UNSUPPORTED),
    (dict(U=0, ws_bytes=1 << 30), fmx._lib.ERR_ARG),
    (dict(N=0, ws_bytes=1 << 30), fmx._lib.ERR_ARG),
    (dict(kp=12, ld_u=12, ld_c=12), fmx._lib.ERR_SHAPE),
    (dict(kp=128, ld_u=128, ld_c=128), fmx._lib.ERR_SHAPE),
    (dict(ld_u=8), fmx._lib.ERR_SHAPE),
    (dict(ld_c=18), fmx._lib.ERR_SHAPE),
    (dict(Su=A + 4), fmx._lib.ERR_ALIGN),
    (dict(Sc=A + 8), fmx._lib.ERR_ALIGN),
    (dict(ws=A + 12), fmx._lib.ERR_ALIGN),
    (dict(Su=None), fmx._lib.ERR_ARG),
    (dict(ac=None), fmx._lib.ERR_ARG),
    (dict(ws=None), fmx._lib.ERR_ARG),
    (dict(tp=None), fmx._lib.ERR_ARG),
    (dict(off=A), fmx._lib.ERR_ARG),           # offsets without positions
    (dict(pos=A), fmx._lib.ERR_ARG),
])
def test_argument_checks_return_their_codes(kw, code):
    assert call(**kw) == code
    assert lib().fmx_last_error_string().decode().startswith("fmx_fm_topk")


def test_short_workspace_is_a_shape_error():
    for U, N, K in ((1, 1, 1), (7, 1000, 10), (300, 176373, 256), (4096, 1 << 20, 100)):
        need = int(lib().fmx_fm_topk_workspace_bytes(U, N, K))
        assert call(U=U, N=N, K=K, ws_bytes=need - 1) == fmx._lib.ERR_SHAPE
        assert call(U=U, N=N, K=K, ws_bytes=0) == fmx._lib.ERR_SHAPE
