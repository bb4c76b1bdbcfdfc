"""CPU-only tests of fmx_mlp_topk's host side: the workspace size, the argument checks (returned before any HIP call: the
pointers below are never dereferenced), and recommend()'s default call on the network classes."""
import ctypes as C
import types

import numpy as np
import pytest

import fmx

A = 1 << 20   # a 16-byte-aligned stand-in address


def lib():
    return fmx._lib.load()


def mlp(k=10, hidden=10, n_layers=5, params=A):
    return fmx._lib.Mlp(params, n_layers, k, hidden, 0)


def ws_bytes(m, U, N, K):
    return int(lib().fmx_mlp_topk_workspace_bytes(C.byref(m), U, N, K))


def call(m=None, fm_term=1, U=4, N=100, K=10, kp=16, ld_u=16, ld_c=16, Su=A, Bu=A, Sc=A, Bc=A, au=A, ac=A, ws=A, ws_n=None,
         off=None, pos=None, tp=A, ts=A):
    m = mlp() if m is None else m
    if ws_n is None:
        ws_n = max(ws_bytes(m, U, N, K), 0)
    return lib().fmx_mlp_topk(C.byref(m), fm_term, Su, Bu, ld_u, au, U, Sc, Bc, ld_c, ac, N, kp, off, pos, K, ws, ws_n, tp, ts,
                              None)


def test_workspace_bytes_is_int64_and_monotone():
    L = lib()
    assert L.fmx_mlp_topk_workspace_bytes.restype is C.c_int64
    assert "fmx_mlp_topk_workspace_bytes" in fmx._lib.I64_RETURNS
    assert ws_bytes(mlp(16, 256, 3), 1 << 20, 1 << 30, 256) > 2 ** 31
    Us = [1, 2, 7, 63, 64, 65, 255, 256, 300, 1024, 2047, 2048, 2049, 4096, 100000]
    Ns = [1, 63, 64, 65, 255, 1000, 1664, 1665, 4097, 176373, 1 << 20, 1 << 24]
    Ks = [1, 2, 10, 64, 65, 100, 128, 129, 192, 193, 256]
    for net in (mlp(10, 10, 5), mlp(16, 256, 3), mlp(1, 1, 1), mlp(63, 33, 2), mlp(64, 64, 8)):
        for N in Ns:
            for K in Ks:
                row = [ws_bytes(net, U, N, K) for U in Us]
                assert all(b > 0 for b in row) and row == sorted(row), (N, K, row)
        for U in Us:
            for K in Ks:
                col = [ws_bytes(net, U, N, K) for N in Ns]
                assert col == sorted(col), (U, K, col)
            for N in Ns:
                ks = [ws_bytes(net, U, N, K) for K in Ks]
                assert ks == sorted(ks), (U, N, ks)


def test_workspace_holds_the_weights():
    # a bigger network needs more: the packed weight copy lives in the workspace
    assert ws_bytes(mlp(16, 256, 3), 1, 1, 1) >= 4 * (256 * 16 + 2 * 256 * 256 + 3 * 256)
    assert ws_bytes(mlp(16, 256, 3), 1, 1, 1) > ws_bytes(mlp(16, 128, 3), 1, 1, 1) > ws_bytes(mlp(10, 10, 5), 1, 1, 1)


def test_workspace_bytes_rejects_bad_sizes_and_networks():
    L = lib()
    E = fmx._lib
    assert ws_bytes(mlp(), 0, 10, 10) == E.ERR_ARG
    assert ws_bytes(mlp(), 10, 0, 10) == E.ERR_ARG
    assert ws_bytes(mlp(), 10, 10, 0) == E.ERR_ARG
    assert ws_bytes(mlp(), 10, 10, 257) == E.ERR_UNSUPPORTED
    assert ws_bytes(mlp(hidden=257), 10, 10, 10) == E.ERR_UNSUPPORTED
    assert ws_bytes(mlp(hidden=0), 10, 10, 10) == E.ERR_UNSUPPORTED
    assert ws_bytes(mlp(n_layers=9), 10, 10, 10) == E.ERR_UNSUPPORTED
    assert ws_bytes(mlp(n_layers=0), 10, 10, 10) == E.ERR_UNSUPPORTED
    assert ws_bytes(mlp(k=0), 10, 10, 10) == E.ERR_UNSUPPORTED
    assert ws_bytes(mlp(k=65), 10, 10, 10) == E.ERR_UNSUPPORTED
    assert L.fmx_mlp_topk_workspace_bytes(None, 10, 10, 10) == E.ERR_ARG
    for net in (mlp(hidden=256, n_layers=8), mlp(k=64, hidden=1, n_layers=1)):
        assert ws_bytes(net, 10, 10, 256) > 0


E = fmx._lib


@pytest.mark.parametrize("kw, code", [
    (dict(K=0), E.ERR_ARG),
    (dict(K=-3), E.ERR_ARG),
    (dict(K=257, ws_n=1 << 30), E.ERR_UNSUPPORTED),
    (dict(U=0, ws_n=1 << 30), E.ERR_ARG),
    (dict(N=0, ws_n=1 << 30), E.ERR_ARG),
    (dict(fm_term=2), E.ERR_ARG),
    (dict(fm_term=-1), E.ERR_ARG),
    (dict(m=mlp(hidden=257), ws_n=1 << 30), E.ERR_UNSUPPORTED),
    (dict(m=mlp(n_layers=9), ws_n=1 << 30), E.ERR_UNSUPPORTED),
    (dict(m=mlp(hidden=0), ws_n=1 << 30), E.ERR_UNSUPPORTED),
    (dict(m=mlp(n_layers=0), ws_n=1 << 30), E.ERR_UNSUPPORTED),
    (dict(m=mlp(k=17)), E.ERR_UNSUPPORTED),        # k > kp = 16
    (dict(kp=12, ld_u=12, ld_c=12), E.ERR_UNSUPPORTED),
    (dict(kp=128, ld_u=128, ld_c=128), E.ERR_UNSUPPORTED),
    (dict(ld_u=8), E.ERR_SHAPE),
    (dict(ld_c=18), E.ERR_SHAPE),
    (dict(ld_u=20, ld_c=21), E.ERR_SHAPE),
    (dict(Su=A + 4), E.ERR_ALIGN),
    (dict(Bu=A + 4), E.ERR_ALIGN),
    (dict(Sc=A + 8), E.ERR_ALIGN),
    (dict(Bc=A + 8), E.ERR_ALIGN),
    (dict(ws=A + 12), E.ERR_ALIGN),
    (dict(m=mlp(params=None)), E.ERR_ARG),
    (dict(Su=None), E.ERR_ARG),
    (dict(Bu=None), E.ERR_ARG),
    (dict(au=None), E.ERR_ARG),
    (dict(Sc=None), E.ERR_ARG),
    (dict(Bc=None), E.ERR_ARG),
    (dict(ac=None), E.ERR_ARG),
    (dict(ws=None), E.ERR_ARG),
    (dict(tp=None), E.ERR_ARG),
    (dict(ts=None), E.ERR_ARG),
    (dict(off=A), E.ERR_ARG),           # offsets without positions
    (dict(pos=A), E.ERR_ARG),
])
def test_argument_checks_return_their_codes(kw, code):
    assert call(**kw) == code
    assert lib().fmx_last_error_string().decode().startswith("fmx_mlp_topk")


def test_null_mlp_is_an_argument_error():
    L = lib()
    assert L.fmx_mlp_topk(None, 1, A, A, 16, A, 4, A, A, 16, A, 100, 16, None, None, 10, A, 1 << 30, A, A, None) == E.ERR_ARG


def test_short_workspace_is_a_shape_error():
    for net in (mlp(10, 10, 5), mlp(16, 256, 3)):
        for U, N, K in ((1, 1, 1), (7, 1000, 10), (300, 176373, 256), (4096, 1 << 20, 100)):
            need = ws_bytes(net, U, N, K)
            assert call(m=net, U=U, N=N, K=K, ws_n=need - 1) == E.ERR_SHAPE
            assert call(m=net, U=U, N=N, K=K, ws_n=0) == E.ERR_SHAPE


def test_kernel_limits_route_the_fallback():
    R = fmx.recommend
    assert R.mlp_kernel_takes((None, 10, 10, 5)) and R.mlp_kernel_takes((None, 16, 256, 3))
    assert not R.mlp_kernel_takes((None, 16, 257, 3)) and not R.mlp_kernel_takes((None, 16, 64, 9))


@pytest.mark.parametrize("cls", ["DeepFMAdam", "NFMAdam", "DeepFMOnn", "NFMOnn"])
def test_default_recommend_still_raises_on_network_classes(cls):
    import importlib
    mod = importlib.import_module("models.models_online_deep." + {"DeepFMAdam": "deepfm_adam", "NFMAdam": "nfm_adam",
                                                                   "DeepFMOnn": "deepfm_onn", "NFMOnn": "nfm_onn"}[cls])
    klass = getattr(mod, cls)
    fake = types.SimpleNamespace(_has_mlp=klass._has_mlp, _name=klass._name)   # constructing a model needs a GPU
    with pytest.raises(NotImplementedError, match="full=True"):
        klass.recommend(fake, np.zeros((1, 3), dtype=np.int64), None, [1], 5)
