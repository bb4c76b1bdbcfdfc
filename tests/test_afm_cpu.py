"""The attentional FM without a GPU: the class module imports and refuses to run, the C ABI is declared and exported, and the
float64 restatement the GPU tests compare against reduces to the plain FM in its uniform-attention limit, evaluates by sample
chunks without changing its values or floors, and states the double-sigmoid loss."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from afm_f64 import afm_f64, fm_second_order_f64, live_params, pairs, tiles  # noqa: E402

AFM_SYMBOLS = ["fmx_afm_forward", "fmx_afm_workspace_bytes", "fmx_afm_step", "fmx_fm_update_occ"]


def test_afm_module_imports():
    from models.models_online_deep.afm_adam import AFMAdam
    from fmx.afm import AFMEngine, afm_param_count
    assert AFMAdam._name == "AFMAdam" and AFMEngine is not None
    assert afm_param_count(16, 4) == 4 * 16 + 2 * 4 + 16


def test_afm_refuses_to_run_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from models.models_online_deep.afm_adam import AFMAdam
    with pytest.raises(RuntimeError, match="gfx950"):
        AFMAdam([3, 4, 5], embedding_size=4, attention_size=4)


def test_afm_abi_declared_and_exported():
    import fmx
    header = open(os.path.join(ROOT, "include", "fmx.h")).read()
    for name in AFM_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/fmx.h"
        assert name in fmx._lib.EXPORTS
    assert "typedef struct fmx_afm" in header
    lib = fmx._lib.load()
    for name in AFM_SYMBOLS:
        assert getattr(lib, name) is not None
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", fmx._lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    defined = set(re.findall(r"\bT\s+(fmx_\w+)", out))
    assert set(AFM_SYMBOLS) <= defined, set(AFM_SYMBOLS) - defined
    assert lib.fmx_afm_workspace_bytes.restype.__name__ == "c_long"


def test_afm_workspace_bytes_refuses_bad_shapes_on_the_host():
    import ctypes as C
    import fmx
    lib = fmx._lib.load()
    offs = np.array([0, 3, 7], dtype=np.int64)
    t = fmx._lib.Table()
    t.rows, t.field_offsets, t.bias = 16, offs.ctypes.data, 16           # host-only arithmetic: the pointers are never read
    t.n_rows, t.n_fields, t.k, t.kp, t.row_stride, t.layout, t.max_field_rows = 7, 2, 4, 4, 8, 0, 4
    ok = fmx._lib.Afm(16, 4, 4)
    assert lib.fmx_afm_workspace_bytes(C.byref(t), C.byref(ok), 64) > 0
    assert lib.fmx_afm_workspace_bytes(C.byref(t), C.byref(fmx._lib.Afm(16, 4, 65)), 64) == fmx._lib.ERR_UNSUPPORTED
    assert lib.fmx_afm_workspace_bytes(C.byref(t), C.byref(fmx._lib.Afm(16, 4, 0)), 64) == fmx._lib.ERR_UNSUPPORTED
    assert lib.fmx_afm_workspace_bytes(C.byref(t), C.byref(fmx._lib.Afm(16, 8, 4)), 64) == fmx._lib.ERR_SHAPE
    t.n_fields = 1
    assert lib.fmx_afm_workspace_bytes(C.byref(t), C.byref(ok), 64) == fmx._lib.ERR_UNSUPPORTED


@pytest.mark.parametrize("F,k,t", [(2, 4, 1), (5, 3, 4), (13, 8, 16)])
def test_f64_restatement_reduces_to_fm(F, k, t):
    """h = 0 makes every score 0 and every a_ij = 1/P; with p = P (1, ..., 1) the attention term is sum_ij <e_i, e_j>: the
    FM second-order term."""
    rng = np.random.default_rng(F)
    R, B = 50, 9
    V, w = rng.normal(size=(R, k)), rng.normal(size=R)
    rows = rng.integers(0, R, size=(B, F))
    xv = rng.uniform(0.5, 1.5, size=(B, F))
    P = F * (F - 1) // 2
    params = np.concatenate([rng.normal(size=t * k), rng.normal(size=t), np.zeros(t), np.full(k, float(P))])
    r = afm_f64(V, w, 0.7, params, k, t, rows, xv)
    fm = 0.7 + (w[rows] * xv).sum(1) + fm_second_order_f64(V, rows, xv)
    np.testing.assert_allclose(r["logit"], fm, rtol=1e-12, atol=1e-12)


def test_pair_tiles_follow_the_kernel():
    """tiles() restates fmx_afm.hip next_tile: whole pair rows, at most 64 pairs, covering the P pairs in order."""
    assert tiles(2) == [(0, 1)]
    assert tiles(12) == [(0, 63), (63, 3)]
    assert len(tiles(39)) == 16
    for F in range(2, 65):
        tl = tiles(F)
        assert sum(n for _, n in tl) == F * (F - 1) // 2
        assert all(0 < n <= 64 for _, n in tl) and all(pb == sum(n for _, n in tl[:i]) for i, (pb, _) in enumerate(tl))
    assert len(tiles(64)) > 32 and tiles(64)[0] == (0, 63)      # k_afm's largest carve: one pair row per tile at first


def _problem(F, k, t, B, seed):
    rng = np.random.default_rng(seed)
    R = 40
    V, w = rng.normal(size=(R, k)) * 0.5, rng.normal(size=R) * 0.3
    rows = rng.integers(0, R, size=(B, F))
    xv = rng.uniform(0.2, 1.8, size=(B, F))
    xv[:, ::4] = 0.0
    valid = rng.uniform(size=(B, F)) > 0.05
    params = rng.normal(size=t * k + 2 * t + k) * 0.5
    y = (rng.uniform(size=B) < 0.4).astype(np.float64)
    return V, w, params, rows, xv, y, valid


@pytest.mark.parametrize("loss", ["logits", "sigmoid"])
def test_f64_chunks_agree_with_the_whole_batch(loss):
    """Chunks of 1, 4 and 7 samples (one a ragged tail) give the whole batch's values and gradients to 1e-12 and the same
    floors -- these depend on B and the grid, not on the chunk."""
    F, k, t, B = 13, 5, 6, 23
    V, w, params, rows, xv, y, valid = _problem(F, k, t, B, 3)
    params = live_params(params, V, k, t, rows, xv * valid)
    ref = afm_f64(V, w, -0.3, params, k, t, rows, xv, y, valid=valid, loss=loss, grid=8)
    for chunk in (1, 4, 7):
        got = afm_f64(V, w, -0.3, params, k, t, rows, xv, y, valid=valid, loss=loss, grid=8, chunk=chunk)
        assert set(got) == set(ref)
        for key in ref:
            a, b = np.asarray(got[key], np.float64), np.asarray(ref[key], np.float64)
            assert a.shape == b.shape, key
            np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-12 * max(1.0, float(np.max(np.abs(b)))), err_msg=key)
    assert ref["unit_live"].all() and ref["pair_live"].any()


def test_f64_sigmoid_loss_is_the_double_sigmoid():
    """loss='sigmoid': the per-sample BCE with logits of sigmoid(logit) and dlogit = (sigmoid(p) - y) p (1 - p) / B,
    p = sigmoid(logit) (FMX_LOSS_BCE_SIGMOID)."""
    F, k, t, B = 6, 4, 3, 17
    V, w, params, rows, xv, y, _ = _problem(F, k, t, B, 4)
    r = afm_f64(V, w, 0.4, params, k, t, rows, xv, y, loss="sigmoid")
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))
    pp = sig(r["logit"])
    want = -(y * np.log(sig(pp)) + (1 - y) * np.log(1 - sig(pp)))
    np.testing.assert_allclose(r["loss_b"], want, rtol=1e-12)
    np.testing.assert_allclose(r["dz"], (sig(pp) - y) * pp * (1 - pp) / B, rtol=1e-12, atol=1e-15)
    assert abs(r["loss"] - want.mean()) <= 1e-12 * want.mean()
    logits = afm_f64(V, w, 0.4, params, k, t, rows, xv, y)
    np.testing.assert_array_equal(logits["logit"], r["logit"])


def test_f64_floors_take_relu_kinks_and_dlogit_noise():
    """A unit with W_u = 0, b_u = 0 sits on its kink for every pair: its whole dL/dz term goes into the floors (db_u's is
    sum |dlogit a (r - att) h_u|); dz_abs adds dz_abs inv_b per sample to the bias floor.  With neither, the floors are
    the relative ones."""
    F, k, t, B = 7, 4, 3, 11
    V, w, params, rows, xv, y, _ = _problem(F, k, t, B, 5)
    params = live_params(params, V, k, t, rows, xv).astype(np.float64)
    base = afm_f64(V, w, 0.1, params, k, t, rows, xv, y)
    assert base["kinks"] == 0
    noisy = afm_f64(V, w, 0.1, params, k, t, rows, xv, y, dz_abs=2.0 ** -23)
    assert abs(noisy["fl_dbias"] - base["fl_dbias"] - 2.0 ** -23) <= 1e-12 * 2.0 ** -23
    assert (noisy["fl_dV"] >= base["fl_dV"]).all() and (noisy["fl_dparams"] > base["fl_dparams"]).any()
    u = 1
    params[u * k:(u + 1) * k] = 0.0
    params[t * k + u] = 0.0
    r = afm_f64(V, w, 0.1, params, k, t, rows, xv, y)
    P = F * (F - 1) // 2
    assert r["kinks"] == B * P
    import torch
    I, J = pairs(F)
    e = V[rows] * xv[..., None]
    q = e[:, I] * e[:, J]
    h = params[t * k + t:t * k + 2 * t]
    s = np.maximum(q @ params[:t * k].reshape(t, k).T + params[t * k:t * k + t], 0) @ h
    a = torch.softmax(torch.as_tensor(s), 1).numpy()
    rr = q @ params[t * k + 2 * t:]
    att = (a * rr).sum(1, keepdims=True)
    whole = float(np.sum(np.abs(r["dz"][:, None] * a * (rr - att) * h[u])))
    assert r["fl_dparams"][t * k + u] >= whole > 0
