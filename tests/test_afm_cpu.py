"""The attentional FM without a GPU: the class module imports and refuses to run, the C ABI is declared and exported, and the
float64 restatement the GPU tests compare against reduces to the plain FM in its uniform-attention limit."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from afm_f64 import afm_f64, fm_second_order_f64  # noqa: E402

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
