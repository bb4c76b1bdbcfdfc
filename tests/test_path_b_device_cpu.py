"""CPU-side checks of the `device=` surface of FM_FTRL and RRF_Online and of their grid() classmethods: the host twin of a
grid pins the order in which the settings draw their parameters (what the device grid must reproduce), explicit
device="host" is today's default bit for bit, and include/fmx.h / libfmx.so carry the four entry points.  Also the slabs a grid
launch packs its settings' parameters into (models/models_online/_device.py) and the host loops' progress lines."""
import itertools
import os
import random
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def seed_all(s):
    torch.manual_seed(s)
    np.random.seed(s)
    random.seed(s)


def fm_ftrl():
    from models.models_online.FM_FTRL import FM_FTRL
    return FM_FTRL


def rrf():
    from models.models_online.RRF_Online import RRF_Online
    return RRF_Online


def stream(n, D, seed, task):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, D)) / np.sqrt(D)
    s = X @ rng.standard_normal(D) + 0.5 * X[:, 0] * X[:, 1] * D
    y = np.where(s >= 0, 1.0, -1.0) if task == "cls" else s
    return torch.DoubleTensor(X), torch.DoubleTensor(y)


@pytest.mark.parametrize("task", ["cls", "reg"])
def test_fm_ftrl_device_keyword(task, capsys):
    X, y = stream(60, 8, 1, task)
    with pytest.raises(ValueError):
        fm_ftrl()(X, y, task, 0.01, 4, device="tpu")
    torch.manual_seed(3)
    a = fm_ftrl()(X, y, task, 0.01, 4)
    pa, ra, _ = a.online_learning()
    torch.manual_seed(3)
    b = fm_ftrl()(X, y, task, 0.01, 4, device="host")
    pb, rb, _ = b.online_learning()
    capsys.readouterr()
    assert a.device == "host" and b.device == "host"
    np.testing.assert_array_equal(pa, pb)
    np.testing.assert_array_equal(ra, rb)
    assert torch.equal(a.w1, b.w1) and torch.equal(a.W2, b.W2)


@pytest.mark.parametrize("task", ["cls", "reg"])
def test_rrf_device_keyword(task, capsys):
    X, y = stream(60, 8, 2, task)
    with pytest.raises(ValueError):
        rrf()(X, y, task, device="tpu")
    seed_all(4)
    a = rrf()(X, y, task, num_sampled_spectral=5)
    pa, ra, _ = a.online_learning()
    seed_all(4)
    b = rrf()(X, y, task, None, None, None, 5, 100, 0.05, 0.05, "host")       # device: appended after the existing keywords
    pb, rb, _ = b.online_learning()
    capsys.readouterr()
    assert a.device == "host" and b.device == "host"
    np.testing.assert_array_equal(pa, pb)
    np.testing.assert_array_equal(ra, rb)
    assert torch.equal(a.w, b.w) and torch.equal(a.gamma, b.gamma) and torch.equal(a.eps, b.eps)


@pytest.mark.parametrize("task", ["cls", "reg"])
def test_fm_ftrl_host_grid_equals_single_runs_in_product_order(task, golden_dir, capsys):
    z = np.load(os.path.join(golden_dir, "FM_FTRL.npz"))
    X, y = torch.DoubleTensor(z[f"{task}/X"]), torch.DoubleTensor(z[f"{task}/y"])
    lrs, ms = [0.005, 0.02], [8, 3, 1]
    torch.manual_seed(5)
    res = fm_ftrl().grid(X, y, task, lrs, ms, device="host")
    assert len(res) == 6
    torch.manual_seed(5)
    for (mdl, pred), (lr, m) in zip(res, itertools.product(lrs, ms)):
        one = fm_ftrl()(X, y, task, lr, m)
        p1, _, _ = one.online_learning()
        assert (mdl.eta, mdl.m) == (lr, m)
        np.testing.assert_array_equal(pred, p1)
        assert torch.equal(mdl.w1, one.w1) and torch.equal(mdl.W2, one.W2)
    capsys.readouterr()
    # the first setting is the fixture's own (seed 5, eta 0.005, m 8: tests/test_host_logic.py)
    mdl, pred = res[0]
    assert pred.shape == ((256, 1) if task == "cls" else (256, 1, 1))
    np.testing.assert_allclose(pred.reshape(-1), z[f"{task}/pred"], rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(mdl.w1.numpy(), z[f"{task}/w1"], rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(mdl.W2.numpy(), z[f"{task}/W2"], rtol=1e-10, atol=1e-13)


@pytest.mark.parametrize("task", ["cls", "reg"])
def test_rrf_host_grid_equals_single_runs_in_product_order(task, golden_dir, capsys):
    z = np.load(os.path.join(golden_dir, "path_b_family.npz"))
    X, y = torch.DoubleTensor(z[f"{task}/X"][:100]), torch.DoubleTensor(z[f"{task}/y"][:100])
    lws, lgs, dss = [0.05, 0.01], [0.05], [6, 3]
    seed_all(17)
    res = rrf().grid(X, y, task, lws, lgs, dss, device="host")
    assert len(res) == 4
    seed_all(17)
    for (mdl, pred), (lw, lg, ds) in zip(res, itertools.product(lws, lgs, dss)):
        one = rrf()(X, y, task, num_sampled_spectral=ds, lr_RRF_w=lw, lr_RRF_gamma=lg)
        p1, _, _ = one.online_learning()
        assert (mdl.lr_RRF_w, mdl.lr_RRF_gamma, mdl.num_sampled_spectral) == (lw, lg, ds)
        np.testing.assert_array_equal(pred, p1)
        assert torch.equal(mdl.w, one.w) and torch.equal(mdl.gamma, one.gamma) and torch.equal(mdl.eps, one.eps)
    capsys.readouterr()
    # the first setting is the fixture's own (seed 17, the default rates, 6 spectral samples: tests/test_host_logic.py)
    mdl, pred = res[0]
    assert tuple(pred.shape) == tuple(z[f"{task}/RRF/pred_shape"])
    np.testing.assert_allclose(pred, z[f"{task}/RRF/pred"].reshape(pred.shape), rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(mdl.w.numpy(), z[f"{task}/RRF/w"], rtol=1e-8, atol=1e-11)
    np.testing.assert_allclose(mdl.gamma.numpy(), z[f"{task}/RRF/gamma"], rtol=1e-8, atol=1e-11)


def test_empty_grids_and_bad_arguments():
    X, y = stream(10, 8, 3, "reg")
    for device in ("host", "gpu"):                       # nothing to run: no library, no device needed
        assert fm_ftrl().grid(X, y, "reg", [], [4], device=device) == []
        assert fm_ftrl().grid(X, y, "reg", [0.1], [], device=device) == []
        assert rrf().grid(X, y, "reg", [0.05], [], [6], device=device) == []
    with pytest.raises(ValueError):
        fm_ftrl().grid(X, y, "reg", [0.1], [4], device="tpu")
    with pytest.raises(ValueError):
        rrf().grid(X, y, "reg", [0.05], [0.05], [6], device="tpu")
    with pytest.raises(NotImplementedError):
        fm_ftrl().grid(X, y, "rank", [0.1], [4], device="host")
    with pytest.raises(NotImplementedError):             # hinge / l1 are refused before anything runs
        rrf().grid(X, y, "reg", [0.05], [0.05], [6], loss_type="l1", device="host")


def test_slab_round_trip():
    """Tensors of 3, 8 and 1 elements -> one zero-filled [3, 8] slab -> equal tensors that own their memory."""
    from models.models_online import _device
    rng = np.random.default_rng(0)
    tensors = [torch.from_numpy(rng.standard_normal(shape)) for shape in ((3,), (2, 4), (1, 1))]
    slab = _device.pack_slab(tensors)
    assert slab.shape == (3, 8) and slab.dtype == torch.float64 and slab.is_contiguous()
    for s, t in enumerate(tensors):
        assert torch.equal(slab[s, :t.numel()], t.reshape(-1))
        assert bool((slab[s, t.numel():] == 0.0).all())
    back = _device.unpack_slab(slab, [t.shape for t in tensors])
    assert len(back) == 3
    for t, b in zip(tensors, back):
        assert b.shape == t.shape and b.dtype == torch.float64 and torch.equal(b, t)
    before = slab.clone()
    for b in back:
        b.fill_(7.0)
    assert torch.equal(slab, before)


def progress_lines(out):
    """the ' <idx> th : pred <p> , real <r> ' lines of an online_learning() run -> [(idx, pred text, real text)]"""
    return [(int(i), p, r) for i, p, r in re.findall(r"^ (\d+) th : pred (\S+) , real (\S+) $", out, flags=re.M)]


@pytest.mark.parametrize("task", ["cls", "reg"])
@pytest.mark.parametrize("name", ["FM_FTRL", "RRF_Online", "SFTRL_CCFM", "SFTRL_Vanila"])
def test_host_progress_lines_every_1000th_sample(name, task, capsys):
    """2,001 samples: the smallest stream on which the lines of samples 0, 1000 and 2000 all appear (the host twin of the device
    tests' test_progress_lines_equal_on_both_devices)."""
    from models.models_online.SFTRL_CCFM import SFTRL_CCFM
    from models.models_online.SFTRL_Vanila import SFTRL_Vanila
    X, y = stream(2001, 8, 7, task)
    seed_all(9)
    if name == "RRF_Online":
        m = rrf()(X, y, task, num_sampled_spectral=6)
    else:
        m = dict(FM_FTRL=fm_ftrl(), SFTRL_CCFM=SFTRL_CCFM, SFTRL_Vanila=SFTRL_Vanila)[name](X, y, task, 0.005 if name == "FM_FTRL" else 0.05, 4)
    m.online_learning()
    out = capsys.readouterr().out
    lines = progress_lines(out)
    assert out.count(" th : pred ") == 3 and [i for i, _, _ in lines] == [0, 1000, 2000]
    assert [float(r) for _, _, r in lines] == [float("%f" % y[i]) for i in (0, 1000, 2000)]
    if task == "cls":
        assert all(p in ("1.000000", "-1.000000") for _, p, _ in lines)


NEW_ENTRY_POINTS = ("fmx_ftrl_dense_run", "fmx_ftrl_dense_grid", "fmx_rrf_run", "fmx_rrf_grid")


def test_header_declares_and_library_exports_the_entry_points():
    import fmx
    header = open(os.path.join(ROOT, "include", "fmx.h")).read()
    declared = set(re.findall(r"\bint\s+(fmx_[a-z_0-9]+)\s*\(", header))
    for name in NEW_ENTRY_POINTS:
        assert name in declared, name
        assert name in fmx._lib.EXPORTS, name
    if not os.path.exists(fmx._lib.LIB_PATH):
        return
    lib = fmx._lib.load()
    for name in NEW_ENTRY_POINTS:
        assert getattr(lib, name) is not None and len(getattr(lib, name).argtypes) > 0
    assert len(lib.fmx_ftrl_dense_run.argtypes) == 14 and len(lib.fmx_ftrl_dense_grid.argtypes) == 16
    assert len(lib.fmx_rrf_run.argtypes) == 14 and len(lib.fmx_rrf_grid.argtypes) == 16


def test_argument_checks_come_before_any_launch():
    """Host arithmetic only: every refusal below returns before a HIP call, so it runs without a device."""
    import ctypes as C
    import fmx
    if not os.path.exists(fmx._lib.LIB_PATH):
        return
    lib = fmx._lib.load()
    buf = (C.c_double * 16)()
    p = C.cast(buf, C.c_void_p)
    msg = lambda: lib.fmx_last_error_string().decode()
    assert lib.fmx_ftrl_dense_run(p, p, 4, 65, 4, 0.1, 0, p, p, p, p, p, p, None) == -5 and "features <= 64" in msg()
    assert lib.fmx_ftrl_dense_run(p, p, 4, 8, 130, 0.1, 0, p, p, p, p, p, p, None) == -5 and "2 m <= 128" in msg()
    assert lib.fmx_ftrl_dense_run(p, p, 4, 8, 5, 0.1, 0, p, p, p, p, p, p, None) == -1          # odd 2 m
    assert lib.fmx_ftrl_dense_run(p, p, 4, 8, 4, 0.1, 2, p, p, p, p, p, p, None) == -1          # task
    assert lib.fmx_ftrl_dense_run(p, p, 4, 8, 4, 0.1, 0, p, None, p, p, p, p, None) == -1       # null W2
    assert lib.fmx_ftrl_dense_run(p, p, -1, 8, 4, 0.1, 0, p, p, p, p, p, p, None) == -1
    assert lib.fmx_ftrl_dense_run(p, p, 0, 8, 4, 0.1, 0, p, p, p, p, p, p, None) == 0           # N = 0: nothing to do
    assert lib.fmx_ftrl_dense_grid(p, p, 4, 8, 2, p, p, 130, 0, p, p, p, p, p, p, None) == -5 and "2 m <= 128" in msg()
    assert lib.fmx_ftrl_dense_grid(p, p, 4, 8, 0, p, p, 4, 0, p, p, p, p, p, p, None) == 0
    assert lib.fmx_ftrl_dense_grid(p, p, 4, 8, -1, p, p, 4, 0, p, p, p, p, p, p, None) == -1
    assert lib.fmx_rrf_run(p, p, 4, 8, 65, 0.05, 0.05, 0, p, p, p, p, p, None) == -5 and "spectral samples <= 64" in msg()
    assert lib.fmx_rrf_run(p, p, 4, 65, 6, 0.05, 0.05, 0, p, p, p, p, p, None) == -5 and "features <= 64" in msg()
    assert lib.fmx_rrf_run(p, p, 4, 8, 6, 0.05, 0.05, 2, p, p, p, p, p, None) == -1 and "not implemented" in msg()
    assert lib.fmx_rrf_run(p, p, 4, 8, 6, 0.05, 0.05, 0, None, p, p, p, p, None) == -1
    assert lib.fmx_rrf_run(p, p, 0, 8, 6, 0.05, 0.05, 0, p, p, p, p, p, None) == 0
    assert lib.fmx_rrf_grid(p, p, 4, 8, 3, p, p, p, 65, 0, p, p, p, p, p, None) == -5
    assert lib.fmx_rrf_grid(p, p, 0, 8, 3, p, p, p, 6, 0, p, p, p, p, p, None) == 0
    assert lib.fmx_rrf_grid(p, p, 4, 8, 3, None, p, p, 6, 0, p, p, p, p, p, None) == -1
