"""FM_FTRL and RRF_Online on the device (fmx_ftrl_dense_run / _grid, fmx_rrf_run / _grid; device="gpu" and Class.grid) against
the fixtures the imported reference produced (tests/golden/FM_FTRL.npz, path_b_family.npz) and against the host fp64 classes
on wider shapes.

Tolerances (figures: tools/path_b_times.py on an MI355X, recorded in profiles/path_b_times.json; each the largest deviation
relative to the largest magnitude of the compared array).  FM_FTRL: the project's number for fp64 reassociation on these streams,
rtol 1e-7 / atol 1e-9 (tests/test_sftrl_gpu.py); measured 7.4e-16 against the golden fixtures and 5.2e-16 against the host class at
D = 64, 2m = 128, far under the 1e-8 that would ask for an explanation.  RRF_Online: the device's exp / sin / cos are not the host
libm's bit for bit and the model's dynamics can amplify that, so cls is compared over the fixture's 100 steps only.  Measured
against the golden w and gamma and the host's y_hat: 5.7e-16 for cls over those 100 steps, 5.7e-16 for l2 over the fixture's 300;
the tolerance is 10 x that, 5.7e-15 (nine orders under the 1e-6 beyond which something other than last-place rounding would be
wrong).  The l2 step multiplies the residual by 1 - lr_w Ds, so the l2 cases keep lr_w Ds <= 0.8: beyond 2 the recurrence itself
diverges.  Every test prints its figures before it asserts."""
import ctypes as C
import itertools
import os
import random
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-7, 1e-9                      # FM_FTRL


RRF_TOL = {"cls": 10 * 5.7e-16, "reg": 10 * 5.7e-16}   # 10 x measured (module docstring), x max |reference|


def seed_all(s):
    torch.manual_seed(s)
    np.random.seed(s)
    random.seed(s)


def FM():
    from models.models_online.FM_FTRL import FM_FTRL
    return FM_FTRL


def RRF():
    from models.models_online.RRF_Online import RRF_Online
    return RRF_Online


def lib():
    import fmx
    return fmx._lib.load()


def dptr(t):
    return C.c_void_p(t.data_ptr())


def cur_stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def make_stream(n, D, seed, task):
    """as tests/test_sftrl_gpu.py's"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, D)) / np.sqrt(D)
    wt = rng.standard_normal(D)
    s = X @ wt + 0.5 * (X[:, 0] * X[:, 1] - X[:, min(2, D - 1)] * X[:, -1]) * D
    y = np.where(s >= 0, 1.0, -1.0) if task == "cls" else s
    return X, y


def rel_dev(got, ref):
    """largest deviation relative to the largest magnitude of the reference"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


def dense_run(X, y, m2, eta, task, w1, W2, g_w1, g_W2):
    """fmx_ftrl_dense_run on device tensors (state in place) -> raw y_hat [N] (numpy), status (numpy)"""
    n, D = X.shape
    pred = torch.full((max(n, 1),), 7.0, dtype=torch.float64, device="cuda")
    status = torch.zeros(2, dtype=torch.int32, device="cuda")
    rc = lib().fmx_ftrl_dense_run(dptr(X), dptr(y), n, D, m2, eta, 0 if task == "cls" else 1, dptr(w1), dptr(W2), dptr(g_w1), dptr(g_W2),
                                  dptr(pred), dptr(status), cur_stream())
    assert rc == 0, lib().fmx_last_error_string()
    torch.cuda.synchronize()
    return pred.cpu().numpy()[:n], status.cpu().numpy()


def rrf_run(X, y, Ds, lr_w, lr_g, loss, eps, gamma, w):
    n, D = X.shape
    pred = torch.full((max(n, 1),), 7.0, dtype=torch.float64, device="cuda")
    status = torch.zeros(2, dtype=torch.int32, device="cuda")
    rc = lib().fmx_rrf_run(dptr(X), dptr(y), n, D, Ds, lr_w, lr_g, loss, dptr(eps), dptr(gamma), dptr(w), dptr(pred), dptr(status), cur_stream())
    assert rc == 0, lib().fmx_last_error_string()
    torch.cuda.synchronize()
    return pred.cpu().numpy()[:n], status.cpu().numpy()


def assert_signs_agree(got_scalar, host_scalar, tol):
    """+-1 predictions must agree wherever the host's |y_hat| exceeds the scalar tolerance at that point"""
    decided = np.abs(host_scalar) > tol
    assert ((got_scalar >= 0) == (host_scalar >= 0))[decided].all()


# ---------------------------------------------------------------- against the golden fixtures

@pytest.mark.parametrize("task", ["cls", "reg"])
def test_fm_ftrl_gpu_vs_reference_fixture(task, golden_dir, capsys):
    z = np.load(os.path.join(golden_dir, "FM_FTRL.npz"))
    X, y = torch.DoubleTensor(z[f"{task}/X"]), torch.DoubleTensor(z[f"{task}/y"])
    torch.manual_seed(5)
    host = FM()(X, y, task, float(z[f"{task}/eta"]), int(z[f"{task}/m"]))
    host.online_learning()
    capsys.readouterr()
    torch.manual_seed(5)
    m = FM()(X, y, task, float(z[f"{task}/eta"]), int(z[f"{task}/m"]), device="gpu")
    pred, real, secs = m.online_learning()
    out = capsys.readouterr().out
    print(f"FM_FTRL {task} vs fixture: w1 {rel_dev(m.w1.numpy(), z[f'{task}/w1']):.3e} W2 {rel_dev(m.W2.numpy(), z[f'{task}/W2']):.3e} "
          f"y_hat vs host {rel_dev(m.y_hat, host.y_hat):.3e}")
    assert out.startswith("FM_FTRL_0.005_8_start\n 0 th : pred ") and "learning time : " in out
    assert out.count(" th : pred ") == 1
    assert pred.shape == ((256, 1) if task == "cls" else (256, 1, 1)) and real.shape == (256,)
    assert isinstance(secs, float) and m.model_name == "FM_FTRL" and m.eta == 0.005 and m.m == 8
    if task == "reg":
        np.testing.assert_allclose(pred.reshape(-1), z[f"{task}/pred"], rtol=RTOL, atol=ATOL)
    else:
        assert set(np.unique(pred)) <= {-1.0, 1.0}
        undecided = np.abs(host.y_hat) <= ATOL + RTOL * np.abs(host.y_hat)
        assert (pred.reshape(-1) == z[f"{task}/pred"])[~undecided].all()
    np.testing.assert_allclose(m.y_hat, host.y_hat, rtol=RTOL, atol=ATOL)
    np.testing.assert_array_equal(real, z[f"{task}/real"])
    np.testing.assert_allclose(m.w1.numpy(), z[f"{task}/w1"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(m.W2.numpy(), z[f"{task}/W2"], rtol=RTOL, atol=ATOL)
    assert m.w1.dtype == torch.float64 and tuple(m.W2.shape) == (16, 7) and tuple(m.w1.shape) == (8, 1)
    assert m.w1.device.type == "cpu" and m.W2.device.type == "cpu"


@pytest.mark.parametrize("task", ["cls", "reg"])
def test_rrf_gpu_vs_reference_fixture(task, golden_dir, capsys):
    z = np.load(os.path.join(golden_dir, "path_b_family.npz"))
    X, y = torch.DoubleTensor(z[f"{task}/X"][:100]), torch.DoubleTensor(z[f"{task}/y"][:100])
    seed_all(17)
    host = RRF()(X, y, task, num_sampled_spectral=6)
    host.online_learning()
    seed_all(17)
    m = RRF()(X, y, task, num_sampled_spectral=6, device="gpu")
    assert m.loss_type == ("logit" if task == "cls" else "l2")
    pred, real, secs = m.online_learning()
    out = capsys.readouterr().out
    tol = RRF_TOL[task]
    figures = dict(w=rel_dev(m.w.numpy(), z[f"{task}/RRF/w"]), gamma=rel_dev(m.gamma.numpy(), z[f"{task}/RRF/gamma"]),
                   y_hat_vs_host=rel_dev(m.y_hat, host.y_hat))
    if task == "reg":
        figures["pred"] = rel_dev(pred, z[f"{task}/RRF/pred"].reshape(pred.shape))
    print(f"RRF {task} vs fixture (100 steps): {figures}  tolerance {tol:.1e}")
    assert out.count("=" * 40) == 2 and " 0 th : pred " in out and "learning time : " in out      # (the host run's lines and this one's)
    assert tuple(pred.shape) == tuple(z[f"{task}/RRF/pred_shape"]) and isinstance(secs, float)
    np.testing.assert_array_equal(real, z[f"{task}/RRF/real"])
    if task == "cls":
        ref = z[f"{task}/RRF/pred"].reshape(pred.shape)
        undecided = (np.abs(host.y_hat) <= tol * np.abs(host.y_hat).max()).reshape(pred.shape)
        assert (pred == ref)[~undecided].all()
    for name, v in figures.items():
        assert v <= tol, (name, v)
    assert m.w.device.type == "cpu" and tuple(m.gamma.shape) == (8, 1) and tuple(m.w.shape) == (12,)


def test_rrf_reg_full_fixture_length_vs_host(golden_dir, capsys):
    """l2 over the fixture's full 300 samples, the host class as the reference"""
    z = np.load(os.path.join(golden_dir, "path_b_family.npz"))
    X, y = torch.DoubleTensor(z["reg/X"]), torch.DoubleTensor(z["reg/y"])
    seed_all(17)
    host = RRF()(X, y, "reg", num_sampled_spectral=6)
    ph, _, _ = host.online_learning()
    seed_all(17)
    m = RRF()(X, y, "reg", num_sampled_spectral=6, device="gpu")
    pg, _, _ = m.online_learning()
    capsys.readouterr()
    figures = dict(pred=rel_dev(pg, ph), w=rel_dev(m.w.numpy(), host.w.numpy()), gamma=rel_dev(m.gamma.numpy(), host.gamma.numpy()))
    tol = RRF_TOL["reg"]
    print(f"RRF reg vs host (300 steps): {figures}  tolerance {tol:.1e}")
    assert pg.shape == ph.shape == (300, 1)
    for name, v in figures.items():
        assert v <= tol, (name, v)


def progress_lines(out):
    """the ' <idx> th : pred <p> , real <r> ' lines of an online_learning() run -> [(idx, pred text, real text)]"""
    return [(int(i), p, r) for i, p, r in re.findall(r"^ (\d+) th : pred (\S+) , real (\S+) $", out, flags=re.M)]


@pytest.mark.parametrize("task", ["cls", "reg"])
@pytest.mark.parametrize("name", ["FM_FTRL", "RRF_Online"])
def test_progress_lines_equal_on_both_devices(name, task, capsys):
    """2,001 samples of 8 features, the smallest stream on which the lines of samples 0, 1000 and 2000 all appear: the device run
    prints what the host loop prints.  cls: the +-1 as text; reg: as numbers under the class's fixture tolerance (%f rounds to 1e-6, so
    scores equal to that tolerance can still differ in the last printed digit)."""
    X, y = make_stream(2001, 8, 7, task)
    Xt, yt = torch.DoubleTensor(X), torch.DoubleTensor(y)
    outs = {}
    for device in ("host", "gpu"):
        seed_all(9)
        m = (FM()(Xt, yt, task, 0.005, 8, device=device) if name == "FM_FTRL"
             else RRF()(Xt, yt, task, num_sampled_spectral=6, device=device))
        m.online_learning()
        outs[device] = capsys.readouterr().out
    h, g = progress_lines(outs["host"]), progress_lines(outs["gpu"])
    print(f"{name} {task} host {h}\n{name} {task} gpu  {g}")
    assert outs["host"].count("\n") == outs["gpu"].count("\n") and len(h) == len(g) == 3
    assert [i for i, _, _ in g] == [i for i, _, _ in h] == [0, 1000, 2000]
    assert [r for _, _, r in g] == [r for _, _, r in h]
    pg, ph = [p for _, p, _ in g], [p for _, p, _ in h]
    if task == "cls":
        assert pg == ph and set(pg) <= {"1.000000", "-1.000000"}
    elif name == "FM_FTRL":
        np.testing.assert_allclose(np.array(pg, dtype=np.float64), np.array(ph, dtype=np.float64), rtol=RTOL, atol=ATOL)
    else:
        assert rel_dev(np.array(pg, dtype=np.float64), np.array(ph, dtype=np.float64)) <= RRF_TOL[task]


# ---------------------------------------------------------------- against the host classes on wider shapes

def fm_initial(X, y, task, eta, m, seed):
    torch.manual_seed(seed)
    mdl = FM()(torch.DoubleTensor(X), torch.DoubleTensor(y), task, eta, m)
    mdl._init_parameter()
    return mdl.w1.reshape(-1).clone(), mdl.W2.clone()


@pytest.mark.parametrize("task,D,m", [("cls", 64, 1), ("reg", 64, 64), ("cls", 63, 20), ("reg", 33, 64), ("reg", 9, 5), ("cls", 2, 3),
                                       ("cls", 64, 64), ("reg", 8, 33)])
def test_fm_ftrl_gpu_equals_host_path(task, D, m, capsys):
    n, n1, eta, seed = 300, 180, 0.03, 11 + D + m
    X, y = make_stream(n, D, seed, task)
    Xt, yt = torch.DoubleTensor(X), torch.DoubleTensor(y)
    torch.manual_seed(seed)
    host = FM()(Xt, yt, task, eta, m)
    ph, _, _ = host.online_learning()
    torch.manual_seed(seed)
    gpu = FM()(Xt, yt, task, eta, m, device="gpu")
    pg, _, _ = gpu.online_learning()
    capsys.readouterr()
    print(f"FM_FTRL {task} D={D} 2m={2 * m}: y_hat {rel_dev(gpu.y_hat, host.y_hat):.3e} w1 {rel_dev(gpu.w1.numpy(), host.w1.numpy()):.3e} "
          f"W2 {rel_dev(gpu.W2.numpy(), host.W2.numpy()):.3e}")
    assert pg.shape == ph.shape
    np.testing.assert_allclose(gpu.y_hat, host.y_hat, rtol=RTOL, atol=ATOL)
    if task == "cls":
        assert_signs_agree(gpu.y_hat, host.y_hat, ATOL + RTOL * np.abs(host.y_hat))
        assert (pg.reshape(-1) == np.where(gpu.y_hat >= 0, 1.0, -1.0)).all()
    else:
        np.testing.assert_allclose(pg, ph, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(gpu.w1.numpy(), host.w1.numpy(), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(gpu.W2.numpy(), host.W2.numpy(), rtol=RTOL, atol=ATOL)
    # the C ABI: one uninterrupted run is the class's run; two legs that hand (w1, W2, g_w1, g_W2) on equal it bit for bit
    w1_0, W2_0 = fm_initial(X, y, task, eta, m, seed)
    Xd, yd = dev(X), dev(y)
    one = [w1_0.cuda(), W2_0.cuda().contiguous(), torch.zeros(D, dtype=torch.float64, device="cuda"),
           torch.zeros((2 * m, D - 1), dtype=torch.float64, device="cuda")]
    p_one, st = dense_run(Xd, yd, 2 * m, eta, task, *one)
    assert tuple(st) == (0, 0)
    np.testing.assert_array_equal(p_one, gpu.y_hat)
    assert torch.equal(one[0].cpu().reshape(-1, 1), gpu.w1) and torch.equal(one[1].cpu(), gpu.W2)
    two = [w1_0.cuda(), W2_0.cuda().contiguous(), torch.zeros(D, dtype=torch.float64, device="cuda"),
           torch.zeros((2 * m, D - 1), dtype=torch.float64, device="cuda")]
    p_a, _ = dense_run(Xd[:n1].contiguous(), yd[:n1].contiguous(), 2 * m, eta, task, *two)
    p_b, _ = dense_run(Xd[n1:].contiguous(), yd[n1:].contiguous(), 2 * m, eta, task, *two)
    np.testing.assert_array_equal(np.concatenate([p_a, p_b]), p_one)
    for a, b in zip(one, two):
        assert torch.equal(a, b)
    assert torch.equal(one[1], -eta * one[3])                    # W2 is the host's rounding of -eta * g_W2


@pytest.mark.parametrize("task,D,Ds", [("reg", 8, 1), ("reg", 40, 20), ("cls", 64, 64), ("cls", 8, 6), ("reg", 64, 64), ("cls", 17, 1)])
def test_rrf_gpu_equals_host_path(task, D, Ds, capsys):
    """The l2 step multiplies the residual by 1 - lr_w |phi|^2 = 1 - lr_w Ds: beyond lr_w Ds = 2 the recurrence itself diverges and
    turns a last-place difference into O(1) within some tens of steps, so nothing can be compared there.  The rate is therefore kept at lr_w Ds <= 0.8 for l2: 0.04 up to Ds = 20, 0.01 at Ds = 64."""
    n, n1, seed = 100, 60, 23 + D + Ds                            # (cls: no more than the 100 steps the fixture pins)
    lr_w = 0.01 if (task == "reg" and Ds > 20) else 0.04
    X, y = make_stream(n, D, seed, task)
    Xt, yt = torch.DoubleTensor(X), torch.DoubleTensor(y)
    seed_all(seed)
    host = RRF()(Xt, yt, task, num_sampled_spectral=Ds, lr_RRF_w=lr_w, lr_RRF_gamma=0.03)
    gamma0, w0, eps0 = host.gamma.reshape(-1).clone(), host.w.clone(), host.eps.clone()
    ph, _, _ = host.online_learning()
    seed_all(seed)
    gpu = RRF()(Xt, yt, task, num_sampled_spectral=Ds, lr_RRF_w=lr_w, lr_RRF_gamma=0.03, device="gpu")
    pg, _, _ = gpu.online_learning()
    capsys.readouterr()
    tol = RRF_TOL[task]
    figures = dict(y_hat=rel_dev(gpu.y_hat, host.y_hat), w=rel_dev(gpu.w.numpy(), host.w.numpy()),
                   gamma=rel_dev(gpu.gamma.numpy(), host.gamma.numpy()))
    print(f"RRF {task} D={D} Ds={Ds} vs host ({n} steps): {figures}  tolerance {tol:.1e}")
    assert pg.shape == ph.shape == (n, 1)
    for name, v in figures.items():
        assert v <= tol, (name, v)
    if task == "cls":
        assert_signs_agree(gpu.y_hat, host.y_hat, tol * np.abs(host.y_hat).max())
    # the C ABI: one run is the class's; two legs handing (gamma, w) on equal it bit for bit
    Xd, yd, eps = dev(X), dev(y), eps0.cuda().contiguous()
    loss = 0 if task == "cls" else 1
    one = [gamma0.cuda(), w0.cuda()]
    p_one, st = rrf_run(Xd, yd, Ds, lr_w, 0.03, loss, eps, *one)
    assert tuple(st) == (0, -1)
    np.testing.assert_array_equal(p_one, gpu.y_hat)
    assert torch.equal(one[0].cpu().reshape(-1, 1), gpu.gamma) and torch.equal(one[1].cpu(), gpu.w)
    two = [gamma0.cuda(), w0.cuda()]
    p_a, _ = rrf_run(Xd[:n1].contiguous(), yd[:n1].contiguous(), Ds, lr_w, 0.03, loss, eps, *two)
    p_b, _ = rrf_run(Xd[n1:].contiguous(), yd[n1:].contiguous(), Ds, lr_w, 0.03, loss, eps, *two)
    np.testing.assert_array_equal(np.concatenate([p_a, p_b]), p_one)
    assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1])
    assert torch.equal(eps.cpu(), eps0)                           # read only


# ---------------------------------------------------------------- grids

@pytest.mark.parametrize("task", ["cls", "reg"])
def test_fm_ftrl_grid_equals_single_runs(task, golden_dir, capsys):
    z = np.load(os.path.join(golden_dir, "FM_FTRL.npz"))
    X, y = torch.DoubleTensor(z[f"{task}/X"]), torch.DoubleTensor(z[f"{task}/y"])
    lrs, ms = [0.005, 0.02, 0.001], [8, 1, 64, 3]
    torch.manual_seed(5)
    res = FM().grid(X, y, task, lrs, ms)
    assert len(res) == 12
    torch.manual_seed(5)
    for (mdl, pred), (lr, m) in zip(res, itertools.product(lrs, ms)):
        one = FM()(X, y, task, lr, m, device="gpu")
        p1, _, _ = one.online_learning()
        assert (mdl.eta, mdl.m) == (lr, m)
        np.testing.assert_array_equal(pred, p1)
        np.testing.assert_array_equal(mdl.y_hat, one.y_hat)
        assert torch.equal(mdl.w1, one.w1) and torch.equal(mdl.W2, one.W2)
        assert mdl.W2.shape == (2 * m, 7) and mdl.w1.shape == (8, 1)
    capsys.readouterr()
    mdl, pred = res[0]                                            # the fixture's own setting
    np.testing.assert_allclose(mdl.w1.numpy(), z[f"{task}/w1"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(mdl.W2.numpy(), z[f"{task}/W2"], rtol=RTOL, atol=ATOL)
    if task == "reg":
        np.testing.assert_allclose(pred.reshape(-1), z[f"{task}/pred"], rtol=RTOL, atol=ATOL)


def test_rrf_grid_equals_single_runs_and_splits_beyond_256(golden_dir, capsys):
    z = np.load(os.path.join(golden_dir, "path_b_family.npz"))
    X, y = torch.DoubleTensor(z["reg/X"][:40]), torch.DoubleTensor(z["reg/y"][:40])
    lws, lgs, dss = [0.05, 0.01, 0.002], [0.05, 0.02, 0.004], list(range(1, 29)) + [64]
    seed_all(17)
    res = RRF().grid(X, y, "reg", lws, lgs, dss)
    assert len(res) == 261                                        # two launches: 256 + 5
    seed_all(17)
    for (mdl, pred), (lw, lg, ds) in zip(res, itertools.product(lws, lgs, dss)):
        one = RRF()(X, y, "reg", num_sampled_spectral=ds, lr_RRF_w=lw, lr_RRF_gamma=lg, device="gpu")
        p1, _, _ = one.online_learning()
        assert (mdl.lr_RRF_w, mdl.lr_RRF_gamma, mdl.num_sampled_spectral) == (lw, lg, ds)
        np.testing.assert_array_equal(pred, p1)
        assert torch.equal(mdl.w, one.w) and torch.equal(mdl.gamma, one.gamma) and torch.equal(mdl.eps, one.eps)
        assert mdl.w.shape == (2 * ds,) and mdl.gamma.shape == (8, 1)
    capsys.readouterr()


def test_rrf_cls_grid_equals_single_runs(golden_dir, capsys):
    z = np.load(os.path.join(golden_dir, "path_b_family.npz"))
    X, y = torch.DoubleTensor(z["cls/X"][:100]), torch.DoubleTensor(z["cls/y"][:100])
    seed_all(17)
    res = RRF().grid(X, y, "cls", [0.05, 0.01], [0.05], [6, 3, 11])
    seed_all(17)
    for (mdl, pred), (lw, lg, ds) in zip(res, itertools.product([0.05, 0.01], [0.05], [6, 3, 11])):
        one = RRF()(X, y, "cls", num_sampled_spectral=ds, lr_RRF_w=lw, lr_RRF_gamma=lg, device="gpu")
        p1, _, _ = one.online_learning()
        np.testing.assert_array_equal(pred, p1)
        np.testing.assert_array_equal(mdl.y_hat, one.y_hat)
        assert torch.equal(mdl.w, one.w) and torch.equal(mdl.gamma, one.gamma)
    capsys.readouterr()
    mdl, pred = res[0]                                            # the fixture's own setting
    tol = RRF_TOL["cls"]
    assert rel_dev(mdl.w.numpy(), z["cls/RRF/w"]) <= tol and rel_dev(mdl.gamma.numpy(), z["cls/RRF/gamma"]) <= tol


def test_grids_refuse_a_setting_beyond_the_launch():
    """A setting outside the range the launch is sized for (only a direct caller of the C ABI can pass one) is not run:
    status (2, value) -- (-2, value) from fmx_rrf_grid, whose status[0] >= 0 counts NaN samples --, its slabs and its neighbours' untouched by it."""
    n, D = 64, 8
    rng = np.random.default_rng(0)
    X, y = dev(rng.normal(size=(n, D)) / 3), dev(np.sign(rng.normal(size=n)))
    # FM_FTRL: m2_max = 8; settings 1, 3, 4 are too large, odd, too small
    m2s = torch.tensor([8, 10, 4, 5, 0], dtype=torch.int32, device="cuda")
    etas = torch.full((5,), 0.05, dtype=torch.float64, device="cuda")
    w1 = dev(rng.normal(size=(5, D)))
    W2 = dev(rng.normal(size=(5, 8 * (D - 1))))
    g_w1, g_W2 = torch.zeros_like(w1), torch.zeros_like(W2)
    w1_0, W2_0 = w1.clone(), W2.clone()
    pred = torch.full((5, n), 7.0, dtype=torch.float64, device="cuda")
    status = torch.zeros((5, 2), dtype=torch.int32, device="cuda")
    rc = lib().fmx_ftrl_dense_grid(dptr(X), dptr(y), n, D, 5, dptr(m2s), dptr(etas), 8, 0, dptr(w1), dptr(W2), dptr(g_w1), dptr(g_W2),
                                   dptr(pred), dptr(status), cur_stream())
    assert rc == 0, lib().fmx_last_error_string()
    torch.cuda.synchronize()
    st, pr = status.cpu().numpy(), pred.cpu().numpy()
    assert [tuple(r) for r in st] == [(0, 0), (2, 10), (0, 0), (2, 5), (2, 0)]
    for s in (1, 3, 4):
        assert (pr[s] == 7.0).all() and torch.equal(w1[s], w1_0[s]) and torch.equal(W2[s], W2_0[s])
        assert float(g_w1[s].abs().sum()) == 0.0 and float(g_W2[s].abs().sum()) == 0.0
    for s, m2 in ((0, 8), (2, 4)):                                # the neighbours equal their own single runs
        one = [w1_0[s].clone(), W2_0[s, :m2 * (D - 1)].clone(), torch.zeros(D, dtype=torch.float64, device="cuda"),
               torch.zeros(m2 * (D - 1), dtype=torch.float64, device="cuda")]
        p1, _ = dense_run(X, y, m2, 0.05, "cls", *one)
        np.testing.assert_array_equal(pr[s], p1)
        assert torch.equal(w1[s], one[0]) and torch.equal(W2[s, :m2 * (D - 1)], one[1]) and torch.equal(g_W2[s, :m2 * (D - 1)], one[3])
        assert torch.equal(W2[s, m2 * (D - 1):], W2_0[s, m2 * (D - 1):])
    # RRF: Ds_max = 4; settings 1 and 3 are out of range
    dss = torch.tensor([4, 5, 2, 0], dtype=torch.int32, device="cuda")
    lws = torch.full((4,), 0.05, dtype=torch.float64, device="cuda")
    lgs = torch.full((4,), 0.03, dtype=torch.float64, device="cuda")
    eps = dev(rng.normal(size=(4, D * 4)))
    gamma = dev(np.log(rng.uniform(0.1, 1.0, size=(4, D))))
    w = dev(0.1 * rng.normal(size=(4, 8)))
    gamma_0, w_0, eps_0 = gamma.clone(), w.clone(), eps.clone()
    pred = torch.full((4, n), 7.0, dtype=torch.float64, device="cuda")
    status = torch.full((4, 2), 9, dtype=torch.int32, device="cuda")
    rc = lib().fmx_rrf_grid(dptr(X), dptr(y), n, D, 4, dptr(dss), dptr(lws), dptr(lgs), 4, 0, dptr(eps), dptr(gamma), dptr(w), dptr(pred),
                            dptr(status), cur_stream())
    assert rc == 0, lib().fmx_last_error_string()
    torch.cuda.synchronize()
    st, pr = status.cpu().numpy(), pred.cpu().numpy()
    assert [tuple(r) for r in st] == [(0, -1), (-2, 5), (0, -1), (-2, 0)]      # negative: never a NaN count
    assert torch.equal(eps, eps_0)
    for s in (1, 3):
        assert (pr[s] == 7.0).all() and torch.equal(gamma[s], gamma_0[s]) and torch.equal(w[s], w_0[s])
    for s, ds in ((0, 4), (2, 2)):
        one = [gamma_0[s].clone(), w_0[s, :2 * ds].clone()]
        p1, _ = rrf_run(X, y, ds, 0.05, 0.03, 0, eps_0[s, :D * ds].clone(), *one)
        np.testing.assert_array_equal(pr[s], p1)
        assert torch.equal(gamma[s], one[0]) and torch.equal(w[s, :2 * ds], one[1]) and torch.equal(w[s, 2 * ds:], w_0[s, 2 * ds:])


# ---------------------------------------------------------------- limits and NaN

def test_limits_raise_and_name_the_limit():
    from fmx import _lib
    X, y = make_stream(10, 65, 1, "reg")
    with pytest.raises(_lib.FmxError, match="features <= 64"):
        FM()(torch.DoubleTensor(X), torch.DoubleTensor(y), "reg", 0.05, 4, device="gpu").online_learning()
    with pytest.raises(_lib.FmxError, match="features <= 64"):
        RRF()(torch.DoubleTensor(X), torch.DoubleTensor(y), "reg", num_sampled_spectral=4, device="gpu").online_learning()
    X, y = make_stream(10, 8, 1, "reg")
    with pytest.raises(_lib.FmxError, match="2 m <= 128"):
        FM()(torch.DoubleTensor(X), torch.DoubleTensor(y), "reg", 0.05, 65, device="gpu").online_learning()
    with pytest.raises(_lib.FmxError, match="spectral samples <= 64"):
        RRF()(torch.DoubleTensor(X), torch.DoubleTensor(y), "reg", num_sampled_spectral=65, device="gpu").online_learning()
    with pytest.raises(_lib.FmxError, match="2 m <= 128"):
        FM().grid(torch.DoubleTensor(X), torch.DoubleTensor(y), "reg", [0.05], [4, 65])
    with pytest.raises(_lib.FmxError, match="spectral samples <= 64"):
        RRF().grid(torch.DoubleTensor(X), torch.DoubleTensor(y), "reg", [0.05], [0.05], [4, 65])
    with pytest.raises(NotImplementedError):                      # refused before any launch, as on the host
        RRF()(torch.DoubleTensor(X), torch.DoubleTensor(y), "reg", loss_type="l1", device="gpu").online_learning()


def test_fm_ftrl_nan_row_raises(capsys):
    X, y = make_stream(20, 8, 1, "reg")
    X[7, 2] = np.nan
    with pytest.raises(ValueError, match="Nan contained"):
        FM()(torch.DoubleTensor(X), torch.DoubleTensor(y), "reg", 0.05, 4, device="gpu").online_learning()
    out = capsys.readouterr().out                                 # the host loop's lines up to the failing sample
    assert out.startswith("FM_FTRL_0.05_4_start\n 0 th : pred ") and "learning time" not in out
    # through the C ABI: status (1, 7), the state is the one in front of sample 7's update
    w1_0, W2_0 = fm_initial(X, y, "reg", 0.05, 4, 3)
    st8 = [w1_0.cuda(), W2_0.cuda().contiguous(), torch.zeros(8, dtype=torch.float64, device="cuda"),
           torch.zeros((8, 7), dtype=torch.float64, device="cuda")]
    p, st = dense_run(dev(X), dev(y), 8, 0.05, "reg", *st8)
    assert tuple(st) == (1, 7) and (p[8:] == 7.0).all() and not np.isnan(p[:7]).any()
    st7 = [w1_0.cuda(), W2_0.cuda().contiguous(), torch.zeros(8, dtype=torch.float64, device="cuda"),
           torch.zeros((8, 7), dtype=torch.float64, device="cuda")]
    p7, _ = dense_run(dev(X[:7]), dev(y[:7]), 8, 0.05, "reg", *st7)
    np.testing.assert_array_equal(p[:7], p7)
    for a, b in zip(st8, st7):
        assert torch.equal(a, b)


@pytest.mark.parametrize("task", ["cls", "reg"])
def test_rrf_nan_row_is_dropped(task, capsys):
    X, y = make_stream(60, 8, 2, task)
    X[9, 3] = np.nan
    X[30, 0] = np.nan
    Xt, yt = torch.DoubleTensor(X), torch.DoubleTensor(y)
    seed_all(6)
    host = RRF()(Xt, yt, task, num_sampled_spectral=5)
    gamma0, w0, eps0 = host.gamma.reshape(-1).clone(), host.w.clone(), host.eps.clone()
    ph, rh, _ = host.online_learning()
    seed_all(6)
    gpu = RRF()(Xt, yt, task, num_sampled_spectral=5, device="gpu")
    pg, rg, _ = gpu.online_learning()
    capsys.readouterr()
    assert pg.shape == ph.shape == (58, 1) and rg.shape == (58,)
    np.testing.assert_array_equal(rg, rh)
    assert np.isnan(gpu.y_hat[[9, 30]]).all() and not np.isnan(np.delete(gpu.y_hat, [9, 30])).any()
    tol = RRF_TOL[task]
    keep = ~np.isnan(host.y_hat)
    assert rel_dev(gpu.y_hat[keep], host.y_hat[keep]) <= tol                      # later samples are still processed
    assert rel_dev(gpu.w.numpy(), host.w.numpy()) <= tol and rel_dev(gpu.gamma.numpy(), host.gamma.numpy()) <= tol
    one = [gamma0.cuda(), w0.cuda()]
    _, st = rrf_run(dev(X), dev(y), 5, 0.05, 0.05, 0 if task == "cls" else 1, eps0.cuda().contiguous(), *one)
    assert tuple(st) == (2, 9)                                                    # two NaN samples, the first at 9


def test_empty_stream_launches_nothing():
    X, y = dev(np.zeros((1, 8))), dev(np.zeros(1))
    state = [torch.full((8,), 3.0, dtype=torch.float64, device="cuda"), torch.full((4, 7), 3.0, dtype=torch.float64, device="cuda"),
             torch.full((8,), 3.0, dtype=torch.float64, device="cuda"), torch.full((4, 7), 3.0, dtype=torch.float64, device="cuda")]
    pred = torch.full((4,), 7.0, dtype=torch.float64, device="cuda")
    status = torch.full((2,), 9, dtype=torch.int32, device="cuda")
    rc = lib().fmx_ftrl_dense_run(dptr(X), dptr(y), 0, 8, 4, 0.1, 0, *[dptr(t) for t in state], dptr(pred), dptr(status), cur_stream())
    assert rc == 0
    eps, gamma, w = (torch.full((8, 3), 3.0, dtype=torch.float64, device="cuda"), torch.full((8,), 3.0, dtype=torch.float64, device="cuda"),
                     torch.full((6,), 3.0, dtype=torch.float64, device="cuda"))
    rc = lib().fmx_rrf_run(dptr(X), dptr(y), 0, 8, 3, 0.05, 0.05, 0, dptr(eps), dptr(gamma), dptr(w), dptr(pred), dptr(status), cur_stream())
    assert rc == 0
    torch.cuda.synchronize()
    for t in state + [eps, gamma, w]:
        assert bool((t == 3.0).all())
    assert bool((pred == 7.0).all()) and bool((status == 9).all())
