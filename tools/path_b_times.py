"""FM_FTRL and RRF_Online on the device against their host classes: what a run deviates by and what it costs.
Writes profiles/path_b_times.json (or --out):
  deviation  largest deviation of a device run from the golden fixtures and from the host class (relative to the largest
             magnitude of the compared array), FM_FTRL cls / reg and RRF_Online cls (100 steps) / reg (100 and 300 steps);
  single     us per sample of ONE device run (the class call, copies included, and the launch alone by device events) against
             the host class on the same machine and stream: 8 features, a few thousand samples;
  grid       sample-updates/s of a 256-setting Class.grid(device="gpu") against the host running the same settings one after
             another (Class.grid(device="host")).
Every step runs in a child process of its own under a time limit; a step that fails or times out ends the run (nothing is
started on the device after a fault).  Needs the GPU: without one it fails."""
import argparse
import contextlib
import ctypes as C
import io
import json
import os
import random
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fm-for-online-recommendation_amd"))
GOLDEN = os.path.join(ROOT, "tests", "golden")
STEPS = (("deviation", 240), ("single", 240), ("grid", 420))      # name, time limit in seconds


def seed_all(s):
    torch.manual_seed(s)
    np.random.seed(s)
    random.seed(s)


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def rel_dev(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


def long_stream(n, task, seed=8, D=8):
    """the fixtures' shape (8 features, unit-scale rows) lengthened"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, D)) / np.sqrt(D)
    s = X @ rng.standard_normal(D) + X[:, 0] * X[:, 1] * D
    y = np.where(s >= 0, 1.0, -1.0) if task == "cls" else s
    return torch.DoubleTensor(X), torch.DoubleTensor(y)


def step_deviation():
    from models.models_online.FM_FTRL import FM_FTRL
    from models.models_online.RRF_Online import RRF_Online
    out = {}
    z = np.load(os.path.join(GOLDEN, "FM_FTRL.npz"))
    for task in ("cls", "reg"):
        X, y = torch.DoubleTensor(z[f"{task}/X"]), torch.DoubleTensor(z[f"{task}/y"])
        runs = {}
        for device in ("host", "gpu"):
            torch.manual_seed(5)
            m = FM_FTRL(X, y, task, float(z[f"{task}/eta"]), int(z[f"{task}/m"]), device=device)
            with quiet():
                m.online_learning()
            runs[device] = m
        g, h = runs["gpu"], runs["host"]
        r = dict(w1_vs_golden=rel_dev(g.w1.numpy(), z[f"{task}/w1"]), W2_vs_golden=rel_dev(g.W2.numpy(), z[f"{task}/W2"]),
                 y_hat_vs_host=rel_dev(g.y_hat, h.y_hat), w1_vs_host=rel_dev(g.w1.numpy(), h.w1.numpy()),
                 W2_vs_host=rel_dev(g.W2.numpy(), h.W2.numpy()),
                 y_hat_vs_host_elementwise=float(np.max(np.abs(g.y_hat - h.y_hat) / np.maximum(np.abs(h.y_hat), 1e-300))))
        if task == "reg":
            r["pred_vs_golden"] = rel_dev(g.y_hat, z[f"{task}/pred"])
        out[f"FM_FTRL/{task}/fixture_256"] = r
    for task, D, m in (("cls", 64, 64), ("reg", 64, 64), ("reg", 33, 20), ("cls", 9, 5)):
        rng = np.random.default_rng(D + m)
        Xn = rng.standard_normal((300, D)) / np.sqrt(D)
        s = Xn @ rng.standard_normal(D) + 0.5 * Xn[:, 0] * Xn[:, 1] * D
        X, y = torch.DoubleTensor(Xn), torch.DoubleTensor(np.where(s >= 0, 1.0, -1.0) if task == "cls" else s)
        runs = {}
        for device in ("host", "gpu"):
            torch.manual_seed(1)
            mdl = FM_FTRL(X, y, task, 0.03, m, device=device)
            with quiet():
                mdl.online_learning()
            runs[device] = mdl
        g, h = runs["gpu"], runs["host"]
        out[f"FM_FTRL/{task}/D{D}_2m{2 * m}_300"] = dict(y_hat_vs_host=rel_dev(g.y_hat, h.y_hat), w1_vs_host=rel_dev(g.w1.numpy(), h.w1.numpy()),
                                                         W2_vs_host=rel_dev(g.W2.numpy(), h.W2.numpy()))
    z = np.load(os.path.join(GOLDEN, "path_b_family.npz"))
    for task, n in (("cls", 100), ("reg", 100), ("reg", 300)):
        X, y = torch.DoubleTensor(z[f"{task}/X"][:n]), torch.DoubleTensor(z[f"{task}/y"][:n])
        runs = {}
        for device in ("host", "gpu"):
            seed_all(17)
            m = RRF_Online(X, y, task, num_sampled_spectral=6, device=device)
            with quiet():
                m.online_learning()
            runs[device] = m
        g, h = runs["gpu"], runs["host"]
        r = dict(y_hat_vs_host=rel_dev(g.y_hat, h.y_hat), w_vs_host=rel_dev(g.w.numpy(), h.w.numpy()),
                 gamma_vs_host=rel_dev(g.gamma.numpy(), h.gamma.numpy()))
        if n == 100:
            r.update(w_vs_golden=rel_dev(g.w.numpy(), z[f"{task}/RRF/w"]), gamma_vs_golden=rel_dev(g.gamma.numpy(), z[f"{task}/RRF/gamma"]))
            if task == "reg":
                r["pred_vs_golden"] = rel_dev(g.y_hat, z[f"{task}/RRF/pred"].reshape(-1))
        out[f"RRF_Online/{task}/fixture_{n}"] = r
    return out


def device_event_us(fn, repeats=5):
    """median device time of fn() in us, by events on the current stream (fn enqueues and does not synchronise)"""
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return float(np.median(times))


def step_single():
    from fmx import _lib
    from models.models_online.FM_FTRL import FM_FTRL
    from models.models_online.RRF_Online import RRF_Online
    lib = _lib.load()
    n, out = 4000, {}
    ptr = lambda t: C.c_void_p(t.data_ptr())
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for task in ("cls", "reg"):
        X, y = long_stream(n, task)
        Xd, yd = X.cuda().contiguous(), y.cuda().contiguous()
        pred, status = torch.empty(n, dtype=torch.float64, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
        # FM_FTRL, the fixture's setting (eta 0.005, m 8)
        wall = {}
        for device in ("host", "gpu", "gpu"):                     # (the second gpu run is the warm one)
            torch.manual_seed(5)
            m = FM_FTRL(X, y, task, 0.005, 8, device=device)
            with quiet():
                t0 = time.perf_counter()
                m.online_learning()
                wall[device] = (time.perf_counter() - t0) / n * 1e6
        w1, W2 = torch.randn(8, dtype=torch.float64).cuda(), torch.randn(16, 7, dtype=torch.float64).cuda()

        keep = []                                                  # the state of every launch, alive until the timing has synchronised

        def launch_fm():
            state = [w1.clone(), W2.clone(), torch.zeros_like(w1), torch.zeros_like(W2)]
            keep.append(state)
            _lib.check(lib.fmx_ftrl_dense_run(ptr(Xd), ptr(yd), n, 8, 16, 0.005, 0 if task == "cls" else 1, ptr(state[0]), ptr(state[1]),
                                              ptr(state[2]), ptr(state[3]), ptr(pred), ptr(status), st()))
        out[f"FM_FTRL/{task}"] = dict(samples=n, features=8, m=8, host_us_per_sample=wall["host"], device_class_us_per_sample=wall["gpu"],
                                      device_launch_us_per_sample=device_event_us(launch_fm) / n)
        # RRF_Online, the fixture's setting (6 spectral samples, the default rates)
        wall = {}
        for device in ("host", "gpu", "gpu"):
            seed_all(17)
            m = RRF_Online(X, y, task, num_sampled_spectral=6, device=device)
            with quiet():
                t0 = time.perf_counter()
                m.online_learning()
                wall[device] = (time.perf_counter() - t0) / n * 1e6
        eps, gamma, w = m.eps.cuda().contiguous(), torch.log(torch.rand(8, dtype=torch.float64)).cuda(), (0.1 * torch.randn(12, dtype=torch.float64)).cuda()

        def launch_rrf():
            state = [gamma.clone(), w.clone()]
            keep.append(state)
            _lib.check(lib.fmx_rrf_run(ptr(Xd), ptr(yd), n, 8, 6, 0.05, 0.05, 0 if task == "cls" else 1, ptr(eps), ptr(state[0]),
                                       ptr(state[1]), ptr(pred), ptr(status), st()))
        out[f"RRF_Online/{task}"] = dict(samples=n, features=8, spectral=6, host_us_per_sample=wall["host"], device_class_us_per_sample=wall["gpu"],
                                         device_launch_us_per_sample=device_event_us(launch_rrf) / n)
    return out


def step_grid():
    from models.models_online.FM_FTRL import FM_FTRL
    from models.models_online.RRF_Online import RRF_Online
    n, out = 3000, {}
    X, y = long_stream(n, "reg")
    lrs = [0.0005 * 1.3 ** i for i in range(16)]
    ms = [1, 2, 3, 4, 6, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56, 64]
    dss = [1, 2, 3, 4, 6, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56, 64]
    jobs = (("FM_FTRL", lambda device, a, b: FM_FTRL.grid(X, y, "reg", a, b, device=device), lrs, ms),
            ("RRF_Online", lambda device, a, b: RRF_Online.grid(X, y, "reg", a, [0.01], b, device=device), [0.001 * 1.15 ** i for i in range(16)], dss))
    for name, run, a, b in jobs:
        with quiet():
            seed_all(3)
            run("gpu", a[:2], b[:2])                              # warm-up: code objects, allocator
            torch.cuda.synchronize()
            tg = []
            for _ in range(3):
                seed_all(3)
                t0 = time.perf_counter()
                res = run("gpu", a, b)
                torch.cuda.synchronize()
                tg.append(time.perf_counter() - t0)
            seed_all(3)
            t0 = time.perf_counter()
            res_h = run("host", a, b)
            th = time.perf_counter() - t0
        S = len(res)
        worst = max(rel_dev(g.y_hat, h.y_hat) for (g, _), (h, _) in zip(res, res_h))
        out[name] = dict(settings=S, samples=n, features=8, device_grid_s=float(np.median(tg)), device_grid_s_all=tg, host_sequential_s=th,
                         device_sample_updates_per_s=S * n / float(np.median(tg)), host_sample_updates_per_s=S * n / th,
                         speedup=th / float(np.median(tg)), worst_y_hat_deviation_vs_host=worst)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=[s for s, _ in STEPS])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "path_b_times.json"))
    args = ap.parse_args()
    if args.step:                                                  # a child: one step, its result as one JSON line
        assert torch.cuda.is_available(), "path_b_times.py needs the GPU"
        res = dict(deviation=step_deviation, single=step_single, grid=step_grid)[args.step]()
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    result = {"device": None}
    for step, limit in STEPS:
        print(f"[{step}] ...", flush=True)
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"[{step}] exceeded {limit} s: stopping, nothing more is started on the device", flush=True)
            return 1
        if p.returncode != 0:
            print(p.stdout[-2000:], p.stderr[-4000:], f"[{step}] failed with status {p.returncode}: stopping", sep="\n", flush=True)
            return 1
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        result[step] = json.loads(line[len("RESULT "):])
        print(json.dumps(result[step], indent=1), flush=True)
    result["device"] = "MI355X (gfx950)"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", args.out, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
