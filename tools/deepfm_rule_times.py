"""What the adaptive rules cost the fused DeepFM step, and what the fused forms gain over the torch-optimizer path.

BASELINE configs[3]: the synthetic Criteo-39 table (1,006,628 rows), k = 16, B = 4,096, 3 x 256 relu MLP, a resident pool of
16 batches.  Every configuration runs in a fresh child process (one GPU context each), under its own time limit; the first
child that fails ends the run.
  stream:<table rule>:<network rule>   us per step of fmx_deepfm_stream_opt (median of --reps runs of --steps steps after a warm
                                       run), and IN THE SAME PROCESS us per step of fmx_deepfm_stream (signadam tables, SGD on
                                       the network) -- the yardstick -- with the ratio of the two
  fit:default                          samples/s of DeepFMAdam(update_rule="adam").fit, fused_optimizer=False: kernel forward,
                                       the MLP through PyTorch autograd, fmx_fm_update, torch.optim.Adam.step() (--fit-steps)
  fit:fused                            the same calls with fused_optimizer=True (forward, fmx_mlp_section_opt, sort, update)
  trainer:stream                       DeepFMTrainer on a HipDeepOptBackend, prepare_stream (adam / adam): one foreign call
  python tools/deepfm_rule_times.py [--steps N] [--reps R] [--fit-steps M] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fm-for-online-recommendation_amd"))

CONFIGS = ["stream:adam:adam", "stream:adagrad:adagrad", "stream:signadam:sgd", "fit:default", "fit:fused", "trainer:stream"]
HIDDEN, LAYERS, LR = 256, 3, 1e-3


def median_us(run, steps, reps, torch):
    """run(steps) timed with device events, reps times after one warm run -> (median us per step, all of them)."""
    st = torch.cuda.current_stream()
    run(steps)
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        run(steps)
        b.record(st)
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / steps)
    return sorted(us)[len(us) // 2], [round(v, 2) for v in us]


def child(config, steps, reps, fit_steps):
    import numpy as np  # noqa: F401
    import torch
    import bench
    import fmx
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    kind, *rest = config.split(":")
    idx_np, y_np = bench.synth_pool(bench.N_POOL, bench.BATCH, bench.CRITEO_SIZES, bench.SEED + 1)
    idx_pool, y_pool = torch.from_numpy(idx_np).to(dev), torch.from_numpy(y_np).to(dev)
    k, B = bench.K_EMB, bench.BATCH
    n_par = sum(HIDDEN * (k if l == 0 else HIDDEN) + HIDDEN for l in range(LAYERS))

    def table_for(rule):
        layout = "moments" if rule in ("adam", "adagrad") else "weights"
        t = fmx.FlatTable(bench.CRITEO_SIZES, k, layout=layout, device=dev)
        g = torch.Generator(device=dev).manual_seed(1)
        t.rows[:, :k] = torch.randn((t.n_rows, k), device=dev, generator=g) * 0.01
        return t

    def network():
        g = torch.Generator(device=dev).manual_seed(2)
        p = torch.randn(n_par, device=dev, generator=g) * (1.0 / HIDDEN ** 0.5)
        return p, torch.zeros_like(p)

    res = dict(config=config, B=B, k=k, hidden=HIDDEN, layers=LAYERS)
    work = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(work):
        if kind == "stream":
            table_rule, net_rule = rest
            t = table_for(table_rule)
            eng = fmx.FMEngine(t, max_batch=B)
            p, g = network()
            opt = fmx.MlpOpt(n_par, net_rule, lr=LR, device=dev)
            run = eng.prepare_deepfm_stream(fmx.Hyper(lr=LR), table_rule, "logits", p, g, k, HIDDEN, LAYERS, LR, idx_pool, y_pool,
                                            stream=work, mlp_opt=opt)
            us, all_us = median_us(run, steps, reps, torch)
            eng.check_error_flag()
            # the yardstick in the same process: fmx_deepfm_stream, signadam tables, SGD on the network
            t0 = table_for("signadam")
            eng0 = fmx.FMEngine(t0, max_batch=B)
            p0, g0 = network()
            run0 = eng0.prepare_deepfm_stream(fmx.Hyper(lr=LR), "signadam", "logits", p0, g0, k, HIDDEN, LAYERS, LR, idx_pool, y_pool,
                                              stream=work)
            us0, all_us0 = median_us(run0, steps, reps, torch)
            eng0.check_error_flag()
            res.update(us_per_step=round(us, 2), runs=all_us, samples_per_s=round(B / us * 1e6), yardstick_us_per_step=round(us0, 2),
                       yardstick_runs=all_us0, ratio_to_yardstick=round(us / us0, 4), finite=bool(torch.isfinite(p).all()))
        elif kind == "fit":
            from models.models_online_deep.deepfm_adam import DeepFMAdam
            torch.manual_seed(3)
            m = DeepFMAdam(bench.CRITEO_SIZES, embedding_size=k, num_hidden_layers=LAYERS, neuron_per_hidden_layer=HIDDEN, n=LR,
                           batch_size=B, update_rule="adam", fused_optimizer=rest[0] == "fused")
            m.strict_index_check = False                 # the error word is read once, after the run

            def run(n):
                for s in range(n):
                    m.fit(idx_pool[s % bench.N_POOL], None, y_pool[s % bench.N_POOL])
            us, all_us = median_us(run, fit_steps, reps, torch)
            m.check_index_flag()
            res.update(us_per_step=round(us, 2), runs=all_us, samples_per_s=round(B / us * 1e6), steps=fit_steps)
        else:
            t = table_for("adam")
            eng = fmx.FMEngine(t, max_batch=B)
            torch.manual_seed(3)
            layers = [torch.nn.Linear(k if j == 0 else HIDDEN, HIDDEN).to(dev) for j in range(LAYERS)]
            opt = fmx.MlpOpt(n_par, "adam", lr=LR, device=dev)
            tr = fmx.DeepFMTrainer(fmx.HipDeepOptBackend(eng, fmx.Hyper(lr=LR), "adam", opt), layers, k, t.kp, mlp_lr=LR)
            run = tr.prepare_stream(idx_pool, y_pool, stream=work)
            us, all_us = median_us(run, steps, reps, torch)
            eng.check_error_flag()
            res.update(us_per_step=round(us, 2), runs=all_us, samples_per_s=round(B / us * 1e6))
    res.setdefault("steps", steps)
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fit-steps", type=int, default=200)
    ap.add_argument("--timeout", type=int, default=150, help="seconds per child")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.steps, args.reps, args.fit_steps)
    rows = []
    for config in CONFIGS:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", config, "--steps", str(args.steps), "--reps", str(args.reps),
               "--fit-steps", str(args.fit_steps)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print(f"{config}: no result within {args.timeout} s; stopping", flush=True)
            return 1
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"{config}: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}", flush=True)
            return 1
        rows.append(json.loads(line[-1][len("RESULT "):]))
        print(json.dumps(rows[-1]), flush=True)
    by = {r["config"]: r for r in rows}
    out = dict(what="DeepFM step at configs[3] under the network's and the tables' update rules", steps=args.steps, reps=args.reps,
               results=rows,
               fused_fit_over_default_fit=round(by["fit:fused"]["samples_per_s"] / by["fit:default"]["samples_per_s"], 2),
               trainer_stream_over_default_fit=round(by["trainer:stream"]["samples_per_s"] / by["fit:default"]["samples_per_s"], 2))
    print(json.dumps({k_: v for k_, v in out.items() if k_ != "results"}), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
