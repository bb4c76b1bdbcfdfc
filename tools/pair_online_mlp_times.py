"""What the device loop gains run_pair_experiment(full=True) of DeepFMAdam: the online predict-then-fit protocol on pairs through
the whole network (fmx_online_run_mlp_pair) next to the loops it replaces.

The criteo39s-shaped model (the golden fixture's 39 small fields, k = 10) at the reference's 5 x 10 network and at 3 x 60 (7,980
parameters of the one-workgroup form's 8,192), under signadam and under adam with fused_optimizer=True.  Every (row, rule) runs in
a fresh child process (one GPU context each) under its own time limit; the first child that fails ends the run.  In each process,
pairs/s, median of --reps timed calls after one warm call, with the run-to-run spread (max - min over the reps):
  (a) one_workgroup   fmx_online_run_mlp_pair, one workgroup walking the stream (k_online_mlp_pair)
  (b) queued          the same call with fmx_set_option("online_persistent", 0): four launches per pair, no host synchronisation
  (c) ctypes_loop     the per-pair sequence from outside: fmx_fm_forward, fmx_mlp_pair_fit, fmx_sort_occurrences, fmx_fm_update
  (d) class_host_loop run_pair_experiment(full=True) with pair_loop_on_device = False: the host loop of one-pair section calls
  (e) pointwise       run_experiment of the same model on as many samples (fmx_online_run_mlp / _opt), in samples/s, for scale
and the ratios (a) / (d), (a) / (b).  Nothing is asserted about them: they are reported as measured.
Writes profiles/pair_online_mlp_times.json.
  python tools/pair_online_mlp_times.py [--pairs N] [--loop-pairs M] [--reps R] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fm-for-online-recommendation_amd"))

ROWS = {"5x10": (5, 10), "3x60": (3, 60)}      # name: (layers, hidden)
RULES = ("signadam", "adam")


def fixture_meta():
    import numpy as np
    z = np.load(os.path.join(ROOT, "tests", "golden", "DeepFMAdam_criteo39s.npz"))
    return json.loads(bytes(z["meta"]).decode())


def child(row, rule, n_dev, n_loop, reps):
    import numpy as np
    import torch
    import fmx
    from models.models_online_deep.deepfm_adam import DeepFMAdam
    torch.cuda.set_device(0)
    lib = fmx._lib.load()
    meta = fixture_meta()
    sizes, k = meta["feature_sizes"], meta["k"]
    L, H = ROWS[row]
    item = int(np.argmax(sizes))
    rng = np.random.default_rng(11)
    N = max(n_dev, n_loop)
    idx = np.stack([rng.integers(0, s, size=N) for s in sizes], axis=1).astype(np.int32)
    neg = ((idx[:, item] + 1 + rng.integers(0, sizes[item] - 1, size=N)) % sizes[item]).astype(np.int32)[:, None]
    y = (rng.uniform(size=N) < 0.3).astype(np.float32)
    xv = np.ones(idx.shape, np.float32)
    rows = np.repeat(idx, 2, axis=0)
    rows[1::2, item] = neg[:, 0]
    rows_d = torch.from_numpy(rows).cuda()

    def model():
        torch.manual_seed(5)
        m = DeepFMAdam(sizes, embedding_size=k, num_hidden_layers=L, neuron_per_hidden_layer=H, n=0.001, update_rule=rule,
                       fused_optimizer=rule != "signadam")
        m.strict_index_check = False
        return m

    def measure(fn, n, m):
        fn()                                           # warm: module load, allocations
        secs = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
        m._engine.check_error_flag()
        per_s = sorted(n / s for s in secs)
        finite = bool(torch.isfinite(m._mlp_flat).all()) and bool(torch.isfinite(m._table.rows).all())
        return dict(items=n, seconds=[round(s, 5) for s in secs], per_s=round(per_s[len(per_s) // 2], 1),
                    spread_per_s=round(per_s[-1] - per_s[0], 1), us_per_item=round(1e6 / per_s[len(per_s) // 2], 3), finite=finite)

    def device_loop(m, n, persistent):
        args = (m._hyper, rule, m._mlp_flat, k, H, L, True, rows_d[:2 * n], None)

        def fn():
            old = lib.fmx_set_option(b"online_persistent", int(persistent))
            try:
                pred, _, _ = m._engine.online_run_mlp_pair(*args, margin=0.0, mlp_opt=m._mlp_fused)
                pred.cpu()                             # as the class call ends: the predictions on the host
            finally:
                lib.fmx_set_option(b"online_persistent", old)
        return fn

    def ctypes_loop(m, n):
        e, t, hyp = m._engine, m._table, m._hyper

        def fn():
            pred = torch.empty(n, dtype=torch.uint8, device="cuda")
            for i in range(n):
                r = rows_d[2 * i:2 * i + 2]
                e.forward(hyp, r, None, want_first=False, want_bi=True)
                dz, gbi, z = e.mlp_pair_fit(m._mlp_flat, k, H, L, hyp, "sgd" if m._mlp_fused is not None else rule, e.logit[:2], 1,
                                            margin=0.0, inv_b=1.0, mlp_opt=m._mlp_fused, want_logit=True)
                pred[i] = z[0] > z[1]
                e.sort(r)
                e.update(hyp, rule, 2, None, dz, dz, gbi, inv_b=1.0, with_loss=False)
            pred.cpu()
        return fn

    res = dict(row=row, rule=rule, layers=L, hidden=H, k=k, fields=len(sizes), n_params=sum(H * (k if l == 0 else H) + H for l in range(L)))
    m = model()
    assert m._pair_device_loop_ok() and fmx.FMEngine.online_run_fits(len(sizes), m._table.kp)
    res["one_workgroup"] = measure(device_loop(m, n_dev, True), n_dev, m)
    m = model()
    res["queued"] = measure(device_loop(m, n_dev, False), n_dev, m)
    m = model()
    res["ctypes_loop"] = measure(ctypes_loop(m, n_loop), n_loop, m)
    m = model()
    assert m.pair_loop_on_device is False
    res["class_host_loop"] = measure(lambda: m.run_pair_experiment(idx[:n_loop], xv[:n_loop], [item], negatives=neg[:n_loop], full=True),
                                     n_loop, m)
    m = model()
    assert m._device_loop_ok()
    res["pointwise"] = measure(lambda: m.run_experiment(idx[:n_dev], xv[:n_dev], y[:n_dev]), n_dev, m)
    a, b, d = (res[n]["per_s"] for n in ("one_workgroup", "queued", "class_host_loop"))
    res["one_workgroup_over_class_host_loop"] = round(a / d, 2)
    res["one_workgroup_over_queued"] = round(a / b, 3)
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8192, help="pairs per call of the device loops (and samples of the pointwise one)")
    ap.add_argument("--loop-pairs", type=int, default=300, help="pairs per call of the two host loops")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=150, help="seconds per child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_online_mlp_times.json"))
    ap.add_argument("--child", default=None, help="ROW:RULE")
    args = ap.parse_args()
    if args.child:
        row, rule = args.child.split(":")
        return child(row, rule, args.pairs, args.loop_pairs, args.reps)
    results = []
    for row in ROWS:
        for rule in RULES:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", f"{row}:{rule}", "--pairs", str(args.pairs), "--loop-pairs",
                   str(args.loop_pairs), "--reps", str(args.reps)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
            except subprocess.TimeoutExpired:
                print(f"{row} {rule}: no result within {args.timeout} s; stopping", flush=True)
                return 1
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                print(f"{row} {rule}: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}", flush=True)
                return 1
            results.append(json.loads(line[-1][len("RESULT "):]))
            print(json.dumps(results[-1]), flush=True)
    out = dict(what="the online pair loop of DeepFMAdam through the whole network (criteo39s-shaped, k = 10): pairs/s (pointwise: "
                    "samples/s), median of reps timed calls after one warm call, spread = max - min over the reps",
               pairs=args.pairs, loop_pairs=args.loop_pairs, reps=args.reps, results=results)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
