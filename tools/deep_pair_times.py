"""What the pair loss costs DeepFM next to the pointwise one, on the Criteo-39 table (1 M rows x 16) with the 3 x 256 network.

  stream   fmx_deepfm_pair_stream at 2,048 pairs (4,096 rows per step) against fmx_deepfm_stream at B = 4,096 on the pair stream's
           own rows with arbitrary labels, so that the loss site of the MLP section is the only difference.  The two sides are
           timed alternately in one process, --reps times each after a warm call; reported are the median us/step of each and the
           run-to-run spread (max - min over the reps).  Two rule settings: signadam tables with an sgd network, and adam tables
           with an adam network (the _opt form).
  classes  DeepFMAdam.fit_pairs(full=True) on 2,048 pairs in pairs/s and rows/s, beside DeepFMAdam.fit on the same 4,096 rows.
Each part runs in a child process of its own under a time limit; the first that fails ends the run.  Writes
profiles/deep_pair_times.json.
  python tools/deep_pair_times.py [--steps N] [--reps R] [--calls N] [--out FILE]
  python tools/deep_pair_times.py --child stream --only pair --steps 300 --reps 1    (one side in this process: the run for
                                                                                     rocprofv3 --kernel-trace --stats)
  python tools/deep_pair_times.py --child stream --pair-first                        (the pair side allocates and is timed first)"""
import argparse
import json
import os
import subprocess
import sys

from pair_times import HYPER, K, N_POOL, ROOT, SEED, criteo_sizes, median, new_table, pair_pool, timed

HIDDEN, LAYERS = 256, 3
SETTINGS = (("signadam", "sgd"), ("adam", "adam"))


def child_stream(args):
    import numpy as np
    import torch
    import fmx
    torch.cuda.set_device(0)
    sizes, P = criteo_sizes(), args.batch_pairs
    pool = torch.from_numpy(pair_pool(np, sizes, N_POOL, P, SEED)).cuda()
    rng = np.random.default_rng(SEED + 1)
    y = torch.from_numpy((rng.uniform(size=(N_POOL, 2 * P)) < 0.3).astype(np.float32)).cuda()
    n_par = sum(HIDDEN * (K if l == 0 else HIDDEN) + HIDDEN for l in range(LAYERS))
    res = dict(rows_per_step=2 * P, pairs_per_step=P, steps_per_call=args.steps, reps=args.reps, table_rows=int(sum(sizes)), k=K,
               hidden=HIDDEN, layers=LAYERS)
    series = tuple(n for n in ("bce_same_rows", "pair") if args.only in (None, n))
    if args.pair_first:                                          # the order in which the two sides allocate and are timed
        series = series[::-1]
    for rule, net_rule in SETTINGS:
        run, keep = {}, []
        for n in series:
            t = new_table(fmx, torch, sizes, rule)
            e, h = fmx.FMEngine(t, max_batch=2 * P), fmx.Hyper(**HYPER)
            g = torch.Generator(device="cuda").manual_seed(SEED + 2)
            params = torch.randn(n_par, generator=g, device="cuda") * (0.5 / HIDDEN ** 0.5)
            grads = torch.zeros_like(params)
            opt = None if net_rule == "sgd" else fmx.MlpOpt(n_par, net_rule, lr=0.001, device="cuda")
            if n == "pair":
                run[n] = e.prepare_deepfm_pair_stream(h, rule, params, grads, K, HIDDEN, LAYERS, 0.001, pool, margin=0.0, mlp_opt=opt)
            else:
                run[n] = e.prepare_deepfm_stream(h, rule, "logits", params, grads, K, HIDDEN, LAYERS, 0.001, pool, y, mlp_opt=opt)
            keep.append((t, e, params))
        for n in series:
            timed(torch, lambda: run[n](args.steps))             # warm: code objects, allocations, the side stream
        us = {n: [] for n in series}
        for _ in range(args.reps):                               # alternating, in one process
            for n in series:
                us[n].append(timed(torch, lambda: run[n](args.steps)) / args.steps * 1e6)
        r = {}
        for n, (t, e, params) in zip(series, keep):
            e.check_error_flag()
            r[n + "_us_per_step"] = round(median(us[n]), 3)
            r[n + "_spread_us"] = round(max(us[n]) - min(us[n]), 3)
            r[n + "_reps_us"] = [round(v, 3) for v in us[n]]
            r[n + "_finite"] = bool(torch.isfinite(t.rows).all()) and bool(torch.isfinite(params).all())
        if len(series) == 2:
            r["pair_minus_bce_same_rows_us"] = round(median(us["pair"]) - median(us["bce_same_rows"]), 3)
        res[f"{rule}_{net_rule}"] = r
    print("RESULT " + json.dumps(res), flush=True)


def child_classes(args):
    import numpy as np
    import torch
    from models.models_online_deep.deepfm_adam import DeepFMAdam
    torch.cuda.set_device(0)
    sizes, P = criteo_sizes(), args.batch_pairs
    item = int(np.argmax(sizes))
    rows = torch.from_numpy(pair_pool(np, sizes, 1, P, SEED + 3)[0]).cuda()
    pos, neg = rows[0::2].contiguous(), rows[1::2][:, [item]].contiguous()
    rng = np.random.default_rng(SEED + 4)
    y = torch.from_numpy((rng.uniform(size=2 * P) < 0.3).astype(np.float32)).cuda()
    res = dict(pairs_per_call=P, rows_per_call=2 * P, calls=args.calls, reps=args.reps, hidden=HIDDEN, layers=LAYERS, k=K)
    for rule in ("signadam", "adam"):
        torch.manual_seed(SEED)
        m = DeepFMAdam(sizes, embedding_size=K, num_hidden_layers=LAYERS, neuron_per_hidden_layer=HIDDEN, batch_size=2 * P, n=0.001,
                       update_rule=rule, fused_optimizer=rule == "adam")
        m.strict_index_check = False                             # the index flag is read once, after the timed calls

        def pairs():
            for _ in range(args.calls):
                m.fit_pairs(pos, None, [item], negatives=neg, full=True)

        def pointwise():
            for _ in range(args.calls):
                m.fit(rows, None, y)
        r = {}
        for name, fn in (("fit_pairs_full", pairs), ("fit", pointwise)):
            timed(torch, fn)                                     # warm
            secs = [timed(torch, fn) for _ in range(args.reps)]
            per_call = median(secs) / args.calls
            r[name] = dict(us_per_call=round(per_call * 1e6, 1), rows_per_s=round(2 * P / per_call, 1),
                           seconds=[round(s, 5) for s in secs])
        r["fit_pairs_full"]["pairs_per_s"] = round(P / (r["fit_pairs_full"]["us_per_call"] * 1e-6), 1)
        m.check_index_flag()
        r["finite"] = bool(torch.isfinite(m._table.rows).all()) and bool(torch.isfinite(m._mlp_flat).all())
        res[rule] = r
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-pairs", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=1000, help="steps per timed call of the streams")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50, help="class-level calls per timed repetition")
    ap.add_argument("--timeout", type=int, default=200, help="seconds per child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deep_pair_times.json"))
    ap.add_argument("--child", default=None)
    ap.add_argument("--only", default=None, choices=("bce_same_rows", "pair"), help="with --child stream: one side alone")
    ap.add_argument("--pair-first", action="store_true", help="with --child stream: the pair side allocates and runs first")
    args = ap.parse_args()
    if args.child:
        return {"stream": child_stream, "classes": child_classes}[args.child](args)
    out = dict(what="the pair loss next to the pointwise one for DeepFM (Criteo-39 table 1 M x 16, 3 x 256 network): us/step of the "
                    "streams, samples/s of the class calls; medians of reps timed calls after one warm call")
    for part in ("stream", "classes"):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", part, "--batch-pairs", str(args.batch_pairs), "--steps", str(args.steps),
               "--reps", str(args.reps), "--calls", str(args.calls)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print(f"{part}: no result within {args.timeout} s; stopping", flush=True)
            return 1
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"{part}: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}", flush=True)
            return 1
        out[part] = json.loads(line[-1][len("RESULT "):])
        print(part, json.dumps(out[part]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
