"""What the listwise (sampled-softmax) step costs next to the pair step on the same positives and negatives, and next to the
pointwise step on the same rows, on the Criteo-39 table (1 M rows x 16) of bench.py.

For G in {2, 4, 8, 16} and 2,048 lists per step, under signadam and ftrl, in one process:
  list           fmx_fm_list_stream: 2,048 G rows per step
  pair           fmx_fm_pair_stream on the same positives and negatives expanded to 2,048 (G - 1) pairs, i.e. 4,096 (G - 1) rows per
                 step.  Where that exceeds the sort's 32,768 rows (G = 16: 61,440) the pairs of a step are split into the fewest equal
                 calls that fit and their times are summed (pair_calls in the result says how many)
  bce_same_rows  fmx_fm_stream under BCE-with-logits on the list rows themselves with arbitrary labels: the same sort and update
                 launches on the same rows, so the difference is the list epilogue and its workgroup shape
The three are timed alternately, --reps times each after a warm call; reported are the median, p10 and p90 us/step of each.
gate_list_p90_below_pair_p10 is the project's usual gate, read at G = 8 (8 rows per positive against 14).
Runs in a child process under a time limit.  Writes profiles/list_times.json.
  python tools/list_times.py [--lists N] [--steps N] [--reps R] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fm-for-online-recommendation_amd"))

K, N_POOL, SEED, MAX_SORT_ROWS = 16, 8, 1234, 32768
GS = (2, 4, 8, 16)
HYPER = dict(lr=0.01, eps=1e-8, alpha=0.05, beta=1.0, l1=0.001, l2=0.01)
LAYOUT = {"ftrl": "ftrl", "signadam": "weights"}


def criteo_sizes():
    import bench
    return list(bench.CRITEO_SIZES)


def new_table(fmx, torch, sizes, rule):
    t = fmx.FlatTable(sizes, K, layout=LAYOUT[rule], ftrl=HYPER)
    g = torch.Generator(device="cuda").manual_seed(SEED)
    t.rows[:, :K] = torch.randn((t.n_rows, K), generator=g, device="cuda") * 0.01
    if rule == "ftrl":
        t.rows[:, t.z_offset:t.z_offset + K] = fmx.table.ftrl_z_for_weight_torch(t.rows[:, :K], t.ftrl)
    return t


def list_pool(np, sizes, n_pool, B, G, seed):
    """[n_pool, B, G, F] int32: a list's negatives are its positive with the largest field (the item) redrawn"""
    rng = np.random.default_rng(seed)
    item = int(np.argmax(sizes))
    pos = np.stack([rng.integers(0, s, size=(n_pool, B)) for s in sizes], axis=2)
    rows = np.repeat(pos[:, :, None, :], G, axis=2)
    rows[:, :, 1:, item] = (pos[:, :, None, item] + 1 + rng.integers(0, sizes[item] - 1, size=(n_pool, B, G - 1))) % sizes[item]
    return rows.astype(np.int32)


def pair_pools(np, lists, max_rows):
    """the lists' (positive, negative) pairs as the fewest equal pools [n_pool, 2 P, F] of at most max_rows rows a step"""
    n_pool, B, G, F = lists.shape
    pairs = np.stack([np.repeat(lists[:, :, :1], G - 1, axis=2), lists[:, :, 1:]], axis=3).reshape(n_pool, B * (G - 1), 2, F)
    n = pairs.shape[1]
    calls = next(c for c in range(1, n + 1) if n % c == 0 and 2 * (n // c) <= max_rows)
    return [np.ascontiguousarray(pairs[:, i * (n // calls):(i + 1) * (n // calls)].reshape(n_pool, 2 * (n // calls), F)) for i in range(calls)]


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def child(args):
    import numpy as np
    import torch
    import fmx
    torch.cuda.set_device(0)
    sizes, B = criteo_sizes(), args.lists
    series = ("list", "pair", "bce_same_rows")
    res = dict(lists_per_step=B, steps_per_call=args.steps, reps=args.reps, n_pool=N_POOL, table_rows=int(sum(sizes)), k=K, fields=len(sizes))
    for rule in ("signadam", "ftrl"):
        tables = {n: new_table(fmx, torch, sizes, rule) for n in series}
        eng = {n: fmx.FMEngine(tables[n], max_batch=min(MAX_SORT_ROWS, 2 * B * (max(GS) - 1))) for n in series}
        hyp = {n: fmx.Hyper(**HYPER) for n in series}
        res[rule] = {}
        for G in GS:
            lists = list_pool(np, sizes, N_POOL, B, G, SEED + G)
            pool_l = torch.from_numpy(lists.reshape(N_POOL, B * G, -1)).cuda()
            pools_p = [torch.from_numpy(p).cuda() for p in pair_pools(np, lists, MAX_SORT_ROWS)]
            y = torch.from_numpy((np.random.default_rng(SEED).uniform(size=(N_POOL, B * G)) < 0.3).astype(np.float32)).cuda()

            def run_pairs():
                for p in pools_p:
                    eng["pair"].pair_stream(hyp["pair"], rule, p, args.steps, margin=0.0)
            run = {"list": lambda: eng["list"].list_stream(hyp["list"], rule, pool_l, G, args.steps),
                   "pair": run_pairs,
                   "bce_same_rows": lambda: eng["bce_same_rows"].stream(hyp["bce_same_rows"], rule, "logits", pool_l, y, args.steps)}
            for n in series:
                timed(torch, run[n])                                 # warm: code objects, allocations, the side stream
            us = {n: [] for n in series}
            for _ in range(args.reps):                               # alternating, in one process
                for n in series:
                    us[n].append(timed(torch, run[n]) / args.steps * 1e6)
            r = dict(list_rows_per_step=B * G, pair_rows_per_step=2 * B * (G - 1), pair_calls=len(pools_p))
            for n in series:
                eng[n].check_error_flag()
                r[n + "_us_per_step"] = round(float(np.median(us[n])), 3)
                r[n + "_p10_us"] = round(float(np.percentile(us[n], 10)), 3)
                r[n + "_p90_us"] = round(float(np.percentile(us[n], 90)), 3)
                r[n + "_reps_us"] = [round(v, 3) for v in us[n]]
            r["list_over_pair"] = round(r["list_us_per_step"] / r["pair_us_per_step"], 3)
            r["list_minus_bce_same_rows_us"] = round(r["list_us_per_step"] - r["bce_same_rows_us_per_step"], 3)
            r["gate_list_p90_below_pair_p10"] = bool(r["list_p90_us"] < r["pair_p10_us"])
            r["finite"] = all(bool(torch.isfinite(tables[n].rows).all()) for n in series)
            res[rule][f"G={G}"] = r
            print(rule, G, json.dumps(r), flush=True)
            del pool_l, pools_p, y
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lists", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=300, help="steps per timed call")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--timeout", type=int, default=400, help="seconds for the child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "list_times.json"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--lists", str(args.lists), "--steps", str(args.steps), "--reps", str(args.reps)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    except subprocess.TimeoutExpired:
        print(f"no result within {args.timeout} s; stopping", flush=True)
        return 1
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        print(f"exit status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}", flush=True)
        return 1
    out = dict(what="the list step next to the pair step on the same positives and negatives and next to the BCE step on the same rows, "
                    "Criteo-39 table (1 M x 16): us/step of the batched streams; median, p10 and p90 of reps calls after one warm call",
               **json.loads(line[-1][len("RESULT "):]))
    print(r.stdout[-4000:], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
