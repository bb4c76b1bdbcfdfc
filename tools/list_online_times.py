"""What the online list loop costs per list on the device next to the only way to do the same work without it -- the host loop of
fmx_fm_list_step on one list at a time -- on the Criteo-39 table (1 M rows x 16) of bench.py.

For G in {2, 8, 16} and a resident stream of lists, under signadam and ftrl, in one process:
  device      fmx_fm_list_online_run on the stream (k_fm_list_online: one workgroup of G waves)
  host_loop   fmx_fm_list_step with B_lists = 1, inv_b = 1 on the same lists, one call per list (sort, list forward, update)
  pair        for orientation: fmx_fm_pair_online_run on as many pairs (one wavefront), per pair
The three are timed alternately, --reps times each after a warm call; reported are the median, p10 and p90 us per list (pair).
gate_device_p90_below_host_p10 is the project's usual gate, read at G = 8.  device_list_over_pair is the per-list cost in per-pair
costs.  Runs in a child process under a time limit.  Writes profiles/list_online_times.json.
  python tools/list_online_times.py [--lists N] [--reps R] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fm-for-online-recommendation_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from list_times import HYPER, K, SEED, criteo_sizes, list_pool, new_table, timed  # noqa: E402

GS = (2, 8, 16)


def child(args):
    import numpy as np
    import torch
    import fmx
    torch.cuda.set_device(0)
    sizes, N = criteo_sizes(), args.lists
    series = ("device", "host_loop", "pair")
    res = dict(lists_per_call=N, reps=args.reps, table_rows=int(sum(sizes)), k=K, fields=len(sizes))
    for rule in ("signadam", "ftrl"):
        tables = {n: new_table(fmx, torch, sizes, rule) for n in series}
        eng = {n: fmx.FMEngine(tables[n], max_batch=16) for n in series}      # (a list at a time: no sort split of the large fields)
        hyp = {n: fmx.Hyper(**HYPER) for n in series}
        assert eng["device"].list_online_run_fits(len(sizes), tables["device"].kp)
        res[rule] = {}
        for G in GS:
            lists = torch.from_numpy(list_pool(np, sizes, 1, N, G, SEED + G).reshape(N * G, -1)).cuda()
            pairs = lists.reshape(N, G, -1)[:, :2].reshape(2 * N, -1).contiguous()

            def host_loop():
                e, h = eng["host_loop"], hyp["host_loop"]
                for i in range(N):
                    e.list_step(h, rule, lists[G * i:G * (i + 1)], G, None, inv_b=1.0)
            run = {"device": lambda: eng["device"].list_online_run(hyp["device"], rule, lists, G),
                   "host_loop": host_loop,
                   "pair": lambda: eng["pair"].pair_online_run(hyp["pair"], rule, pairs)}
            for n in series:
                timed(torch, run[n])                                 # warm: code objects, allocations
            us = {n: [] for n in series}
            for _ in range(args.reps):                               # alternating, in one process
                for n in series:
                    us[n].append(timed(torch, run[n]) / N * 1e6)
            r = dict(G=G)
            for n in series:
                eng[n].check_error_flag()
                r[n + "_us"] = round(float(np.median(us[n])), 3)
                r[n + "_p10_us"] = round(float(np.percentile(us[n], 10)), 3)
                r[n + "_p90_us"] = round(float(np.percentile(us[n], 90)), 3)
                r[n + "_reps_us"] = [round(v, 3) for v in us[n]]
            r["host_over_device"] = round(r["host_loop_us"] / r["device_us"], 2)
            r["device_list_over_pair"] = round(r["device_us"] / r["pair_us"], 2)
            r["gate_device_p90_below_host_p10"] = bool(r["device_p90_us"] < r["host_loop_p10_us"])
            r["finite"] = all(bool(torch.isfinite(tables[n].rows).all()) for n in series)
            res[rule][f"G={G}"] = r
            print(rule, G, json.dumps(r), flush=True)
            del lists, pairs
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lists", type=int, default=2048, help="lists per timed call")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--timeout", type=int, default=400, help="seconds for the child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "list_online_times.json"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--lists", str(args.lists), "--reps", str(args.reps)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    except subprocess.TimeoutExpired:
        print(f"no result within {args.timeout} s; stopping", flush=True)
        return 1
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        print(f"exit status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}", flush=True)
        return 1
    out = dict(what="the online list loop on the device next to the host loop of single-list steps on the same lists, and the pair "
                    "walker per pair, Criteo-39 table (1 M x 16): us per list (pair); median, p10 and p90 of reps calls after one warm call",
               **json.loads(line[-1][len("RESULT "):]))
    print(r.stdout[-4000:], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
