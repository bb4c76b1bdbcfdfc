"""What the pairwise-ranking (BPR) loss costs next to the pointwise one, on the Criteo-39 table (1 M rows x 16) of bench.py.

  batched   fmx_fm_pair_stream at B = 2048 pairs (2B = 4096 rows per step) against fmx_fm_stream at B = 4096 under BCE-with-logits,
            under ftrl and signadam, in one process: the two issue the same sort and update launches and differ in the forward's
            epilogue and workgroup shape.  A batch of pairs names fewer distinct rows than a batch of independent samples (the
            two samples of a pair share their context columns), so the BCE stream is timed twice: on independent samples
            (bce) and on the pair stream's own rows with arbitrary labels (bce_same_rows), which leaves the epilogue as the
            only difference.  The three are timed alternately, --reps times each after a warm call; reported are the median
            us/step of each and the run-to-run spread (max - min over the reps) of each.
  online    fmx_fm_pair_online_run (pairs/s) against a ctypes loop of fmx_fm_pair_step(B_pairs = 1) in the same process, under
            signadam and adam, with fmx_fm_online_run's samples/s alongside for scale.
Each part runs in a child process of its own under a time limit; the first that fails ends the run.  Writes profiles/pair_times.json.
  python tools/pair_times.py [--steps N] [--reps R] [--pairs N] [--loop-pairs M] [--out FILE]

  --ab-lib PATH   instead of the above: the stream walkers' instantiations one by one (k_fm_pair_online at every kp, under signadam
            and sgd, at 2, 3 and 4 fields per lane group; k_fm_online at kp = 4, 16 and 64; two more as controls), this tree's
            library against another build of the same ABI at PATH, for a change that moved their instruction streams.  Fresh
            child processes alternate PATH, this tree, PATH, ... (--ab-rounds each; --ab-this-first: this tree, PATH, ...); every
            child times every instantiation (median of --reps calls after a warm call) and sums the table it leaves.  Writes
            --out (give one): per instantiation both sides' us per item, the spread of PATH's processes (max - min), the
            difference, and whether the tables' sums agree."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fm-for-online-recommendation_amd"))

K, N_POOL, SEED = 16, 16, 1234
HYPER = dict(lr=0.01, eps=1e-8, alpha=0.05, beta=1.0, l1=0.001, l2=0.01)
LAYOUT = {"ftrl": "ftrl", "signadam": "weights", "adam": "moments"}


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


def pair_pool(np, sizes, n_pool, B, seed):
    """[n_pool, 2B, F] int32: the negative is the positive with the largest field (the item) redrawn"""
    rng = np.random.default_rng(seed)
    item = int(np.argmax(sizes))
    pos = np.stack([rng.integers(0, s, size=(n_pool, B)) for s in sizes], axis=2)
    neg = pos.copy()
    neg[:, :, item] = (pos[:, :, item] + 1 + rng.integers(0, sizes[item] - 1, size=(n_pool, B))) % sizes[item]
    rows = np.empty((n_pool, 2 * B, len(sizes)), np.int32)
    rows[:, 0::2], rows[:, 1::2] = pos, neg
    return rows


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def median(v):
    return sorted(v)[len(v) // 2]


def child_batched(args):
    import numpy as np
    import torch
    import fmx
    torch.cuda.set_device(0)
    sizes, Bp = criteo_sizes(), args.batch_pairs
    pool2 = torch.from_numpy(pair_pool(np, sizes, N_POOL, Bp, SEED)).cuda()
    rng = np.random.default_rng(SEED + 1)
    pool1 = torch.from_numpy(np.stack([rng.integers(0, s, size=(N_POOL, 2 * Bp)) for s in sizes], axis=2).astype(np.int32)).cuda()
    y1 = torch.from_numpy((rng.uniform(size=(N_POOL, 2 * Bp)) < 0.3).astype(np.float32)).cuda()
    series = ("bce", "bce_same_rows", "pair")
    res = dict(rows_per_step=2 * Bp, pairs_per_step=Bp, steps_per_call=args.steps, reps=args.reps, table_rows=int(sum(sizes)), k=K)
    for rule in ("ftrl", "signadam"):
        tables = {n: new_table(fmx, torch, sizes, rule) for n in series}
        eng = {n: fmx.FMEngine(tables[n], max_batch=2 * Bp) for n in series}
        hyp = {n: fmx.Hyper(**HYPER) for n in series}
        run = {"bce": lambda: eng["bce"].stream(hyp["bce"], rule, "logits", pool1, y1, args.steps),
               "bce_same_rows": lambda: eng["bce_same_rows"].stream(hyp["bce_same_rows"], rule, "logits", pool2, y1, args.steps),
               "pair": lambda: eng["pair"].pair_stream(hyp["pair"], rule, pool2, args.steps, margin=0.0)}
        for n in series:
            timed(torch, run[n])                                 # warm: code objects, allocations, the side stream
        us = {n: [] for n in series}
        for _ in range(args.reps):                               # alternating, in one process
            for n in series:
                us[n].append(timed(torch, run[n]) / args.steps * 1e6)
        r = {}
        for n in series:
            eng[n].check_error_flag()
            r[n + "_us_per_step"] = round(median(us[n]), 3)
            r[n + "_spread_us"] = round(max(us[n]) - min(us[n]), 3)
            r[n + "_reps_us"] = [round(v, 3) for v in us[n]]
        r["pair_minus_bce_us"] = round(median(us["pair"]) - median(us["bce"]), 3)
        r["pair_minus_bce_same_rows_us"] = round(median(us["pair"]) - median(us["bce_same_rows"]), 3)
        r["finite"] = all(bool(torch.isfinite(tables[n].rows).all()) for n in series)
        res[rule] = r
    print("RESULT " + json.dumps(res), flush=True)


def child_online(args):
    import numpy as np
    import torch
    import fmx
    L = fmx._lib
    torch.cuda.set_device(0)
    sizes = criteo_sizes()
    N, M = args.pairs, args.loop_pairs
    rows = torch.from_numpy(pair_pool(np, sizes, 1, N, SEED + 2)[0]).cuda()
    rng = np.random.default_rng(SEED + 3)
    y = torch.from_numpy((rng.uniform(size=2 * N) < 0.3).astype(np.float32)).cuda()
    res = dict(pairs_per_call=N, loop_pairs_per_call=M, reps=args.reps, table_rows=int(sum(sizes)), k=K, fields=len(sizes))
    for rule in ("signadam", "adam"):
        t = new_table(fmx, torch, sizes, rule)
        e = fmx.FMEngine(t, max_batch=64)
        h = fmx.Hyper(**HYPER)
        lib, ts = e.lib, t.c_struct()
        out = e._fwd_out(want_first=False, want_bi=False)
        st = e._stream()

        def loop():                                              # the per-pair calls the online kernel replaces
            base, step0 = rows.data_ptr(), t.step
            stride = 2 * rows.shape[1] * 4
            for i in range(M):
                h.c.step = step0 + i
                rc = lib.fmx_fm_pair_step(ts, h.ref(), L.RULES[rule], base + i * stride, None, 1, 0.0, 1.0, e.workspace.data_ptr(),
                                          e._ws_bytes(), C.byref(out), e.loss_out.data_ptr(), st)
                if rc != L.OK:
                    L.check(rc)
            t.step = step0 + M if t.layout == "moments" else t.step
        device = lambda: e.pair_online_run(h, rule, rows, None, margin=0.0)
        single = lambda: e.online_run(h, rule, "logits", rows, None, y)
        r = {}
        for name, fn, n in (("pair_online_run", device, N), ("pair_step_loop", loop, M), ("fm_online_run", single, 2 * N)):
            timed(torch, fn)                                     # warm
            secs = [timed(torch, fn) for _ in range(args.reps)]
            r[name] = dict(items_per_call=n, items_per_s=round(n / median(secs), 1), us_per_item=round(median(secs) / n * 1e6, 3),
                           seconds=[round(s, 5) for s in secs])
        e.check_error_flag()
        r["finite"] = bool(torch.isfinite(t.rows).all())
        r["online_over_loop"] = round(r["pair_online_run"]["items_per_s"] / r["pair_step_loop"]["items_per_s"], 2)
        res[rule] = r
    print("RESULT " + json.dumps(res), flush=True)


def walker_grid():
    """(name as the kernel is instantiated, kind, kp, rule, fields): LAYOUT 0 = weights, 2 = moments; RULE 0 = signadam, 1 = sgd, 4 = adam"""
    rule_id = {"signadam": 0, "sgd": 1, "adam": 4}
    grid = []
    for kp in (4, 8, 16, 32, 64):
        lpr, slots = kp // 4, 64 // (kp // 4)
        for rule in ("signadam", "sgd"):
            for np_ in (2, 3, 4):
                grid.append((f"k_fm_pair_online<{lpr}, 0, {rule_id[rule]}, {np_}>", "pair", kp, rule, np_ * slots))
    grid += [(f"k_fm_online<1, 0, {rule_id[r]}, 1>", "fm", 4, r, 39) for r in ("signadam", "sgd")]
    grid += [("k_fm_online<4, 0, 1, 3>", "fm", 16, "sgd", 39)]      # (kp = 16 under signadam is the control below)
    grid += [(f"k_fm_online<16, 0, {rule_id[r]}, 4>", "fm", 64, r, 16) for r in ("signadam", "sgd")]
    grid += [("control k_fm_online<4, 0, 0, 3>", "fm", 16, "signadam", 39), ("control k_fm_pair_online<4, 2, 4, 3>", "pair", 16, "adam", 39)]
    return grid


def child_walkers(args):
    import numpy as np
    import torch
    import fmx
    torch.cuda.set_device(0)
    n = args.pairs
    res = {}
    for name, kind, kp, rule, F in walker_grid():
        sizes = [2000] * F
        t = fmx.FlatTable(sizes, kp, layout=LAYOUT[rule] if rule in LAYOUT else "weights")
        g = torch.Generator(device="cuda").manual_seed(SEED)
        t.rows[:, :kp] = torch.randn((t.n_rows, kp), generator=g, device="cuda") * 0.01
        e = fmx.FMEngine(t, max_batch=64)
        h = fmx.Hyper(**HYPER)
        if kind == "pair":
            rows = torch.from_numpy(pair_pool(np, sizes, 1, n, SEED + 2)[0]).cuda()
            fn = lambda: e.pair_online_run(h, rule, rows, None, margin=0.0)
        else:
            rng = np.random.default_rng(SEED + 3)
            rows = torch.from_numpy(np.stack([rng.integers(0, s, size=n) for s in sizes], axis=1).astype(np.int32)).cuda()
            y = torch.from_numpy((rng.uniform(size=n) < 0.3).astype(np.float32)).cuda()
            fn = lambda: e.online_run(h, rule, "logits", rows, None, y)
        timed(torch, fn)                                         # warm
        secs = [timed(torch, fn) for _ in range(args.reps)]
        e.check_error_flag()
        res[name] = dict(us_per_item=round(median(secs) / n * 1e6, 4), table_sum=float(t.rows.double().sum().item()),
                         finite=bool(torch.isfinite(t.rows).all()))
        del e, t, rows
    print("RESULT " + json.dumps(res), flush=True)


def main_ab(args):
    libs = (("other", os.path.abspath(args.ab_lib)), ("this", ""))
    if args.ab_this_first:
        libs = libs[::-1]
    runs = {"other": [], "this": []}
    for r in range(args.ab_rounds):
        for side, lib in libs:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "walkers", "--reps", str(args.reps), "--pairs", str(args.pairs)]
            try:
                p = subprocess.run(cmd, env=dict(os.environ, FMX_LIB_PATH=lib), capture_output=True, text=True, timeout=args.timeout)
            except subprocess.TimeoutExpired:
                print(f"{side}, round {r}: no result within {args.timeout} s; stopping", flush=True)
                return 1
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                print(f"{side}, round {r}: exit status {p.returncode}; stopping\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}", flush=True)
                return 1
            runs[side].append(json.loads(line[-1][len("RESULT "):]))
            print(side, r, "done", flush=True)
    table, slower = {}, []
    for name, kind, kp, rule, F in walker_grid():
        a = [x[name]["us_per_item"] for x in runs["other"]]
        b = [x[name]["us_per_item"] for x in runs["this"]]
        spread, diff = max(a) - min(a), median(b) - median(a)
        sums = {x[name]["table_sum"] for x in runs["other"] + runs["this"]}
        row = dict(kp=kp, rule=rule, fields=F, other_us_per_item=a, this_us_per_item=b, other_median=median(a), this_median=median(b),
                   other_spread=round(spread, 4), this_minus_other=round(diff, 4), percent=round(100 * diff / median(a), 2),
                   not_slower_than_twice_other_spread=bool(diff <= 2 * spread), faster_by_more_than_twice_other_spread=bool(-diff > 2 * spread),
                   same_table_sum=len(sums) == 1, finite=all(x[name]["finite"] for x in runs["other"] + runs["this"]))
        if not (row["not_slower_than_twice_other_spread"] and row["same_table_sum"] and row["finite"]):
            slower.append(name)
        table[name] = row
        print(name, json.dumps(row), flush=True)
    with open(args.out, "w") as fh:
        json.dump(dict(what="us per item (pair or sample) of fmx_fm_pair_online_run / fmx_fm_online_run per kernel instantiation: this tree's "
                            "library (this) against another build of the same ABI (other), fresh processes alternating other, this; each "
                            "figure the median of reps calls of `items` items after a warm call; spread = max - min over other's processes",
                       items=args.pairs, reps=args.reps, rounds=args.ab_rounds, rows_per_field=2000, instantiations=table,
                       slower_or_different=slower), fh, indent=1)
        fh.write("\n")
    if slower:
        print(f"slower than twice the other build's spread, or other results: {slower}", flush=True)
        return 1
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-pairs", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=4000, help="steps per timed call of the batched loops")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pairs", type=int, default=16384, help="pairs per call of fmx_fm_pair_online_run")
    ap.add_argument("--loop-pairs", type=int, default=2000, help="pairs per call of the fmx_fm_pair_step loop")
    ap.add_argument("--timeout", type=int, default=200, help="seconds per child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_times.json"))
    ap.add_argument("--ab-lib", default=None, help="time the walkers' instantiations against this build of the same ABI (see above)")
    ap.add_argument("--ab-rounds", type=int, default=3)
    ap.add_argument("--ab-this-first", action="store_true", help="with --ab-lib: start each round with this tree's library")
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        return {"batched": child_batched, "online": child_online, "walkers": child_walkers}[args.child](args)
    if args.ab_lib:
        return main_ab(args)
    out = dict(what="the pair loss next to the pointwise one on the Criteo-39 table (1 M x 16): us/step of the batched streams, "
                    "pairs/s of the online loop; medians of reps calls after one warm call")
    for part in ("batched", "online"):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", part, "--batch-pairs", str(args.batch_pairs), "--steps", str(args.steps),
               "--reps", str(args.reps), "--pairs", str(args.pairs), "--loop-pairs", str(args.loop_pairs)]
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
