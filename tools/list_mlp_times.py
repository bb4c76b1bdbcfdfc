"""What the list loss costs DeepFM next to the pair and the pointwise one, on the Criteo-39 table (1 M rows x 16) at 2,048 lists
per step, with the 3 x 256 and the 3 x 64 network, under signadam tables with an sgd network and adam tables with an adam network.

Per list size G = 2 / 4 / 8 / 16 (2,048 G rows per step), timed alternately in one process, --reps times each after a warm call:
  list            fmx_deepfm_list_stream on the lists
  pair            fmx_deepfm_pair_stream on the same positives and negatives as (G - 1) 2,048 pairs -- 2 (G - 1) 2,048 rows; where
                  they exceed one exact step (32,768 rows: G = 16), two calls of half the pairs each, summed
  point           fmx_deepfm_stream on the list's own rows with arbitrary labels: the list stream minus its loss site, and -- at
                  3 x 256 -- with k_mlp_chain where the list section runs the separate GEMM launches
  point_no_chain  (3 x 256 only) the same under mlp_chain = 0: the separate GEMM launches on both sides, so list - point_no_chain
                  is the list loss site alone and point_no_chain - point is what the missing chain kernel costs
Reported per series: the median us/step with p10 and p90 of the reps; per G the gate "list p90 < pair p10" as met or missed.
Each (network, rules) setting runs in a child process of its own under a time limit; the first that fails ends the run.  Writes
profiles/list_mlp_times.json.
  python tools/list_mlp_times.py [--steps N] [--reps R] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys

from pair_times import HYPER, K, ROOT, SEED, criteo_sizes, median, new_table, timed

LISTS, LAYERS, N_POOL, MAX_ROWS = 2048, 3, 4, 32768
GS = (2, 4, 8, 16)
HIDDENS = (256, 64)
SETTINGS = (("signadam", "sgd"), ("adam", "adam"))


def list_pool(np, sizes, n_pool, B, G, seed):
    """[n_pool, B G, F] int32: a list's negatives are its positive with the largest field (the item) redrawn"""
    rng = np.random.default_rng(seed)
    item = int(np.argmax(sizes))
    pos = np.stack([rng.integers(0, s, size=(n_pool, B)) for s in sizes], axis=2)
    rows = np.repeat(pos[:, :, None, :], G, axis=2)
    rows[:, :, 1:, item] = (pos[:, :, None, item] + 1 + rng.integers(0, sizes[item] - 1, size=(n_pool, B, G - 1))) % sizes[item]
    return rows.reshape(n_pool, B * G, len(sizes)).astype(np.int32)


def pairs_of(np, lists, B, G):
    """the lists' positives and negatives as (G - 1) B pairs: [n_pool, 2 (G - 1) B, F], pair (b, j) = (positive b, negative j of b)"""
    n_pool, _, F = lists.shape
    l4 = lists.reshape(n_pool, B, G, F)
    pairs = np.empty((n_pool, B, G - 1, 2, F), np.int32)
    pairs[:, :, :, 0] = l4[:, :, :1]
    pairs[:, :, :, 1] = l4[:, :, 1:]
    return pairs.reshape(n_pool, 2 * (G - 1) * B, F)


def pct(v, q):
    s = sorted(v)
    return s[int(round(q * (len(s) - 1)))]


def child(args):
    import numpy as np
    import torch
    import fmx
    torch.cuda.set_device(0)
    lib = fmx._lib.load()
    sizes, B, H = criteo_sizes(), args.lists, args.hidden
    rule, net_rule = args.rule, args.net_rule
    n_par = sum(H * (K if l == 0 else H) + H for l in range(LAYERS))
    res = dict(lists_per_step=B, steps_per_call=args.steps, reps=args.reps, table_rows=int(sum(sizes)), k=K, hidden=H, layers=LAYERS,
               rule=rule, net_rule=net_rule)

    def side():
        t = new_table(fmx, torch, sizes, rule)
        g = torch.Generator(device="cuda").manual_seed(SEED + 2)
        params = torch.randn(n_par, generator=g, device="cuda") * (0.5 / H ** 0.5)
        opt = None if net_rule == "sgd" else fmx.MlpOpt(n_par, net_rule, lr=0.001, device="cuda")
        return t, fmx.Hyper(**HYPER), params, torch.zeros_like(params), opt

    for G in GS:
        rows = B * G
        lists_h = list_pool(np, sizes, N_POOL, B, G, SEED + G)
        lists = torch.from_numpy(lists_h).cuda()
        pairs_h = pairs_of(np, lists_h, B, G)
        halves = 2 if pairs_h.shape[1] > MAX_ROWS else 1
        cut = pairs_h.shape[1] // halves
        pair_pools = [torch.from_numpy(np.ascontiguousarray(pairs_h[:, i * cut:(i + 1) * cut])).cuda() for i in range(halves)]
        y = torch.from_numpy((np.random.default_rng(SEED + 1).uniform(size=(N_POOL, rows)) < 0.3).astype(np.float32)).cuda()
        run, keep = {}, {}
        t, h, params, grads, opt = keep.setdefault("list", side())
        run["list"] = fmx.FMEngine(t, max_batch=rows).prepare_deepfm_list_stream(h, rule, params, grads, K, H, LAYERS, 0.001, lists, G, mlp_opt=opt)
        t, h, params, grads, opt = keep.setdefault("pair", side())
        e = fmx.FMEngine(t, max_batch=cut)
        pair_runs = [e.prepare_deepfm_pair_stream(h, rule, params, grads, K, H, LAYERS, 0.001, p, margin=0.0, mlp_opt=opt) for p in pair_pools]
        run["pair"] = lambda n: [r(n) for r in pair_runs]
        t, h, params, grads, opt = keep.setdefault("point", side())
        point = fmx.FMEngine(t, max_batch=rows).prepare_deepfm_stream(h, rule, "logits", params, grads, K, H, LAYERS, 0.001, lists, y, mlp_opt=opt)
        run["point"] = point
        if H == 256:
            def no_chain(n, point=point):
                prev = lib.fmx_set_option(b"mlp_chain", 0)
                try:
                    point(n)
                finally:
                    lib.fmx_set_option(b"mlp_chain", prev)
            run["point_no_chain"] = no_chain
        series = tuple(run)
        for n in series:
            timed(torch, lambda: run[n](args.steps))             # warm: code objects, allocations, the side stream
        us = {n: [] for n in series}
        for _ in range(args.reps):                               # alternating, in one process
            for n in series:
                us[n].append(timed(torch, lambda: run[n](args.steps)) / args.steps * 1e6)
        r = dict(rows_per_step=rows, pair_rows_per_step=int(pairs_h.shape[1]), pair_calls_per_step=halves)
        for n in series:
            r[n] = dict(us_per_step=round(median(us[n]), 3), p10=round(pct(us[n], 0.1), 3), p90=round(pct(us[n], 0.9), 3),
                        reps_us=[round(v, 3) for v in us[n]])
        r["gate_list_p90_below_pair_p10"] = "met" if r["list"]["p90"] < r["pair"]["p10"] else "missed"
        r["list_minus_point_us"] = round(r["list"]["us_per_step"] - r["point"]["us_per_step"], 3)
        if H == 256:
            r["list_loss_site_us"] = round(r["list"]["us_per_step"] - r["point_no_chain"]["us_per_step"], 3)
            r["no_chain_kernel_us"] = round(r["point_no_chain"]["us_per_step"] - r["point"]["us_per_step"], 3)
        r["finite"] = all(bool(torch.isfinite(k_[0].rows).all()) and bool(torch.isfinite(k_[2]).all()) for k_ in keep.values())
        res[f"G{G}"] = r
        if not r["finite"]:                                      # a run that left non-finite tables or parameters is a failed run
            print(f"G = {G}: non-finite table rows or network parameters after the timed calls; stopping\n" + json.dumps(r), flush=True)
            return 1
        del run, keep, pair_runs, point, lists, pair_pools, y
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lists", type=int, default=LISTS)
    ap.add_argument("--steps", type=int, default=100, help="steps per timed call of the streams")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "list_mlp_times.json"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--rule", default="signadam")
    ap.add_argument("--net-rule", default="sgd")
    args = ap.parse_args()
    if args.child:
        return child(args)
    out = dict(what="the list loss next to the pair and the pointwise one for DeepFM (Criteo-39 table 1 M x 16, 2,048 lists per step): "
                    "us/step of the streams, medians of reps timed calls after one warm call, with p10 and p90")
    for H in HIDDENS:
        for rule, net_rule in SETTINGS:
            name = f"{LAYERS}x{H}_{rule}_{net_rule}"
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--hidden", str(H), "--rule", rule, "--net-rule", net_rule,
                   "--lists", str(args.lists), "--steps", str(args.steps), "--reps", str(args.reps)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
            except subprocess.TimeoutExpired:
                print(f"{name}: no result within {args.timeout} s; stopping", flush=True)
                return 1
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                print(f"{name}: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}", flush=True)
                return 1
            out[name] = json.loads(line[-1][len("RESULT "):])
            print(name, json.dumps(out[name]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
