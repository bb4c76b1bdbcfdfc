"""Times the AFM's list step next to the pair step on the same positives and negatives, and next to the pointwise step and forward it
is built from, at Criteo-39 (a 1 M x 16 table over 39 fields) under signadam, for attention sizes t in {4, 16} and 2,048 lists of
G in {2, 4, 8, 16} rows, in one process:

    list      fmx_afm_list_step_opt: 2,048 G rows per step (fmx_afm_list_stream over a pool of one batch)
    pair      fmx_afm_pair_step_opt on the same positives and negatives laid out as 2,048 (G - 1) pairs, i.e. 4,096 (G - 1) rows per
              step.  Where that exceeds the sort's 32,768 rows (G = 16: 61,440) the pairs of a step are split into the fewest equal
              calls that fit and their times are summed (pair_calls says how many)
    bce       fmx_afm_step_opt on the list batch's own 2,048 G rows with arbitrary labels
    forward   fmx_afm_forward on those rows

A sample is --steps steps of one series between two device events, divided by --steps; the four series are taken in turn, --reps
times each after a warm call, so that they see the same machine state.  Reported per (t, G): the median, p10 and p90 us/step of each;
the list step against (a) the pair form -- list_over_pair, and the gate the FM list work used, list p90 < pair p10 (read at
G = 8) -- and against (b) what it is by construction, expected = bce + (G - 1) / G forward (every negative's forward runs twice):
excess_us = list - expected, spreads_us = the p90 - p10 of the two sides added, excess_in_spreads their quotient.

The online form (G = 8): lists/s of fmx_afm_list_online_run against a ctypes loop of fmx_afm_list_step_opt(B_lists = 1) -- the run is
that queue of launches issued from one call, so the two are expected to be equal -- wall time around a device synchronisation.

    python tools/afm_list_times.py [--out profiles/afm_list_times.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fm-for-online-recommendation_amd")]

import fmx  # noqa: E402
from fmx.afm import AFMEngine, AfmOpt  # noqa: E402

F, K, LISTS, RULE, MAX_SORT_ROWS = 39, 16, 2048, "signadam", 32768
GS = (2, 4, 8, 16)


def window_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0


def alternate(fns, reps, steps):
    """{name: [us per step] * reps}: a warm call of each, then reps rounds of one timed window each, in turn"""
    for fn in fns.values():
        fn()
    out = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            out[name].append(window_us(fn) / steps)
    return out


def summary(us):
    return dict(median_us=round(float(np.median(us)), 1), p10_us=round(float(np.percentile(us, 10)), 1),
                p90_us=round(float(np.percentile(us, 90)), 1))


def wall_per_item_us(fn, runs, n):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6 / n)
    return float(np.median(out))


def pair_calls(n_pairs):
    """the fewest equal calls whose 2 * pairs rows fit the sort"""
    return next(c for c in range(1, n_pairs + 1) if n_pairs % c == 0 and 2 * (n_pairs // c) <= MAX_SORT_ROWS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--steps", type=int, default=10, help="steps per timed window")
    ap.add_argument("--online-lists", type=int, default=1000)
    ap.add_argument("--online-runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "afm_list_times.json"))
    args = ap.parse_args()
    sizes = [1_000_000 // F] * F
    rng = np.random.default_rng(0)
    lib = fmx._lib.load()
    res = dict(what="the AFM list step next to the pair step on the same positives and negatives and next to the pointwise step and "
                    "forward on the same rows, Criteo-39 table (1 M x 16), signadam: us/step; median, p10 and p90 of reps windows of "
                    "`steps` steps after one warm call, the series taken in turn",
               F=F, k=K, rule=RULE, lists=LISTS, reps=args.reps, steps=args.steps)
    for t in (4, 16):
        tb = fmx.FlatTable(sizes, K)
        tb.rows[:, :K] = torch.randn(tb.rows.shape[0], K, device="cuda") * 0.1
        params = (torch.randn(t * K + 2 * t + K, device="cuda") * 0.3).contiguous()
        eng = AFMEngine(tb, params, t, max_batch=MAX_SORT_ROWS)
        opt = AfmOpt(params.numel(), RULE, lr=1e-4, device="cuda")
        hyper = fmx.Hyper(lr=1e-4)
        res[f"t={t}"] = {}
        for G in GS:
            pos = torch.from_numpy(np.stack([rng.integers(0, s, size=LISTS) for s in sizes], axis=1).astype(np.int32)).cuda()
            neg = torch.from_numpy((pos[:, -1:].cpu().numpy() + 1 + rng.integers(0, sizes[-1] - 1, size=(LISTS, G - 1))) % sizes[-1])
            neg = neg.reshape(LISTS, G - 1, 1).cuda()
            rows_l, _ = fmx.pairwise.assemble_lists(pos, None, [F - 1], neg)
            rows_p, _ = fmx.pairwise.assemble_pairs(pos, None, [F - 1], neg)
            n_pairs = LISTS * (G - 1)
            calls = pair_calls(n_pairs)
            per = n_pairs // calls
            pools_p = [rows_p[2 * per * c:2 * per * (c + 1)].contiguous() for c in range(calls)]
            y_d = torch.from_numpy((rng.uniform(size=LISTS * G) < 0.25).astype(np.float32)).cuda()
            S = args.steps

            def run_pairs():
                for p in pools_p:
                    eng.pair_stream(hyper, RULE, p, None, per, S, opt)

            def run_forward():
                for _ in range(S):
                    eng.forward(hyper, rows_l)

            us = alternate(dict(list=lambda: eng.list_stream(hyper, RULE, rows_l, None, LISTS, G, S, opt), pair=run_pairs,
                                bce=lambda: eng.stream(hyper, RULE, rows_l, None, y_d, LISTS * G, S, opt), forward=run_forward),
                           args.reps, S)
            eng.check_error_flag()
            s = {name: summary(v) for name, v in us.items()}
            share = (G - 1) / G
            expected = s["bce"]["median_us"] + share * s["forward"]["median_us"]
            spread = lambda n: s[n]["p90_us"] - s[n]["p10_us"]
            spreads = spread("list") + spread("bce") + share * spread("forward")
            r = dict(G=G, list_rows=LISTS * G, pair_rows=2 * n_pairs, pair_calls=calls, **s,
                     list_over_pair=round(s["list"]["median_us"] / s["pair"]["median_us"], 3),
                     gate_list_p90_below_pair_p10=bool(s["list"]["p90_us"] < s["pair"]["p10_us"]),
                     expected_us=round(expected, 1), excess_us=round(s["list"]["median_us"] - expected, 1),
                     spreads_us=round(spreads, 1), excess_in_spreads=round((s["list"]["median_us"] - expected) / max(spreads, 1e-9), 2),
                     finite=bool(torch.isfinite(tb.rows).all()) and bool(torch.isfinite(params).all()))
            res[f"t={t}"][f"G={G}"] = r
            print(t, json.dumps(r), flush=True)

        # ---- the online form, G = 8 ----
        N, G = args.online_lists, 8
        on_rows = rows_l_online(pos, rng, sizes, N, G)
        logits = torch.empty(N * G, device="cuda")

        def run():
            eng.list_online_run(hyper, RULE, on_rows, G, None, opt, logits=logits)

        def raw_loop():        # the same steps through ctypes alone, the step counts advanced by the caller
            st, h, r_, afm = tb.c_struct(), hyper.ref(), fmx._lib.RULES[RULE], C.byref(eng.c_afm)
            ws, nb = eng._list_ws.data_ptr(), eng._list_ws.numel() * 4
            ip, g, lg, lo, er = on_rows.data_ptr(), eng.grad.data_ptr(), logits.data_ptr(), eng.loss_out.data_ptr(), eng.error.data_ptr()
            step0 = opt.step
            for i in range(N):
                opt.c.step = step0 + i
                lib.fmx_afm_list_step_opt(st, h, r_, afm, ip + 4 * G * F * i, None, 1, G, 1.0, ws, nb, g, C.byref(opt.c), lg + 4 * G * i, lo,
                                          er, None)
            opt.step += N

        one, loop = wall_per_item_us(run, args.online_runs, N), wall_per_item_us(raw_loop, args.online_runs, N)
        eng.check_error_flag()
        res[f"t={t}"]["online"] = dict(G=G, lists=N, runs=args.online_runs, online_run_lists_per_s=round(1e6 / one, 1),
                                       ctypes_loop_lists_per_s=round(1e6 / loop, 1), online_run_over_ctypes_loop=round(loop / one, 3))
        print(t, json.dumps(res[f"t={t}"]["online"]), flush=True)
        del eng, tb
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


def rows_l_online(pos, rng, sizes, N, G):
    """N lists of G rows from the first N positives, their negatives redrawn"""
    p = pos[:N]
    neg = torch.from_numpy((p[:, -1:].cpu().numpy() + 1 + rng.integers(0, sizes[-1] - 1, size=(N, G - 1))) % sizes[-1])
    rows, _ = fmx.pairwise.assemble_lists(p, None, [F - 1], neg.reshape(N, G - 1, 1).cuda())
    return rows.contiguous()


if __name__ == "__main__":
    main()
