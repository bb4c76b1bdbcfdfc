"""Times the AFM's pair step next to the pointwise step it is built from, at Criteo-39 (a 1 M x 16 table over 39 fields) for
attention sizes t in {4, 16}, in one process:

    pair_step   fmx_afm_pair_step_opt at 2,048 pairs (4,096 rows)
    bce_step    fmx_afm_step_opt at B = 4,096 on the pair batch's own 4,096 rows with arbitrary labels
    forward     fmx_afm_forward on those rows

Each is one timed call (device events around it), 7 times after a warm one, the three taken in turn so that they see the same
machine state; the median and the spread (max - min) of each are recorded.  By construction the pair step is the pointwise step
plus one more forward of half the rows: expected = bce_step + 0.5 forward, and `excess_over_expected_in_spreads` says how far the
measurement lies from that in units of the larger spread.

The online form: pairs/s of fmx_afm_pair_online_run against a ctypes loop of fmx_afm_pair_step_opt(B_pairs = 1), wall time around
a device synchronisation.  One JSON line per t, written to the file given with --out.

    python tools/afm_pair_times.py --out profiles/afm_pair_times.json
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


def one_call_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0


def alternate(fns, n):
    """{name: [us] * n}: a warm call of each, then n rounds of one timed call each, in turn"""
    for fn in fns.values():
        fn()
    out = {name: [] for name in fns}
    for _ in range(n):
        for name, fn in fns.items():
            out[name].append(one_call_us(fn))
    return out


def summary(us):
    return dict(median_us=round(float(np.median(us)), 1), spread_us=round(float(max(us) - min(us)), 1))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--online-pairs", type=int, default=1000)
    ap.add_argument("--online-runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    F, k, P, rule = 39, 16, 2048, "signadam"
    sizes = [1_000_000 // F] * F
    rng = np.random.default_rng(0)
    pos = np.stack([rng.integers(0, s, size=P) for s in sizes], axis=1).astype(np.int32)
    neg = rng.integers(0, sizes[-1], size=P)
    neg = np.where(neg == pos[:, -1], (neg + 1) % sizes[-1], neg)
    y = (rng.uniform(size=2 * P) < 0.25).astype(np.float32)
    lib = fmx._lib.load()
    lines = []
    for t in (4, 16):
        tb = fmx.FlatTable(sizes, k)
        tb.rows[:, :k] = torch.randn(tb.rows.shape[0], k, device="cuda") * 0.1
        params = (torch.randn(t * k + 2 * t + k, device="cuda") * 0.3).contiguous()
        eng = AFMEngine(tb, params, t, max_batch=2 * P)
        opt = AfmOpt(params.numel(), rule, lr=1e-4, device="cuda")
        hyper = fmx.Hyper(lr=1e-4)
        rows, _ = fmx.pairwise.assemble_pairs(torch.from_numpy(pos).cuda(), None, [F - 1], torch.from_numpy(neg).cuda())
        y_d = torch.from_numpy(y).cuda()
        us = alternate(dict(pair_step=lambda: eng.pair_step(hyper, rule, rows, None, opt=opt),
                            bce_step=lambda: eng.step(hyper, rule, rows, None, y_d, opt=opt),
                            forward=lambda: eng.forward(hyper, rows)), args.calls)
        s = {name: summary(v) for name, v in us.items()}
        expected = s["bce_step"]["median_us"] + 0.5 * s["forward"]["median_us"]
        spread = max(v["spread_us"] for v in s.values())
        line = dict(F=F, k=k, t=t, rule=rule, pairs=P, rows=2 * P, calls=args.calls, table_rows=int(tb.rows.shape[0]), **s,
                    expected_us=round(expected, 1), pair_over_bce=round(s["pair_step"]["median_us"] / s["bce_step"]["median_us"], 3),
                    excess_over_expected_us=round(s["pair_step"]["median_us"] - expected, 1),
                    excess_over_expected_in_spreads=round((s["pair_step"]["median_us"] - expected) / max(spread, 1e-9), 2))

        # ---- the online form ----
        N = args.online_pairs
        on_rows = rows[:2 * N].contiguous()
        logits = torch.empty(2 * N, device="cuda")

        def run():
            eng.pair_online_run(hyper, rule, on_rows, None, opt, logits=logits)

        def raw_loop():        # the same steps through ctypes alone, the step counts advanced by the caller
            st, h, r, afm, ws, nb = tb.c_struct(), hyper.ref(), fmx._lib.RULES[rule], C.byref(eng.c_afm), eng.workspace.data_ptr(), \
                eng.workspace.numel() * 4
            ip, g, lg, lo, er = on_rows.data_ptr(), eng.grad.data_ptr(), logits.data_ptr(), eng.loss_out.data_ptr(), eng.error.data_ptr()
            step0 = opt.step
            for i in range(N):
                opt.c.step = step0 + i
                lib.fmx_afm_pair_step_opt(st, h, r, afm, ip + 8 * F * i, None, 1, 0.0, 1.0, ws, nb, g, C.byref(opt.c), lg + 8 * i, lo, er, None)
            opt.step += N

        one, loop = wall_per_item_us(run, args.online_runs, N), wall_per_item_us(raw_loop, args.online_runs, N)
        assert int(eng.error.item()) == 0
        line.update(online_pairs=N, online_run_pairs_per_s=round(1e6 / one, 1), ctypes_loop_pairs_per_s=round(1e6 / loop, 1),
                    online_speedup_over_ctypes_loop=round(loop / one, 2))
        print(json.dumps(line), flush=True)
        lines.append(line)
        del eng, tb
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
