"""Times the AFM's online predict-then-fit loop on a criteo39-shaped model (a 1 M x 16 table over 39 fields, k = 16) for attention
sizes t in {4, 16} under the rules adam and signadam, three ways in one process on one stream of N samples:

    one_workgroup   fmx_afm_online_run (k_afm_online: one workgroup walks the stream)
    queued          fmx_afm_online_run with fmx_set_option("afm_online_persistent", 0): the per-sample launches, queued
    ctypes_loop     N calls of fmx_afm_step_opt(B = 1, inv_b = 1) through ctypes, the step counts advanced by the caller

Each is repeated --runs times (wall time around a device synchronisation); per-sample median, p10 and p90 in microseconds and
samples/s are printed as one JSON line per (t, rule) and written to the file given with --out.

    python tools/afm_online_times.py --out profiles/afm_online_times.json
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


def stats(us):
    us = np.asarray(us)
    med = float(np.median(us))
    return dict(median_us=round(med, 2), p10_us=round(float(np.percentile(us, 10)), 2), p90_us=round(float(np.percentile(us, 90)), 2),
                samples_per_s=round(1e6 / med, 1))


def timed(fn, runs, N, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6 / N)
    return stats(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    F, k, N = 39, 16, args.samples
    sizes = [1_000_000 // F] * F
    rng = np.random.default_rng(0)
    idx = np.stack([rng.integers(0, s, size=N) for s in sizes], axis=1).astype(np.int32)
    y = (rng.uniform(size=N) < 0.25).astype(np.float32)
    lib = fmx._lib.load()
    lines = []
    for t in (4, 16):
        for rule in ("adam", "signadam"):
            tb = fmx.FlatTable(sizes, k, layout="moments" if rule == "adam" else "weights")
            tb.rows[:, :k] = torch.randn(tb.rows.shape[0], k, device="cuda") * 0.1
            params = (torch.randn(t * k + 2 * t + k, device="cuda") * 0.3).contiguous()
            eng = AFMEngine(tb, params, t, max_batch=64)
            opt = AfmOpt(params.numel(), rule, lr=1e-4, device="cuda")
            hyper = fmx.Hyper(lr=1e-4)
            idx_d, _, y_d = eng.to_device(idx, None, y)
            logits = torch.empty(N, device="cuda")

            def run():
                eng.online_run(hyper, rule, idx_d, None, y_d, opt, logits=logits)

            def raw_loop():        # the same calls without the engine's Python around them: ctypes alone
                st, h, r, afm, ws, nb = tb.c_struct(), hyper.ref(), fmx._lib.RULES[rule], C.byref(eng.c_afm), eng.workspace.data_ptr(), \
                    eng.workspace.numel() * 4
                ip, yp, g, lo, er = idx_d.data_ptr(), y_d.data_ptr(), eng.grad.data_ptr(), eng.loss_out.data_ptr(), eng.error.data_ptr()
                step0, tstep0 = opt.step, tb.step
                for i in range(N):
                    opt.c.step = step0 + i
                    hyper.c.step = tstep0 + i
                    lib.fmx_afm_step_opt(st, h, r, afm, ip + 4 * F * i, None, yp + 4 * i, 1, 1.0, ws, nb, g, C.byref(opt.c), lo, er, None)
                opt.step += N
                if tb.layout == "moments":
                    tb.step += N

            one = timed(run, args.runs, N)
            lib.fmx_set_option(b"afm_online_persistent", 0)
            try:
                queued = timed(run, args.runs, N)
            finally:
                lib.fmx_set_option(b"afm_online_persistent", 1)
            ctl = timed(raw_loop, args.runs, N)
            assert int(eng.error.item()) == 0
            line = dict(F=F, k=k, t=t, rule=rule, samples=N, runs=args.runs, table_rows=int(tb.rows.shape[0]), one_workgroup=one,
                        queued=queued, ctypes_loop=ctl, speedup_over_queued=round(queued["median_us"] / one["median_us"], 2),
                        speedup_over_ctypes_loop=round(ctl["median_us"] / one["median_us"], 2),
                        p90_below_both_p10=bool(one["p90_us"] < min(queued["p10_us"], ctl["p10_us"])))
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
