"""Times the AFM's online predict-then-fit loop on a criteo39-shaped model (a 1 M x 16 table over 39 fields, k = 16) for attention
sizes t in {4, 16} under the rules adam and signadam (--settings kp64: F = 64, k = 33, t = 7 under ftrl with signadam on the
attention parameters, the shape at which a thread holds two rows of kp = 64), in one process on one stream of N samples:

    one_workgroup   fmx_afm_online_run (k_afm_online: one workgroup walks the stream)
    queued          fmx_afm_online_run with fmx_set_option("afm_online_persistent", 0): the per-sample launches, queued
    ctypes_loop     N calls of fmx_afm_step_opt(B = 1, inv_b = 1) through ctypes, the step counts advanced by the caller
    parent          --parent-lib: fmx_afm_online_run of another build of the library (the parent commit), loaded beside this one
                    and timed in the same process on the same buffers -- the yardstick of a change to the kernel

Each is one warm call and --runs timed calls (wall time around a device synchronisation), the forms timed in turn within each
round; --order says whether the parent or this build goes first in a round.  Per-sample median, p10 and p90 in microseconds and
samples/s are printed as one JSON line per setting and written to the file given with --out.  With --only a line holds the forms
named alone, and the speedup_over_* / p90_below_both_p10 keys only where both of their forms were timed.

    python tools/afm_online_times.py --out profiles/afm_online_times.json
    python tools/afm_online_times.py --parent-lib <parent build>/libfmx.so --order parent-first --only one_workgroup,parent
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


def timed_in_turn(forms, runs, N):
    """forms: {name: fn}.  One warm call of each, then `runs` rounds that time every form once, in turn (in the dict's order), so
    that a drift of the machine falls on all of them alike -> {name: stats of the per-sample times}."""
    for fn in forms.values():
        fn()
    torch.cuda.synchronize()
    out = {name: [] for name in forms}
    for _ in range(runs):
        for name, fn in forms.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out[name].append((time.perf_counter() - t0) * 1e6 / N)
    return {name: stats(us) for name, us in out.items()}


CRITEO39 = [(39, 16, t, rule, rule) for t in (4, 16) for rule in ("adam", "signadam")]    # (F, k, t, the tables' rule, the attention's)
KP64 = [(64, 33, 7, "ftrl", "signadam")]
LAYOUT = {"adam": "moments", "signadam": "weights", "ftrl": "ftrl"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--settings", choices=("criteo39", "kp64", "all"), default="criteo39")
    ap.add_argument("--parent-lib", default=None, help="libfmx.so of the parent commit: its fmx_afm_online_run is the yardstick")
    ap.add_argument("--order", choices=("parent-first", "head-first"), default="head-first",
                    help="which of the parent and this build is timed first in a round")
    ap.add_argument("--only", default="", help="comma-separated forms to time (default: all)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    only = set(filter(None, args.only.split(",")))
    N = args.samples
    lib = fmx._lib.load()
    parent = None
    if args.parent_lib:
        parent = C.CDLL(args.parent_lib)
        parent.fmx_afm_online_run.argtypes = lib.fmx_afm_online_run.argtypes
        parent.fmx_afm_online_run.restype = C.c_int
    lines = []
    for F, k, t, rule, arule in {"criteo39": CRITEO39, "kp64": KP64, "all": CRITEO39 + KP64}[args.settings]:
        sizes = [1_000_000 // F] * F
        rng = np.random.default_rng(0)
        idx = np.stack([rng.integers(0, s, size=N) for s in sizes], axis=1).astype(np.int32)
        y = (rng.uniform(size=N) < 0.25).astype(np.float32)
        tb = fmx.FlatTable(sizes, k, layout=LAYOUT[rule])
        tb.rows[:, :k] = torch.randn(tb.rows.shape[0], k, device="cuda") * 0.1
        params = (torch.randn(t * k + 2 * t + k, device="cuda") * 0.3).contiguous()
        eng = AFMEngine(tb, params, t, max_batch=64)
        opt = AfmOpt(params.numel(), arule, lr=1e-4, device="cuda")
        hyper = fmx.Hyper(lr=1e-4)
        idx_d, _, y_d = eng.to_device(idx, None, y)
        logits = torch.empty(N, device="cuda")

        def run():
            eng.online_run(hyper, rule, idx_d, None, y_d, opt, logits=logits)

        def raw(fn_lib):       # fmx_afm_online_run of `fn_lib` on the engine's buffers
            hyper.c.step = tb.step
            rc = fn_lib.fmx_afm_online_run(tb.c_struct(), hyper.ref(), fmx._lib.RULES[rule], C.byref(eng.c_afm), idx_d.data_ptr(), None,
                                           y_d.data_ptr(), N, eng.workspace.data_ptr(), eng.workspace.numel() * 4, eng.grad.data_ptr(),
                                           opt.ref(), logits.data_ptr(), None, eng.error.data_ptr(), None)
            assert rc == 0, rc
            opt.step += N
            if tb.layout == "moments":
                tb.step += N

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

        def queued():
            lib.fmx_set_option(b"afm_online_persistent", 0)
            try:
                run()
            finally:
                lib.fmx_set_option(b"afm_online_persistent", 1)

        forms = dict(one_workgroup=run, queued=queued, ctypes_loop=raw_loop)
        if parent is not None:
            yardstick = dict(parent=lambda: raw(parent))
            forms = {**yardstick, **forms} if args.order == "parent-first" else {**forms, **yardstick}
        line = dict(F=F, k=k, t=t, rule=rule, attn_rule=arule, samples=N, runs=args.runs, table_rows=int(tb.rows.shape[0]))
        if parent is not None:
            line["order"] = args.order
        line.update(timed_in_turn({name: f for name, f in forms.items() if not only or name in only}, args.runs, N))
        assert int(eng.error.item()) == 0
        one = line.get("one_workgroup")
        if one:
            for other in ("queued", "ctypes_loop", "parent"):
                if other in line:
                    line[f"speedup_over_{other}"] = round(line[other]["median_us"] / one["median_us"], 2)
            if "queued" in line and "ctypes_loop" in line:
                line["p90_below_both_p10"] = bool(one["p90_us"] < min(line["queued"]["p10_us"], line["ctypes_loop"]["p10_us"]))
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
