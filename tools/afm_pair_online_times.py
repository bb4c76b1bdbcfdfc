"""Times the AFM's online PAIR loop on a criteo39-shaped model (a 1 M x 16 table over 39 fields, k = 16) for attention sizes t in
{4, 16} under the rules adam and signadam (--settings kp64: F = 64, k = 33, t = 7 under ftrl with signadam on the attention
parameters, the shape at which a thread holds two slots of kp = 64), on one stream of N pairs in one process:

    one_workgroup   fmx_afm_pair_online_run (k_afm_pair_online: one workgroup walks the stream)
    queued          fmx_afm_pair_online_run with fmx_set_option("afm_pair_online_persistent", 0): the pair steps' launches, queued
    ctypes_loop     N calls of fmx_afm_pair_step_opt(B_pairs = 1, inv_b = 1) through ctypes, the step counts advanced by the caller
    pointwise       fmx_afm_online_run on the same 2 N rows as single samples, for scale (per ROW; two rows make a pair)
    parent          --parent-lib: fmx_afm_pair_online_run of another build of the library (the commit before the one-workgroup
                    form), loaded beside this one and timed in the same process on the same buffers -- the yardstick of the gate

Each is one warm call and --runs timed calls (wall time around a device synchronisation), the forms timed in turn within each round
(--order: whether the parent or this build goes first in a round);
per-pair median, p10 and p90 in microseconds and pairs/s are printed as one JSON line per (t, rule) and written to the file given with --out.  The gate of a line:
the one-workgroup form's p10 in pairs/s (its p90 in microseconds) lies above the parent's p90 in pairs/s (its p10 in microseconds).

    python tools/afm_pair_online_times.py --parent-lib <parent build>/libfmx.so --out profiles/afm_pair_online_times.json
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
    med, p10, p90 = float(np.median(us)), float(np.percentile(us, 10)), float(np.percentile(us, 90))
    return dict(median_us=round(med, 2), p10_us=round(p10, 2), p90_us=round(p90, 2), pairs_per_s=round(1e6 / med, 1),
                pairs_per_s_p10=round(1e6 / p90, 1), pairs_per_s_p90=round(1e6 / p10, 1))


def timed_in_turn(forms, runs):
    """forms: {name: (fn, N)}.  One warm call of each, then `runs` rounds that time every form once, in turn, so that a drift of
    the machine falls on all of them alike -> {name: stats of the per-pair times}."""
    for fn, _ in forms.values():
        fn()
    torch.cuda.synchronize()
    out = {name: [] for name in forms}
    for _ in range(runs):
        for name, (fn, N) in forms.items():
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
    ap.add_argument("--pairs", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--margin", type=float, default=0.0)
    ap.add_argument("--parent-lib", default=None, help="libfmx.so of the parent commit: its fmx_afm_pair_online_run is the yardstick")
    ap.add_argument("--order", choices=("parent-first", "head-first"), default="head-first",
                    help="which of the parent and this build is timed first in a round")
    ap.add_argument("--settings", choices=("criteo39", "kp64", "all"), default="criteo39")
    ap.add_argument("--only", default="", help="comma-separated forms to time (default: all)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    only = set(filter(None, args.only.split(",")))
    N = args.pairs
    lib = fmx._lib.load()
    parent = None
    if args.parent_lib:
        parent = C.CDLL(args.parent_lib)
        parent.fmx_afm_pair_online_run.argtypes = lib.fmx_afm_pair_online_run.argtypes
        parent.fmx_afm_pair_online_run.restype = C.c_int
    lines = []
    for F, k, t, rule, arule in {"criteo39": CRITEO39, "kp64": KP64, "all": CRITEO39 + KP64}[args.settings]:
        sizes = [1_000_000 // F] * F
        rng = np.random.default_rng(0)
        pos = np.stack([rng.integers(0, s, size=N) for s in sizes], axis=1).astype(np.int32)
        neg = pos.copy()                                     # the negative: another item (the last field), the context kept
        neg[:, -1] = (pos[:, -1] + 1 + rng.integers(0, sizes[-1] - 1, size=N)) % sizes[-1]
        idx = np.empty((2 * N, F), np.int32)
        idx[0::2], idx[1::2] = pos, neg
        y = np.tile(np.array([1.0, 0.0], np.float32), N)
        tb = fmx.FlatTable(sizes, k, layout=LAYOUT[rule])
        tb.rows[:, :k] = torch.randn(tb.rows.shape[0], k, device="cuda") * 0.1
        params = (torch.randn(t * k + 2 * t + k, device="cuda") * 0.3).contiguous()
        eng = AFMEngine(tb, params, t, max_batch=64)
        opt = AfmOpt(params.numel(), arule, lr=1e-4, device="cuda")
        hyper = fmx.Hyper(lr=1e-4)
        idx_d, _, y_d = eng.to_device(idx, None, y)
        logits = torch.empty(2 * N, device="cuda")
        nb, mom = eng.pair_online_form(arule)
        assert nb > 0, "the shape does not take the one-workgroup form"

        def run():
            eng.pair_online_run(hyper, rule, idx_d, None, opt, margin=args.margin, logits=logits)

        def raw(fn_lib):       # fmx_afm_pair_online_run of `fn_lib` on the engine's buffers
            hyper.c.step = tb.step
            rc = fn_lib.fmx_afm_pair_online_run(tb.c_struct(), hyper.ref(), fmx._lib.RULES[rule], C.byref(eng.c_afm), idx_d.data_ptr(),
                                                None, N, args.margin, eng.workspace.data_ptr(), eng.workspace.numel() * 4,
                                                eng.grad.data_ptr(), opt.ref(), logits.data_ptr(), None, eng.error.data_ptr(), None)
            assert rc == 0, rc
            opt.step += N
            if tb.layout == "moments":
                tb.step += N

        def raw_loop():        # one-pair steps without the engine's Python around them: ctypes alone
            st, h, r, afm, ws, nbytes = tb.c_struct(), hyper.ref(), fmx._lib.RULES[rule], C.byref(eng.c_afm), eng.workspace.data_ptr(), \
                eng.workspace.numel() * 4
            ip, g, lg, lo, er = idx_d.data_ptr(), eng.grad.data_ptr(), eng.logit.data_ptr(), eng.loss_out.data_ptr(), eng.error.data_ptr()
            step0, tstep0 = opt.step, tb.step
            for i in range(N):
                opt.c.step = step0 + i
                hyper.c.step = tstep0 + i
                lib.fmx_afm_pair_step_opt(st, h, r, afm, ip + 8 * F * i, None, 1, args.margin, 1.0, ws, nbytes, g, C.byref(opt.c), lg, lo, er, None)
            opt.step += N
            if tb.layout == "moments":
                tb.step += N

        def pointwise():
            eng.online_run(hyper, rule, idx_d, None, y_d, opt, logits=logits)

        line = dict(F=F, k=k, t=t, rule=rule, attn_rule=arule, pairs=N, runs=args.runs, margin=args.margin, table_rows=int(tb.rows.shape[0]),
                    tile_buffers=nb, moments_in_lds=mom)
        def queued():
            lib.fmx_set_option(b"afm_pair_online_persistent", 0)
            try:
                run()
            finally:
                lib.fmx_set_option(b"afm_pair_online_persistent", 1)

        forms = dict(one_workgroup=(run, N), queued=(queued, N), ctypes_loop=(raw_loop, N), pointwise=(pointwise, 2 * N))
        if parent is not None:
            yardstick = dict(parent=(lambda: raw(parent), N))
            forms = {**yardstick, **forms} if args.order == "parent-first" else {**forms, **yardstick}
            line["order"] = args.order
        line.update(timed_in_turn({name: f for name, f in forms.items() if not only or name in only}, args.runs))
        if "pointwise" in line:
            pw = line.pop("pointwise")
            line["pointwise_per_row"] = dict(median_us=pw["median_us"], p10_us=pw["p10_us"], p90_us=pw["p90_us"],
                                             rows_per_s=pw["pairs_per_s"])
        assert int(eng.error.item()) == 0
        one = line.get("one_workgroup")
        if one:
            for other in ("queued", "ctypes_loop", "parent"):
                if other in line:
                    line[f"speedup_over_{other}"] = round(line[other]["median_us"] / one["median_us"], 2)
            if "parent" in line:
                line["gate_p10_above_parent_p90"] = bool(one["pairs_per_s_p10"] > line["parent"]["pairs_per_s_p90"])
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
