"""Microseconds per step of the online loop (fmx_fm_stream) under each of the five update rules.

bench.py's configs[1]+[2] shape: the synthetic Criteo-39 table (1,006,628 rows), k = 16, B = 4,096, a resident pool of 16
batches; and the same fields at 8 x the rows (8,053,024 rows: 2 GB in the FTRL / moments layout), a table far beyond the
256 MB Infinity Cache, so that every row comes from HBM.  Each rule runs on the layout it pairs with:
  signadam, sgd   weights layout  (row 128 B: V | w)
  ftrl            ftrl layout     (row 256 B: V | w, z, n | zV | nV)
  adagrad, adam   moments layout  (row 256 B: V | w, m, v | mV | vV; adagrad neither reads nor writes the m half)
Per (table, rule): the production loop timed with device events over --steps steps after --warmup (us per step), then the
measuring mode of fmx_fm_stream (per-launch sort / forward / update times, see include/fmx.h).
  python tools/rule_times.py [--steps N] [--warmup W] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fm-for-online-recommendation_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import fmx  # noqa: E402

RULES = [("signadam", "weights"), ("sgd", "weights"), ("ftrl", "ftrl"), ("adagrad", "moments"), ("adam", "moments")]


def make_table(sizes, layout):
    dev = torch.device("cuda")
    t = fmx.FlatTable(sizes, bench.K_EMB, layout=layout, device=dev, ftrl=bench.HYPER)
    g = torch.Generator(device=dev).manual_seed(1)
    V = torch.randn((t.n_rows, bench.K_EMB), device=dev, generator=g) * 0.01
    if layout == "ftrl":
        t.rows[:, t.z_offset:t.z_offset + bench.K_EMB] = fmx.table.ftrl_z_for_weight_torch(V, t.ftrl)
    t.rows[:, :bench.K_EMB] = V
    return t


def time_rule(sizes, rule, layout, idx_pool, y_pool, steps, warmup):
    t = make_table(sizes, layout)
    eng = fmx.FMEngine(t, max_batch=bench.BATCH)
    hyp = fmx.Hyper(lr=1e-3, eps=1e-8, alpha=bench.HYPER["alpha"], beta=bench.HYPER["beta"], l1=bench.HYPER["l1"], l2=bench.HYPER["l2"])
    st = torch.cuda.current_stream()
    eng.stream(hyp, rule, "logits", idx_pool, y_pool, warmup)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    eng.stream(hyp, rule, "logits", idx_pool, y_pool, steps)
    b.record(st)
    torch.cuda.synchronize()
    us_step = a.elapsed_time(b) * 1e3 / steps
    ms = eng.stream(hyp, rule, "logits", idx_pool, y_pool, min(steps, 64), timed=True)
    n = min(steps, 64)
    res = dict(rule=rule, layout=layout, rows=t.n_rows, row_bytes=4 * t.row_stride, us_per_step=round(us_step, 2),
               kernel_us=dict(sort_per_launch_of_8_batches=round(ms[0] * 1e3 / n, 2), forward=round(ms[1] * 1e3 / n, 2),
                              update=round(ms[2] * 1e3 / n, 2)))
    eng.check_error_flag()
    if not np.isfinite(t.rows[:1024].float().cpu().numpy()).all():
        res["warning"] = "non-finite values in the table"
    del eng, t
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    out = dict(what="fmx_fm_stream us per step by update rule", B=bench.BATCH, k=bench.K_EMB, n_pool=bench.N_POOL,
               steps=args.steps, warmup=args.warmup, device=torch.cuda.get_device_name(0), tables=[])
    for name, scale in (("criteo39 (configs[1]+[2])", 1), ("criteo39 x 8 rows (HBM-resident)", 8)):
        sizes = [s * scale for s in bench.CRITEO_SIZES]
        idx_np, y_np = bench.synth_pool(bench.N_POOL, bench.BATCH, sizes, bench.SEED + 1)
        idx_pool, y_pool = torch.from_numpy(idx_np).cuda(), torch.from_numpy(y_np).cuda()
        rows = []
        for rule, layout in RULES:
            r = time_rule(sizes, rule, layout, idx_pool, y_pool, args.steps, args.warmup)
            print(json.dumps(dict(table=name, **r)), flush=True)
            rows.append(r)
        out["tables"].append(dict(table=name, rows_total=int(sum(sizes)), results=rows))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
