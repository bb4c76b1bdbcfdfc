"""Times of hard-negative mining (fmx_fm_mine_negatives) at Criteo-39: a 1 M x 16 table, the largest field as the candidates
(N = 176,373), U = 2,048 positives, for (n_draw, n_neg) in {(1, 1), (32, 1), (256, 4), (1024, 16)} -- a fresh process per
setting, in each:

    kernel      (a) one fmx_fm_mine_negatives call on resident Su / au / Sc / ac (device events)
    model       (b) FMAdam.mine_negatives end to end: candidates' refresh, context side, positions_of, the call, the items and
                    its one host read (wall time around a device synchronisation)
    model_kept  (b') the same with refresh_every = 2^30: the kept candidates' sums are reused, so this is (b) without the
                    forward over the N candidate rows
    torch       (c) the torch path it replaces: sample_negatives with n_neg = n_draw, gathered Sc / ac, a batched dot, topk (wall
                    time: sample_negatives reads a count back)
    pair_step   (d) fmx_fm_pair_step at 2,048 pairs on the same table (device events)

Medians of --calls (9) timed calls after --warm (3) warm ones, with p10 / p90.  The five are timed in turn, so they see the same
machine state.  One JSON line per setting, written to the file given with --out.

    python tools/mine_times.py --out profiles/mine_times.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fm-for-online-recommendation_amd")]

SETTINGS = [(1, 1), (32, 1), (256, 4), (1024, 16)]
U = 2048
K_EMB = 16


def stats(us):
    import numpy as np
    return dict(median_us=round(float(np.median(us)), 1), p10_us=round(float(np.percentile(us, 10)), 1),
                p90_us=round(float(np.percentile(us, 90)), 1))


def child(n_draw, n_neg, warm, calls):
    import numpy as np
    import torch

    import bench
    import fmx
    from fmx import pairwise as pw
    from fmx import recommend as rec
    from models.models_online_deep.fm_adam import FMAdam

    sizes = list(bench.CRITEO_SIZES)
    item = int(np.argmax(sizes))
    N, F = sizes[item], len(sizes)
    torch.manual_seed(0)
    m = FMAdam(sizes, embedding_size=K_EMB, n=1e-4)
    t = m._table
    rng = np.random.default_rng(0)
    Xi = torch.from_numpy(np.stack([rng.integers(0, s, U) for s in sizes], 1).astype(np.int32)).cuda()
    cands = rec.Candidates.whole_field(t, item, hyper=m._hyper)
    ctx = [f for f in range(F) if f != item]
    Su, au = rec.side_sums(t, Xi, None, ctx, m._hyper)
    own = Xi[:, item].contiguous()
    out = (torch.empty((U, n_neg), dtype=torch.int32, device="cuda"), torch.empty((U, n_neg), dtype=torch.float32, device="cuda"))
    neg = torch.from_numpy(((Xi[:, item].cpu().numpy() + 1 + rng.integers(0, N - 1, U)) % N).astype(np.int64)).cuda()
    rows, _ = pw.assemble_pairs(Xi, None, [item], neg)
    state = {"offset": 0}

    def kernel():
        state["offset"] += 1
        pw.fm_mine_negatives(Su, au, cands.Sc, cands.ac, n_draw, n_neg, own, 0, state["offset"], 0, out=out)

    def model():
        m.mine_negatives(Xi, None, [item], n_draw, n_neg=n_neg)

    def model_kept():
        m.mine_negatives(Xi, None, [item], n_draw, n_neg=n_neg, refresh_every=1 << 30)

    def torch_path():
        drawn = pw.sample_negatives(Xi, [item], [N], n_neg=n_draw)[:, :, 0]
        score = (au[:, None] + cands.ac[drawn]) + torch.bmm(cands.Sc[drawn], Su[:, :, None])[:, :, 0]
        top = torch.topk(score, n_neg, dim=1)
        return torch.gather(drawn, 1, top.indices), top.values

    def pair_step():
        m._engine.pair_step(m._hyper, m.update_rule, rows, None)

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1000.0

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6

    fns = dict(kernel=(kernel, events), model=(model, wall), model_kept=(model_kept, wall), torch=(torch_path, wall),
               pair_step=(pair_step, events))
    for _ in range(warm):
        for fn, _ in fns.values():
            fn()
    us = {name: [] for name in fns}
    for _ in range(calls):
        for name, (fn, timer) in fns.items():
            us[name].append(timer(fn))
    m._engine.check_error_flag()
    s = {name: stats(v) for name, v in us.items()}
    line = dict(table_rows=int(t.n_rows), k=K_EMB, N=N, U=U, n_draw=n_draw, n_neg=n_neg, pairs=U, warm=warm, calls=calls, **s,
                kernel_over_pair_step=round(s["kernel"]["median_us"] / s["pair_step"]["median_us"], 3),
                kernel_p90_below_pair_step_p10=bool(s["kernel"]["p90_us"] < s["pair_step"]["p10_us"]),
                torch_over_model=round(s["torch"]["median_us"] / s["model"]["median_us"], 2),
                torch_over_model_kept=round(s["torch"]["median_us"] / s["model_kept"]["median_us"], 2))
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--setting", default=None, help="n_draw,n_neg: time this one setting in this process")
    args = ap.parse_args()
    if args.setting:
        n_draw, n_neg = (int(v) for v in args.setting.split(","))
        child(n_draw, n_neg, args.warm, args.calls)
        return
    lines = []
    for n_draw, n_neg in SETTINGS:      # one after the other: never two processes on the GPU
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--setting", f"{n_draw},{n_neg}", "--calls", str(args.calls),
                            "--warm", str(args.warm)], capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit(r.returncode)
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
