"""Times of popularity-sampled negatives and the log-Q corrected list loss at Criteo-39: a 1 M x 16 table, the largest field as the
items (N = 176,373), 2,048 lists, Zipf weights (1 / rank^1.1 over a seeded permutation of the items).  One process; in each block
the variants are timed in turn, call by call, so they see the same machine state:

    step     (a) fmx_fm_list_step_q against fmx_fm_list_step on the same rows at G = 2 / 8 / 16 (device events).  From the code the
                 correction adds one 4-byte load per row to the forward; corrected_p10_above_plain_p90 says whether the difference
                 stands clear of the spread.
    sampler  (b) fmx_alias_sample_negatives at n_neg = 1 / 7 / 15, n_try = max(64, 8 n_neg), with log Q (device events), against
                 the torch path it replaces: torch.multinomial with replacement, a redraw loop for the rows that drew their own
                 item (one count read back per round), a gather of log q (wall time around a device synchronisation)
    fit      (c) FMAdam.fit_lists end to end at n_neg = 7 under uniform, popularity (corrected) and hard (n_draw = 32) negatives
                 (wall time)

Medians of --calls (9) timed calls after --warm (3) warm ones, with p10 / p90.  One JSON line per setting, written to --out.

    python tools/popularity_times.py --out profiles/popularity_times.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fm-for-online-recommendation_amd")]

LISTS = 2048
K_EMB = 16


def stats(us):
    import numpy as np
    return dict(median_us=round(float(np.median(us)), 1), p10_us=round(float(np.percentile(us, 10)), 1),
                p90_us=round(float(np.percentile(us, 90)), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import bench
    from fmx import pairwise as pw
    from models.models_online_deep.fm_adam import FMAdam

    sizes = list(bench.CRITEO_SIZES)
    item = int(np.argmax(sizes))
    N = sizes[item]
    torch.manual_seed(0)
    m = FMAdam(sizes, embedding_size=K_EMB, n=1e-4)
    e, hyp, rule = m._engine, m._hyper, m.update_rule
    rng = np.random.default_rng(0)
    Xi = torch.from_numpy(np.stack([rng.integers(0, s, LISTS) for s in sizes], 1).astype(np.int32)).cuda()
    weights = np.empty(N)
    weights[rng.permutation(N)] = 1.0 / np.arange(1, N + 1) ** 1.1
    pop = pw.PopularityNegatives(weights)
    thresh, alias, logq = pop.table("cuda")
    w_d = torch.from_numpy(weights).cuda()
    own = Xi[:, item].contiguous()
    state = {"offset": 0}

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

    def timed(fns):
        for _ in range(args.warm):
            for fn, _ in fns.values():
                fn()
        us = {name: [] for name in fns}
        for _ in range(args.calls):
            for name, (fn, timer) in fns.items():
                us[name].append(timer(fn))
        return {name: stats(v) for name, v in us.items()}

    def sample(n_neg):
        state["offset"] += 1
        return e.alias_sample(thresh, alias, logq, n_neg, pop.tries(n_neg), own, 0, state["offset"])

    lines = []
    base = dict(table_rows=int(m._table.n_rows), k=K_EMB, N=N, lists=LISTS, warm=args.warm, calls=args.calls)

    # (a) the corrected step against the plain one, the same rows
    for G in (2, 8, 16):
        neg_pos, neg_logq = sample(G - 1)
        rows, _ = pw.assemble_lists(Xi, None, [item], neg_pos.long().unsqueeze(-1))
        corr = torch.cat([logq[own.long()].clamp(min=pop.floor_logq())[:, None], neg_logq], dim=1).reshape(-1).contiguous()
        s = timed(dict(plain=(lambda: e.list_step(hyp, rule, rows, G), events),
                       corrected=(lambda: e.list_step_q(hyp, rule, rows, G, corr), events)))
        lines.append(dict(part="step", G=G, **base, **s,
                          corrected_over_plain=round(s["corrected"]["median_us"] / s["plain"]["median_us"], 3),
                          corrected_p10_above_plain_p90=bool(s["corrected"]["p10_us"] > s["plain"]["p90_us"])))

    # (b) the sampler against the torch path
    def torch_path(n_neg):
        drawn = torch.multinomial(w_d, LISTS * n_neg, replacement=True).reshape(LISTS, n_neg)
        while True:
            again = drawn == own[:, None]
            n = int(again.sum())
            if n == 0:
                break
            drawn[again] = torch.multinomial(w_d, n, replacement=True)
        return drawn, logq[drawn]

    for n_neg in (1, 7, 15):
        s = timed(dict(kernel=(lambda: sample(n_neg), events), torch=(lambda: torch_path(n_neg), wall)))
        lines.append(dict(part="sampler", n_neg=n_neg, n_try=pop.tries(n_neg), **base, **s,
                          torch_over_kernel=round(s["torch"]["median_us"] / s["kernel"]["median_us"], 2)))

    # (c) fit_lists end to end
    n_neg = 7
    s = timed(dict(uniform=(lambda: m.fit_lists(Xi, None, [item], n_neg=n_neg), wall),
                   popularity=(lambda: m.fit_lists(Xi, None, [item], negatives=pop, n_neg=n_neg), wall),
                   hard=(lambda: m.fit_lists(Xi, None, [item], negatives="hard", n_neg=n_neg), wall)))
    lines.append(dict(part="fit", n_neg=n_neg, **base, **s,
                      popularity_over_uniform=round(s["popularity"]["median_us"] / s["uniform"]["median_us"], 2),
                      popularity_over_hard=round(s["popularity"]["median_us"] / s["hard"]["median_us"], 2)))
    e.check_error_flag()

    text = "\n".join(json.dumps(line) for line in lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
