"""Times the rank calls (fmx_fm_rank, fmx_mlp_rank, fmx_afm_rank) at Criteo-39 with the largest field as the candidates
(N = 176,373), a 1 M x 16 table, T = 1 target per context, U = 1 / 256 / 4096, against the family's own top-K call at K = 10 in
the same process (the yardstick: the same loads and products plus a selection) and, where one exists, a torch baseline:
  fm:   the chunked Su @ Sc.T + au + ac followed by a comparison count
  mlp:  fmx.recommend.mlp_rank_torch (U <= 256; at U = 4096 it would take minutes per call)
  afm:  none -- it would be the assembled-sample forward, which profiles/afm_topk_times.txt has at 68-113 x the top-K call
Both sides of every call are precomputed; device events, median of --reps calls.  Every family runs in a child process of its
own under a time limit, and the tool stops at the first one that fails or runs out of time.
  python tools/rank_times.py --out profiles/rank_times.txt
  python tools/rank_times.py --step afm --us 1      (one family and size in this process: the run for rocprofv3 --kernel-trace --stats)"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ("fm", "mlp", "afm")
US = (1, 256, 4096)
HEADER = "family U rank_ms topk10_ms rank/topk torch_ms torch/rank"


def event_ms(fn, reps, warm=2):
    import numpy as np
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def fm_torch_rank(Su, au, Sc, ac, tg, chunk=1 << 25):
    """the count of candidates ahead of the target from chunked score blocks (ties by position)"""
    import torch
    U, N = Su.shape[0], Sc.shape[0]
    ub = max(1, min(U, chunk // N))
    rank = torch.empty(U, dtype=torch.int64, device=Su.device)
    pos = torch.arange(N, device=Su.device)[None, :]
    for u0 in range(0, U, ub):
        u1 = min(U, u0 + ub)
        s = Su[u0:u1] @ Sc.T + au[u0:u1, None] + ac[None, :]
        p = tg[u0:u1].long()
        sp = s.gather(1, p)
        rank[u0:u1] = ((s > sp) | ((s == sp) & (pos < p))).sum(1)
    return rank


def step(family, reps, us=US):
    """one family's rows, printed; runs in the child process"""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "fm-for-online-recommendation_amd")]
    import numpy as np
    import torch
    import bench
    import fmx
    from fmx import recommend as rec

    sizes, k = bench.CRITEO_SIZES, 16
    F = len(sizes)
    item = int(np.argmax(sizes))
    N = sizes[item]
    tb = fmx.FlatTable(sizes, k)
    torch.manual_seed(0)
    tb.rows[:, :k] = torch.randn(tb.rows.shape[0], k, device="cuda") * 0.1
    tb.rows[:, tb.kp] = torch.randn(tb.rows.shape[0], device="cuda") * 0.1
    rng = np.random.default_rng(0)
    cand = np.zeros((N, F), np.int32)
    cand[:, item] = np.arange(N)
    ctx_fields = [f for f in range(F) if f != item]
    net = None
    if family == "fm":
        cands = rec.Candidates(tb, [item], cand)
    elif family == "mlp":
        H, L = 64, 3
        net = ((torch.randn(H * k + H + (L - 1) * (H * H + H), device="cuda") * 0.1).contiguous(), k, H, L)
        cands = rec.NetworkCandidates(tb, [item], cand, fm_term=1)
    else:
        t = 16
        afm = ((torch.randn(t * k + 2 * t + k, device="cuda") * 0.3).contiguous(), t)
        cands = rec.AFMCandidates(tb, afm, [item], cand)
    for U in us:
        ctx = np.stack([rng.integers(0, s, size=U) for s in sizes], axis=1).astype(np.int32)
        tg = torch.from_numpy(rng.integers(0, N, size=(U, 1)).astype(np.int32)).cuda()
        base = float("nan")
        if family == "fm":
            Su, au = rec.side_sums(tb, ctx, None, ctx_fields)
            rank_call = lambda: rec.fm_rank(Su, au, cands.Sc, cands.ac, tg)                      # noqa: E731
            topk_call = lambda: rec.fm_topk(Su, au, cands.Sc, cands.ac, 10)                      # noqa: E731
            base = event_ms(lambda: fm_torch_rank(Su, au, cands.Sc, cands.ac, tg), max(3, reps // 4))
        elif family == "mlp":
            S, bi, sfirst, sbi, logit = rec.side_terms(tb, ctx, None, ctx_fields)
            au = rec.network_bases(tb, sfirst, sbi, logit, 1, context=True).contiguous()
            args = (net, 1, S, bi, au, cands.Sc, cands.Bc, cands.ac)
            rank_call = lambda: rec.mlp_rank(*args, tg)                                          # noqa: E731
            topk_call = lambda: rec.mlp_topk(*args, 10)                                          # noqa: E731
            if U <= 256:
                base = event_ms(lambda: rec.mlp_rank_torch(*args, tg), 3, warm=1)
        else:
            Eu, su = rec.afm_side(tb, afm, ctx, None, ctx_fields, True)
            args = (afm, tb.k, Eu, su, cands.Ec, cands.stats)
            rank_call = lambda: rec.afm_rank(*args, tg)                                          # noqa: E731
            topk_call = lambda: rec.afm_topk(*args, 10)                                          # noqa: E731
        r, s, n = rank_call()
        pos, val = topk_call()
        torch.cuda.synchronize()
        inside = (r[:, 0] >= 0) & (r[:, 0] < 10)                   # the cross-check of the two epilogues on the timed inputs
        at = pos.gather(1, r[:, :1].clamp(0, 9).long())[:, 0]
        assert bool((at[inside] == tg[inside, 0]).all()) and bool((n == N).all())
        rk = event_ms(rank_call, reps)
        tk = event_ms(topk_call, reps)
        print(f"{family} {U} {rk:.3f} {tk:.3f} {rk / tk:.2f} {base:.1f} {base / rk:.1f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=240, help="seconds a family's child process may take")
    ap.add_argument("--step", default=None, choices=FAMILIES, help="run one family in this process (what the children run)")
    ap.add_argument("--us", default=None, help="with --step: the U values, comma separated")
    args = ap.parse_args()
    if args.step:
        step(args.step, args.reps, tuple(int(u) for u in args.us.split(",")) if args.us else US)
        return 0
    lines = [f"# rank calls at Criteo-39 (1 M x 16 table), the largest field as candidates (N = 176,373), T = 1; device events, "
             f"median of {args.reps}",
             "# rank_ms: fmx_*_rank (keys + counting scan + finish); topk10_ms: the family's top-K call at K = 10, same process and inputs",
             "# torch_ms: fm: chunked Su @ Sc.T + au + ac and a comparison count; mlp (hidden 64, 3 layers): mlp_rank_torch, U <= 256; afm (t = 16): none",
             HEADER]
    print(HEADER, flush=True)
    rc = 0
    for family in FAMILIES:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", family, "--reps", str(args.reps)],
                               capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            lines.append(f"# {family}: stopped at its time limit of {args.limit} s; nothing after it was run")
            rc = 124
            break
        rows = [ln for ln in p.stdout.splitlines() if ln.startswith(family + " ")]
        print("\n".join(rows), flush=True)
        lines += rows
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-2000:])
            lines.append(f"# {family}: failed with status {p.returncode}; nothing after it was run")
            rc = p.returncode
            break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
