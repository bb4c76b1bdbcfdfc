"""Times of the fused network top-K call (fmx_mlp_topk) against the chunked torch path (fmx.recommend.mlp_topk_torch: the
fallback of networks the kernel does not take) over the same side terms.

Candidates: every row of the largest field of the synthetic Criteo table (176,373 rows); contexts: U random users.  Both
sides come out of the table through fmx.recommend.side_terms, so the inputs are those a recommend(full=True) call scores.
Networks: the reference experiments' 5 x 10 on k = 10 (U = 1, 256, 4096) and BASELINE configs[3]'s 3 x 256 on k = 16
(U = 1, 64, 256), DeepFM scoring (fm_term = 1), K = 10 and 100.  Device events, a warm-up, then the median of --reps calls
(fewer for the torch path).  Reported: time per call, the network's FLOP/s (2 (k H + (L - 1) H^2) per pair, the padding the
kernel multiplies not counted) against the fp32 peak (157.3 TFLOP/s), the arithmetic floor at that peak, and the speed-up.
  python tools/mlp_topk_times.py [--out FILE] [--quick] [--reps R]
--quick: one call of each size, no torch path (for a kernel trace under rocprofv3)."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fm-for-online-recommendation_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import fmx  # noqa: E402
from fmx import recommend as rec  # noqa: E402

PEAK_FP32 = 157.3e12
POINTS = [(10, 10, 5, (1, 256, 4096)), (16, 256, 3, (1, 64, 256))]   # (k, hidden, layers, users)


def table(k):
    dev = torch.device("cuda")
    t = fmx.FlatTable(bench.CRITEO_SIZES, k, layout="weights")
    g = torch.Generator(device=dev).manual_seed(1)
    t.rows[:, :k] = torch.randn((t.n_rows, k), device=dev, generator=g) * 0.1
    t.rows[:, t.kp] = torch.randn(t.n_rows, device=dev, generator=g) * 0.1
    t.set_bias_weight(0.1)
    return t


def network(k, H, L):
    torch.manual_seed(2)
    layers = [torch.nn.Linear(k if l == 0 else H, H) for l in range(L)]
    flat = torch.cat([p.detach().reshape(-1) for m in layers for p in (m.weight, m.bias)])
    return (flat.cuda().contiguous(), k, H, L)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit(f"# tools/mlp_topk_times.py on {torch.cuda.get_device_name(0)}; DeepFM scoring; median of {args.reps} fused calls "
         f"({max(2, args.reps // 4)} torch) after a warm-up")
    emit("# columns: network U K | fused ms, TFLOP/s (% of 157.3), floor at peak ms | torch ms | fused speed-up | K-th score gap")
    big = int(np.argmax(bench.CRITEO_SIZES))
    lib = fmx._lib.load()
    for k, H, L, Us in POINTS:
        t = table(k)
        net = network(k, H, L)
        N = t.feature_sizes[big]
        idx = torch.zeros((N, t.n_fields), dtype=torch.int32, device=t.device)
        idx[:, big] = torch.arange(N, dtype=torch.int32, device=t.device)
        cand = rec.NetworkCandidates(t, [big], idx, fm_term=1)
        ctx = [f for f in range(t.n_fields) if f != big]
        flop_pair = 2.0 * (k * H + (L - 1) * H * H)
        emit(f"## {L} x {H} on k = {k} (kp = {t.kp}): N = {N} (criteo field {big}), {flop_pair / 1e3:.1f} K FLOP per pair")
        for U in Us:
            rng = np.random.default_rng(U)
            Xi = np.stack([rng.integers(0, s, U) for s in t.feature_sizes], 1)
            S, bi, sfirst, sbi, logit = rec.side_terms(t, Xi, None, ctx)
            au = rec.network_bases(t, sfirst, sbi, logit, 1, context=True).contiguous()
            for K in (10, 100):
                ws = torch.empty(int(lib.fmx_mlp_topk_workspace_bytes(C.byref(rec._mlp_struct(net)), U, N, K)), dtype=torch.uint8, device="cuda")
                out = (torch.empty((U, K), dtype=torch.int32, device="cuda"), torch.empty((U, K), device="cuda"))
                args_ = (net, 1, S, bi, au, cand.Sc, cand.Bc, cand.ac, K)

                def fused():
                    rec.mlp_topk(*args_, workspace=ws, out=out)
                if args.quick:
                    fused()
                    torch.cuda.synchronize()
                    emit(f"{L}x{H} {U} {K} | one call (trace run)")
                    continue
                tf = timed(fused, args.reps)
                tt = timed(lambda: rec.mlp_topk_torch(*args_), max(2, args.reps // 4))
                _, tv = rec.mlp_topk_torch(*args_)
                gap = float((tv[:, -1] - out[1][:, -1]).abs().max())
                flop = flop_pair * U * N
                emit(f"{L}x{H} {U} {K} | fused {tf:.3f} ms, {flop / tf / 1e9:.2f} TFLOP/s ({100 * flop / tf / 1e9 / (PEAK_FP32 / 1e12):.1f} %), "
                     f"floor {flop / PEAK_FP32 * 1e3:.3f} ms | torch {tt:.3f} ms | x{tt / tf:.2f} | gap {gap:.2e}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
