"""Times of the fused top-K call (fmx_fm_topk) against the plain torch path over the same candidate sums.

Candidates: every row of the largest field of the synthetic Criteo table (176,373 rows) and of a 1 M-row item field, k = 16
(kp = 16); contexts: U random users.  Both sides come out of the table through fmx.recommend (fmx_fm_forward with the other
side's fields masked), so the inputs are those a recommend() call scores.  Per (N, U, K):
  fused   one fmx_fm_topk call (scan + merge)
  torch   Su @ Sc.T + au[:, None] + ac[None, :] over candidate chunks of at most 2^28 scores, torch.topk per chunk, then
          torch.topk over the chunks' winners
Device events, a warm-up, then the median of --reps calls.  Reported: time per call, scores/s, the fused call's FLOP/s
(2 U N kp) against the fp32 peak (157.3 TFLOP/s), and Sc's bytes against an fmx_stream_read of a buffer of the same size
measured in the same run (the time one read of Sc takes from HBM).
  python tools/topk_times.py [--out FILE] [--quick] [--reps R]
--quick: one call of each size, no torch path (for a kernel trace under rocprofv3)."""
import argparse
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
K_EMB = 16


def tables():
    """(name, table, item field): the synthetic Criteo table and a three-field table with a 1 M-row item field."""
    dev = torch.device("cuda")
    out = []
    big = int(np.argmax(bench.CRITEO_SIZES))
    for name, sizes, item in (("criteo field %d (%d rows)" % (big, bench.CRITEO_SIZES[big]), bench.CRITEO_SIZES, big),
                              ("1 M-row item field", [100000, 24, 1000000], 2)):
        t = fmx.FlatTable(sizes, K_EMB, layout="weights")
        g = torch.Generator(device=dev).manual_seed(1)
        t.rows[:, :K_EMB] = torch.randn((t.n_rows, K_EMB), device=dev, generator=g) * 0.1
        t.rows[:, t.kp] = torch.randn(t.n_rows, device=dev, generator=g) * 0.1
        t.set_bias_weight(0.1)
        out.append((name, t, item))
    return out


def candidates(t, item):
    N = t.feature_sizes[item]
    idx = torch.zeros((N, t.n_fields), dtype=torch.int32, device=t.device)
    idx[:, item] = torch.arange(N, dtype=torch.int32, device=t.device)
    return rec.Candidates(t, [item], idx)


def users(t, item, U, seed):
    rng = np.random.default_rng(seed)
    Xi = np.stack([rng.integers(0, s, U) for s in t.feature_sizes], 1)
    ctx = [f for f in range(t.n_fields) if f != item]
    return rec.side_sums(t, Xi, None, ctx)


def torch_topk(Su, au, Sc, ac, K):
    U, N = Su.shape[0], Sc.shape[0]
    step = max(K, (1 << 28) // U)
    vals, poss = [], []
    for c0 in range(0, N, step):
        s = Su @ Sc[c0:c0 + step].T + au[:, None] + ac[None, c0:c0 + step]
        v, p = torch.topk(s, min(K, s.shape[1]), dim=1)
        vals.append(v)
        poss.append(p + c0)
    if len(vals) == 1:
        return poss[0], vals[0]
    v, j = torch.topk(torch.cat(vals, 1), K, dim=1)
    return torch.cat(poss, 1).gather(1, j), v


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


def stream_read_ms(nbytes, reps):
    lib = fmx._lib.load()
    nbytes = (nbytes + 15) // 16 * 16
    buf = torch.ones(nbytes // 4, device="cuda")
    sink = torch.zeros(1, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    return timed(lambda: fmx._lib.check(lib.fmx_stream_read(buf.data_ptr(), nbytes, sink.data_ptr(), st)), reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit(f"# tools/topk_times.py on {torch.cuda.get_device_name(0)}; k = {K_EMB} (kp = 16); median of {args.reps} calls after a warm-up")
    emit("# columns: N U K | fused ms, Gscores/s, TFLOP/s (% of 157.3) | torch ms | fused speed-up | Sc MB, HBM read of Sc ms")
    for name, t, item in tables():
        cand = candidates(t, item)
        N, kp = cand.N, t.kp
        sc_bytes = N * kp * 4 + N * 4
        rd = stream_read_ms(sc_bytes, args.reps)
        emit(f"## {name}: N = {N}, Sc + ac = {sc_bytes / 1e6:.1f} MB, one HBM read of that many bytes {rd * 1e3:.1f} us "
             f"({sc_bytes / rd / 1e6:.0f} GB/s)")
        for U in (1, 256, 4096):
            Su, au = users(t, item, U, seed=U)
            for K in (10, 100):
                ws = torch.empty(int(fmx._lib.load().fmx_fm_topk_workspace_bytes(U, N, K)), dtype=torch.uint8, device="cuda")
                out = (torch.empty((U, K), dtype=torch.int32, device="cuda"), torch.empty((U, K), device="cuda"))

                def fused():
                    rec.fm_topk(Su, au, cand.Sc, cand.ac, K, workspace=ws, out=out)
                if args.quick:
                    fused()
                    torch.cuda.synchronize()
                    emit(f"{N} {U} {K} | one call (trace run)")
                    continue
                tf = timed(fused, args.reps)
                tt = timed(lambda: torch_topk(Su, au, cand.Sc, cand.ac, K), max(3, args.reps // 4))
                # same answer up to near-ties: the torch path's K-th score against the fused one
                tp, tv = torch_topk(Su, au, cand.Sc, cand.ac, K)
                gap = float((tv[:, -1] - out[1][:, -1]).abs().max())
                flop = 2.0 * U * N * kp
                emit(f"{N} {U} {K} | fused {tf:.3f} ms, {U * N / tf / 1e6:.1f} Gscores/s, {flop / tf / 1e9:.2f} TFLOP/s "
                     f"({100 * flop / tf / 1e9 / (PEAK_FP32 / 1e12):.1f} %) | torch {tt:.3f} ms | x{tt / tf:.2f} | "
                     f"Sc {sc_bytes / 1e6:.1f} MB, read {rd:.3f} ms | K-th score gap to torch {gap:.2e}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
