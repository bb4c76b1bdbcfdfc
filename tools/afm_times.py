"""Times fmx_afm_step and fmx_afm_forward at Criteo-39 (a 1 M x 16 table over 39 fields, B = 4096) for attention sizes
t in {4, 16, 64}, next to a same-process torch-autograd implementation of the same model on the same GPU (the baseline: the
reference's formulation with its bugs fixed, tests/afm_f64.py's statement in fp32).  Prints one JSON line per t and writes them
to the file given with --out.

    python tools/afm_times.py --out profiles/afm_times.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fm-for-online-recommendation_amd")]

import fmx  # noqa: E402
from fmx.afm import AFMEngine  # noqa: E402

PEAK_FP32_TFLOPS = 157.3     # MI355X vector / MFMA fp32 peak


def flop_per_step(F, k, t):
    """Per sample and training step: forward (q: k, W q + b: 2tk, relu + h: 2t, p.q: 2k) twice (the backward recomputes it) and
    the backward (dq: 2tk + 2k, dW: 2tk, the scatter to both fields: 4k) -- the attention's arithmetic, not the table update."""
    P = F * (F - 1) // 2
    fwd = k + 2 * t * k + 2 * t + 2 * k
    bwd = 2 * t * k + 2 * k + 2 * t * k + 4 * k + 3 * t
    return P * (2 * fwd + bwd), P * fwd


def torch_step(V, w, bias, W, b, h, p, rows, y, I, J):
    e = V[rows]
    q = e[:, I] * e[:, J]
    s = torch.relu(q @ W.t() + b) @ h
    a = torch.softmax(s, dim=1)
    logit = bias + w[rows].sum(1) + (a * (q @ p)).sum(1)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(logit, y)
    return loss


def timed(fn, n, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    F, k, B = 39, 16, 4096
    sizes = [1_000_000 // F] * F
    rng = np.random.default_rng(0)
    tb = fmx.FlatTable(sizes, k)
    tb.rows[:, :k] = torch.randn(tb.rows.shape[0], k, device="cuda") * 0.1
    idx = np.stack([rng.integers(0, s, size=B) for s in sizes], axis=1).astype(np.int32)
    y = (rng.uniform(size=B) < 0.25).astype(np.float32)
    hyper = fmx.Hyper(lr=1e-4)
    lines = []
    for t in (4, 16, 64):
        params = (torch.randn(t * k + 2 * t + k, device="cuda") * 0.3).contiguous()
        eng = AFMEngine(tb, params, t, max_batch=B)
        idx_d, _, y_d = eng.to_device(idx, None, y)
        step_us = timed(lambda: eng.step(hyper, "sgd", idx_d, None, y_d), args.steps, args.warmup)
        fwd_us = timed(lambda: eng.forward(hyper, idx_d), args.steps, args.warmup)
        # the torch-autograd baseline: the same model on the same table's weights, gradients of every parameter
        offs = torch.as_tensor(np.concatenate([[0], np.cumsum(sizes)[:-1]]), device="cuda")
        rows = idx_d.long() + offs[None, :]
        V = tb.rows[:, :k].clone().requires_grad_(True)
        w = tb.rows[:, tb.kp].clone().requires_grad_(True)
        bias = torch.zeros((), device="cuda", requires_grad=True)
        W = params[:t * k].view(t, k).clone().requires_grad_(True)
        b_, h = params[t * k:t * k + t].clone().requires_grad_(True), params[t * k + t:t * k + 2 * t].clone().requires_grad_(True)
        p = params[t * k + 2 * t:].clone().requires_grad_(True)
        I, J = (torch.as_tensor(a, device="cuda") for a in np.triu_indices(F, 1))
        yt = y_d

        def tstep():
            loss = torch_step(V, w, bias, W, b_, h, p, rows, yt, I, J)
            loss.backward()
            with torch.no_grad():       # SGD on the rows of the batch and on the attention parameters
                u = rows.reshape(-1).unique()
                V[u] -= 1e-4 * V.grad[u]
                w[u] -= 1e-4 * w.grad[u]
                for prm in (bias, W, b_, h, p):
                    prm -= 1e-4 * prm.grad
            for prm in (V, w, bias, W, b_, h, p):
                prm.grad = None

        def tfwd():
            with torch.no_grad():
                torch_step(V, w, bias, W, b_, h, p, rows, yt, I, J)

        torch_step_us = timed(tstep, max(5, args.steps // 5), 2)
        torch_fwd_us = timed(tfwd, max(5, args.steps // 5), 2)
        fl_step, fl_fwd = flop_per_step(F, k, t)
        line = dict(F=F, k=k, t=t, B=B, table_rows=int(tb.rows.shape[0]), afm_step_us=round(step_us, 1), afm_forward_us=round(fwd_us, 1),
                    step_gflop=round(fl_step * B / 1e9, 3), step_frac_fp32_peak=round(fl_step * B / (step_us * 1e-6) / (PEAK_FP32_TFLOPS * 1e12), 4),
                    forward_frac_fp32_peak=round(fl_fwd * B / (fwd_us * 1e-6) / (PEAK_FP32_TFLOPS * 1e12), 4),
                    torch_autograd_step_us=round(torch_step_us, 1), torch_forward_us=round(torch_fwd_us, 1),
                    speedup_step=round(torch_step_us / step_us, 2), speedup_forward=round(torch_fwd_us / fwd_us, 2))
        print(json.dumps(line), flush=True)
        lines.append(line)
        del eng, V, w
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
