"""Times of the in-batch step with a cross-batch item bank (fmx_fm_inbatch_bank_step) at Criteo-39: a 1 M x 16 table, the largest
field as the item field, signadam, Zipf items, log q and keys (the item's index: a key that holds across batches); the bank full.
(B, M) = (256, 4,096), (1,024, 4,096) and (256, 65,536).  One process; at every setting the variants are timed in turn, call by
call, so they see the same machine state.  Wall time around a device synchronisation:

    bank       fmx_fm_inbatch_bank_step through FMEngine.inbatch_bank_step, the bank full (every call pushes B items and wraps on)
    plain      (a) fmx_fm_inbatch_step at the same B: bank - plain is what the bank costs; extra_launches is what it adds
    plain4096  (b) fmx_fm_inbatch_step at B = 4,096: without a bank the cheapest way to that many negatives per positive
    torch      (c) the torch formulation of the same loss (tools/inbatch_times.py's variant (a)) with the bank's columns
                   concatenated and detached; it reads a bank of the same size and does not push

Medians of --calls (9) timed calls after --warm (3) warm ones, with p10 / p90.  bank_p90_below_plain4096_p10 and
bank_p90_below_torch_p10 are the two expectations.  One JSON line per setting, written to --out.

    python tools/inbatch_bank_times.py --out profiles/inbatch_bank_times.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fm-for-online-recommendation_amd")]

K_EMB = 16
BIG_B = 4096
SETTINGS = [(256, 4096), (1024, 4096), (256, 65536)]
POOL = 4


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
    from fmx import _lib as L
    from fmx import pairwise as pw
    from models.models_online_deep.fm_adam import FMAdam

    lib = L.load()
    sizes = list(bench.CRITEO_SIZES)
    F = len(sizes)
    item = int(np.argmax(sizes))
    N = sizes[item]
    torch.manual_seed(0)
    m = FMAdam(sizes, embedding_size=K_EMB, n=1e-4)
    e, hyp, rule, t = m._engine, m._hyper, m.update_rule, m._table
    kp = t.kp
    rng = np.random.default_rng(0)
    weights = np.empty(N)
    weights[rng.permutation(N)] = 1.0 / np.arange(1, N + 1) ** 1.1
    logq = torch.from_numpy(pw.alias_table(weights)[3]).cuda()
    offs = torch.as_tensor(np.asarray(t.offsets_host[:-1], np.int64)).cuda()
    keep = torch.zeros(F, dtype=torch.bool, device="cuda")
    keep[item] = True
    st = torch.cuda.current_stream().cuda_stream

    def batches(B):
        """POOL batches of B rows: Zipf items, uniform contexts -> (idx [POOL, B, F], key [POOL, B], corr [POOL, B])"""
        pool = np.stack([np.stack([rng.integers(0, s, B) for s in sizes], 1) for _ in range(POOL)])
        pool[:, :, item] = rng.choice(N, size=(POOL, B), p=weights / weights.sum())
        idx = torch.from_numpy(pool.astype(np.int32)).cuda().contiguous()
        return idx, idx[:, :, item].contiguous(), logq[idx[:, :, item].long()].contiguous()

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6

    def timed(fns):
        for _ in range(args.warm):
            for fn in fns.values():
                fn()
        us = {name: [] for name in fns}
        for _ in range(args.calls):
            for name, fn in fns.items():
                us[name].append(wall(fn))
        return {name: stats(v) for name, v in us.items()}

    big_idx, big_key, big_corr = batches(BIG_B)
    lines = []
    for B, M in SETTINGS:
        idx_pool, key_pool, corr_pool = batches(B)
        e._ensure(max(B, BIG_B))
        bank = pw.ItemBank(M, kp, "cuda")
        turn = [0]

        def bank_step():
            p = turn[0] % POOL
            turn[0] += 1
            e.inbatch_bank_step(hyp, rule, idx_pool[p], [item], bank, None, corr=corr_pool[p], key=key_pool[p])
        for _ in range(-(-M // B) + 1):                                          # fill the ring, and wrap once
            bank_step()
        torch.cuda.synchronize()
        assert bank.count() == M
        frozen = [b.clone() for b in (bank.S, bank.a, bank.corr, bank.key)]      # what (c) reads: a full bank that stays put

        idx, key, corr = idx_pool[0], key_pool[0], corr_pool[0]
        ones = torch.ones((B, F), device="cuda")
        zi, zx = torch.zeros_like(idx), torch.zeros_like(ones)
        S = [torch.empty((B, kp), device="cuda") for _ in range(2)]
        au, sfirst, sbi = (torch.empty(B, device="cuda") for _ in range(3))
        occ = torch.empty((B, F, kp), device="cuda")
        loss_out = torch.zeros(1, device="cuda")
        ws = torch.zeros(int(lib.fmx_workspace_bytes(t.c_struct(), B)) // 4, dtype=torch.int32, device="cuda")

        def torch_step():
            bS, ba, bcorr, bkey = frozen
            idx_u, xv_u = torch.where(keep[None, :], zi, idx), torch.where(keep[None, :], zx, ones)
            idx_c, xv_c = torch.where(keep[None, :], idx, zi), torch.where(keep[None, :], ones, zx)
            ou, oc = L.FwdOut(), L.FwdOut()
            ou.S, ou.logit, ou.error = S[0].data_ptr(), au.data_ptr(), e.error.data_ptr()
            oc.S, oc.sfirst, oc.sbi, oc.error = S[1].data_ptr(), sfirst.data_ptr(), sbi.data_ptr(), e.error.data_ptr()
            L.check(lib.fmx_sort_occurrences(t.c_struct(), idx.data_ptr(), B, ws.data_ptr(), ws.numel() * 4, e.error.data_ptr(), st))
            L.check(lib.fmx_fm_forward(t.c_struct(), hyp.ref(), idx_u.data_ptr(), xv_u.data_ptr(), None, B, L.LOSS_NONE, 1.0, C.byref(ou), st))
            L.check(lib.fmx_fm_forward(t.c_struct(), hyp.ref(), idx_c.data_ptr(), xv_c.data_ptr(), None, B, L.LOSS_NONE, 1.0, C.byref(oc), st))
            Su, Sc = S[0].detach().requires_grad_(), S[1].detach().requires_grad_()
            ac = (sfirst + sbi).requires_grad_()
            z = torch.cat([Su @ Sc.T + au[:, None] + ac[None, :] - corr[None, :], Su @ bS.T + au[:, None] + ba[None, :] - bcorr[None, :]], dim=1)
            hit = torch.cat([(key[:, None] == key[None, :]) & ~torch.eye(B, dtype=torch.bool, device="cuda"), key[:, None] == bkey[None, :]], dim=1)
            loss_b = -torch.log_softmax(z.masked_fill(hit, float("-inf")), dim=1).diagonal()
            gSu, gSc, gac = torch.autograd.grad(loss_b.sum() / B, (Su, Sc, ac))
            v = t.rows[(idx[:, item].long() + offs[item])][:, :kp]
            occ[:] = gSu[:, None, :]
            occ[:, item] = gac[:, None] * (Sc.detach() - v) + gSc
            L.check(lib.fmx_fm_update_occ(t.c_struct(), hyp.ref(), L.RULES[rule], ws.data_ptr(), ws.numel() * 4, xv_c.data_ptr(),
                                          gac.contiguous().data_ptr(), occ.data_ptr(), F * kp, B, loss_b.detach().contiguous().data_ptr(),
                                          1.0 / B, loss_out.data_ptr(), st))

        s = timed(dict(bank=bank_step,
                       plain=lambda: e.inbatch_step(hyp, rule, idx, [item], None, corr=corr, key=key),
                       plain4096=lambda: e.inbatch_step(hyp, rule, big_idx[0], [item], None, corr=big_corr[0], key=big_key[0]),
                       torch=torch_step))
        splits, splits_q = int(lib.fmx_fm_inbatch_splits(B, kp)), int(lib.fmx_fm_inbatch_bank_splits(M, kp))
        lines.append(dict(B=B, M=M, table_rows=int(t.n_rows), k=K_EMB, N=N, rule=rule, warm=args.warm, calls=args.calls, splits=splits,
                          splits_q=splits_q, negatives_per_positive=B - 1 + M, extra_launches=4 if splits > 1 else 5, **s,
                          bank_cost_us=round(s["bank"]["median_us"] - s["plain"]["median_us"], 1),
                          plain4096_over_bank=round(s["plain4096"]["median_us"] / s["bank"]["median_us"], 2),
                          torch_over_bank=round(s["torch"]["median_us"] / s["bank"]["median_us"], 2),
                          bank_p90_below_plain4096_p10=bool(s["bank"]["p90_us"] < s["plain4096"]["p10_us"]),
                          bank_p90_below_torch_p10=bool(s["bank"]["p90_us"] < s["torch"]["p10_us"])))
    e.check_error_flag()

    text = "\n".join(json.dumps(line) for line in lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
