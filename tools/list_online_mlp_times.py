"""What the device loop gains run_list_experiment(full=True) of DeepFMAdam: the online predict-then-fit protocol on lists through
the whole network (fmx_online_run_mlp_list) next to the loops it stands beside.

The criteo39s-shaped model of the pair-online table (the golden fixture's 39 small fields, k = 10) at the reference's 5 x 10
network and at 3 x 60 (7,980 parameters of the one-workgroup form's 8,192), under signadam and under adam with
fused_optimizer=True, at lists of G = 2, 4, 8, 16 rows.  Every (row, rule) runs in a fresh child process (one GPU context each)
under its own time limit; the first child that fails ends the run.  In each process and for each G, lists/s as the median of
--reps timed calls after one warm call, with the 10th and the 90th percentile over the reps:
  (a) class_host_loop run_list_experiment(full=True) with list_loop_on_device = False: the host loop of one-list section calls,
                      the default path
  (b) queued          fmx_online_run_mlp_list with fmx_set_option("online_persistent", 0): four launches per list, no host
                      synchronisation
  (c) one_workgroup   the same call as it runs by default: one workgroup walking the stream (k_online_mlp_list) at G <= 8; at
                      G = 16 the call queues its launches under either setting, so (c) is (b) measured again
and gate = (c)'s p10 above both others' p90.  A missed gate is reported as measured, not tuned away.  Beside them, for scale and on
the same model: the pointwise loop (run_experiment: fmx_online_run_mlp / _opt) and the pair loop (fmx_online_run_mlp_pair) in
samples/s and pairs/s.
Writes profiles/list_online_mlp_times.json.
  python tools/list_online_mlp_times.py [--lists N] [--loop-lists M] [--reps R] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fm-for-online-recommendation_amd"))

ROWS = {"5x10": (5, 10), "3x60": (3, 60)}      # name: (layers, hidden)
RULES = ("signadam", "adam")
GS = (2, 4, 8, 16)


def fixture_meta():
    import numpy as np
    z = np.load(os.path.join(ROOT, "tests", "golden", "DeepFMAdam_criteo39s.npz"))
    return json.loads(bytes(z["meta"]).decode())


def child(row, rule, n_dev, n_loop, reps):
    import numpy as np
    import torch
    import fmx
    from models.models_online_deep.deepfm_adam import DeepFMAdam
    torch.cuda.set_device(0)
    lib = fmx._lib.load()
    meta = fixture_meta()
    sizes, k = meta["feature_sizes"], meta["k"]
    L, H = ROWS[row]
    item = int(np.argmax(sizes))
    rng = np.random.default_rng(11)
    N = max(n_dev, n_loop)
    idx = np.stack([rng.integers(0, s, size=N) for s in sizes], axis=1).astype(np.int32)
    neg = ((idx[:, item, None] + 1 + rng.integers(0, sizes[item] - 1, size=(N, max(GS) - 1))) % sizes[item]).astype(np.int64)[:, :, None]
    y = (rng.uniform(size=N) < 0.3).astype(np.float32)
    xv = np.ones(idx.shape, np.float32)

    def model():
        torch.manual_seed(5)
        m = DeepFMAdam(sizes, embedding_size=k, num_hidden_layers=L, neuron_per_hidden_layer=H, n=0.001, update_rule=rule,
                       fused_optimizer=rule != "signadam")
        m.strict_index_check = False
        return m

    def measure(fn, n, m):
        fn()                                           # warm: module load, allocations
        secs = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
        m._engine.check_error_flag()
        per_s = np.asarray([n / s for s in secs])
        finite = bool(torch.isfinite(m._mlp_flat).all()) and bool(torch.isfinite(m._table.rows).all())
        return dict(items=n, seconds=[round(s, 5) for s in secs], per_s=round(float(np.median(per_s)), 1),
                    p10=round(float(np.percentile(per_s, 10)), 1), p90=round(float(np.percentile(per_s, 90)), 1),
                    us_per_item=round(1e6 / float(np.median(per_s)), 3), finite=finite)

    def lists_of(G, n):
        rows = np.repeat(idx[:n], G, axis=0)
        rows.reshape(n, G, -1)[:, 1:, item] = neg[:n, :G - 1, 0]
        return torch.from_numpy(rows).cuda()

    def device_loop(m, rows_d, G, persistent):
        def fn():
            old = lib.fmx_set_option(b"online_persistent", int(persistent))
            try:
                rank, _, _ = m._engine.online_run_mlp_list(m._hyper, rule, m._mlp_flat, k, H, L, True, rows_d, G, None, mlp_opt=m._mlp_fused)
                rank.cpu()                             # as the class call ends: the ranks on the host
            finally:
                lib.fmx_set_option(b"online_persistent", old)
        return fn

    res = dict(row=row, rule=rule, layers=L, hidden=H, k=k, fields=len(sizes), n_params=sum(H * (k if l == 0 else H) + H for l in range(L)),
               by_G={})
    for G in GS:
        rows_d = lists_of(G, n_dev)
        r = {}
        m = model()
        assert m.list_loop_on_device is False
        r["class_host_loop"] = measure(lambda: m.run_list_experiment(idx[:n_loop], xv[:n_loop], [item], negatives=neg[:n_loop, :G - 1],
                                                                     full=True), n_loop, m)
        m = model()
        assert m._list_device_loop_ok(G)
        r["queued"] = measure(device_loop(m, rows_d, G, False), n_dev, m)
        m = model()
        r["one_workgroup"] = measure(device_loop(m, rows_d, G, True), n_dev, m)
        r["gate"] = bool(r["one_workgroup"]["p10"] > max(r["queued"]["p90"], r["class_host_loop"]["p90"]))
        r["one_workgroup_over_class_host_loop"] = round(r["one_workgroup"]["per_s"] / r["class_host_loop"]["per_s"], 2)
        r["one_workgroup_over_queued"] = round(r["one_workgroup"]["per_s"] / r["queued"]["per_s"], 3)
        res["by_G"][str(G)] = r
    m = model()
    assert m._device_loop_ok()
    res["pointwise"] = measure(lambda: m.run_experiment(idx[:n_dev], xv[:n_dev], y[:n_dev]), n_dev, m)
    m = model()
    pairs_d = lists_of(2, n_dev)
    res["pair"] = measure(lambda: m._engine.online_run_mlp_pair(m._hyper, rule, m._mlp_flat, k, H, L, True, pairs_d, None, margin=0.0,
                                                                mlp_opt=m._mlp_fused)[0].cpu(), n_dev, m)
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lists", type=int, default=4096, help="lists per call of the device loops (samples / pairs of the other two)")
    ap.add_argument("--loop-lists", type=int, default=200, help="lists per call of the host loop")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--timeout", type=int, default=200, help="seconds per child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "list_online_mlp_times.json"))
    ap.add_argument("--child", default=None, help="ROW:RULE")
    args = ap.parse_args()
    if args.child:
        row, rule = args.child.split(":")
        return child(row, rule, args.lists, args.loop_lists, args.reps)
    results = []
    for row in ROWS:
        for rule in RULES:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", f"{row}:{rule}", "--lists", str(args.lists), "--loop-lists",
                   str(args.loop_lists), "--reps", str(args.reps)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
            except subprocess.TimeoutExpired:
                print(f"{row} {rule}: no result within {args.timeout} s; stopping", flush=True)
                return 1
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                print(f"{row} {rule}: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}", flush=True)
                return 1
            results.append(json.loads(line[-1][len("RESULT "):]))
            print(json.dumps(results[-1]), flush=True)
    out = dict(what="the online list loop of DeepFMAdam through the whole network (criteo39s-shaped, k = 10): lists/s (pointwise: "
                    "samples/s, pair: pairs/s), median of reps timed calls after one warm call with the 10th and 90th percentile; "
                    "gate: the one-workgroup form's p10 above the queued form's and the host loop's p90",
               lists=args.lists, loop_lists=args.loop_lists, reps=args.reps, results=results)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
