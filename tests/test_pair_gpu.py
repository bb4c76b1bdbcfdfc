"""Pairwise-ranking (BPR) training of the FM on the device: fmx_fm_pair_forward / _step / _stream / _online_run and the class
methods on top of them.

Shapes: small vocabularies, so rows repeat -- long runs, runs that cross the update's 64-occurrence tiles, and rows both
samples of a pair name.  (a) kp 4, (b) k 10 padded to kp 16, (c) 39 fields: three unrolled passes, (d) k 64: the generic field
loop, (e) 70 fields: the generic loop at kp 16.  B pairs per batch in {1, 3, 33, 130}: 2B = 6 leaves a partly filled workgroup
at 4 waves, 2B = 66 and 260 cross tiles."""
import numpy as np
import pytest
import torch

from oracle.fm_oracle import EPS32
from helpers import assert_ftrl_step_within_f64, assert_within_f64
from pair_f64 import pair_loss_f64, pair_step_f64
from test_kernels_gpu import HYP, WALK_GEOMETRY, WALK_STEPS, ftrl_state, ftrl_table, make_problem, walk_sizes, weights_table

pytestmark = pytest.mark.gpu

SMALL = [7, 5, 11, 3, 6]
SHAPES = {"a": (SMALL, 4), "b": (SMALL, 10), "c": ([3 + i for i in range(38)] + [40], 16), "d": ([3 + i for i in range(20)], 64),
          "e": ([3 + i % 9 for i in range(70)], 16)}
RULES = {"signadam": "weights", "sgd": "weights", "ftrl": "ftrl", "adagrad": "moments", "adam": "moments"}
BS = [1, 3, 33, 130]


@pytest.fixture(scope="module")
def fmx():
    import fmx as _fmx
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _fmx


def make_pairs(sizes, B, seed, n_item=1, real_x=False, free_context=False):
    """-> (rows int32 [2B, F] local indices, x float32 [2B, F] or None, item fields).  The negative is the positive with the item
    columns (the last n_item fields) redrawn -- with two item fields every third pair keeps one of the two item rows -- and, with
    free_context, two pairs of three get a context of their own as well."""
    rng = np.random.default_rng(seed)
    F = len(sizes)
    item = list(range(F - n_item, F))
    pos = np.stack([rng.integers(0, s, size=B) for s in sizes], axis=1)
    neg = pos.copy()
    for f in item:
        neg[:, f] = (pos[:, f] + 1 + rng.integers(0, sizes[f] - 1, size=B)) % sizes[f]      # never the positive's row
    if n_item == 2:
        neg[0::3, item[0]] = pos[0::3, item[0]]
    if free_context:
        other = np.stack([rng.integers(0, s, size=B) for s in sizes], axis=1)
        for f in range(F - n_item):
            neg[1::3, f], neg[2::3, f] = other[1::3, f], other[2::3, f]
    rows = np.empty((2 * B, F), np.int32)
    rows[0::2], rows[1::2] = pos, neg
    x = rng.uniform(0.5, 1.5, size=(2 * B, F)).astype(np.float32) if real_x else None
    return rows, x, item


def build_table(fmx, sizes, k, layout, seed=3):
    pr = make_problem(sizes, k, 1, seed)
    if layout == "weights":
        return weights_table(fmx, sizes, k, pr), pr
    if layout == "ftrl":
        st = ftrl_state(pr, HYP)
        pr["ftrl_state"] = st
        return ftrl_table(fmx, sizes, k, st), pr
    rng = np.random.default_rng(seed + 1)
    t = fmx.FlatTable(sizes, k, layout="moments")
    R, kp, zo = pr["R"], t.kp, t.z_offset
    t.rows[:, :k] = torch.from_numpy(pr["V"]).cuda()
    t.rows[:, kp] = torch.from_numpy(pr["w"]).cuda()
    t.rows[:, kp + 1] = torch.from_numpy((rng.normal(size=R) * 1e-3).astype(np.float32)).cuda()
    t.rows[:, kp + 2] = torch.from_numpy((rng.uniform(size=R) * 1e-4).astype(np.float32)).cuda()
    t.rows[:, zo:zo + k] = torch.from_numpy((rng.normal(size=(R, k)) * 1e-3).astype(np.float32)).cuda()
    t.rows[:, zo + kp:zo + kp + k] = torch.from_numpy((rng.uniform(size=(R, k)) * 1e-4).astype(np.float32)).cuda()
    t.bias[0], t.bias[1], t.bias[2] = float(pr["bias"]), 1e-3, 1e-4
    t.step = 3
    return t, pr


def clone_table(fmx, t):
    c = fmx.FlatTable(t.feature_sizes, t.k, layout=t.layout, ftrl=t.ftrl)
    c.rows.copy_(t.rows)
    c.bias.copy_(t.bias)
    c.step = t.step
    return c


def same_bits(a, b, what):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), \
        f"{what}: {int((a.view(torch.int32) != b.view(torch.int32)).sum())} of {a.numel()} words differ"


def dev(eng, rows, x):
    idx_d, xv_d, _ = eng.to_device(rows, x)
    return idx_d, xv_d


# ---- 1. the forward's outputs are fmx_fm_forward's ----
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("B", [3, 33])
def test_forward_identity(fmx, shape, B):
    sizes, k = SHAPES[shape]
    for layout in ("weights", "ftrl"):
        t, _ = build_table(fmx, sizes, k, layout)
        eng = fmx.FMEngine(t, max_batch=2 * B)
        hyp = fmx.Hyper(**HYP)
        for real_x in (False, True):
            rows, x, _ = make_pairs(sizes, B, seed=B + len(sizes), n_item=1 + real_x, real_x=real_x)
            idx_d, xv_d = dev(eng, rows, x)
            eng.forward(hyp, idx_d, xv_d)                                 # FMX_LOSS_NONE
            want = [b[:2 * B].clone() for b in (eng.S, eng.sfirst, eng.sbi, eng.logit, eng.bi, eng.first)]
            for b in (eng.S, eng.sfirst, eng.sbi, eng.logit, eng.bi, eng.first):
                b.fill_(float("nan"))
            eng.pair_forward(hyp, idx_d, xv_d, margin=0.1 * real_x, want_first=True, want_bi=True)
            torch.cuda.synchronize()
            eng.check_error_flag()
            for name, w, b in zip(("S", "sfirst", "sbi", "logit", "bi", "first"), want,
                                  (eng.S, eng.sfirst, eng.sbi, eng.logit, eng.bi, eng.first)):
                same_bits(b[:2 * B], w, f"{shape} {layout} x={real_x} {name}")


# ---- 2. the epilogue from the device's own logits ----
def check_epilogue(eng, B, margin, what):
    z = eng.logit[:2 * B].double().cpu().numpy()
    loss, dz = eng.loss_b[:2 * B].cpu(), eng.dz[:2 * B].cpu()
    assert np.isfinite(loss.numpy()).all() and np.isfinite(dz.numpy()).all(), what
    inv_b = 1.0 / B
    ref_loss, g = pair_loss_f64(z[0::2] - z[1::2], margin)
    ref_dz = g * inv_b
    for name, got, ref, floor in (("loss", loss[0::2], ref_loss, 4 * EPS32 * (1 + np.abs(ref_loss))), ("dz", dz[0::2], ref_dz, 4 * EPS32 * inv_b)):
        err = np.abs(got.double().numpy() - ref)
        tol = 1e-5 * np.abs(ref) + floor
        print(f"{what} {name}: worst err/tol {float((err / tol).max()):.3f}")
        assert (err <= tol).all(), f"{what} {name}: worst err/tol {float((err / tol).max()):.3f}"
    same_bits(dz[1::2], -dz[0::2], what + " dz[2i+1] == -dz[2i]")
    assert (loss[1::2].view(torch.int32) == 0).all(), what + " loss[2i+1] == +0"
    return z


@pytest.mark.parametrize("margin", [0.0, 0.1])
@pytest.mark.parametrize("shape,B", [("a", 33), ("b", 130), ("c", 3), ("e", 33)])
def test_epilogue(fmx, shape, B, margin):
    sizes, k = SHAPES[shape]
    t, _ = build_table(fmx, sizes, k, "weights")
    eng = fmx.FMEngine(t, max_batch=2 * B)
    hyp = fmx.Hyper(**HYP)
    rows, x, item = make_pairs(sizes, B, seed=5, n_item=1 + (B == 33), real_x=(shape in "ac"))
    idx_d, xv_d = dev(eng, rows, x)
    eng.pair_forward(hyp, idx_d, xv_d, margin=margin)
    torch.cuda.synchronize()
    check_epilogue(eng, B, margin, f"{shape} B={B}")
    # logit differences from -30 to 30: small factors, first-order weights of the item field spread over [-15, 15]
    f = item[-1]
    lo, n = int(t.offsets_host[f]), sizes[f]
    t.rows[:, :t.kp] *= 0.01
    t.rows[lo:lo + n, t.kp] = torch.linspace(-15, 15, n, device="cuda")
    wide = rows.copy()
    wide[0::2, f], wide[1::2, f] = np.arange(B) % n, (n - 1 - np.arange(B)) % n
    idx_d, _ = dev(eng, wide, None)
    eng.pair_forward(hyp, idx_d, None, margin=margin)
    torch.cuda.synchronize()
    z = check_epilogue(eng, B, margin, f"{shape} B={B} wide")
    if B >= n:
        d = z[0::2] - z[1::2]
        assert d.min() < -25 and d.max() > 25


# ---- 3. the step is sort + pair forward + update, bit for bit, under every rule ----
@pytest.mark.parametrize("rule", list(RULES))
@pytest.mark.parametrize("shape", ["b", "c"])
def test_step_is_sort_forward_update(fmx, rule, shape):
    sizes, k = SHAPES[shape]
    t1, _ = build_table(fmx, sizes, k, RULES[rule])
    t2 = clone_table(fmx, t1)
    e1, e2 = fmx.FMEngine(t1, max_batch=2 * max(BS)), fmx.FMEngine(t2, max_batch=2 * max(BS))
    h1, h2 = fmx.Hyper(**HYP), fmx.Hyper(**HYP)
    offs = np.asarray(t1.offsets_host[:-1], np.int64)
    for i, B in enumerate(BS):
        margin, real_x = (0.0, 0.1)[i % 2], i >= 2
        rows, x, _ = make_pairs(sizes, B, seed=11 * B, n_item=1 + (i % 2), real_x=real_x)
        before = t1.rows.clone()
        idx1, xv1 = dev(e1, rows, x)
        e1.pair_step(h1, rule, idx1, xv1, margin=margin)
        idx2, xv2 = dev(e2, rows, x)
        e2.sort(idx2)
        e2.pair_forward(h2, idx2, xv2, margin=margin)
        e2.update(h2, rule, 2 * B, xv2, e2.dz, dz_bi=e2.dz, inv_b=1.0 / B)
        torch.cuda.synchronize()
        e1.check_error_flag()
        e2.check_error_flag()
        what = f"{rule} {shape} B={B}"
        same_bits(t1.rows, t2.rows, what + " rows")
        same_bits(t1.bias, t2.bias, what + " bias")
        same_bits(e1.loss_out, e2.loss_out, what + " loss_out")
        assert t1.step == t2.step
        touched = np.zeros(t1.n_rows, bool)
        touched[np.unique(rows.astype(np.int64) + offs[None, :])] = True
        keep = torch.from_numpy(~touched).cuda()
        same_bits(t1.rows[keep], before[keep], what + " rows no pair touches")
        assert not torch.equal(t1.rows[~keep], before[~keep])


# ---- 4. the step against its float64 evaluation ----
@pytest.mark.parametrize("rule", ["sgd", "ftrl"])
@pytest.mark.parametrize("shape", ["a", "b", "c", "d"])
@pytest.mark.parametrize("B", [33, 130])
def test_step_within_float64(fmx, rule, shape, B):
    sizes, k = SHAPES[shape]
    margin, real_x = (0.1 if shape in "bd" else 0.0), shape in "ac"
    t, pr = build_table(fmx, sizes, k, RULES[rule], seed=7)
    eng = fmx.FMEngine(t, max_batch=2 * B)
    rows, x, _ = make_pairs(sizes, B, seed=B + k, n_item=1 + (B == 33), real_x=real_x)
    idx_d, xv_d = dev(eng, rows, x)
    eng.pair_step(fmx.Hyper(**HYP), rule, idx_d, xv_d, margin=margin)
    torch.cuda.synchronize()
    eng.check_error_flag()
    grows = rows.astype(np.int64) + np.asarray(t.offsets_host[:-1], np.int64)[None, :]
    xx = x if x is not None else np.ones(rows.shape, np.float32)
    if rule == "ftrl":
        st0 = pr["ftrl_state"]
        h = dict(alpha=HYP["alpha"], beta=HYP["beta"], l1=HYP["l1"], l2=HYP["l2"])
        ref = pair_step_f64(st0, grows, xx, margin, "ftrl", h, inv_b=1.0 / B)
        assert_within_f64(float(eng.loss_out.item()), ref["loss"], ref["floor"]["loss"], "loss")
        zV, nV, zw, nw = [a.numpy() for a in t.export_ftrl_state()]
        assert_ftrl_step_within_f64(dict(zV=zV, nV=nV, zw=zw, nw=nw, zb=t.bias[0].item(), nb=t.bias[1].item()), ref, before=st0)
        return
    st0 = dict(V=pr["V"], w=pr["w"], bias=pr["bias"])
    ref = pair_step_f64(st0, grows, xx, margin, "sgd", dict(lr=HYP["lr"]), inv_b=1.0 / B)
    assert_within_f64(float(eng.loss_out.item()), ref["loss"], ref["floor"]["loss"], "loss")
    u, new, fl = ref["urows"], ref["new"], ref["floor"]
    got = dict(V=t.rows[:, :k].cpu().numpy(), w=t.rows[:, t.kp].cpu().numpy())
    for kk in ("V", "w"):
        b0 = np.asarray(st0[kk], np.float64)[u]
        assert_within_f64(got[kk][u], new[kk][u], fl[kk], kk)
        assert_within_f64(got[kk][u].astype(np.float64) - b0, new[kk][u] - b0, fl[kk], kk + " (the step)")
        mask = np.ones(len(got[kk]), bool)
        mask[u] = False
        np.testing.assert_array_equal(got[kk][mask], st0[kk][mask], err_msg=kk + " untouched rows")
        assert np.abs(new[kk][u] - b0).max() > 0
    assert_within_f64(t.bias[0].item(), new["bias"], fl["bias"], "bias")
    assert_within_f64(t.bias[0].item() - float(st0["bias"]), new["bias"] - float(st0["bias"]), fl["bias"], "bias (the step)")


# ---- 5. the stream is its steps ----
@pytest.mark.parametrize("rule", ["signadam", "ftrl", "adam"])
@pytest.mark.parametrize("shape,B", [("b", 33), ("c", 130), ("b", 256)])          # 2B = 512: the sorts run ahead on the side stream
def test_stream_is_its_steps(fmx, rule, shape, B):
    stream_is_its_steps(fmx, rule, shape, B, n_pool=3, n_steps=7)


@pytest.mark.parametrize("own_stream", [False, True])
@pytest.mark.parametrize("rule", ["signadam", "adam"])
@pytest.mark.parametrize("B", [130, 256])
def test_stream_is_its_steps_through_the_whole_loop(fmx, rule, B, own_stream):
    """37 steps over a pool of 5: sort groups of 4 + 16 + 16 + 1, so both halves of the sorted ring are used again and the pool
    wraps.  2B = 512 rows is OVERLAP_MIN_BATCH (the sorts run ahead on the side stream), 2B = 260 is under it (every group is
    sorted in front of its steps).  From torch's default stream (handle 0: the loop detours off it) and from a stream of its own."""
    stream_is_its_steps(fmx, rule, "b", B, n_pool=5, n_steps=37, own_stream=own_stream)


def stream_is_its_steps(fmx, rule, shape, B, n_pool, n_steps, own_stream=False):
    sizes, k = SHAPES[shape]
    margin = 0.1 if B == 33 else 0.0
    t1, _ = build_table(fmx, sizes, k, RULES[rule])
    t2 = clone_table(fmx, t1)
    e1, e2 = fmx.FMEngine(t1, max_batch=2 * B), fmx.FMEngine(t2, max_batch=2 * B)
    pool = np.stack([make_pairs(sizes, B, seed=100 + j, n_item=1 + j % 2)[0] for j in range(n_pool)])
    pool_d = torch.from_numpy(pool).cuda().contiguous()
    losses1 = torch.full((n_steps,), float("nan"), device="cuda")
    side = torch.cuda.Stream() if own_stream else torch.cuda.default_stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert (torch.cuda.current_stream().cuda_stream == 0) != own_stream
        e1.pair_stream(fmx.Hyper(**HYP), rule, pool_d, n_steps, margin=margin, loss_out=losses1)
        h2, losses2 = fmx.Hyper(**HYP), []
        for s in range(n_steps):
            e2.pair_step(h2, rule, pool_d[s % n_pool], None, margin=margin)
            losses2.append(e2.loss_out.clone())
    torch.cuda.synchronize()
    e1.check_error_flag()
    e2.check_error_flag()
    same_bits(t1.rows, t2.rows, "rows")
    same_bits(t1.bias, t2.bias, "bias")
    same_bits(losses1, torch.cat(losses2), "loss_out")
    assert t1.step == t2.step == (3 + n_steps if rule == "adam" else t1.step)


# ---- 6. the online loop is N steps of one pair ----
# ... and over the walkers' field geometry (test_kernels_gpu.WALK_GEOMETRY): one, two and four passes, a partly live last pass
WALK_SHAPES = {f"k{k}-F{F}": (walk_sizes(F), k) for k, F in WALK_GEOMETRY}


@pytest.mark.parametrize("shape,rule", [(shape, rule) for shape in ["a", "b", "c"] for rule in RULES] +
                         [(shape, rule) for shape in WALK_SHAPES for rule in ("signadam", "adam")])
def test_online_run_is_single_pair_steps(fmx, rule, shape):
    sizes, k = SHAPES[shape] if shape in SHAPES else WALK_SHAPES[shape]
    N = 40 if shape in SHAPES else WALK_STEPS
    margin, real_x = (0.1 if shape == "b" else 0.0), shape != "b"
    rows, x, _ = make_pairs(sizes, N, seed=9, n_item=2, real_x=real_x, free_context=True)
    t1, _ = build_table(fmx, sizes, k, RULES[rule])
    t2 = clone_table(fmx, t1)
    e1, e2 = fmx.FMEngine(t1, max_batch=2 * N), fmx.FMEngine(t2, max_batch=8)
    idx_d, xv_d = dev(e1, rows, x)
    pred, logit, loss = e1.pair_online_run(fmx.Hyper(**HYP), rule, idx_d, xv_d, margin=margin, want_logit=True, want_loss=True)
    h2, logits2, losses2 = fmx.Hyper(**HYP), [], []
    for i in range(N):
        xi = None if xv_d is None else xv_d[2 * i:2 * i + 2]
        e2.pair_step(h2, rule, idx_d[2 * i:2 * i + 2], xi, margin=margin, inv_b=1.0)
        logits2.append(e2.logit[:2].clone())                     # the step's own forward: before its update
        losses2.append(e2.loss_out.clone())
    torch.cuda.synchronize()
    e1.check_error_flag()
    e2.check_error_flag()
    same_bits(t1.rows, t2.rows, "rows")
    same_bits(t1.bias, t2.bias, "bias")
    assert t1.step == t2.step
    logits2 = torch.cat(logits2)
    same_bits(logit, logits2, "logit_out")
    same_bits(loss, torch.cat(losses2), "loss_out")
    assert torch.equal(pred.bool().cpu(), (logits2[0::2] > logits2[1::2]).cpu())
    assert 0 < int(pred.sum()) < N or N < 4


def test_online_run_flags_an_out_of_range_index(fmx):
    sizes, k = SHAPES["a"]
    t, _ = build_table(fmx, sizes, k, "weights")
    eng = fmx.FMEngine(t, max_batch=16)
    rows, _, _ = make_pairs(sizes, 8, seed=1)
    rows[7, 2] = sizes[2] + 3                                     # the negative of pair 3
    idx_d, _ = dev(eng, rows, None)
    pred, _, _ = eng.pair_online_run(fmx.Hyper(**HYP), "sgd", idx_d, None)
    torch.cuda.synchronize()
    assert int(eng.error.item()) == 1
    with pytest.raises(IndexError):
        eng.check_error_flag()
    wide = fmx.FlatTable([7] * 70, 16)
    e2 = fmx.FMEngine(wide, max_batch=4)
    with pytest.raises(fmx._lib.FmxError) as ei:
        e2.pair_online_run(fmx.Hyper(**HYP), "sgd", torch.zeros((4, 70), dtype=torch.int32, device="cuda"), None)
    assert ei.value.code == fmx._lib.ERR_UNSUPPORTED


# ---- 7. the classes ----
def new_model(rule, sizes=SMALL, k=10, seed=21):
    from models.models_online_deep.fm_adam import FMAdam
    torch.manual_seed(seed)
    return FMAdam(sizes, embedding_size=k, n=0.01, update_rule=rule)


def class_data(B, seed=4):
    rows, x, item = make_pairs(SMALL, B, seed=seed, n_item=2, real_x=True)
    return rows[0::2].copy(), x[0::2].copy(), item, rows[1::2][:, item].copy()


def test_fit_pairs_is_the_engine_call(fmx):
    Xi, Xv, item, neg = class_data(33)
    a, b = new_model("signadam"), new_model("signadam")
    same_bits(a._table.rows, b._table.rows, "the same seed gives the same model")
    la = a.fit_pairs(Xi, Xv, item, negatives=neg, margin=0.1)
    rows, xv = fmx.pairwise.assemble_pairs(torch.from_numpy(Xi).cuda(), torch.from_numpy(Xv).cuda(), item, torch.from_numpy(neg).cuda())
    b._engine.pair_step(b._hyper, "signadam", rows, xv, margin=0.1)
    torch.cuda.synchronize()
    same_bits(a._table.rows, b._table.rows, "rows")
    same_bits(a._table.bias, b._table.bias, "bias")
    same_bits(la.reshape(1), b._engine.loss_out, "loss")
    assert float(la) > 0
    # sampled negatives under a seeded generator: two models end identical; another seed gives another model
    models = []
    for seed in (5, 5, 6):
        m = new_model("adam")
        g = torch.Generator(device="cuda").manual_seed(seed)
        for _ in range(3):
            m.fit_pairs(Xi, Xv, item, n_neg=2, generator=g)
        models.append(m)
    torch.cuda.synchronize()
    same_bits(models[0]._table.rows, models[1]._table.rows, "seeded sampling")
    assert models[0]._table.step == 3 and not torch.equal(models[0]._table.rows, models[2]._table.rows)
    with pytest.raises(IndexError):
        a.fit_pairs(Xi, Xv, item, negatives=neg + 100)


@pytest.mark.parametrize("rule", ["signadam", "adam"])
def test_run_pair_experiment_is_the_host_loop(fmx, rule):
    N = 64
    Xi, Xv, item, neg = class_data(N, seed=8)
    a, b, c = new_model(rule), new_model(rule), new_model(rule)
    assert a._device_loop_ok()
    secs, acc, checkpoints, counts = a.run_pair_experiment(Xi, Xv, item, negatives=neg, margin=0.0)
    correct = 0
    rows, xv = fmx.pairwise.assemble_pairs(torch.from_numpy(Xi), torch.from_numpy(Xv), item, torch.from_numpy(neg))
    for i in range(N):
        z = b.forward_fm(rows[2 * i:2 * i + 2].numpy(), xv[2 * i:2 * i + 2].numpy())
        correct += int(z[0] > z[1])
        b.fit_pairs(Xi[i:i + 1], Xv[i:i + 1], item, negatives=neg[i:i + 1])
    torch.cuda.synchronize()
    same_bits(a._table.rows, b._table.rows, "rows")
    same_bits(a._table.bias, b._table.bias, "bias")
    assert counts == {"correct": correct, "wrong": N - correct} and a._table.step == b._table.step
    assert acc == checkpoints[-1] == pytest.approx(100.0 * correct / N) and len(checkpoints) == 2 and secs > 0
    # the same call where the device loop is not taken: the loop over fit_pairs inside run_pair_experiment
    c.device_online_loop = False
    _, acc_c, cp_c, counts_c = c.run_pair_experiment(Xi, Xv, item, negatives=neg, margin=0.0)
    same_bits(a._table.rows, c._table.rows, "rows (host loop)")
    assert counts_c == counts and cp_c == checkpoints and acc_c == acc
