"""Listwise (sampled-softmax) training of the FM on the device: fmx_fm_list_forward / _step / _stream and FMAdam.fit_lists.

Shapes: four small fields, so rows repeat -- runs in the update, rows several rows of a list name (the shared context, a negative
that equals its positive).  k in {4, 16} (kp 4 and 16); G in {2, 3, 4, 5, 8, 16} gives 4, 3, 4, 5, 8, 16 waves per workgroup;
B_lists in {1, 3}: G = 2 with three lists leaves the second workgroup half empty, G = 3 and 5 and larger put every list in a
workgroup of its own.  The tolerance against tests/list_f64.py is test_pair_gpu.py's: 1e-5 |ref| + the fp32 floor."""
import ctypes as C

import numpy as np
import pytest
import torch

from abi_geometry import PATTERN, Guarded
from helpers import assert_ftrl_step_within_f64, assert_within_f64
from list_f64 import list_step_f64
from test_kernels_gpu import HYP
from test_pair_gpu import RULES, build_table, clone_table, dev, same_bits

pytestmark = pytest.mark.gpu

SIZES = [7, 5, 11, 3]
ITEM = [2, 3]
GS = [2, 3, 4, 5, 8, 16]
FLT_MIN = 1.1754944e-38


@pytest.fixture(scope="module")
def fmx():
    import fmx as _fmx
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _fmx


def make_lists(B, G, seed, real_x=False):
    """-> (rows int32 [B G, F] local indices, x float32 [B G, F] or None): a list's negatives are its positive with the item columns
    (ITEM) redrawn; the last negative of list 0 keeps its positive's items (and values): a negative that equals its positive."""
    rng = np.random.default_rng(seed)
    F = len(SIZES)
    pos = np.stack([rng.integers(0, s, size=B) for s in SIZES], axis=1)
    rows = np.repeat(pos[:, None, :], G, axis=1)
    for f in ITEM:
        rows[:, 1:, f] = rng.integers(0, SIZES[f], size=(B, G - 1))
    if G >= 3:                                            # (at G = 2 the list would be two equal rows: no gradient at all)
        rows[0, G - 1] = rows[0, 0]
    x = None
    if real_x:
        x = rng.uniform(0.5, 1.5, size=(B, G, F)).astype(np.float32)
        x[:, :, :2] = x[:, :1, :2]                        # the context's values are the list's
        if G >= 3:
            x[0, G - 1] = x[0, 0]
        x = x.reshape(B * G, F)
    return rows.reshape(B * G, F).astype(np.int32), x


def reference(t, pr, rows, x, G, rule, B):
    grows = rows.astype(np.int64) + np.asarray(t.offsets_host[:-1], np.int64)[None, :]
    xx = x if x is not None else np.ones(rows.shape, np.float32)
    if rule == "ftrl":
        h = dict(alpha=HYP["alpha"], beta=HYP["beta"], l1=HYP["l1"], l2=HYP["l2"])
        return list_step_f64(pr["ftrl_state"], grows, xx, G, "ftrl", h, inv_b=1.0 / B)
    return list_step_f64(dict(V=pr["V"], w=pr["w"], bias=pr["bias"]), grows, xx, G, "sgd", dict(lr=HYP["lr"]), inv_b=1.0 / B)


def within(got, ref, floor, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err, tol = np.abs(got - ref), 1e-5 * np.abs(ref) + floor
    print(f"{what}: worst err/tol {float((err / np.maximum(tol, 1e-300)).max()):.3f}")
    assert_within_f64(got, ref, floor, what)


# ---- 1. forward: fmx_fm_forward's outputs bit for bit, the epilogue and the step within the float64 evaluation ----
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("k", [4, 16])
def test_forward_and_step_within_float64(fmx, k, G, B):
    N = B * G
    hyp = fmx.Hyper(**HYP)
    for real_x in (False, True):
        rows, x = make_lists(B, G, seed=31 * G + B, real_x=real_x)
        for rule in ("sgd", "ftrl"):
            what = f"k={k} G={G} B={B} x={real_x} {rule}"
            t, pr = build_table(fmx, SIZES, k, RULES[rule], seed=7)
            eng = fmx.FMEngine(t, max_batch=N)
            idx_d, xv_d = dev(eng, rows, x)
            eng.forward(hyp, idx_d, xv_d)                                   # FMX_LOSS_NONE
            want = [b[:N].clone() for b in (eng.S, eng.sfirst, eng.sbi, eng.logit, eng.bi, eng.first)]
            for b in (eng.S, eng.sfirst, eng.sbi, eng.logit, eng.bi, eng.first, eng.loss_b, eng.dz):
                b.fill_(float("nan"))
            assert eng.list_forward(hyp, idx_d, G, xv_d, want_first=True, want_bi=True) == B
            torch.cuda.synchronize()
            eng.check_error_flag()
            for name, w, b in zip(("S", "sfirst", "sbi", "logit", "bi", "first"), want,
                                  (eng.S, eng.sfirst, eng.sbi, eng.logit, eng.bi, eng.first)):
                same_bits(b[:N], w, f"{what} {name}")
            ref = reference(t, pr, rows, x, G, rule, B)
            loss, dz = eng.loss_b[:N].cpu().numpy(), eng.dz[:N].cpu().numpy()
            assert np.isfinite(loss).all() and np.isfinite(dz).all(), what
            within(loss, ref["loss_b"], ref["floor"]["loss_b"], what + " loss")
            within(dz, ref["dz"], ref["floor"]["dz"], what + " dz")
            slots = loss.reshape(B, G)[:, 1:]
            assert (slots.view(np.int32) == 0).all(), what + ": the negatives' loss slots hold +0"
            assert (dz.reshape(B, G)[:, 0] < 0).all() and (dz.reshape(B, G)[:, 1:] > 0).all(), what
            # the step
            bias0 = t.bias.clone()
            eng.list_step(hyp, rule, idx_d, G, xv_d)
            torch.cuda.synchronize()
            eng.check_error_flag()
            same_bits(t.bias, bias0, what + " bias")
            within(float(eng.loss_out.item()), ref["loss"], ref["floor"]["loss"], what + " loss_out")
            if rule == "ftrl":
                st0 = pr["ftrl_state"]
                zV, nV, zw, nw = [a.numpy() for a in t.export_ftrl_state()]
                assert_ftrl_step_within_f64(dict(zV=zV, nV=nV, zw=zw, nw=nw, zb=t.bias[0].item(), nb=t.bias[1].item()), ref, before=st0)
                continue
            u, new, fl = ref["urows"], ref["new"], ref["floor"]
            got = dict(V=t.rows[:, :k].cpu().numpy(), w=t.rows[:, t.kp].cpu().numpy())
            for kk in ("V", "w"):
                b0 = np.asarray(pr[kk], np.float64)[u]
                within(got[kk][u], new[kk][u], fl[kk], f"{what} {kk}")
                within(got[kk][u].astype(np.float64) - b0, new[kk][u] - b0, fl[kk], f"{what} {kk} (the step)")
                mask = np.ones(len(got[kk]), bool)
                mask[u] = False
                np.testing.assert_array_equal(got[kk][mask], pr[kk][mask], err_msg=kk + " untouched rows")
                assert np.abs(new[kk][u] - b0).max() > 0
            assert float(t.bias[0].item()) == float(new["bias"])


# ---- 2. one list whose logits lie 200 apart ----
@pytest.mark.parametrize("row", [0, 2])
@pytest.mark.parametrize("k", [4, 16])
def test_logits_200_apart(fmx, k, row):
    G, B = 4, 1
    rows, x = make_lists(B, G, seed=3, real_x=True)
    rows[G - 1, ITEM[0]] = (rows[0, ITEM[0]] + 1) % SIZES[ITEM[0]]          # (no twin of the positive here)
    t, pr = build_table(fmx, SIZES, k, "weights", seed=7)
    others = [j for j in range(G) if j != row]
    for _ in range(40):                                                     # scale one row's values until it is 200 from the rest
        z = reference(t, pr, rows, x, G, "sgd", B)["logit"]                 # (201: the fp32 logits then differ by 200 as well)
        if np.abs(z[row] - z[others]).min() >= 201:
            break
        x[row] *= 1.5
    assert np.abs(z[row] - z[others]).min() >= 201 and np.abs(z).max() < 1e6
    eng = fmx.FMEngine(t, max_batch=G)
    idx_d, xv_d = dev(eng, rows, x)
    eng.list_forward(fmx.Hyper(**HYP), idx_d, G, xv_d)
    torch.cuda.synchronize()
    ref = reference(t, pr, rows, x, G, "sgd", B)
    loss, dz, zd = eng.loss_b[:G].cpu().numpy(), eng.dz[:G].cpu().numpy(), eng.logit[:G].cpu().numpy().astype(np.float64)
    assert np.isfinite(loss).all() and np.isfinite(dz).all() and np.isfinite(zd).all()
    within(loss, ref["loss_b"], ref["floor"]["loss_b"], f"k={k} row={row} loss")
    within(dz, ref["dz"], ref["floor"]["dz"], f"k={k} row={row} dz")
    lost = zd <= zd.max() - 200
    assert lost.any()
    for j in np.flatnonzero(lost):
        if j >= 1 or zd[0] == zd.max():
            assert abs(dz[j]) < FLT_MIN, (j, dz[j])                          # a negative 200 below the best: exp(-200) / s is 0 in fp32
    if zd[0] == zd.max():
        assert abs(dz[0]) < FLT_MIN and abs(loss[0]) <= ref["floor"]["loss_b"][0]
    elif lost[0]:
        assert loss[0] >= 200 and dz[0] < 0


# ---- 3. the bias and its state are bit-unchanged by a step, under every rule ----
@pytest.mark.parametrize("rule", list(RULES))
def test_bias_is_bit_unchanged(fmx, rule):
    G, B = 5, 3
    t, _ = build_table(fmx, SIZES, 10, RULES[rule])             # moments tables: bias moments 1e-3 / 1e-4 and step 3 beforehand
    if RULES[rule] == "moments":
        assert float(t.bias[1]) != 0 and float(t.bias[2]) != 0
    eng = fmx.FMEngine(t, max_batch=B * G)
    hyp = fmx.Hyper(**HYP)
    rows0 = t.rows.clone()
    for s in range(3):
        rows, x = make_lists(B, G, seed=40 + s, real_x=bool(s % 2))
        idx_d, xv_d = dev(eng, rows, x)
        bias0 = t.bias.clone()
        eng.list_step(hyp, rule, idx_d, G, xv_d)
        torch.cuda.synchronize()
        eng.check_error_flag()
        same_bits(t.bias, bias0, f"{rule} step {s}: bias and its state")
    assert not torch.equal(t.rows, rows0)
    assert t.step == (6 if RULES[rule] == "moments" else t.step)


# ---- 4. the stream is its steps ----
@pytest.mark.parametrize("rule", ["signadam", "adam"])
@pytest.mark.parametrize("B", [7, 171])                         # 171 lists of 3: 513 rows, the sorts run ahead on the side stream
def test_stream_is_its_steps(fmx, rule, B):
    stream_is_its_steps(fmx, rule, B, n_pool=3, n_steps=5)


@pytest.mark.parametrize("own_stream", [False, True])
@pytest.mark.parametrize("rule", ["signadam", "adam"])
@pytest.mark.parametrize("B", [7, 171])
def test_stream_is_its_steps_through_the_whole_loop(fmx, rule, B, own_stream):
    """37 steps over a pool of 5: sort groups of 4 + 16 + 16 + 1, so both halves of the sorted ring are used again and the pool
    wraps.  171 lists of 3 are 513 rows, over OVERLAP_MIN_BATCH (the sorts run ahead on the side stream); 7 lists are under it
    (every group is sorted in front of its steps).  From torch's default stream (handle 0: the loop detours off it) and from a
    stream of its own."""
    stream_is_its_steps(fmx, rule, B, n_pool=5, n_steps=37, own_stream=own_stream)


def stream_is_its_steps(fmx, rule, B, n_pool, n_steps, own_stream=False):
    G, k = 3, 10
    t1, _ = build_table(fmx, SIZES, k, RULES[rule])
    t2 = clone_table(fmx, t1)
    e1, e2 = fmx.FMEngine(t1, max_batch=B * G), fmx.FMEngine(t2, max_batch=B * G)
    pool = np.stack([make_lists(B, G, seed=100 + j)[0] for j in range(n_pool)])
    pool_d = torch.from_numpy(pool).cuda().contiguous()
    losses1 = torch.full((n_steps,), float("nan"), device="cuda")
    side = torch.cuda.Stream() if own_stream else torch.cuda.default_stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert (torch.cuda.current_stream().cuda_stream == 0) != own_stream
        e1.list_stream(fmx.Hyper(**HYP), rule, pool_d, G, n_steps, loss_out=losses1)
        h2, losses2 = fmx.Hyper(**HYP), []
        for s in range(n_steps):
            e2.list_step(h2, rule, pool_d[s % n_pool], G)
            losses2.append(e2.loss_out.clone())
    torch.cuda.synchronize()
    e1.check_error_flag()
    e2.check_error_flag()
    same_bits(t1.rows, t2.rows, "rows")
    same_bits(t1.bias, t2.bias, "bias")
    same_bits(losses1, torch.cat(losses2), "loss_out")
    assert t1.step == t2.step == (3 + n_steps if rule == "adam" else t1.step)


# ---- 5. a list's result does not depend on its place in the batch ----
@pytest.mark.parametrize("G", [2, 3, 8, 16])
def test_a_list_alone_and_inside_a_batch(fmx, G):
    t, _ = build_table(fmx, SIZES, 10, "weights")
    eng = fmx.FMEngine(t, max_batch=3 * G)
    hyp = fmx.Hyper(**HYP)
    rows, x = make_lists(3, G, seed=G, real_x=True)
    idx_d, xv_d = dev(eng, rows, x)
    eng.list_forward(hyp, idx_d, G, xv_d, inv_b=0.25)
    torch.cuda.synchronize()
    loss3, dz3, z3 = eng.loss_b[G:2 * G].clone(), eng.dz[G:2 * G].clone(), eng.logit[G:2 * G].clone()
    eng.loss_b.fill_(float("nan"))
    eng.dz.fill_(float("nan"))
    eng.list_forward(hyp, idx_d[G:2 * G].contiguous(), G, xv_d[G:2 * G].contiguous(), inv_b=0.25)   # list 2 of 3, alone
    torch.cuda.synchronize()
    same_bits(eng.logit[:G], z3, "logit")
    same_bits(eng.loss_b[:G], loss3, "loss")
    same_bits(eng.dz[:G], dz3, "dz")


# ---- 6. nothing is written behind loss, dz, S or the workspace (the 16 scratch bytes are its last) ----
@pytest.mark.parametrize("rule", ["signadam", "ftrl", "adam"])
@pytest.mark.parametrize("G,B", [(5, 3), (16, 3), (2, 3)])
def test_guard_bands(fmx, rule, G, B):
    L = fmx._lib
    lib = L.load()
    N = B * G
    t, _ = build_table(fmx, SIZES, 10, RULES[rule])
    rows, x = make_lists(B, G, seed=9, real_x=True)
    idx_d = torch.from_numpy(rows).cuda().contiguous()
    xv_d = torch.from_numpy(x).cuda().contiguous()
    need = int(lib.fmx_fm_list_workspace_bytes(t.c_struct(), B, G))
    assert need == int(lib.fmx_workspace_bytes(t.c_struct(), N)) + 16
    bufs = dict(S=Guarded(N * t.kp * 4, name="S"), loss=Guarded(N * 4, name="loss"), dz=Guarded(N * 4, name="dz"),
                logit=Guarded(N * 4, name="logit"), ws=Guarded(need, torch.int32, name="workspace"),
                loss_out=Guarded(4, name="loss_out"), error=Guarded(4, torch.int32, name="error"))
    out = L.FwdOut()
    out.S, out.loss, out.dz, out.logit, out.error = (bufs[n].ptr for n in ("S", "loss", "dz", "logit", "error"))
    hyp = fmx.Hyper(**HYP)
    hyp.c.step = t.step
    st = torch.cuda.current_stream().cuda_stream
    bias0 = t.bias.clone()
    L.check(lib.fmx_fm_list_forward(t.c_struct(), hyp.ref(), idx_d.data_ptr(), xv_d.data_ptr(), B, G, 1.0 / B, C.byref(out), st))
    L.check(lib.fmx_fm_list_step(t.c_struct(), hyp.ref(), L.RULES[rule], idx_d.data_ptr(), xv_d.data_ptr(), B, G, 1.0 / B,
                                 bufs["ws"].ptr, need, C.byref(out), bufs["loss_out"].ptr, st))
    torch.cuda.synchronize()
    for g in bufs.values():
        g.check()
    assert int(bufs["error"].t.item()) == 0
    assert np.isfinite(bufs["loss_out"].t.cpu().numpy()).all() and float(bufs["loss_out"].t.item()) > 0
    assert (bufs["loss"].t.view(torch.int32) != PATTERN).all() and (bufs["dz"].t.view(torch.int32) != PATTERN).all()
    same_bits(t.bias, bias0, "bias")
    # a workspace without the scratch bytes is refused, nothing launched
    rc = lib.fmx_fm_list_step(t.c_struct(), hyp.ref(), L.RULES[rule], idx_d.data_ptr(), xv_d.data_ptr(), B, G, 1.0 / B,
                              bufs["ws"].ptr, need - 16, C.byref(out), bufs["loss_out"].ptr, st)
    assert rc == L.ERR_SHAPE


# ---- 7. the classes ----
def new_model(rule, sizes, k=10, seed=21):
    from models.models_online_deep.fm_adam import FMAdam
    torch.manual_seed(seed)
    return FMAdam(sizes, embedding_size=k, n=0.01, update_rule=rule)


def test_fit_lists_is_the_engine_call(fmx):
    B, n_neg = 33, 3
    rows, x = make_lists(B, 1 + n_neg, seed=4, real_x=True)
    lists, xl = rows.reshape(B, 1 + n_neg, -1), x.reshape(B, 1 + n_neg, -1)
    Xi, Xv, neg = lists[:, 0].copy(), xl[:, 0].copy(), lists[:, 1:][:, :, ITEM].copy()
    a, b = new_model("signadam", SIZES), new_model("signadam", SIZES)
    same_bits(a._table.rows, b._table.rows, "the same seed gives the same model")
    la = a.fit_lists(Xi, Xv, ITEM, negatives=neg)
    idx, xv = fmx.pairwise.assemble_lists(torch.from_numpy(Xi).cuda(), torch.from_numpy(Xv).cuda(), ITEM, torch.from_numpy(neg).cuda())
    assert idx.shape == (B * (1 + n_neg), len(SIZES))
    bias0 = b._table.bias.clone()
    b._engine.list_step(b._hyper, "signadam", idx, 1 + n_neg, xv)
    torch.cuda.synchronize()
    same_bits(a._table.rows, b._table.rows, "rows")
    same_bits(a._table.bias, b._table.bias, "bias")
    same_bits(a._table.bias, bias0, "bias untouched")
    same_bits(la.reshape(1), b._engine.loss_out, "loss")
    assert float(la) > 0
    with pytest.raises(IndexError):
        a.fit_lists(Xi, Xv, ITEM, negatives=neg + 100)
    with pytest.raises(ValueError, match="15"):
        a.fit_lists(Xi, Xv, ITEM, negatives=np.zeros((B, 16, 2), np.int64))
    # uniform draws under a seeded generator: two models end identical; another seed gives another model
    models = []
    for seed in (5, 5, 6):
        m = new_model("adam", SIZES)
        g = torch.Generator(device="cuda").manual_seed(seed)
        for _ in range(3):
            m.fit_lists(Xi, Xv, ITEM, generator=g)                          # n_neg = 4
        models.append(m)
    torch.cuda.synchronize()
    same_bits(models[0]._table.rows, models[1]._table.rows, "seeded sampling")
    assert models[0]._table.step == 3 and not torch.equal(models[0]._table.rows, models[2]._table.rows)


def test_fit_lists_hard_negatives_are_reproducible(fmx):
    sizes, item = [7, 5, 11], [2]
    rng = np.random.default_rng(2)
    Xi = np.stack([rng.integers(0, s, size=24) for s in sizes], axis=1).astype(np.int32)
    models, losses = [], []
    for seed in (5, 5, 6):
        m = new_model("signadam", sizes)
        g = torch.Generator(device="cuda").manual_seed(seed)
        hard = fmx.pairwise.HardNegatives(n_draw=8)
        losses.append([float(m.fit_lists(Xi, None, item, negatives=hard, n_neg=3, generator=g)) for _ in range(3)])
        models.append(m)
    torch.cuda.synchronize()
    same_bits(models[0]._table.rows, models[1]._table.rows, "the same state, seed and call numbers: the same model")
    assert losses[0] == losses[1] and all(np.isfinite(losses[0]))
    assert not torch.equal(models[0]._table.rows, models[2]._table.rows)
    assert models[0]._mining_offset == 3


def test_fit_lists_raises_the_positive_items_rank(fmx):
    sizes, item, fav = [6, 4, 20], [2], 13
    rng = np.random.default_rng(1)
    ctx = np.stack([rng.integers(0, s, size=64) for s in sizes[:2]], axis=1)
    Xi = np.concatenate([ctx, np.full((64, 1), fav)], axis=1).astype(np.int32)
    m = new_model("signadam", sizes)
    targets = np.full(64, fav)
    before = m.evaluate_ranking(Xi, None, item, targets)
    g = torch.Generator(device="cuda").manual_seed(7)
    for _ in range(50):
        m.fit_lists(Xi, None, item, n_neg=4, generator=g)
    after = m.evaluate_ranking(Xi, None, item, targets)
    print("before", before, "after", after)
    assert after["n"] == before["n"] == 64
    assert after["auc"] > before["auc"]                                     # auc = 1 - mean rank / (N - 1): the mean rank went down
    assert after["mrr"] > before["mrr"]
