"""fmx_afm_side / fmx_afm_topk and AFMAdam.recommend on the GPU: the kernels against the float64 AFM of every assembled
(context, candidate) sample (tests/afm_f64.py) with its fp32 floor (score, order, set optimality, padding), bit-identical scores
across user subsets, candidate permutations, splits and repeated calls, exclusions / NaN rows / -0 / single-field sides, and
recommend() against forward() on the assembled samples, fresh and after training under every rule."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from afm_f64 import U32, afm_f64, live_params  # noqa: E402
from test_afm_gpu import make  # noqa: E402
from test_recommend_mlp_gpu import check_rows  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _rec():
    from fmx import recommend
    return recommend


def sizes_for(F, seed):
    rng = np.random.default_rng(seed)
    return [int(s) for s in rng.integers(2, 60, size=F)]


def inputs(sizes, U, N, seed, xv_kind):
    rng = np.random.default_rng(seed)
    ctx = np.stack([rng.integers(0, s, size=U) for s in sizes], axis=1).astype(np.int32)
    cand = np.stack([rng.integers(0, s, size=N) for s in sizes], axis=1).astype(np.int32)
    cx = kx = None
    if xv_kind == "random":
        cx = rng.uniform(0.2, 1.8, size=ctx.shape).astype(np.float32)
        kx = rng.uniform(0.2, 1.8, size=cand.shape).astype(np.float32)
    return ctx, cx, cand, kx


def assembled(sizes, item, ctx, cx, cand, kx, users=None):
    """rows [U * N, F] (global row numbers) and xv of every (u, c) sample: item columns from c, the others from u"""
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    users = np.arange(ctx.shape[0]) if users is None else np.asarray(users)
    U, N, F = len(users), cand.shape[0], len(sizes)
    isitem = np.zeros(F, bool)
    isitem[item] = True
    idx = np.where(isitem[None, None, :], cand[None, :, :], ctx[users][:, None, :]).reshape(U * N, F)
    ones_c = np.ones(ctx.shape, np.float32) if cx is None else cx
    ones_k = np.ones(cand.shape, np.float32) if kx is None else kx
    xv = np.where(isitem[None, None, :], ones_k[None, :, :], ones_c[users][:, None, :]).reshape(U * N, F)
    return idx, idx.astype(np.int64) + offs[:-1][None, :], xv


def brute(st, k, t, rows, xv, U, N, params=None):
    F = rows.shape[1]
    chunk = max(1, (1 << 22) // max(1, F * F * max(k, t)))
    out = afm_f64(st["V"], st["w"], st["bias"], st["params"] if params is None else params, k, t, rows, xv, chunk=chunk)
    score = torch.from_numpy(out["logit"]).reshape(U, N).to(DEV)
    tol = torch.from_numpy(4 * out["floor_logit"] + 16 * U32 * np.abs(out["logit"])).reshape(U, N).to(DEV) + 1e-30
    return score, tol


def run(F, item, k, t, U, N, K, xv_kind="random", live=False, seed=0, exclude=None):
    rec = _rec()
    sizes = sizes_for(F, seed)
    tb, params, st = make(sizes, k, t, seed=seed)
    ctx, cx, cand, kx = inputs(sizes, U, N, seed + 1, xv_kind)
    _, rows, xv = assembled(sizes, item, ctx, cx, cand, kx)
    if live:
        p = live_params(st["params"], st["V"], k, t, rows, xv, chunk=4096)
        params.copy_(torch.from_numpy(p))
        st["params"] = p
    afm = (params, t)
    cands = rec.AFMCandidates(tb, afm, item, cand, kx)
    pos, val = rec.topk_afm(tb, afm, ctx, cx, cands, K, exclude=exclude)
    torch.cuda.synchronize()
    score, tol = brute(st, k, t, rows, xv, U, N)
    return dict(tb=tb, afm=afm, cands=cands, ctx=ctx, cx=cx, cand=cand, kx=kx, pos=pos, val=val, score=score, tol=tol, sizes=sizes)


CASES = [  # (F, item fields, k, t, U, N, K, live)
    (2, [1], 4, 1, 17, 2049, 10, False),           # both sides a single field (m = -inf)
    (2, [0], 10, 4, 1, 63, 256, True),
    (3, [0], 10, 4, 1, 100003, 100, False),        # several splits, the merge
    (3, [1], 4, 64, 17, 1, 10, True),              # N < K: padding
    (13, [6], 16, 16, 17, 2049, 256, True),
    (13, [2, 9], 64, 4, 300, 63, 1, False),        # two non-adjacent item fields
    (13, [12], 16, 64, 7, 2049, 100, False),
    (39, [38], 16, 16, 17, 63, 10, True),
    (39, [0], 10, 1, 300, 31, 10, False),
]


@pytest.mark.parametrize("F, item, k, t, U, N, K, live", CASES)
def test_topk_matches_f64(F, item, k, t, U, N, K, live):
    r = run(F, item, k, t, U, N, K, live=live)
    check_rows(r["pos"], r["val"], r["score"], r["tol"], K)
    valid = r["pos"] >= 0
    assert bool(torch.isfinite(r["val"][valid]).all())


def test_topk_ones_xv_large_split():
    r = run(5, [2], 16, 16, 3, 120000, 10, xv_kind="ones", seed=3)
    check_rows(r["pos"], r["val"], r["score"], r["tol"], 10)


def test_user_alone_is_bit_identical_to_inside_a_batch():
    rec = _rec()
    r = run(13, [6], 16, 16, 300, 2049, 10, seed=5)
    for u in (0, 151, 299):
        cx = None if r["cx"] is None else r["cx"][u:u + 1]
        p1, v1 = rec.topk_afm(r["tb"], r["afm"], r["ctx"][u:u + 1], cx, r["cands"], 10)
        assert torch.equal(p1[0], r["pos"][u])
        assert torch.equal(v1[0].view(torch.int32), r["val"][u].view(torch.int32))


def test_permuted_candidates_and_repeated_calls_give_the_same_bits():
    rec = _rec()
    r = run(13, [2, 9], 16, 16, 17, 63, 100, seed=7)          # K > N: every candidate comes back with its score
    perm = np.random.default_rng(0).permutation(63)
    c2 = rec.AFMCandidates(r["tb"], r["afm"], [2, 9], r["cand"][perm], r["kx"][perm])
    p2, v2 = rec.topk_afm(r["tb"], r["afm"], r["ctx"], r["cx"], c2, 100)
    s1 = torch.full((17, 63), float("nan"), device=DEV)
    s2 = torch.full((17, 63), float("nan"), device=DEV)
    ok1, ok2 = r["pos"] >= 0, p2 >= 0
    for u in range(17):
        s1[u, r["pos"][u][ok1[u]]] = r["val"][u][ok1[u]]
        s2[u, torch.from_numpy(perm).to(DEV)[p2[u][ok2[u]]]] = v2[u][ok2[u]]
    assert torch.equal(s1.view(torch.int32), s2.view(torch.int32))
    p3, v3 = rec.topk_afm(r["tb"], r["afm"], r["ctx"], r["cx"], r["cands"], 100)
    assert torch.equal(p3, r["pos"]) and torch.equal(v3.view(torch.int32), r["val"].view(torch.int32))


def test_exclusions_as_lists_and_csr():
    rec = _rec()
    U, N, K = 17, 2049, 10
    r = run(13, [6], 16, 16, U, N, K, seed=9)
    rng = np.random.default_rng(1)
    lists = [np.concatenate([r["pos"][u, :5].cpu().numpy(), rng.integers(0, N, size=30), [N + 5, -3]]) for u in range(U)]
    excl = torch.zeros(U, N, dtype=torch.bool, device=DEV)
    for u, l in enumerate(lists):
        l = l[(l >= 0) & (l < N)]
        excl[u, torch.from_numpy(l).to(DEV)] = True
    p1, v1 = rec.topk_afm(r["tb"], r["afm"], r["ctx"], r["cx"], r["cands"], K, exclude=lists)
    check_rows(p1, v1, r["score"], r["tol"], K, excluded=excl)
    off = np.concatenate([[0], np.cumsum([len(l) for l in lists])])
    p2, v2 = rec.topk_afm(r["tb"], r["afm"], r["ctx"], r["cx"], r["cands"], K, exclude=(off, np.concatenate(lists)))
    assert torch.equal(p1, p2) and torch.equal(v1.view(torch.int32), v2.view(torch.int32))
    # every candidate excluded for user 0: a padded row
    lists[0] = np.arange(N)
    p3, v3 = rec.topk_afm(r["tb"], r["afm"], r["ctx"], r["cx"], r["cands"], K, exclude=lists)
    assert bool((p3[0] == -1).all()) and bool((v3[0] == float("-inf")).all())


def test_nan_row_is_never_returned():
    rec = _rec()
    sizes = sizes_for(5, 11)
    tb, params, st = make(sizes, 16, 16, seed=11)
    ctx, cx, cand, kx = inputs(sizes, 4, 200, 12, "random")
    offs = np.concatenate([[0], np.cumsum(sizes)])
    bad = int(cand[0, 3])
    tb.rows[int(offs[3]) + bad, 2] = float("nan")
    cands = rec.AFMCandidates(tb, (params, 16), [3], cand, kx)
    pos, val = rec.topk_afm(tb, (params, 16), ctx, cx, cands, 200)
    nan_pos = set(np.nonzero(cand[:, 3] == bad)[0].tolist())
    got = set(pos[pos >= 0].cpu().numpy().tolist())
    assert not (got & nan_pos)
    assert bool(((pos >= 0).sum(1) == 200 - len(nan_pos)).all())
    assert not bool(torch.isnan(val).any())


def test_negative_zero_is_returned_as_positive_zero():
    rec = _rec()
    k, t = 4, 2
    params = torch.zeros(t * k + 2 * t + k, device=DEV)
    params[:t * k] = torch.randn(t * k, device=DEV)                # W; b = h = p = 0: every cross s and r is 0
    Eu = torch.randn(1, 1, 4, device=DEV)
    Ec = torch.randn(3, 1, 4, device=DEV)
    su = torch.tensor([[-0.0, 0.0, 1e30, -1e-30]], device=DEV)     # R / Z underflows to -0, lin = -0
    sc = torch.tensor([[-0.0, float("-inf"), 0.0, 0.0]] * 3, device=DEV)
    pos, val = rec.afm_topk((params, t), k, Eu, su, Ec, sc, 5)
    torch.cuda.synchronize()
    assert pos[0, :3].tolist() == [0, 1, 2] and pos[0, 3:].tolist() == [-1, -1]
    assert val[0, :3].view(torch.int32).tolist() == [0, 0, 0]


# ---------------------------------------------------------------------------------------------------------------------------
# AFMAdam.recommend against forward() on the assembled samples
# ---------------------------------------------------------------------------------------------------------------------------
def _model(rule, sizes, k=8, t=8, seed=0):
    from models.models_online_deep.afm_adam import AFMAdam
    torch.manual_seed(seed)
    return AFMAdam(sizes, embedding_size=k, attention_size=t, batch_size=64, n=0.05, update_rule=rule)


def _train(m, sizes, steps, seed=1):
    rng = np.random.default_rng(seed)
    for _ in range(steps):
        Xi = np.stack([rng.integers(0, s, size=64) for s in sizes], axis=1)
        Xv = rng.uniform(0.5, 1.5, size=Xi.shape).astype(np.float32)
        y = (rng.uniform(size=64) < 0.4).astype(np.float32)
        m.update_embedding(Xi, Xv, y)


def _check_against_forward(m, sizes, item, Xi, Xv, pos, logit, cand_idx=None, cand_xv=None):
    U, K = pos.shape
    if cand_idx is None:
        f = item[0]
        cand_idx = np.zeros((sizes[f], len(sizes)), np.int64)
        cand_idx[:, f] = np.arange(sizes[f])
    N = cand_idx.shape[0]
    idx, _, xv = assembled(sizes, item, np.asarray(Xi), Xv, np.asarray(cand_idx), cand_xv)
    ref = m.forward(idx, xv).detach().reshape(U, N).double().cpu().numpy()
    tol = 2e-5 * (1 + np.abs(ref))
    for u in range(U):
        ok = pos[u] >= 0
        assert ok.sum() == min(K, N)
        got = logit[u][ok].astype(np.float64)
        assert np.all(np.abs(got - ref[u, pos[u][ok]]) <= tol[u, pos[u][ok]])
        assert np.all(np.diff(got) <= 0)
        rest = np.setdiff1d(np.arange(N), pos[u][ok])
        if len(rest):
            assert ref[u, rest].max() <= got.min() + 2 * tol[u].max()


@pytest.mark.parametrize("rule", ["adam", "adagrad", "signadam", "sgd", "ftrl"])
def test_recommend_matches_forward_after_training(rule):
    sizes = [7, 120, 5, 33, 9, 14]
    m = _model(rule, sizes)
    rng = np.random.default_rng(2)
    Xi = np.stack([rng.integers(0, s, size=9) for s in sizes], axis=1)
    Xv = rng.uniform(0.5, 1.5, size=Xi.shape).astype(np.float32)
    pos, logit = m.recommend(Xi, Xv, [1], 10)
    assert pos.dtype == np.int64 and logit.dtype == np.float32 and pos.shape == (9, 10)
    _check_against_forward(m, sizes, [1], Xi, Xv, pos, logit)
    before = logit.copy()
    _train(m, sizes, 3)
    pos, logit = m.recommend(Xi, Xv, [1], 10)
    assert not np.array_equal(before, logit)                      # the live tables and attention buffer are read
    _check_against_forward(m, sizes, [1], Xi, Xv, pos, logit)


def test_recommend_two_item_fields_with_explicit_candidates():
    sizes = [7, 120, 5, 33, 9, 14]
    m = _model("adam", sizes, k=10, t=4)
    _train(m, sizes, 2)
    rng = np.random.default_rng(4)
    Xi = np.stack([rng.integers(0, s, size=5) for s in sizes], axis=1)
    cand = np.stack([rng.integers(0, s, size=300) for s in sizes], axis=1)
    cxv = rng.uniform(0.5, 1.5, size=cand.shape).astype(np.float32)
    pos, logit = m.recommend(Xi, None, [1, 4], 20, candidates=(cand, cxv), full=True)
    _check_against_forward(m, sizes, [1, 4], Xi, None, pos, logit, cand, cxv)


def test_recommend_errors():
    rec = _rec()
    sizes = [7, 120, 5, 33]
    m = _model("sgd", sizes)
    Xi = np.zeros((2, 4), np.int64)
    bad = Xi.copy()
    bad[1, 2] = 5                                                 # field 2 has 5 rows
    with pytest.raises(IndexError):
        m.recommend(bad, None, [1], 5)
    with pytest.raises(ValueError):
        m.recommend(Xi, None, [0, 1, 2, 3], 5, candidates=(np.zeros((3, 4), np.int64), None))
    for K in (0, 257):
        with pytest.raises((ValueError, RuntimeError)):
            m.recommend(Xi, None, [1], K)
    other = _model("sgd", sizes, seed=1)
    cands = rec.AFMCandidates(other._table, (other._attn_flat, 8), [1], np.zeros((3, 4), np.int64))
    with pytest.raises(ValueError):
        rec.topk_afm(m._table, (m._attn_flat, 8), Xi, None, cands, 3)
    p4 = torch.zeros(8 * 4 + 2 * 4 + 8, device=DEV)
    c4 = rec.AFMCandidates(m._table, (p4, 4), [1], np.zeros((3, 4), np.int64))
    with pytest.raises(ValueError):
        rec.topk_afm(m._table, (m._attn_flat, 8), Xi, None, c4, 3)
