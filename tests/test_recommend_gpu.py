"""fmx_fm_topk and OnlineFMBase.recommend on the GPU: the kernel against a float64 brute force (score, order, set optimality,
padding), determinism and batch independence, exclusions and NaN rows, the model-level call against forward() on the
assembled samples, and the argument checks with real device buffers."""
import numpy as np
import pytest
import torch

import fmx
from fmx import recommend as rec

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 4e-6


def make(kp, U, N, seed, pad=0, dup=True):
    """Su [U, kp] (row stride kp + pad), au [U], Sc [N, kp] (stride kp + pad), ac [N]; about 2 % of the candidates are exact
    copies of another one (equal scores: the position decides)."""
    g = torch.Generator().manual_seed(seed)
    Su = torch.randn(U, kp + pad, generator=g) * 0.5
    Sc = torch.randn(N, kp + pad, generator=g) * 0.5
    au = torch.randn(U, generator=g)
    ac = torch.randn(N, generator=g)
    if dup and N > 4:
        src = torch.randint(0, N, (max(1, N // 50),), generator=g)
        dst = torch.randint(0, N, (src.numel(),), generator=g)
        Sc[dst], ac[dst] = Sc[src], ac[src]
    t = [x.to(DEV) for x in (Su, au, Sc, ac)]
    return t[0][:, :kp], t[1], t[2][:, :kp], t[3]


def brute(Su, au, Sc, ac):
    """float64 scores [U, N] and the tolerance of every pair, 4e-6 (|au| + |ac| + sum_d |Su Sc|)."""
    S64, C64 = Su.double(), Sc.double()
    score = au.double()[:, None] + ac.double()[None, :] + S64 @ C64.T
    mag = au.double().abs()[:, None] + ac.double().abs()[None, :] + S64.abs() @ C64.abs().T
    return score, TOL * mag


def check_rows(pos, val, Su, au, Sc, ac, K, excluded=None):
    """Every property of the stated contract for every row.  excluded: bool [U, N] of positions that must not appear."""
    U, N = Su.shape[0], Sc.shape[0]
    score, tol = brute(Su, au, Sc, ac)
    eligible = ~torch.isnan(score)
    if excluded is not None:
        eligible &= ~excluded
    pos, val = pos.long(), val
    n_elig = eligible.sum(1)
    n_ret = torch.clamp(n_elig, max=K)
    valid = pos >= 0
    # padding: exactly min(K, eligible) results, then -1 / -inf
    assert torch.equal(valid.sum(1), n_ret)
    ar = torch.arange(K, device=DEV)[None, :]
    assert torch.equal(valid, ar < n_ret[:, None])
    assert bool((val[~valid] == float("-inf")).all()) and bool((pos[~valid] == -1).all())
    assert bool((pos < N).all())
    p = torch.where(valid, pos, torch.zeros_like(pos))
    # returned positions are eligible and distinct
    assert bool(eligible.gather(1, p)[valid].all())
    sp = torch.sort(torch.where(valid, pos, -1 - ar), 1).values
    assert bool((sp[:, 1:] != sp[:, :-1]).all())
    # the stated order on the returned fp32 values, exactly: score descending, then position ascending
    a, b = val[:, :-1], val[:, 1:]
    both = valid[:, :-1] & valid[:, 1:]
    ordered = (a > b) | ((a == b) & (pos[:, :-1] < pos[:, 1:]))
    assert bool(ordered[both].all())
    # each returned score is its pair's score
    s64, t64 = score.gather(1, p), tol.gather(1, p)
    assert bool(((val.double() - s64).abs() <= t64)[valid].all())
    # set optimality: no unreturned eligible candidate beats the K-th returned one by more than the tolerance
    full = n_ret == K
    if bool(full.any()):
        returned = torch.zeros(U, N, dtype=torch.bool, device=DEV)
        returned.scatter_(1, p, valid)
        rest = torch.where(eligible & ~returned, score - tol, torch.full_like(score, float("-inf")))
        kth = s64[:, K - 1] + t64[:, K - 1]
        assert bool((rest.max(1).values <= kth)[full].all())


CASES = sorted({(kp, U, N, K) for kp in (4, 8, 16, 32, 64) for K in (1, 10, 100, 256) for N in (1, max(K - 1, 1), 1000, 176373)
                for U in (1, 7, 300) if not (N == 176373 and U == 300 and kp not in (16, 64))})


@pytest.mark.parametrize("kp, U, N, K", CASES)
def test_topk_against_float64_brute_force(kp, U, N, K):
    Su, au, Sc, ac = make(kp, U, N, seed=kp * 1000003 + U * 1009 + N * 7 + K, pad=4 if (U + K) % 2 else 0)
    pos, val = rec.fm_topk(Su, au, Sc, ac, K)
    check_rows(pos, val, Su, au, Sc, ac, K)


@pytest.mark.parametrize("kp", [4, 16, 64])
@pytest.mark.parametrize("K", [10, 256])
def test_deterministic_and_batch_independent(kp, K):
    U, N = 300, 20000
    Su, au, Sc, ac = make(kp, U, N, seed=kp + K)
    p1, v1 = rec.fm_topk(Su, au, Sc, ac, K)
    p2, v2 = rec.fm_topk(Su, au, Sc, ac, K)
    assert torch.equal(p1, p2) and torch.equal(v1.view(torch.int32), v2.view(torch.int32))
    for u in (0, 1, 17, 150, 299):   # a user alone (U = 1: other tile, other splits) gives its row inside U = 300
        pu, vu = rec.fm_topk(Su[u:u + 1], au[u:u + 1], Sc, ac, K)
        assert torch.equal(pu[0], p1[u]) and torch.equal(vu[0].view(torch.int32), v1[u].view(torch.int32))
    # a permuted candidate list: every pair keeps its score bits
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(K)).to(DEV)
    pp, vp = rec.fm_topk(Su, au, Sc[perm].contiguous(), ac[perm].contiguous(), K)
    orig = perm[pp.long()]
    assert torch.equal(torch.sort(vp, 1).values.view(torch.int32), torch.sort(v1, 1).values.view(torch.int32))
    for u in range(0, U, 37):
        mine = dict(zip(p1[u].tolist(), v1[u].view(torch.int32).tolist()))
        for c, bits in zip(orig[u].tolist(), vp[u].view(torch.int32).tolist()):
            if c in mine:
                assert mine[c] == bits


def test_exclusions():
    kp, U, N, K = 16, 6, 3000, 10
    Su, au, Sc, ac = make(kp, U, N, seed=5)
    rng = np.random.default_rng(0)
    lists = [np.array([], dtype=np.int64),                                   # empty
             rng.permutation(N)[:N - (K - 1)],                               # all but K - 1: the row is padded
             np.concatenate([rng.integers(0, N, 400), rng.integers(0, N, 50)]),   # unsorted, duplicates
             np.arange(N)[::-1].copy(),                                      # everything
             np.array([N + 5, -3, 7]),                                        # out of range entries are ignored
             rng.integers(0, N, 2000)]
    excl = torch.zeros(U, N, dtype=torch.bool)
    for u, l in enumerate(lists):
        l = l[(l >= 0) & (l < N)]
        excl[u, torch.as_tensor(l, dtype=torch.long)] = True
    excl = excl.to(DEV)
    off, pos_l = rec.exclusions_csr(lists, U, DEV)
    pos, val = rec.fm_topk(Su, au, Sc, ac, K, off, pos_l)
    check_rows(pos, val, Su, au, Sc, ac, K, excluded=excl)
    assert int((pos[1] >= 0).sum()) == K - 1 and int((pos[3] >= 0).sum()) == 0
    # the same exclusions as an unsorted CSR pair give the same result
    offs = np.concatenate([[0], np.cumsum([len(l) for l in lists])])
    p2, v2 = rec.fm_topk(Su, au, Sc, ac, K, *rec.exclusions_csr((offs, np.concatenate(lists)), U, DEV))
    assert torch.equal(p2, pos) and torch.equal(v2, val)


def test_nan_candidates_are_never_returned():
    kp, U, N, K = 16, 7, 5000, 100
    Su, au, Sc, ac = make(kp, U, N, seed=9)
    Sc = Sc.clone()
    ac = ac.clone()
    Sc[3, 5] = float("nan")
    ac[11] = float("nan")
    Sc[::97, 0] = float("nan")
    pos, val = rec.fm_topk(Su, au, Sc, ac, K)
    check_rows(pos, val, Su, au, Sc, ac, K)
    bad = {3, 11} | set(range(0, N, 97))
    assert not bad & set(pos.flatten().tolist())
    # only NaN candidates: everything padded
    p2, v2 = rec.fm_topk(Su, au, torch.full_like(Sc[:50], float("nan")), ac[:50].contiguous(), K)
    assert bool((p2 == -1).all()) and bool((v2 == float("-inf")).all())


def test_argument_errors_on_device_buffers():
    lib = fmx._lib.load()
    kp, U, N, K = 16, 4, 500, 10
    Su, au, Sc, ac = make(kp, U, N, seed=1)
    need = int(lib.fmx_fm_topk_workspace_bytes(U, N, K))
    ws = torch.zeros(need + 64, dtype=torch.uint8, device=DEV)
    tp = torch.empty(U, 257, dtype=torch.int32, device=DEV)
    ts = torch.empty(U, 257, dtype=torch.float32, device=DEV)
    flat = torch.zeros(U * kp + 8, device=DEV)

    def call(Su_p=Su.data_ptr(), Sc_p=Sc.data_ptr(), kp_=kp, K_=K, ws_p=ws.data_ptr(), ws_b=need):
        return lib.fmx_fm_topk(Su_p, kp, au.data_ptr(), U, Sc_p, kp, ac.data_ptr(), N, kp_, None, None, K_, ws_p, ws_b,
                               tp.data_ptr(), ts.data_ptr(), None)
    assert call() == fmx._lib.OK
    torch.cuda.synchronize()
    assert call(K_=0) == fmx._lib.ERR_ARG
    assert call(K_=257, ws_b=1 << 40) == fmx._lib.ERR_UNSUPPORTED
    assert call(kp_=12) == fmx._lib.ERR_SHAPE
    assert call(Su_p=flat.data_ptr() + 4) == fmx._lib.ERR_ALIGN
    assert call(Sc_p=flat.data_ptr() + 8) == fmx._lib.ERR_ALIGN
    assert call(ws_p=ws.data_ptr() + 4) == fmx._lib.ERR_ALIGN
    assert call(ws_b=need - 1) == fmx._lib.ERR_SHAPE
    with pytest.raises(fmx._lib.FmxError):
        rec.fm_topk(Su, au, Sc, ac, 257)


# ---------------------------------------------------------------------------------------------------------------------
# end to end through the model classes
# ---------------------------------------------------------------------------------------------------------------------
SIZES = [13, 40, 300, 9, 25]   # field 2 is the item field
ITEM = 2


def model(rule, k=10):
    from models.models_online_deep.fm_adam import FMAdam
    torch.manual_seed(3)
    return FMAdam(SIZES, embedding_size=k, n=0.05, update_rule=rule, ftrl=dict(alpha=0.1, l1=0.001, l2=0.01))


def contexts(U, seed):
    rng = np.random.default_rng(seed)
    Xi = np.stack([rng.integers(0, s, U) for s in SIZES], 1).astype(np.int64)
    Xv = rng.uniform(0.5, 1.5, (U, len(SIZES))).astype(np.float32)
    return Xi, Xv


def assembled_forward(m, Xi, Xv, cand_cols, cand_Xi, cand_Xv, pos):
    """model.forward on the samples (context row u with candidate pos[u, j]'s item columns) -> [U, K] (nan where padded)."""
    U, K = pos.shape
    out = np.full((U, K), np.nan, dtype=np.float64)
    u_idx, j_idx = np.nonzero(pos >= 0)
    if len(u_idx) == 0:
        return out
    c = pos[u_idx, j_idx]
    xi, xv = Xi[u_idx].copy(), Xv[u_idx].copy()
    xi[:, cand_cols] = cand_Xi[c][:, cand_cols]
    xv[:, cand_cols] = cand_Xv[c][:, cand_cols]
    out[u_idx, j_idx] = m.forward(xi, xv).double().cpu().numpy()
    return out


def check_model(m, Xi, Xv, K, items=(ITEM,), cand=None):
    F = len(SIZES)
    if cand is None:
        N = SIZES[ITEM]
        cand_Xi = np.zeros((N, F), dtype=np.int64)
        cand_Xi[:, ITEM] = np.arange(N)
        cand_Xv = np.ones((N, F), dtype=np.float32)
        pos, logit = m.recommend(Xi, Xv, list(items), K)
    else:
        cand_Xi, cand_Xv = cand
        pos, logit = m.recommend(Xi, Xv, list(items), K, candidates=(cand_Xi, cand_Xv))
    assert pos.dtype == np.int64 and logit.dtype == np.float32 and pos.shape == (Xi.shape[0], K)
    ref = assembled_forward(m, Xi, Xv, list(items), cand_Xi, cand_Xv, pos)
    ok = pos >= 0
    scale = np.abs(ref[ok]).max()
    np.testing.assert_allclose(logit[ok], ref[ok], rtol=1e-5, atol=1e-5 * scale)
    # the returned set is the top K of forward() over every candidate, up to near-ties
    U, N = Xi.shape[0], cand_Xi.shape[0]
    allpos = np.tile(np.arange(N), (U, 1))
    every = assembled_forward(m, Xi, Xv, list(items), cand_Xi, cand_Xv, allpos)
    kth = np.sort(every, 1)[:, ::-1][:, K - 1]
    near = 1e-5 * np.abs(every).max()
    assert (ref[ok] >= np.repeat(kth, ok.sum(1)) - near).all()
    return pos, logit


@pytest.mark.parametrize("rule", ["signadam", "ftrl"])
def test_recommend_matches_forward_before_and_after_training(rule):
    m = model(rule)
    Xi, Xv = contexts(33, seed=1)
    check_model(m, Xi, Xv, K=10)
    rng = np.random.default_rng(2)
    for step in range(4):
        bXi, bXv = contexts(64, seed=10 + step)
        m.update_embedding(bXi, bXv, (rng.uniform(size=64) < 0.4).astype(np.float32))
    p1, _ = check_model(m, Xi, Xv, K=10)
    check_model(m, Xi, Xv, K=256)
    # two item fields, explicit candidates with their own values
    N = 120
    cand_Xi = np.stack([rng.integers(0, s, N) for s in SIZES], 1).astype(np.int64)
    cand_Xv = rng.uniform(0.5, 1.5, (N, len(SIZES))).astype(np.float32)
    check_model(m, Xi, Xv, K=17, items=(ITEM, 4), cand=(cand_Xi, cand_Xv))
    # exclusions at the model level: the excluded positions disappear, the rest keeps its order
    pos, _ = m.recommend(Xi, Xv, [ITEM], 10, exclude=[p1[u, :3][::-1] for u in range(Xi.shape[0])])
    for u in range(Xi.shape[0]):
        assert not set(p1[u, :3]) & set(pos[u])
        assert list(pos[u, :7]) == list(p1[u, 3:])


def test_recommend_item_columns_of_the_context_are_ignored():
    m = model("signadam")
    Xi, Xv = contexts(9, seed=4)
    p1, l1 = m.recommend(Xi, Xv, [ITEM], 12)
    Xi2, Xv2 = Xi.copy(), Xv.copy()
    Xi2[:, ITEM] = 299
    Xv2[:, ITEM] = 7.0
    p2, l2 = m.recommend(Xi2, Xv2, [ITEM], 12)
    assert np.array_equal(p1, p2) and np.array_equal(l1.view(np.int32), l2.view(np.int32))


def test_recommend_never_returns_a_nan_row():
    m = model("signadam")
    with torch.no_grad():
        off = int(m._table.offsets_host[ITEM])
        m._table.rows[off + 17, 1] = float("nan")
        m._table.rows[off + 250, m._table.kp] = float("nan")   # the first-order weight
    Xi, Xv = contexts(20, seed=5)
    pos, logit = m.recommend(Xi, Xv, [ITEM], 256)
    assert not {17, 250} & set(pos.flatten().tolist())
    assert not np.isnan(logit).any()


def test_recommend_errors():
    m = model("signadam")
    Xi, Xv = contexts(5, seed=6)
    Xi[3, 0] = SIZES[0]          # a context index outside its field
    with pytest.raises(IndexError):
        m.recommend(Xi, Xv, [ITEM], 5)
    Xi, Xv = contexts(5, seed=6)
    with pytest.raises(ValueError):
        m.recommend(Xi, Xv, [ITEM, 4], 5)      # candidates=None needs one item field
    cand_Xi = np.zeros((4, len(SIZES)), dtype=np.int64)
    cand_Xi[2, ITEM] = SIZES[ITEM]              # a candidate index outside its field
    with pytest.raises(IndexError):
        m.recommend(Xi, Xv, [ITEM], 2, candidates=(cand_Xi, None))
    from models.models_online_deep.deepfm_adam import DeepFMAdam
    from models.models_online_deep.nfm_adam import NFMAdam
    for cls in (DeepFMAdam, NFMAdam):
        d = cls(SIZES, embedding_size=8, num_hidden_layers=2, neuron_per_hidden_layer=16)
        with pytest.raises(NotImplementedError):
            d.recommend(Xi, Xv, [ITEM], 5)
