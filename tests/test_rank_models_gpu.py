"""model.rank / model.evaluate_ranking on the GPU for FMAdam, DeepFMAdam and NFMOnn (full=True) and AFMAdam: agreement with
model.recommend(K=256) bit for bit, with the order of forward() over the assembled (context, candidate) samples within the
tolerances the recommend tests of each class use, training and Candidates.refresh(), exclusions as lists and as a CSR pair."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fmx  # noqa: E402
from fmx import recommend as rec  # noqa: E402
from rank_checks import check_against_topk, check_bracket  # noqa: E402
import test_recommend_gpu as fm_t  # noqa: E402
import test_recommend_mlp_gpu as mlp_t  # noqa: E402
import test_recommend_afm_gpu as afm_t  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES, ITEM, U = fm_t.SIZES, fm_t.ITEM, 5
N = SIZES[ITEM]


def build(kind):
    if kind == "FMAdam":
        return fm_t.model("sgd"), {}
    if kind == "AFMAdam":
        return afm_t._model("adam", SIZES), {}
    return mlp_t.model(kind, "sgd"), dict(full=True)


def every_logit(m, kind, Xi, Xv, rtol=2e-5):
    """forward()'s logit of every (context, candidate) sample, float64 [U, N], and the recommend tests' tolerance of the class"""
    cand_Xi = np.zeros((N, len(SIZES)), dtype=np.int64)
    cand_Xi[:, ITEM] = np.arange(N)
    cand_Xv = np.ones((N, len(SIZES)), dtype=np.float32)
    allpos = np.tile(np.arange(N), (U, 1))
    if kind == "FMAdam":
        ev = fm_t.assembled_forward(m, Xi, Xv, [ITEM], cand_Xi, cand_Xv, allpos)
        tol = np.full_like(ev, 1e-5 * np.abs(ev).max())
    elif kind == "AFMAdam":
        idx, _, xv = afm_t.assembled(SIZES, [ITEM], Xi, Xv, cand_Xi, None)
        ev = m.forward(idx, xv).detach().reshape(U, N).double().cpu().numpy()
        tol = 2e-5 * (1 + np.abs(ev))
    else:
        ev = mlp_t.assembled(m, Xi, Xv, cand_Xi, cand_Xv, [ITEM], allpos)
        tol = np.full_like(ev, rtol * np.abs(ev).max())
    return torch.from_numpy(ev).to(DEV), torch.from_numpy(tol).to(DEV)


def train(m, kind):
    if kind == "FMAdam":
        rng = np.random.default_rng(10)
        for step in range(3):
            bXi, bXv = fm_t.contexts(64, seed=10 + step)
            m.update_embedding(bXi, bXv, (rng.uniform(size=64) < 0.4).astype(np.float32))
    elif kind == "AFMAdam":
        afm_t._train(m, SIZES, 3)
    else:
        mlp_t.train(m, 3, seed=10)


@pytest.mark.parametrize("kind", ["FMAdam", "DeepFMAdam", "NFMOnn", "AFMAdam"])
def test_model_rank(kind):
    m, kw = build(kind)
    Xi, Xv = fm_t.contexts(U, seed=1)
    rng = np.random.default_rng(3)
    targets = rng.integers(0, N, size=(U, 4))
    targets[1, 3] = -1

    def check():
        ranks, scores, n_cand = m.rank(Xi, Xv, [ITEM], targets, **kw)
        assert ranks.dtype == np.int64 and scores.dtype == np.float32 and ranks.shape == (U, 4) and n_cand.tolist() == [N] * U
        pos, logit = m.recommend(Xi, Xv, [ITEM], 256, **kw)
        n_in = check_against_topk(torch.from_numpy(ranks), torch.from_numpy(scores), torch.from_numpy(targets),
                                  torch.from_numpy(pos), torch.from_numpy(logit))
        assert n_in > 0
        ev, tol = every_logit(m, kind, Xi, Xv)
        check_bracket(torch.from_numpy(ranks), ev, tol, torch.from_numpy(targets), torch.ones(U, N, dtype=torch.bool, device=DEV))
        return ranks

    before = check()
    train(m, kind)
    after = check()
    assert not np.array_equal(before, after)                       # the trained tables are what is ranked
    # evaluate_ranking is ranking_metrics of rank
    ranks, _, n_cand = m.rank(Xi, Xv, [ITEM], targets, **kw)
    want = rec.ranking_metrics(torch.from_numpy(ranks), torch.from_numpy(n_cand), ks=(1, 5, 10))
    got = m.evaluate_ranking(Xi, Xv, [ITEM], targets, **kw)
    assert got.keys() == want.keys() and all(got[k] == want[k] for k in got) and got["n"] == U * 4 - 1
    # exclusions as lists and as a CSR pair; an excluded target is not ranked and n_cand drops
    excl = [[int(targets[u, 0]), 3, 3, 250 + u] for u in range(U)]
    a = m.rank(Xi, Xv, [ITEM], targets, exclude=excl, **kw)
    off, pos = rec.exclusions_csr(excl, U, "cpu")
    b = m.rank(Xi, Xv, [ITEM], targets, exclude=(off, pos), **kw)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    assert (a[0][:, 0] == -1).all() and a[2].tolist() == [N - len(set(e)) for e in excl]
    # the filtered rank never exceeds the raw one
    f = m.rank(Xi, Xv, [ITEM], targets, filtered=True, **kw)
    assert (f[0] <= ranks).all() and (f[0][ranks >= 0] >= 0).all()


SIZES3, ITEM3 = [13, 300, 25], 1     # three fields; the item field's 300 rows are the candidates


def build3(kind):
    """one model per hook that hands recommend / rank their scorer: the FM's, the network's (full=True), the attentional one"""
    torch.manual_seed(3)
    if kind == "FMAdam":
        from models.models_online_deep.fm_adam import FMAdam
        return FMAdam(SIZES3, embedding_size=10, n=0.05, update_rule="sgd"), {}
    if kind == "DeepFMAdam":
        from models.models_online_deep.deepfm_adam import DeepFMAdam
        return DeepFMAdam(SIZES3, embedding_size=10, num_hidden_layers=3, neuron_per_hidden_layer=16, n=0.05,
                          update_rule="sgd"), dict(full=True)
    return afm_t._model("adam", SIZES3), {}


@pytest.mark.parametrize("kind", ["FMAdam", "DeepFMAdam", "AFMAdam"])
def test_the_methods_the_classes_share(kind):
    """rank's scores at the head of recommend's row are recommend's logits bit for bit, at the row's indices; evaluate_ranking
    is ranking_metrics of rank"""
    m, kw = build3(kind)
    rng = np.random.default_rng(7)
    Xi = np.stack([rng.integers(0, s, U) for s in SIZES3], 1).astype(np.int64)
    Xv = rng.uniform(0.5, 1.5, (U, len(SIZES3))).astype(np.float32)
    K, T = 10, 4
    pos, logit = m.recommend(Xi, Xv, [ITEM3], K, **kw)
    assert pos.shape == (U, K) and pos.dtype == np.int64 and logit.dtype == np.float32 and (pos >= 0).all()
    head = np.ascontiguousarray(pos[:, :T])
    ranks, scores, n_cand = m.rank(Xi, Xv, [ITEM3], head, **kw)
    np.testing.assert_array_equal(ranks, np.tile(np.arange(T), (U, 1)))
    np.testing.assert_array_equal(scores.view(np.int32), np.ascontiguousarray(logit[:, :T]).view(np.int32))
    assert n_cand.tolist() == [SIZES3[ITEM3]] * U
    targets = head.copy()
    targets[:, 3] = rng.integers(0, SIZES3[ITEM3], U)
    targets[0, 2] = -1
    ranks, _, n_cand = m.rank(Xi, Xv, [ITEM3], targets, **kw)
    want = rec.ranking_metrics(torch.from_numpy(ranks), torch.from_numpy(n_cand), ks=(1, 5))
    got = m.evaluate_ranking(Xi, Xv, [ITEM3], targets, ks=(1, 5), **kw)
    assert got.keys() == want.keys() and all(got[k] == want[k] for k in got) and got["n"] == U * T - 1


def test_refresh_is_honoured_and_mlp_classes_need_full():
    m, _ = build("FMAdam")
    Xi, Xv = fm_t.contexts(U, seed=1)
    targets = np.arange(U)[:, None] * 7
    cand_idx = torch.zeros((N, len(SIZES)), dtype=torch.int32, device=DEV)
    cand_idx[:, ITEM] = torch.arange(N, dtype=torch.int32, device=DEV)
    cands = rec.Candidates(m._table, [ITEM], cand_idx, None, hyper=m._hyper)
    r0 = rec.rank(m._table, Xi, Xv, cands, targets, hyper=m._hyper)
    train(m, "FMAdam")
    stale = rec.rank(m._table, Xi, Xv, cands, targets, hyper=m._hyper)      # the candidate side is still the old one
    cands.refresh()
    fresh = rec.rank(m._table, Xi, Xv, cands, targets, hyper=m._hyper)
    want = m.rank(Xi, Xv, [ITEM], targets)
    np.testing.assert_array_equal(fresh[0].cpu().numpy(), want[0])
    assert not torch.equal(fresh[1], stale[1]) and not torch.equal(fresh[1], r0[1])
    d = mlp_t.model("DeepFMAdam", "sgd")
    with pytest.raises(NotImplementedError) as e1:
        d.rank(Xi, Xv, [ITEM], targets)
    with pytest.raises(NotImplementedError) as e2:
        d.recommend(Xi, Xv, [ITEM], 5)
    assert str(e1.value) == str(e2.value)


def test_model_rank_full_on_a_hidden_300_network():
    """hidden > 256: model.rank(full=True) goes through rank_network's torch path; it agrees with forward()'s order within the
    tolerance the recommend test of the large network uses (5e-5) and with rank_network on the model's own buffers"""
    m = mlp_t.model("DeepFMAdam", "sgd", H=300, L=2)
    Xi, Xv = fm_t.contexts(U, seed=1)
    targets = np.random.default_rng(4).integers(0, N, size=(U, 3))
    excl = [[int(targets[u, 0]), 5 + u] for u in range(U)]
    ranks, scores, n_cand = m.rank(Xi, Xv, [ITEM], targets, exclude=excl, full=True)
    mlp = (m._mlp_flat, m.embedding_size, m.neuron_per_hidden_layer, m.num_hidden_layers)
    assert not rec.mlp_kernel_takes(mlp)
    ev, tol = every_logit(m, "DeepFMAdam", Xi, Xv, rtol=5e-5)
    elig = torch.ones(U, N, dtype=torch.bool, device=DEV)
    for u in range(U):
        elig[u, torch.tensor(excl[u], device=DEV)] = False
    check_bracket(torch.from_numpy(ranks), ev, tol, torch.from_numpy(targets), elig)
    assert (ranks[:, 0] == -1).all() and n_cand.tolist() == [N - 2] * U
    f = m.rank(Xi, Xv, [ITEM], targets, exclude=excl, full=True, filtered=True)
    assert (f[0] <= ranks).all() and (f[0][ranks >= 0] >= 0).all()
