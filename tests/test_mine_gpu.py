"""fmx_fm_mine_negatives on the GPU: the kernel bit for bit against its definition (tests/mine_ref.py: the numpy draws, then
fmx_fm_topk over the drawn, non-own candidates), padding, ties and de-duplication, determinism and independence of the batch
cut, the scores against float64, and the model level -- FMAdam.mine_negatives, fit_pairs / run_pair_experiment under
negatives="hard", the kept candidates' refresh, pickling, and the refusals of the classes the miner does not score for."""
import pickle

import numpy as np
import pytest
import torch

import fmx
from fmx import pairwise as pw
from fmx import recommend as rec
import mine_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 4e-6           # test_topk_against_float64_brute_force's: 4e-6 (|au| + |ac| + sum_d |Su Sc|) per pair
GUARD = 0x7FC0DEAD   # a NaN pattern around the outputs


def make(kp, U, N, seed, dup=True):
    """Su [U, kp], au [U], Sc [N, kp], ac [N]; with dup a fifth of the candidates are exact copies of another one (equal
    scores among a user's draws: the position decides)."""
    g = torch.Generator().manual_seed(seed)
    Su = torch.randn(U, kp, generator=g) * 0.5
    Sc = torch.randn(N, kp, generator=g) * 0.5
    au = torch.randn(U, generator=g)
    ac = torch.randn(N, generator=g)
    if dup and N > 4:
        src = torch.randint(0, N, (max(1, N // 5),), generator=g)
        dst = torch.randint(0, N, (src.numel(),), generator=g)
        Sc[dst], ac[dst] = Sc[src], ac[src]
    return tuple(x.to(DEV).contiguous() for x in (Su, au, Sc, ac))


def mine(Su, au, Sc, ac, n_draw, n_neg, own=None, excl=None, seed=0, offset=0, u_base=0):
    """The raw call with its outputs inside guard bands that must survive -> (neg_pos int32 [U, n_neg], neg_score fp32) numpy"""
    U = Su.shape[0]
    P = torch.full((U + 2, n_neg), GUARD, dtype=torch.int32, device=DEV)
    S = torch.full((U + 2, n_neg), GUARD, dtype=torch.int32, device=DEV).view(torch.float32)
    own_d = None if own is None else torch.as_tensor(own, dtype=torch.int32).to(DEV)
    off, pos = rec.exclusions_csr(excl, U, DEV)
    pw.fm_mine_negatives(Su, au, Sc, ac, n_draw, n_neg, own_d, seed, offset, u_base, off, pos, out=(P[1:-1], S[1:-1]))
    torch.cuda.synchronize()
    for band in (P[0], P[-1], S.view(torch.int32)[0], S.view(torch.int32)[-1]):
        assert bool((band == GUARD).all())
    return P[1:-1].cpu().numpy(), S[1:-1].cpu().numpy()


def oracle(Su, au, Sc, ac, n_draw, n_neg, own=None, excl=None, seed=0, offset=0, u_base=0):
    drawn = mine_ref.draws(seed, offset, u_base, Su.shape[0], n_draw, Sc.shape[0])

    def topk_call(u, positions, K):
        p = torch.as_tensor(positions, device=DEV)
        tp, ts = rec.fm_topk(Su[u:u + 1], au[u:u + 1], Sc[p].contiguous(), ac[p].contiguous(), K)
        return tp[0].cpu().numpy(), ts[0].cpu().numpy()

    return mine_ref.select(drawn, own, excl, n_neg, topk_call) + (drawn,)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float32).view(np.int32), np.asarray(b, dtype=np.float32).view(np.int32))


def biting(drawn, N, rng, with_own, with_excl):
    """own positions and exclusion lists that meet the draws: own = a drawn position for two users in three (-1 for some),
    exclusions = some drawn positions plus random ones (unsorted, with duplicates and out-of-range entries)"""
    U = drawn.shape[0]
    own = excl = None
    if with_own:
        own = np.where(np.arange(U) % 3 == 2, rng.integers(0, N, U), drawn[:, 0])
        own[np.arange(U) % 7 == 5] = -1
    if with_excl:
        excl = [np.concatenate([drawn[u, 1:1 + min(3, drawn.shape[1] - 1)], rng.integers(0, N, min(N, 40)), [N + 3, -2]])
                for u in range(U)]
        excl[0] = np.array([], dtype=np.int64)
    return own, excl


SHAPES = [(1, 2, 1, 1), (3, 2, 4, 3), (3, 5, 4, 3), (3, 5, 5, 1), (65, 255, 64, 16), (3, 300, 65, 3), (65, 300, 1024, 16),
          (1, 70001, 5, 1), (65, 70001, 1024, 16), (3, 70001, 64, 16)]
CASES = [(kp, s, oe) for kp in (4, 16, 64) for s in SHAPES for oe in ((False, False), (True, True))]
CASES += [(16, s, oe) for s in SHAPES for oe in ((True, False), (False, True))]


@pytest.mark.parametrize("kp, shape, own_excl", CASES)
def test_exact_against_the_definition(kp, shape, own_excl):
    U, N, n_draw, n_neg = shape
    seed = kp * 1000003 + U * 1009 + N * 7 + n_draw
    Su, au, Sc, ac = make(kp, U, N, seed)
    kw = dict(seed=seed, offset=U + 2 ** 33, u_base=n_draw)
    drawn = mine_ref.draws(kw["seed"], kw["offset"], kw["u_base"], U, n_draw, N)
    own, excl = biting(drawn, N, np.random.default_rng(seed), *own_excl)
    pos, score = mine(Su, au, Sc, ac, n_draw, n_neg, own, excl, **kw)
    want_pos, want_score, _ = oracle(Su, au, Sc, ac, n_draw, n_neg, own, excl, **kw)
    assert np.array_equal(pos, want_pos)
    assert same_bits(score, want_score)
    for u in range(U):                                  # what the oracle's construction implies, stated on the result itself
        got = pos[u][pos[u] >= 0]
        assert set(got) <= set(drawn[u]) and len(set(got)) == len(got)
        if own is not None:
            assert own[u] not in got
        if excl is not None:
            assert not set(got) & set(excl[u].tolist())


def test_padding_nan_and_minus_zero():
    kp = 16
    Su, au, Sc, ac = make(kp, 4, 2, seed=3)
    drawn = mine_ref.draws(1, 0, 0, 4, 16, 2)
    assert all(set(drawn[u]) == {0, 1} for u in range(4))
    own = np.array([0, 1, 0, -1])
    pos, score = mine(Su, au, Sc, ac, 16, 3, own, seed=1)
    assert pos[:3].tolist() == [[1, -1, -1], [0, -1, -1], [1, -1, -1]] and sorted(pos[3].tolist()) == [-1, 0, 1]
    assert np.isneginf(score[:3, 1:]).all() and np.isfinite(score[:, 0]).all()
    # every position excluded: nothing but padding
    pos, score = mine(Su, au, Sc, ac, 16, 3, None, [np.array([1, 0])] * 4, seed=1)
    assert (pos == -1).all() and np.isneginf(score).all()
    # two NaN candidates out of five are never returned
    Su, au, Sc, ac = make(kp, 9, 5, seed=4, dup=False)
    Sc[1, 3] = float("nan")
    ac[4] = float("nan")
    pos, score = mine(Su, au, Sc, ac, 64, 5, seed=2)
    drawn = mine_ref.draws(2, 0, 0, 9, 64, 5)
    for u in range(9):
        assert set(drawn[u]) == {0, 1, 2, 3, 4}
        assert sorted(pos[u, :3].tolist()) == [0, 2, 3] and pos[u, 3:].tolist() == [-1, -1]
    assert not np.isnan(score).any()
    want = oracle(Su, au, Sc, ac, 64, 5, seed=2)
    assert np.array_equal(pos, want[0]) and same_bits(score, want[1])
    # a candidate scoring -0 is returned as +0: (-0 + -0) + fma(-0, 1, ... (-0 * 1)) = -0
    Su0 = torch.full((2, kp), -0.0, device=DEV)
    au0 = torch.full((2,), -0.0, device=DEV)
    Sc0 = torch.ones((3, kp), device=DEV)
    ac0 = torch.full((3,), -0.0, device=DEV)
    pos, score = mine(Su0, au0, Sc0, ac0, 32, 3, seed=5)
    assert pos.tolist() == [[0, 1, 2], [0, 1, 2]] and (score.view(np.int32) == 0).all()


def test_ties_and_duplicate_draws():
    kp, U, N = 16, 7, 5
    Su, au, _, _ = make(kp, U, N, seed=6)
    Sc = torch.full((N, kp), 0.25, device=DEV)           # five copies of one candidate: the position alone decides
    ac = torch.full((N,), 0.5, device=DEV)
    drawn = mine_ref.draws(9, 1, 0, U, 64, N)
    pos, score = mine(Su, au, Sc, ac, 64, 5, seed=9, offset=1)
    for u in range(U):
        assert set(drawn[u]) == set(range(N)) and len(drawn[u]) > N      # every position drawn, each more than once
        assert pos[u].tolist() == [0, 1, 2, 3, 4]                        # ... and returned once, the lower one first
        assert len(set(score[u].view(np.int32).tolist())) == 1


def test_deterministic_and_independent_of_the_batch_cut():
    kp, U, N = 16, 65, 70001
    Su, au, Sc, ac = make(kp, U, N, seed=8)
    own = np.arange(U) * 11
    excl = [np.arange(u, N, 97) for u in range(U)]
    a = mine(Su, au, Sc, ac, 64, 4, own, excl, seed=21, offset=5)
    b = mine(Su, au, Sc, ac, 64, 4, own, excl, seed=21, offset=5)
    assert np.array_equal(a[0], b[0]) and same_bits(a[1], b[1])
    c = mine(Su[10:20].contiguous(), au[10:20].contiguous(), Sc, ac, 64, 4, own[10:20], excl[10:20], seed=21, offset=5, u_base=10)
    assert np.array_equal(c[0], a[0][10:20]) and same_bits(c[1], a[1][10:20])
    # another offset or seed draws other positions: with n_neg = n_draw = 16 and nothing excluded the result is the draw set
    sets = {}
    for name, kw in (("base", dict(seed=21, offset=5)), ("offset", dict(seed=21, offset=6)), ("seed", dict(seed=22, offset=5)),
                     ("offset hi", dict(seed=21, offset=5 + 2 ** 32)), ("seed hi", dict(seed=21 + 2 ** 32, offset=5))):
        pos, _ = mine(Su, au, Sc, ac, 16, 16, **kw)
        drawn = mine_ref.draws(kw["seed"], kw["offset"], 0, U, 16, N)
        for u in range(U):
            got = pos[u][pos[u] >= 0]
            assert set(got) == set(drawn[u])
        sets[name] = [frozenset(pos[u].tolist()) for u in range(U)]
    for name in ("offset", "seed", "offset hi", "seed hi"):
        assert all(x != y for x, y in zip(sets[name], sets["base"])), name


@pytest.mark.parametrize("kp", [4, 16, 64])
def test_scores_against_float64(kp):
    U, N, n_draw, n_neg = 65, 300, 256, 16
    Su, au, Sc, ac = make(kp, U, N, seed=kp + 1)
    pos, score = mine(Su, au, Sc, ac, n_draw, n_neg, seed=3)
    S64, C64 = Su.double().cpu().numpy(), Sc.double().cpu().numpy()
    a64, c64 = au.double().cpu().numpy(), ac.double().cpu().numpy()
    assert (pos >= 0).all()
    for u in range(U):
        c = pos[u]
        ref = a64[u] + c64[c] + C64[c] @ S64[u]
        tol = TOL * (abs(a64[u]) + np.abs(c64[c]) + np.abs(C64[c]) @ np.abs(S64[u]))
        assert (np.abs(score[u].astype(np.float64) - ref) <= tol).all()
        assert ((score[u, :-1] > score[u, 1:]) | ((score[u, :-1] == score[u, 1:]) & (pos[u, :-1] < pos[u, 1:]))).all()


# ---------------------------------------------------------------------------------------------------------------------
# the model level
# ---------------------------------------------------------------------------------------------------------------------
SIZES = [7, 50, 5]
ITEM = 1
B = 33
RULES = ["signadam", "adam"]


def model(rule, k=10):
    from models.models_online_deep.fm_adam import FMAdam
    torch.manual_seed(3)
    return FMAdam(SIZES, embedding_size=k, n=0.05, update_rule=rule)


def positives(n, seed):
    rng = np.random.default_rng(seed)
    Xi = np.stack([rng.integers(0, s, n) for s in SIZES], 1).astype(np.int64)
    Xv = rng.uniform(0.5, 1.5, (n, len(SIZES))).astype(np.float32)
    Xv[:, ITEM] = 1.0              # the candidates are scored with value 1 in the item column
    return Xi, Xv


def state_bits(m):
    return (m._table.rows.detach().cpu().numpy().view(np.int32).copy(), m._table.bias.detach().cpu().numpy().view(np.int32).copy())


def same_state(a, b):
    return all(np.array_equal(x, y) for x, y in zip(state_bits(a), state_bits(b)))


def check_mined(m, Xi, Xv, n_draw, n_neg, exclude=None):
    items, scores = m.mine_negatives(Xi, Xv, [ITEM], n_draw, n_neg=n_neg, exclude=exclude)
    assert items.dtype == torch.int64 and tuple(items.shape) == (Xi.shape[0], n_neg, 1) and tuple(scores.shape) == (Xi.shape[0], n_neg)
    it, sc = items.cpu().numpy()[:, :, 0], scores.cpu().numpy()
    assert (it >= 0).all() and (it < SIZES[ITEM]).all()
    assert (it != Xi[:, ITEM:ITEM + 1]).all()                       # never the row's own item
    if exclude is not None:
        for u in range(Xi.shape[0]):
            assert not set(it[u]) & set(np.asarray(exclude[u]).tolist())
    # the scores are forward() on the assembled (context, negative) rows, within check_model's tolerance for recommend's logits
    xi = np.repeat(Xi, n_neg, axis=0)
    xv = np.repeat(Xv, n_neg, axis=0)
    xi[:, ITEM] = it.reshape(-1)
    ref = m.forward(xi, xv).double().cpu().numpy().reshape(it.shape)
    np.testing.assert_allclose(sc, ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max())
    return it


@pytest.mark.parametrize("rule", RULES)
def test_mine_negatives_matches_forward_before_and_after_training(rule):
    m = model(rule)
    Xi, Xv = positives(B, seed=1)
    exclude = [[(Xi[u, ITEM] + d) % SIZES[ITEM] for d in (1, 2, 3)] for u in range(B)]
    check_mined(m, Xi, Xv, 32, 2)
    check_mined(m, Xi, Xv, 32, 2, exclude)
    for step in range(3):
        bXi, bXv = positives(B, seed=10 + step)
        m.fit_pairs(bXi, bXv, [ITEM], negatives="hard")
    check_mined(m, Xi, Xv, 32, 2, exclude)
    check_mined(m, Xi, Xv, 1024, 16)
    assert m._mining_offset == 7
    # a row whose every candidate is excluded has nothing to return
    everything = [np.arange(SIZES[ITEM])] + [[]] * (B - 1)
    with pytest.raises(ValueError, match="no eligible candidate"):
        m.mine_negatives(Xi, Xv, [ITEM], 32, exclude=everything)
    with pytest.raises(ValueError, match="exactly one item field"):
        m.mine_negatives(Xi, Xv, [ITEM, 2], 32)


@pytest.mark.parametrize("rule", RULES)
def test_fit_pairs_hard_is_fit_pairs_on_the_mined_items(rule):
    a, b = model(rule), model(rule)
    assert same_state(a, b)
    Xi, Xv = positives(B, seed=2)
    for step, n_neg in enumerate((1, 2)):
        gen = None if step == 0 else torch.Generator().manual_seed(77)
        hard = "hard" if step == 0 else pw.HardNegatives(n_draw=64)
        la = a.fit_pairs(Xi, Xv, [ITEM], negatives=hard, n_neg=n_neg, generator=gen)
        items, _ = b.mine_negatives(Xi, Xv, [ITEM], 32 if step == 0 else 64, n_neg=n_neg, generator=gen)
        lb = b.fit_pairs(Xi, Xv, [ITEM], negatives=items)
        assert same_bits(la.cpu().numpy(), lb.cpu().numpy()) and same_state(a, b)
    # explicit candidate items, two item fields
    cand = torch.tensor([[i % 50, i % 5] for i in range(0, 90, 3)])
    la = a.fit_pairs(Xi, Xv, [ITEM, 2], negatives="hard", candidates=cand)
    items, _ = b.mine_negatives(Xi, Xv, [ITEM, 2], 32, candidates=cand)
    assert tuple(items.shape) == (B, 1, 2)
    rows = {tuple(r) for r in cand.tolist()}
    assert all(tuple(r) in rows for r in items[:, 0].tolist())
    assert not (items[:, 0].cpu().numpy() == Xi[:, [ITEM, 2]]).all(1).any()
    lb = b.fit_pairs(Xi, Xv, [ITEM, 2], negatives=items)
    assert same_bits(la.cpu().numpy(), lb.cpu().numpy()) and same_state(a, b)


def test_kept_candidates_are_refreshed_every_third_call():
    m = model("signadam")
    Xi, Xv = positives(B, seed=4)
    stale = None
    for call in range(4):
        m.mine_negatives(Xi, Xv, [ITEM], 16, refresh_every=3)
        kept = m._mining_kept["cands"]
        fresh = rec.Candidates.whole_field(m._table, ITEM, hyper=m._hyper)
        if call in (0, 3):
            assert torch.equal(kept.Sc, fresh.Sc) and torch.equal(kept.ac, fresh.ac)
            stale = (kept.Sc.clone(), kept.ac.clone())
        else:
            assert torch.equal(kept.Sc, stale[0]) and torch.equal(kept.ac, stale[1])
            assert not torch.equal(kept.Sc, fresh.Sc)
        bXi, bXv = positives(B, seed=20 + call)
        m.fit_pairs(bXi, bXv, [ITEM], negatives=np.ascontiguousarray((bXi[:, ITEM] + 1) % SIZES[ITEM]))   # the table moves on


@pytest.mark.parametrize("rule", RULES)
def test_pickled_model_continues_in_the_same_bits(rule):
    m = model(rule)
    Xi, Xv = positives(B, seed=5)
    for _ in range(2):
        m.fit_pairs(Xi, Xv, [ITEM], negatives="hard")
    m2 = pickle.loads(pickle.dumps(m))
    assert m2._mining_offset == m._mining_offset == 2 and same_state(m, m2)
    for _ in range(2):
        la = m.fit_pairs(Xi, Xv, [ITEM], negatives="hard")
        lb = m2.fit_pairs(Xi, Xv, [ITEM], negatives="hard")
        assert same_bits(la.cpu().numpy(), lb.cpu().numpy()) and same_state(m, m2)


def test_run_pair_experiment_hard_in_blocks():
    m = model("signadam")
    Xi, Xv = positives(20, seed=6)
    out = m.run_pair_experiment(Xi, Xv, [ITEM], negatives=pw.HardNegatives(n_draw=16, remine_every=8))
    assert len(out) == 4
    seconds, acc, curve, counts = out
    assert seconds > 0 and 0.0 <= acc <= 100.0 and curve[-1] == acc
    assert set(counts) == {"correct", "wrong"} and counts["correct"] + counts["wrong"] == 20
    assert m._mining_offset == 3                                     # blocks of 8, 8 and 4 positives
    out = m.run_pair_experiment(Xi, Xv, [ITEM], negatives="hard", n_neg=2)
    assert out[3]["correct"] + out[3]["wrong"] == 40 and m._mining_offset == 4


def test_hard_negatives_are_refused_outside_the_pure_fm():
    from models.models_online_deep.afm_adam import AFMAdam
    from models.models_online_deep.deepfm_adam import DeepFMAdam
    from models.models_online_deep.deepfm_onn import DeepFMOnn
    Xi, Xv = positives(4, seed=7)
    d = DeepFMAdam(SIZES, embedding_size=8, num_hidden_layers=2, neuron_per_hidden_layer=16)
    o = DeepFMOnn(SIZES, embedding_size=8, num_hidden_layers=2, neuron_per_hidden_layer=16)
    a = AFMAdam(SIZES, embedding_size=8, attention_size=4)
    for obj, kw in ((d, dict(full=True)), (d, dict()), (o, dict()), (a, dict(attention=True))):
        for name in ("fit_pairs", "run_pair_experiment"):
            with pytest.raises(NotImplementedError, match="negatives='hard' mines under the pure FM score"):
                getattr(obj, name)(Xi, Xv, [ITEM], negatives="hard", **kw)
    with pytest.raises(NotImplementedError, match="pure FM score"):
        d.mine_negatives(Xi, Xv, [ITEM], 8)
