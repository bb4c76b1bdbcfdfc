"""fmx_mlp_topk and recommend(full=True) on the GPU: the kernel against a float64 brute force with a per-pair fp32 noise
bound (score, order, set optimality, padding), bit-identical scores across runs, user subsets, candidate permutations and
splits, exclusions / NaN rows / -0, the four network classes against forward() on the assembled samples, and the chunked
torch path of networks the kernel does not take."""
import numpy as np
import pytest
import torch

import fmx
from fmx import recommend as rec

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -24


def make_net(k, H, L, seed, zero=False):
    """flat params (W_l [H, in] then b_l), nn.Linear's init scale; biases shifted up so that most units stay live."""
    g = torch.Generator().manual_seed(seed)
    parts = []
    for l in range(L):
        n_in = k if l == 0 else H
        s = 1.0 / n_in ** 0.5
        parts.append((torch.rand(H * n_in, generator=g) * 2 - 1) * s)
        parts.append((torch.rand(H, generator=g) * 2 - 1) * s + 0.3 * s)
    p = torch.cat(parts)
    if zero:
        p = torch.full_like(p, -0.0)
    return (p.to(DEV).contiguous(), k, H, L)


def make_sides(k, kp, U, N, seed, pad=0, dup=True):
    """Su / Bu [U, kp] sharing a row stride (kp + pad), Sc / Bc [N, kp] likewise, au [U], ac [N].  S's pad columns are 0 (the
    dot reads them), bi's pad columns are NaN (x0 must not read them).  About 2 % of the candidates repeat another one."""
    g = torch.Generator().manual_seed(seed)

    def side(R):
        S = torch.zeros(R, kp + pad)
        B = torch.full((R, kp + pad), float("nan"))
        S[:, :k] = torch.randn(R, k, generator=g) * 0.6
        B[:, :k] = torch.randn(R, k, generator=g) * 0.4
        return S, B
    Su, Bu = side(U)
    Sc, Bc = side(N)
    au, ac = torch.randn(U, generator=g), torch.randn(N, generator=g)
    if dup and N > 4:
        src = torch.randint(0, N, (max(1, N // 50),), generator=g)
        dst = torch.randint(0, N, (src.numel(),), generator=g)
        Sc[dst], Bc[dst], ac[dst] = Sc[src], Bc[src], ac[src]
    t = [x.to(DEV) for x in (Su, Bu, au, Sc, Bc, ac)]
    return t[0][:, :kp], t[1][:, :kp], t[2], t[3][:, :kp], t[4][:, :kp], t[5]


def layers64(net):
    params, k, H, L = net
    p, out, off = params.double(), [], 0
    for l in range(L):
        n_in = k if l == 0 else H
        out.append((p[off:off + H * n_in].view(H, n_in), p[off + H * n_in:off + H * n_in + H]))
        off += H * n_in + H
    return out


def brute(net, fm_term, Su, Bu, au, Sc, Bc, ac):
    """float64 scores [U, N] of the same fp32 inputs and a per-pair bound on the fp32 evaluation's error: every sum's
    rounding is bounded by (terms) * eps * |its terms|, carried through the later layers by |W| (relu is 1-Lipschitz)."""
    _, k, H, L = net
    kp = Sc.shape[1]
    Ws = layers64(net)
    U, N = Su.shape[0], Sc.shape[0]
    score = torch.empty(U, N, dtype=torch.float64, device=DEV)
    tol = torch.empty(U, N, dtype=torch.float64, device=DEV)
    S64c, B64c, a64c = Sc.double(), Bc[:, :k].double(), ac.double()
    ub = max(1, (1 << 23) // max(1, N * max(H, k)))
    for u0 in range(0, U, ub):
        u1 = min(U, u0 + ub)
        Su64, Bu64, au64 = Su[u0:u1].double(), Bu[u0:u1, :k].double(), au[u0:u1].double()
        prod = Su64[:, None, :k] * S64c[None, :, :k]
        x = Bu64[:, None] + B64c[None] + prod
        err = 2 * EPS * (Bu64[:, None].abs() + B64c[None].abs() + prod.abs())
        for W, b in Ws:
            n_in = W.shape[1]
            Wa = W.abs()
            pre = x @ W.T + b
            mag = x.abs() @ Wa.T + b.abs()
            err = err @ Wa.T + (n_in + 1) * EPS * mag
            x = torch.relu(pre)
        s = x.sum(-1)
        err_s = err.sum(-1) + H * EPS * x.abs().sum(-1)
        base = au64[:, None] + a64c[None]
        err_b = EPS * base.abs()
        if fm_term:
            dot = Su64 @ S64c.T
            err_b = err_b + EPS * (au64.abs()[:, None] + a64c.abs()[None]) + kp * EPS * (Su64.abs() @ S64c.abs().T)
            base = base + dot
        sc = base + s
        score[u0:u1] = sc
        tol[u0:u1] = 2 * (err_b + err_s + EPS * (base.abs() + s.abs())) + 1e-30
    return score, tol


def check_rows(pos, val, score, tol, K, excluded=None):
    """Every property of the stated contract for every row (as for fmx_fm_topk).  excluded: bool [U, N] never to appear."""
    U, N = score.shape
    eligible = ~torch.isnan(score)
    if excluded is not None:
        eligible &= ~excluded
    pos = pos.long()
    n_ret = torch.clamp(eligible.sum(1), max=K)
    valid = pos >= 0
    assert torch.equal(valid.sum(1), n_ret)
    ar = torch.arange(K, device=DEV)[None, :]
    assert torch.equal(valid, ar < n_ret[:, None])
    assert bool((val[~valid] == float("-inf")).all()) and bool((pos[~valid] == -1).all())
    assert bool((pos < N).all())
    p = torch.where(valid, pos, torch.zeros_like(pos))
    assert bool(eligible.gather(1, p)[valid].all())
    sp = torch.sort(torch.where(valid, pos, -1 - ar), 1).values
    assert bool((sp[:, 1:] != sp[:, :-1]).all())
    a, b = val[:, :-1], val[:, 1:]
    both = valid[:, :-1] & valid[:, 1:]
    ordered = (a > b) | ((a == b) & (pos[:, :-1] < pos[:, 1:]))
    assert bool(ordered[both].all())
    s64, t64 = score.gather(1, p), tol.gather(1, p)
    bad = ((val.double() - s64).abs() > t64) & valid
    assert not bool(bad.any()), f"{int(bad.sum())} scores outside their bound; worst err/tol " \
        f"{float(((val.double() - s64).abs() / t64)[valid].max()):.3g}"
    full = n_ret == K
    if bool(full.any()):
        returned = torch.zeros(U, N, dtype=torch.bool, device=DEV)
        returned.scatter_(1, p, valid)
        rest = torch.where(eligible & ~returned, score - tol, torch.full_like(score, float("-inf")))
        kth = s64[:, K - 1] + t64[:, K - 1]
        assert bool((rest.max(1).values <= kth)[full].all())


NETS = [(10, 5), (256, 3), (64, 8), (1, 1), (33, 2)]
KPS = [(4, 3), (16, 11), (64, 63)]          # (kp, k): k < kp, k odd
UNK = [(1, 1, 1), (7, 255, 10), (300, 5000, 10), (1, 5000, 256), (7, 1, 10), (300, 255, 256), (7, 5000, 1), (1, 255, 10),
       (300, 1, 256), (7, 5000, 256)]
CASES = [(H, L, kp, k, fm, *UNK[(i * 6 + j * 2 + fm) % len(UNK)])
         for i, (H, L) in enumerate(NETS) for j, (kp, k) in enumerate(KPS) for fm in (0, 1)]


@pytest.mark.parametrize("H, L, kp, k, fm_term, U, N, K", CASES)
def test_mlp_topk_against_float64_brute_force(H, L, kp, k, fm_term, U, N, K):
    seed = H * 7919 + L * 131 + kp * 17 + U + N + K + fm_term
    net = make_net(k, H, L, seed)
    Su, Bu, au, Sc, Bc, ac = make_sides(k, kp, U, N, seed, pad=4 if (U + K) % 2 else 0)
    pos, val = rec.mlp_topk(net, fm_term, Su, Bu, au, Sc, Bc, ac, K)
    score, tol = brute(net, fm_term, Su, Bu, au, Sc, Bc, ac)
    check_rows(pos, val, score, tol, K)


def bits(v):
    return v.view(torch.int32)


@pytest.mark.parametrize("H, L, fm_term", [(256, 3, 1), (33, 2, 0), (10, 5, 1)])
def test_scores_are_bit_identical_across_runs_subsets_permutations_and_splits(H, L, fm_term):
    k, kp, K, N = 11, 16, 64, 3000
    U = 2048 if H < 256 else 300          # U = 2048: one split per user; alone: several
    net = make_net(k, H, L, seed=H + L)
    Su, Bu, au, Sc, Bc, ac = make_sides(k, kp, U, N, seed=H)
    p1, v1 = rec.mlp_topk(net, fm_term, Su, Bu, au, Sc, Bc, ac, K)
    p2, v2 = rec.mlp_topk(net, fm_term, Su, Bu, au, Sc, Bc, ac, K)
    assert torch.equal(p1, p2) and torch.equal(bits(v1), bits(v2))
    for u in (0, 1, 17, 150, U - 1):
        pu, vu = rec.mlp_topk(net, fm_term, Su[u:u + 1], Bu[u:u + 1], au[u:u + 1], Sc, Bc, ac, K)
        assert torch.equal(pu[0], p1[u]) and torch.equal(bits(vu[0]), bits(v1[u]))
    sub = torch.arange(3, U, 7, device=DEV)
    ps, vs = rec.mlp_topk(net, fm_term, Su[sub], Bu[sub], au[sub], Sc, Bc, ac, K)
    assert torch.equal(ps, p1[sub]) and torch.equal(bits(vs), bits(v1[sub]))
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(H)).to(DEV)
    pp, vp = rec.mlp_topk(net, fm_term, Su, Bu, au, Sc[perm].contiguous(), Bc[perm].contiguous(), ac[perm].contiguous(), K)
    orig = perm[pp.long()]
    assert torch.equal(torch.sort(vp, 1).values, torch.sort(v1, 1).values)
    for u in range(0, U, 97):
        mine = dict(zip(p1[u].tolist(), bits(v1[u]).tolist()))
        for c, b in zip(orig[u].tolist(), bits(vp[u]).tolist()):
            if c in mine:
                assert mine[c] == b


def test_exclusions():
    k, kp, U, N, K = 15, 16, 6, 3000, 10
    net = make_net(k, 64, 3, seed=2)
    Su, Bu, au, Sc, Bc, ac = make_sides(k, kp, U, N, seed=5)
    rng = np.random.default_rng(0)
    lists = [np.array([], dtype=np.int64), rng.permutation(N)[:N - (K - 1)],
             np.concatenate([rng.integers(0, N, 400), rng.integers(0, N, 50)]), np.arange(N)[::-1].copy(),
             np.array([N + 5, -3, 7]), rng.integers(0, N, 2000)]
    excl = torch.zeros(U, N, dtype=torch.bool)
    for u, l in enumerate(lists):
        l = l[(l >= 0) & (l < N)]
        excl[u, torch.as_tensor(l, dtype=torch.long)] = True
    excl = excl.to(DEV)
    off, pos_l = rec.exclusions_csr(lists, U, DEV)
    for fm_term in (0, 1):
        pos, val = rec.mlp_topk(net, fm_term, Su, Bu, au, Sc, Bc, ac, K, off, pos_l)
        score, tol = brute(net, fm_term, Su, Bu, au, Sc, Bc, ac)
        check_rows(pos, val, score, tol, K, excluded=excl)
        assert int((pos[1] >= 0).sum()) == K - 1 and int((pos[3] >= 0).sum()) == 0
        pt, vt = rec.mlp_topk_torch(net, fm_term, Su, Bu, au, Sc, Bc, ac, K, off, pos_l)
        check_rows(pt, vt, score, tol, K, excluded=excl)


@pytest.mark.parametrize("fm_term", [0, 1])
def test_nan_rows_are_never_returned(fm_term):
    k, kp, U, N, K = 11, 16, 7, 5000, 100
    net = make_net(k, 256, 3, seed=4)
    Su, Bu, au, Sc, Bc, ac = make_sides(k, kp, U, N, seed=9)
    Sc, Bc, ac = Sc.clone(), Bc.clone(), ac.clone()
    Sc[3, 5] = float("nan")
    Bc[8, 2] = float("nan")
    ac[11] = float("nan")
    Sc[::97, 0] = float("nan")
    pos, val = rec.mlp_topk(net, fm_term, Su, Bu, au, Sc, Bc, ac, K)
    score, tol = brute(net, fm_term, Su, Bu, au, Sc, Bc, ac)
    check_rows(pos, val, score, tol, K)
    assert not ({3, 8, 11} | set(range(0, N, 97))) & set(pos.flatten().tolist())
    p2, v2 = rec.mlp_topk(net, fm_term, Su, Bu, au, torch.full_like(Sc[:50], float("nan")), Bc[:50].contiguous(),
                          ac[:50].contiguous(), K)
    assert bool((p2 == -1).all()) and bool((v2 == float("-inf")).all())


def test_negative_zero_scores_are_returned_as_zero_by_position():
    """-0 weights and biases with positive inputs: every hidden unit and the sum are -0, the base -0 + -0: every score is
    a signed zero, returned as +0 in position order (by the kernel and by the torch path)."""
    k, kp, U, N, K = 8, 8, 3, 700, 20
    net = make_net(k, 16, 2, seed=1, zero=True)
    Su, Bu, au, Sc, Bc, ac = make_sides(k, kp, U, N, seed=3, dup=False)
    Su, Bu, Sc, Bc = Su.abs(), Bu.abs(), Sc.abs(), Bc.abs()
    au, ac = torch.full_like(au, -0.0), torch.full_like(ac, -0.0)
    for fn in (rec.mlp_topk, rec.mlp_topk_torch):
        pos, val = fn(net, 0, Su, Bu, au, Sc, Bc, ac, K)
        assert torch.equal(pos.long().cpu(), torch.arange(K)[None].repeat(U, 1))
        assert bool((bits(val.float().contiguous()) == 0).all())


@pytest.mark.parametrize("fm_term", [0, 1])
def test_torch_fallback_on_a_network_the_kernel_refuses(fm_term):
    k, kp, U, N, K = 11, 16, 5, 700, 25
    net = make_net(k, 300, 2, seed=6)
    Su, Bu, au, Sc, Bc, ac = make_sides(k, kp, U, N, seed=7)
    with pytest.raises(fmx._lib.FmxError):
        rec.mlp_topk(net, fm_term, Su, Bu, au, Sc, Bc, ac, K)          # hidden = 300: FMX_ERR_UNSUPPORTED
    pos, val = rec.mlp_topk_torch(net, fm_term, Su, Bu, au, Sc, Bc, ac, K, max_elems=1 << 20)   # several chunks
    score, tol = brute(net, fm_term, Su, Bu, au, Sc, Bc, ac)
    check_rows(pos, val, score, 4 * tol, K)         # torch's GEMM sums in its own order: a looser constant


# ---------------------------------------------------------------------------------------------------------------------
# end to end through the model classes
# ---------------------------------------------------------------------------------------------------------------------
SIZES = [13, 40, 300, 9, 25]   # field 2 is the item field
ITEM = 2
CLASSES = ["DeepFMAdam", "NFMAdam", "DeepFMOnn", "NFMOnn"]


def model(cls, rule, k=10, H=16, L=3, batch=64):
    import importlib
    mod = importlib.import_module("models.models_online_deep." + {"DeepFMAdam": "deepfm_adam", "NFMAdam": "nfm_adam",
                                                                   "DeepFMOnn": "deepfm_onn", "NFMOnn": "nfm_onn"}[cls])
    torch.manual_seed(3)
    kw = dict(embedding_size=k, num_hidden_layers=L, neuron_per_hidden_layer=H, n=0.05, update_rule=rule,
              ftrl=dict(alpha=0.1, l1=0.001, l2=0.01))
    if cls.endswith("Onn"):
        kw["batch_size"] = batch
    return getattr(mod, cls)(SIZES, **kw)


def contexts(U, seed):
    rng = np.random.default_rng(seed)
    Xi = np.stack([rng.integers(0, s, U) for s in SIZES], 1).astype(np.int64)
    Xv = rng.uniform(0.5, 1.5, (U, len(SIZES))).astype(np.float32)
    return Xi, Xv


def network_logit(m, xi, xv):
    """What recommend(full=True) ranks by: forward() for the Adam classes; for the ONN classes the logit whose sigmoid
    forward() returns (its last layer), base + sum of the last hidden layer."""
    if not m._onn:
        return m.forward(xi, xv).double()
    B = m._fm_forward(xi, xv)
    with torch.no_grad():
        logit = m._base_logit(B) + m._mlp(m._engine.bi[:B, :m.embedding_size])[-1].sum(1)
        last, _ = m.forward(xi, xv)
        torch.testing.assert_close(torch.sigmoid(logit), last, rtol=1e-5, atol=1e-6)
    return logit.double()


def assembled(m, Xi, Xv, cand_Xi, cand_Xv, items, pos):
    U, K = pos.shape
    out = np.full((U, K), np.nan, dtype=np.float64)
    u_idx, j_idx = np.nonzero(pos >= 0)
    if len(u_idx) == 0:
        return out
    c = pos[u_idx, j_idx]
    xi, xv = Xi[u_idx].copy(), Xv[u_idx].copy()
    xi[:, items] = cand_Xi[c][:, items]
    xv[:, items] = cand_Xv[c][:, items]
    for r0 in range(0, len(u_idx), 4096):
        out[u_idx[r0:r0 + 4096], j_idx[r0:r0 + 4096]] = network_logit(m, xi[r0:r0 + 4096], xv[r0:r0 + 4096]).cpu().numpy()
    return out


def check_model(m, Xi, Xv, K, items=(ITEM,), cand=None, rtol=2e-5):
    F = len(SIZES)
    if cand is None:
        N = SIZES[ITEM]
        cand_Xi = np.zeros((N, F), dtype=np.int64)
        cand_Xi[:, ITEM] = np.arange(N)
        cand_Xv = np.ones((N, F), dtype=np.float32)
        pos, logit = m.recommend(Xi, Xv, list(items), K, full=True)
    else:
        cand_Xi, cand_Xv = cand
        pos, logit = m.recommend(Xi, Xv, list(items), K, candidates=(cand_Xi, cand_Xv), full=True)
    assert pos.dtype == np.int64 and logit.dtype == np.float32 and pos.shape == (Xi.shape[0], K)
    ref = assembled(m, Xi, Xv, cand_Xi, cand_Xv, list(items), pos)
    ok = pos >= 0
    assert ok.all() or K > cand_Xi.shape[0]
    scale = np.abs(ref[ok]).max()
    np.testing.assert_allclose(logit[ok], ref[ok], rtol=rtol, atol=rtol * scale)
    U, N = Xi.shape[0], cand_Xi.shape[0]
    every = assembled(m, Xi, Xv, cand_Xi, cand_Xv, list(items), np.tile(np.arange(N), (U, 1)))
    kth = np.sort(every, 1)[:, ::-1][:, min(K, N) - 1]
    assert (ref[ok] >= np.repeat(kth, ok.sum(1)) - rtol * np.abs(every).max()).all()
    return pos, logit


def train(m, steps, seed):
    rng = np.random.default_rng(seed)
    for step in range(steps):
        bXi, bXv = contexts(64, seed=seed + step)
        y = (rng.uniform(size=64) < 0.4).astype(np.float32)
        m.update_embedding(bXi, bXv, y)
        m.fit(bXi, bXv, y)


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("rule", ["signadam", "sgd", "ftrl"])
def test_recommend_full_matches_forward_before_and_after_training(cls, rule):
    m = model(cls, rule)
    Xi, Xv = contexts(21, seed=1)
    check_model(m, Xi, Xv, K=10)
    before = m._mlp_flat.clone()
    train(m, 3, seed=10)
    assert not torch.equal(before, m._mlp_flat)            # the network did train
    p1, _ = check_model(m, Xi, Xv, K=10)
    check_model(m, Xi, Xv, K=256)
    rng = np.random.default_rng(2)
    N = 120
    cand_Xi = np.stack([rng.integers(0, s, N) for s in SIZES], 1).astype(np.int64)
    cand_Xv = rng.uniform(0.5, 1.5, (N, len(SIZES))).astype(np.float32)
    check_model(m, Xi, Xv, K=17, items=(ITEM, 4), cand=(cand_Xi, cand_Xv))
    pos, _ = m.recommend(Xi, Xv, [ITEM], 10, exclude=[p1[u, :3][::-1] for u in range(Xi.shape[0])], full=True)
    for u in range(Xi.shape[0]):
        assert not set(p1[u, :3]) & set(pos[u])
        assert list(pos[u, :7]) == list(p1[u, 3:])


@pytest.mark.parametrize("cls", ["DeepFMAdam", "NFMOnn"])
def test_recommend_full_at_the_large_network_and_the_fallback(cls):
    # 3 x 256 on the kernel; hidden = 300 through the chunked torch path, both against forward()
    for H, L in ((256, 3), (300, 2)):
        m = model(cls, "signadam", k=16, H=H, L=L)
        Xi, Xv = contexts(5, seed=7)
        check_model(m, Xi, Xv, K=12, rtol=5e-5)


def test_recommend_default_still_raises_and_fm_full_is_the_default():
    Xi, Xv = contexts(5, seed=6)
    for cls in CLASSES:
        with pytest.raises(NotImplementedError):
            model(cls, "signadam").recommend(Xi, Xv, [ITEM], 5)
    from models.models_online_deep.fm_adam import FMAdam
    torch.manual_seed(3)
    m = FMAdam(SIZES, embedding_size=10, n=0.05)
    p1, l1 = m.recommend(Xi, Xv, [ITEM], 12)
    p2, l2 = m.recommend(Xi, Xv, [ITEM], 12, full=True)
    assert np.array_equal(p1, p2) and np.array_equal(l1.view(np.int32), l2.view(np.int32))


def test_recommend_full_errors():
    m = model("DeepFMAdam", "signadam")
    Xi, Xv = contexts(5, seed=6)
    Xi[3, 0] = SIZES[0]
    with pytest.raises(IndexError):
        m.recommend(Xi, Xv, [ITEM], 5, full=True)
    Xi, Xv = contexts(5, seed=6)
    with pytest.raises(ValueError):
        m.recommend(Xi, Xv, [ITEM, 4], 5, full=True)
    cand_Xi = np.zeros((4, len(SIZES)), dtype=np.int64)
    cand_Xi[2, ITEM] = SIZES[ITEM]
    with pytest.raises(IndexError):
        m.recommend(Xi, Xv, [ITEM], 2, candidates=(cand_Xi, None), full=True)
    with pytest.raises(fmx._lib.FmxError):
        m.recommend(Xi, Xv, [ITEM], 257, full=True)
