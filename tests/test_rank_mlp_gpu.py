"""fmx_mlp_rank on the GPU (the DeepFM / NFM network on every pair): the bit-exact cross-check with fmx_mlp_topk, the float64
bracket with the evaluation and the per-pair error bound of tests/test_recommend_mlp_gpu.py, determinism and batch independence,
and the torch path of networks the kernel does not take.  Shapes: around the scan's chunk of 64 pairs (N = 63 / 65), a few
chunks (N = 300), and past each network's split minimum (MlpTopkGeom: 1664 candidates for the 16-wide network, 64 for the
256-wide one), so N = 65 and 300 split the wide network, N = 1665 and 5000 the narrow one."""
import numpy as np
import pytest
import torch

import fmx
from fmx import recommend as rec
from rank_checks import bits, check_against_topk, check_bracket
from test_recommend_mlp_gpu import brute, check_rows, make_net, make_sides

pytestmark = pytest.mark.gpu
DEV = "cuda"
NETS = [(10, 16, 10, 5), (16, 16, 256, 3)]      # (k, kp, hidden, layers)
SHAPES = [(3, 63), (3, 65), (2, 300), (2, 1665), (5, 5000)]


def targets_for(top_pos, U, N, seed):
    """the head of the top-K row (inside it), random positions (mostly outside when N > 256), padding and a position >= N"""
    g = torch.Generator().manual_seed(seed)
    tg = torch.cat([top_pos[:, :6].to(torch.int32), torch.randint(0, N, (U, 10), generator=g).to(DEV, torch.int32)], 1)
    tg[0, 15] = -1
    tg[-1, 14] = N + 1
    return tg.contiguous()


@pytest.mark.parametrize("fm_term", [0, 1])
@pytest.mark.parametrize("k, kp, H, L", NETS)
@pytest.mark.parametrize("U, N", SHAPES)
def test_mlp_rank_against_topk_and_float64(U, N, k, kp, H, L, fm_term):
    net = make_net(k, H, L, seed=H + L)
    sides = make_sides(k, kp, U, N, seed=N + H)
    top_pos, top_score = rec.mlp_topk(net, fm_term, *sides, 256)
    score, tol = brute(net, fm_term, *sides)
    elig = torch.ones(U, N, dtype=torch.bool, device=DEV)
    if N <= 256:
        cols = torch.arange(N, dtype=torch.int32, device=DEV)[None, :].repeat(U, 1)
        chunks = [cols[:, c0:c0 + 16].contiguous() for c0 in range(0, N, 16)]
    else:
        chunks = [targets_for(top_pos, U, N, seed=N)]
    for tg in chunks:
        for T in ((1, 2, 16) if len(chunks) == 1 else (tg.shape[1],)):
            t = tg[:, :T].contiguous()
            r, s, n = rec.mlp_rank(net, fm_term, *sides, t, False)
            check_against_topk(r, s, torch.where(t < N, t, torch.full_like(t, -1)), top_pos, top_score)
            check_bracket(r, score, tol, t, elig)
            assert bool((n == N).all())


# hidden sizes on both sides of every boundary of the network scan's map from column tiles (hidden / 16, rounded up) to its wave
# grid: 1, 2, 3, 4, 5..8, 9..12 and 13..16 tiles
WAVE_GRID_HIDDEN = [16, 17, 32, 33, 48, 49, 64, 65, 128, 129, 192, 193, 256]


@pytest.mark.parametrize("fm_term", [0, 1])
@pytest.mark.parametrize("H", WAVE_GRID_HIDDEN)
def test_every_wave_grid_under_both_calls(H, fm_term):
    """N = 65: one full chunk of 64 candidates and a ragged one"""
    L, k, kp, U, N, K, T = 2, 3, 4, 2, 65, 10, 2
    net = make_net(k, H, L, seed=H)
    sides = make_sides(k, kp, U, N, seed=H + fm_term)
    score, tol = brute(net, fm_term, *sides)
    top_pos, top_score = rec.mlp_topk(net, fm_term, *sides, K)
    check_rows(top_pos, top_score, score, tol, K)
    tg = torch.stack([top_pos[:, 1].to(torch.int32), torch.tensor([N - 1, 7], dtype=torch.int32, device=DEV)], 1).contiguous()
    assert tg.shape == (U, T)
    r, s, n = rec.mlp_rank(net, fm_term, *sides, tg, False)
    assert check_against_topk(r, s, tg, top_pos, top_score) >= U       # the targets taken from the row are found in it
    check_bracket(r, score, tol, tg, torch.ones(U, N, dtype=torch.bool, device=DEV))
    assert bool((n == N).all())


@pytest.mark.parametrize("k, kp, H, L", NETS)
def test_determinism_batch_independence_filtered_and_exclusions(k, kp, H, L):
    U, N, fm_term = 5, 2100, 1
    net = make_net(k, H, L, seed=1)
    sides = make_sides(k, kp, U, N, seed=2)
    Su, Bu, au, Sc, Bc, ac = sides
    g = torch.Generator().manual_seed(4)
    tg = torch.randint(0, N, (U, 16), generator=g).to(DEV, torch.int32)
    a = rec.mlp_rank(net, fm_term, *sides, tg, False)
    b = rec.mlp_rank(net, fm_term, *sides, tg, False)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    for u in range(U):
        one = rec.mlp_rank(net, fm_term, Su[u:u + 1], Bu[u:u + 1], au[u:u + 1], Sc, Bc, ac, tg[u:u + 1].contiguous(), False)
        assert torch.equal(one[0][0], a[0][u]) and torch.equal(bits(one[1][0]), bits(a[1][u]))
    for t in range(16):
        one = rec.mlp_rank(net, fm_term, *sides, tg[:, t:t + 1].contiguous(), False)
        assert torch.equal(one[0][:, 0], a[0][:, t]) and torch.equal(bits(one[1][:, 0]), bits(a[1][:, t]))
    # filtered: every target loses the user's other distinct targets ahead of it (from the unfiltered ranks themselves)
    f = rec.mlp_rank(net, fm_term, *sides, tg, True)
    r = a[0].long()
    for u in range(U):
        seen = {}
        for t in range(16):
            seen.setdefault(int(tg[u, t]), int(r[u, t]))
        for t in range(16):
            ahead = sum(1 for p, rp in seen.items() if rp < int(r[u, t]))
            assert int(f[0][u, t]) == int(r[u, t]) - ahead
    # exclusions: an excluded target is not ranked, the others lose the excluded candidates ahead of them
    excl = [[int(tg[u, 0])] + list(range(0, N, 7)) for u in range(U)]
    off, pos = rec.exclusions_csr(excl, U, DEV)
    e = rec.mlp_rank(net, fm_term, *sides, tg, False, off, pos)
    score, tol = brute(net, fm_term, *sides)
    elig = torch.ones(U, N, dtype=torch.bool, device=DEV)
    for u in range(U):
        elig[u, torch.tensor(sorted(set(excl[u])), device=DEV)] = False
    check_bracket(e[0], score, tol, tg, elig)
    assert bool((e[0][:, 0] == -1).all()) and torch.equal(e[2].long(), elig.sum(1))


@pytest.mark.parametrize("fm_term", [0, 1])
def test_rank_torch_on_a_network_the_kernel_refuses(fm_term):
    k, kp, H, L, U, N = 10, 16, 300, 2, 3, 500
    net = make_net(k, H, L, seed=5)
    assert not rec.mlp_kernel_takes(net)
    sides = make_sides(k, kp, U, N, seed=6)
    g = torch.Generator().manual_seed(7)
    tg = torch.randint(0, N, (U, 5), generator=g).to(DEV, torch.int32)
    tg[0, 4] = -1
    r, s, n = rec.mlp_rank_torch(net, fm_term, *sides, tg, False)
    score, tol = brute(net, fm_term, *sides)
    elig = torch.ones(U, N, dtype=torch.bool, device=DEV)
    check_bracket(r, score, 4 * tol, tg, elig)       # torch's GEMM sums in its own order: mlp_topk_torch's looser constant
    assert bool((n == N).all()) and int(r[0, 4]) == -1


@pytest.mark.parametrize("fm_term", [0, 1])
def test_rank_network_takes_the_torch_path_for_a_hidden_300_network(fm_term):
    """rank_network on a table, with exclusions, 20 targets per user (two calls under _rank_chunks) and filtered off and on:
    the kernel refuses the network, the result is mlp_rank_torch's on the same sides, and it lies in the float64 bracket of its
    own scores (4 x tol, mlp_topk_torch's constant in tests/test_recommend_mlp_gpu.py)."""
    sizes, item, k, H, L, U = [13, 40, 300, 9, 25], 2, 10, 300, 2, 4
    N, F = sizes[item], len(sizes)
    tb = fmx.FlatTable(sizes, k)
    torch.manual_seed(fm_term)
    tb.rows[:, :k] = torch.randn(tb.rows.shape[0], k, device=DEV) * 0.3
    tb.rows[:, tb.kp] = torch.randn(tb.rows.shape[0], device=DEV) * 0.3
    net = make_net(k, H, L, seed=5)
    assert not rec.mlp_kernel_takes(net)
    rng = np.random.default_rng(8)
    cand = np.zeros((N, F), np.int32)
    cand[:, item] = np.arange(N)
    cands = rec.NetworkCandidates(tb, [item], cand, fm_term=fm_term)
    ctx = np.stack([rng.integers(0, s, size=U) for s in sizes], axis=1).astype(np.int32)
    xv = rng.uniform(0.5, 1.5, size=ctx.shape).astype(np.float32)
    tg = rng.integers(0, N, size=(U, 20)).astype(np.int32)
    tg[:, 18] = tg[:, 1]                   # a duplicate in the other chunk
    tg[0, 3] = -1
    tg[1, 17] = N + 2
    excl = [[int(tg[u, 0])] + list(range(u, N, 9)) for u in range(U)]
    off, pos = rec.exclusions_csr(excl, U, DEV)
    ctx_fields = [f for f in range(F) if f != item]
    S, bi, sfirst, sbi, logit = rec.side_terms(tb, ctx, xv, ctx_fields)
    au = rec.network_bases(tb, sfirst, sbi, logit, fm_term, context=True).contiguous()
    sides = (S, bi, au, cands.Sc, cands.Bc, cands.ac)
    with pytest.raises(fmx._lib.FmxError):
        rec.mlp_rank(net, fm_term, *sides, torch.from_numpy(tg[:, :16].copy()).to(DEV))
    score, tol = brute(net, fm_term, *sides)
    elig = torch.ones(U, N, dtype=torch.bool, device=DEV)
    for u in range(U):
        elig[u, torch.tensor(sorted(set(excl[u])), device=DEV)] = False
    tgd = torch.from_numpy(tg).to(DEV)
    for filtered in (False, True):
        r, s, n = rec.rank_network(tb, net, fm_term, ctx, xv, cands, tg, exclude=excl, filtered=filtered)
        want = rec._rank_chunks(lambda ch, f: rec.mlp_rank_torch(net, fm_term, *sides, ch, f, off, pos), tg, U, DEV, filtered)
        for x, y in zip((r, s, n), want):
            assert torch.equal(x, y)
        assert r.dtype == torch.int64 and r.shape == (U, 20) and torch.equal(n, elig.sum(1))
        assert bool((r[:, 0] == -1).all()) and int(r[0, 3]) == -1 and int(r[1, 17]) == -1
        if not filtered:
            check_bracket(r, score, 4 * tol, tgd, elig)
            raw = r
        else:                              # per target: the user's other eligible targets are not candidates
            for t in range(20):
                e = elig.clone()
                for u in range(U):
                    others = [int(q) for q in tg[u] if 0 <= q < N and q != tg[u, t]]
                    if others:
                        e[u, torch.tensor(others, device=DEV)] = False
                check_bracket(r[:, t:t + 1], score, 4 * tol, tgd[:, t:t + 1], e)
            assert bool((r <= raw).all()) and bool((r < raw).any())
