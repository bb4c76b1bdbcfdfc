"""fmx_fm_rank on the GPU: exact agreement with the numpy statement of its definition on inputs whose scores are exact in
fp32 (ties, exclusions, padding, NaN rows, filtered ranks, duplicate targets), the bit-exact cross-check with fmx_fm_topk, the
float64 bracket on random floats, determinism and batch independence.  The shapes cross every boundary of the scan: one pair,
the chunk of 256 (N = 255 / 257), the user tile of 16 (U = 17), the split minimum of 2048 (N = 2049) and several splits
(N = 70,000 with U = 33)."""
import numpy as np
import pytest
import torch

from fmx import recommend as rec
from rank_checks import bits, bracket, check_against_topk, check_bracket, np_ranks
from test_recommend_gpu import make

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1, 1), (3, 255), (3, 257), (17, 300), (2, 2049), (33, 70000)]
TS = (1, 2, 16)


def exact_inputs(kp, U, N, seed):
    """multiples of 1/8 in [-2, 2]: every product and partial sum is exact in fp32, so float64 numpy gives the device's bits"""
    rng = np.random.default_rng(seed)
    d = lambda *s: (rng.integers(-16, 17, size=s) / 8.0).astype(np.float32)   # noqa: E731
    return d(U, kp), d(U), d(N, kp), d(N)


def score64(Su, au, Sc, ac):
    return au.astype(np.float64)[:, None] + ac.astype(np.float64)[None, :] + Su.astype(np.float64) @ Sc.astype(np.float64).T


def draw_targets(rng, U, N, T, dup=True):
    tg = rng.integers(0, N, size=(U, T)).astype(np.int32)
    if dup and T > 1:
        tg[:, -1] = tg[:, 0]                          # a duplicated target
    return tg


def run(Su, au, Sc, ac, tg, filtered, off=None, pos=None):
    dev = [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in (Su, au, Sc, ac, tg)]
    r, s, n = rec.fm_rank(dev[0], dev[1], dev[2], dev[3], dev[4], filtered, off, pos)
    torch.cuda.synchronize()
    return r.cpu().numpy(), s.cpu(), n.cpu().numpy()


def assert_exact(got, want):
    (r, s, n), (wr, ws, wn) = got, want
    np.testing.assert_array_equal(r, wr)
    np.testing.assert_array_equal(n, wn)
    assert torch.equal(bits(s), bits(torch.from_numpy(ws.astype(np.float32)))), "scores differ in their bits"


# every shape at kp 4, 16 and 64; the other two widths the dispatch knows at one pair and past one chunk
KP_CASES = [(U, N, kp) for U, N in SHAPES for kp in (4, 16, 64)] + [(U, N, kp) for U, N in ((1, 1), (3, 257)) for kp in (8, 32)]


@pytest.mark.parametrize("variant", ["plain", "excl", "pad", "nan"])
@pytest.mark.parametrize("U, N, kp", KP_CASES)
def test_fm_rank_is_the_definition_exactly(U, N, kp, variant):
    rng = np.random.default_rng(1000 * kp + N + U)
    Su, au, Sc, ac = exact_inputs(kp, U, N, seed=N + kp)
    ref = score64(Su, au, Sc, ac)
    for T in TS:
        tg = draw_targets(rng, U, N, T)
        excl, off, pos = None, None, None
        if variant == "excl":       # per-user lists, one of them holding the user's first target; a position beyond N too
            excl = [sorted(set(rng.integers(0, N, size=min(N, 5 + 3 * u)).tolist()) | ({int(tg[u, 0])} if u % 2 == 0 else set())
                           | {N + 7}) for u in range(U)]
            off, pos = rec.exclusions_csr(excl, U, DEV)
        if variant == "pad":
            tg[:, T // 2] = -1
            if T > 1:
                tg[0, 0] = N + 3
            else:
                tg[-1, 0] = N
        if variant == "nan":
            ac = ac.copy()
            ac[rng.integers(0, N, size=max(1, N // 40))] = np.nan
            ac[tg[0, 0]] = np.nan                                     # one NaN row is a target
            ref = score64(Su, au, Sc, ac)
        for filtered in (False, True):
            assert_exact(run(Su, au, Sc, ac, tg, filtered, off, pos), np_ranks(ref, tg, excl, filtered))


def test_the_tie_break_is_exercised():
    """the exact inputs are full of ties: some target has equal-score candidates on both sides of its position, and the rank
    counts the one in front only"""
    U, N, kp = 17, 300, 4
    Su, au, Sc, ac = exact_inputs(kp, U, N, seed=N + kp)
    ref = score64(Su, au, Sc, ac)
    tg = draw_targets(np.random.default_rng(5), U, N, 16, dup=False)
    both = 0
    for u in range(U):
        for p in tg[u]:
            same = np.nonzero(ref[u] == ref[u, p])[0]
            both += int((same < p).any() and (same > p).any())
    assert both >= 1
    assert_exact(run(Su, au, Sc, ac, tg, False), np_ranks(ref, tg))


@pytest.mark.parametrize("kp, U, N", [(16, 1, 1), (4, 3, 255), (16, 17, 256), (64, 3, 257), (16, 2, 2049), (16, 33, 70000)])
def test_fm_rank_agrees_with_topk_bit_for_bit(kp, U, N):
    Su, au, Sc, ac = make(kp, U, N, seed=N + kp)
    top_pos, top_score = rec.fm_topk(Su, au, Sc, ac, 256)
    if N <= 256:        # every candidate is a target: the top-K row pins every rank
        tg = torch.arange(N, dtype=torch.int32, device=DEV)[None, :].repeat(U, 1)
    else:               # the head of the row, and random positions mostly outside it
        g = torch.Generator().manual_seed(N)
        tg = torch.cat([top_pos[:, :24], torch.randint(0, N, (U, 24), generator=g).to(DEV, torch.int32)], 1).to(torch.int32)
    n_in = 0
    for c0 in range(0, tg.shape[1], 16):
        ch = tg[:, c0:c0 + 16].contiguous()
        r, s, n = rec.fm_rank(Su, au, Sc, ac, ch, False)
        n_in += check_against_topk(r, s, ch, top_pos, top_score)
        assert bool((n == N).all())
    assert n_in >= U * min(N, 24)


def fm_tol(Su, au, Sc, ac, kp):
    """2 (kp + 2) eps32 max_c (|au| + |ac| + sum_d |Su_d Sc_d|): the forward error bound of the stated chain (kp + 2 roundings
    per score, two scores in a comparison), taken at its maximum over the row"""
    mag = au.double().abs()[:, None] + ac.double().abs()[None, :] + Su.double().abs() @ Sc.double().abs().T
    return (kp + 2) * 2.0 ** -24 * mag.max(1, keepdim=True).values     # bracket() adds the candidate's and the target's


@pytest.mark.parametrize("kp, U, N", [(4, 3, 257), (16, 17, 2049), (64, 5, 2049), (16, 33, 70000)])
def test_fm_rank_within_the_float64_bracket(kp, U, N):
    Su, au, Sc, ac = make(kp, U, N, seed=7 * N + kp)
    s64 = au.double()[:, None] + ac.double()[None, :] + Su.double() @ Sc.double().T
    tol = fm_tol(Su, au, Sc, ac, kp)
    elig = torch.ones(U, N, dtype=torch.bool, device=DEV)
    g = torch.Generator().manual_seed(kp)
    tg = torch.randint(0, N, (U, 16), generator=g).to(DEV, torch.int32)
    # the test is not vacuous: on the CPU, the float64 order brackets nearly every target within 2 places
    lo, hi, ok = bracket(s64.cpu(), tol.cpu(), tg.cpu(), elig.cpu())
    assert float(((hi - lo) <= 2)[ok].double().mean()) >= 0.95
    for filtered in (False,):
        r, s, n = rec.fm_rank(Su, au, Sc, ac, tg, filtered)
        check_bracket(r, s64, tol, tg, elig)
        sp = s64.gather(1, tg.long())
        assert bool(((s.double() - sp).abs() <= tol).all())


def test_determinism_batch_independence_and_one_target_at_a_time():
    kp, U, N = 16, 19, 5000
    Su, au, Sc, ac = make(kp, U, N, seed=3)
    g = torch.Generator().manual_seed(1)
    tg = torch.randint(0, N, (U, 16), generator=g).to(DEV, torch.int32)
    a = rec.fm_rank(Su, au, Sc, ac, tg, False)
    b = rec.fm_rank(Su, au, Sc, ac, tg, False)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    for u in range(U):
        one = rec.fm_rank(Su[u:u + 1], au[u:u + 1], Sc, ac, tg[u:u + 1].contiguous(), False)
        assert torch.equal(one[0][0], a[0][u]) and torch.equal(bits(one[1][0]), bits(a[1][u])) and int(one[2][0]) == int(a[2][u])
    for t in range(16):
        one = rec.fm_rank(Su, au, Sc, ac, tg[:, t:t + 1].contiguous(), False)
        assert torch.equal(one[0][:, 0], a[0][:, t]) and torch.equal(bits(one[1][:, 0]), bits(a[1][:, t]))


def test_rank_chunks_over_more_than_16_targets_and_filters_across_them():
    """fmx.recommend._rank_chunks: 40 targets per user run as three calls; the filtered ranks equal the definition's"""
    U, N, kp = 5, 700, 16
    Su, au, Sc, ac = exact_inputs(kp, U, N, seed=11)
    ref = score64(Su, au, Sc, ac)
    rng = np.random.default_rng(2)
    tg = rng.integers(0, N, size=(U, 40)).astype(np.int32)
    tg[:, 33] = tg[:, 2]            # a duplicate in another chunk
    tg[:, 5] = -1
    dev = [torch.from_numpy(x).to(DEV) for x in (Su, au, Sc, ac)]
    for filtered in (False, True):
        r, s, n = rec._rank_chunks(lambda ch, f: rec.fm_rank(dev[0], dev[1], dev[2], dev[3], ch, f), tg, U, DEV, filtered)
        wr, ws, wn = np_ranks(ref, tg, None, filtered)
        np.testing.assert_array_equal(r.cpu().numpy(), wr)
        np.testing.assert_array_equal(n.cpu().numpy(), wn)
        np.testing.assert_array_equal(s.cpu().numpy(), ws.astype(np.float32))
