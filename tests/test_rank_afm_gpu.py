"""fmx_afm_rank on the GPU: the bit-exact cross-check with fmx_afm_topk, the float64 bracket with the forward and the tolerance of
tests/test_recommend_afm_gpu.py, determinism and batch independence.  Layouts: the smallest that file uses (one field a side),
three fields, and one with two item fields; t = 4 and 16; N = 257 (past the chunk of 256) and N = 8193 (past the scan's
largest split minimum, 8192: several splits for every layout)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rank_checks import bits, check_against_topk, check_bracket  # noqa: E402
from test_recommend_afm_gpu import run  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
LAYOUTS = [(2, [1], 4, 4), (3, [0], 10, 16), (5, [1, 3], 10, 4), (5, [1, 3], 16, 16)]      # (F, item fields, k, t)


def _rec():
    from fmx import recommend
    return recommend


def targets_for(top_pos, U, N, seed):
    g = torch.Generator().manual_seed(seed)
    tg = torch.cat([top_pos[:, :6].to(torch.int32), torch.randint(0, N, (U, 10), generator=g).to(DEV, torch.int32)], 1)
    tg[0, 15] = -1
    tg[-1, 14] = N + 1
    return tg.contiguous()


def check_layout(F, item, k, t, N, Ts):
    rec, U = _rec(), 3
    r0 = run(F, item, k, t, U, N, 256, seed=N % 7)
    tg = targets_for(r0["pos"], U, N, seed=N)
    elig = torch.ones(U, N, dtype=torch.bool, device=DEV)
    for T in Ts:
        tt = tg[:, :T].contiguous() if T < 16 else tg
        r, s, n = rec.rank_afm(r0["tb"], r0["afm"], r0["ctx"], r0["cx"], r0["cands"], tt)
        check_against_topk(r, s, torch.where(tt < N, tt, torch.full_like(tt, -1)), r0["pos"], r0["val"])
        check_bracket(r, r0["score"], r0["tol"], tt, elig)
        assert bool((n == N).all())


@pytest.mark.parametrize("N", [257, 8193])
@pytest.mark.parametrize("F, item, k, t", LAYOUTS)
def test_afm_rank_against_topk_and_float64(F, item, k, t, N):
    check_layout(F, item, k, t, N, (1, 2, 16))


@pytest.mark.parametrize("k", [5, 17, 33])
def test_afm_rank_at_the_other_row_widths(k):
    """LAYOUTS reaches kp 4 and 16; these are kp 8, 32 and 64 of the rank call's dispatch, under the same checks"""
    check_layout(3, [1], k, 4, 257, (1, 16))


def test_determinism_batch_independence_and_one_target_at_a_time():
    rec, U, N = _rec(), 3, 8193
    r0 = run(5, [1, 3], 10, 4, U, N, 10, seed=2)
    g = torch.Generator().manual_seed(3)
    tg = torch.randint(0, N, (U, 16), generator=g).to(DEV, torch.int32)
    args = (r0["tb"], r0["afm"])
    a = rec.rank_afm(*args, r0["ctx"], r0["cx"], r0["cands"], tg)
    b = rec.rank_afm(*args, r0["ctx"], r0["cx"], r0["cands"], tg)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    for u in range(U):
        one = rec.rank_afm(*args, r0["ctx"][u:u + 1], r0["cx"][u:u + 1], r0["cands"], tg[u:u + 1])
        assert torch.equal(one[0][0], a[0][u]) and torch.equal(bits(one[1][0]), bits(a[1][u]))
    for t in range(16):
        one = rec.rank_afm(*args, r0["ctx"], r0["cx"], r0["cands"], tg[:, t:t + 1])
        assert torch.equal(one[0][:, 0], a[0][:, t]) and torch.equal(bits(one[1][:, 0]), bits(a[1][:, t]))
    # exclusions (lists and CSR alike) and the filtered rank
    excl = [[int(tg[u, 0])] + list(range(u, N, 5)) for u in range(U)]
    e = rec.rank_afm(*args, r0["ctx"], r0["cx"], r0["cands"], tg, exclude=excl)
    off, pos = rec.exclusions_csr(excl, U, "cpu")
    e2 = rec.rank_afm(*args, r0["ctx"], r0["cx"], r0["cands"], tg, exclude=(off, pos))
    for x, y in zip(e, e2):
        assert torch.equal(x, y)
    elig = torch.ones(U, N, dtype=torch.bool, device=DEV)
    for u in range(U):
        elig[u, torch.tensor(sorted(set(excl[u])), device=DEV)] = False
    check_bracket(e[0], r0["score"], r0["tol"], tg, elig)
    assert bool((e[0][:, 0] == -1).all()) and torch.equal(e[2], elig.sum(1))
    f = rec.rank_afm(*args, r0["ctx"], r0["cx"], r0["cands"], tg, filtered=True)
    for u in range(U):
        seen = {}
        for t in range(16):
            seen.setdefault(int(tg[u, t]), int(a[0][u, t]))
        for t in range(16):
            assert int(f[0][u, t]) == int(a[0][u, t]) - sum(1 for rp in seen.values() if rp < int(a[0][u, t]))
