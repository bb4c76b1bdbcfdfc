"""Checks shared by the rank tests (test_rank_*_gpu.py): the numpy statement of fmx_*_rank's definition (include/fmx.h), the
bit-exact cross-check with the family's top-K rows, and the float64 bracket."""
import numpy as np
import torch


def np_ranks(score, targets, excl=None, filtered=False):
    """The definition, literally.  score: float64 [U, N] (NaN: not eligible); targets: int [U, T]; excl: None or U
    collections of positions.  Returns (rank int64 [U, T], score float64 [U, T], n_cand int64 [U])."""
    U, N = score.shape
    T = targets.shape[1]
    rank = np.full((U, T), -1, dtype=np.int64)
    sc = np.full((U, T), -np.inf)
    n_cand = np.zeros(U, dtype=np.int64)
    for u in range(U):
        s = score[u] + 0.0
        elig = ~np.isnan(s)
        if excl is not None:
            e = np.asarray(sorted(excl[u]), dtype=np.int64)
            elig[e[(e >= 0) & (e < N)]] = False
        idx = np.nonzero(elig)[0]
        order = idx[np.lexsort((idx, -s[idx]))]          # score descending, then position ascending
        at = np.full(N, -1, dtype=np.int64)
        at[order] = np.arange(order.size)
        n_cand[u] = order.size
        good = [int(p) for p in targets[u] if 0 <= p < N and elig[p]]
        for t in range(T):
            p = int(targets[u, t])
            if not (0 <= p < N and elig[p]):
                continue
            r = int(at[p])
            if filtered:
                r -= sum(1 for q in set(good) if at[q] < at[p])
            rank[u, t], sc[u, t] = r, s[p]
    return rank, sc, n_cand


def bits(x):
    return x.contiguous().view(torch.int32)


def check_against_topk(rank, score, targets, top_pos, top_score):
    """With filtered = 0: a target has 0 <= rank < K exactly when it appears in the top-K row, then at index `rank` and with
    the same score bits.  rank, score, targets [U, T]; top_pos, top_score [U, K]."""
    K = top_pos.shape[1]
    rank, targets, top_pos = rank.long().cpu(), targets.long().cpu(), top_pos.long().cpu()
    sb, tb = bits(score.cpu()), bits(top_score.cpu())
    n_in = 0
    for u in range(rank.shape[0]):
        row = {int(p): i for i, p in enumerate(top_pos[u].tolist()) if p >= 0}
        for t in range(rank.shape[1]):
            p, r = int(targets[u, t]), int(rank[u, t])
            if p < 0:
                assert r == -1
                continue
            assert (0 <= r < K) == (p in row), (u, t, p, r)
            if p in row:
                assert row[p] == r, (u, t, p, r, row[p])
                assert int(tb[u, r]) == int(sb[u, t]), (u, t, p)
                n_in += 1
    return n_in


def bracket(score64, tol, targets, eligible):
    """lo, hi [U, T] of the float64 order: lo = #{eligible c != p: s(c) > s(p) + tol}, hi = #{eligible c != p: s(c) >= s(p) -
    tol}, tol = tol(u, c) + tol(u, p) (each score carries its own error); -1 where the target is not eligible.  score64, tol
    [U, N] float64 tensors (tol may be [U, 1]), eligible bool [U, N], targets int [U, T]."""
    U, N = score64.shape
    tg = targets.long().to(score64.device)
    inside = (tg >= 0) & (tg < N)
    tgc = torch.where(inside, tg, torch.zeros_like(tg))
    ok = inside & eligible.gather(1, tgc)
    tol = tol.expand(U, N)
    lo = torch.full_like(tg, -1)
    hi = torch.full_like(tg, -1)
    ar = torch.arange(N, device=score64.device)[None, :]
    for t in range(tg.shape[1]):
        sp, tp = score64.gather(1, tgc[:, t:t + 1]), tol.gather(1, tgc[:, t:t + 1])
        other = eligible & (ar != tgc[:, t:t + 1])
        lo[:, t] = (other & (score64 > sp + (tol + tp))).sum(1)
        hi[:, t] = (other & (score64 >= sp - (tol + tp))).sum(1)
    lo[~ok], hi[~ok] = -1, -1
    return lo, hi, ok


def check_bracket(rank, score64, tol, targets, eligible):
    lo, hi, ok = bracket(score64, tol, targets, eligible)
    r = rank.long().to(lo.device)
    assert bool((r[~ok] == -1).all())
    assert bool(((lo <= r) & (r <= hi))[ok].all()), (lo[ok], r[ok], hi[ok])
    return lo, hi, ok
