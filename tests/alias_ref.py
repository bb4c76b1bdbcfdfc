"""The reference of fmx_alias_sample_negatives (include/fmx.h) for the tests, in numpy over mine_ref.philox4x32_10: the draw layout,
the alias lookup and the selection of a row's first n_neg eligible draws -- integers throughout, so the comparison with the kernel
is bit for bit -- and the bound on |q - w / sum(w)| of fmx.pairwise.alias_table.  Helper module, not collected."""
import numpy as np

import mine_ref

ONE = 1 << 24


def draws(thresh, alias, seed, offset, u_base, U, n_try):
    """The drawn positions int64 [U, n_try]: draw t of row u takes words 2 (t & 1) and 2 (t & 1) + 1 of the block with key
    (seed lo, seed hi) and counter (offset lo, offset hi, (u_base + u) mod 2^32, 0x80000000 + (t >> 1)); p = (a * N) >> 32,
    position = p if (b >> 8) < thresh[p] else alias[p]."""
    thresh, alias = np.asarray(thresh, dtype=np.int64), np.asarray(alias, dtype=np.int64)
    N = len(thresh)
    seed, offset = int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)
    nb = (n_try + 1) // 2
    ctr = np.zeros((U, nb, 4), dtype=np.uint64)
    ctr[..., 0] = offset & mine_ref.MASK
    ctr[..., 1] = offset >> 32
    ctr[..., 2] = ((int(u_base) + np.arange(U, dtype=np.uint64)) & mine_ref.MASK)[:, None]
    ctr[..., 3] = (0x80000000 + np.arange(nb, dtype=np.uint64))[None, :]
    words = mine_ref.philox4x32_10(ctr, np.array([seed & mine_ref.MASK, seed >> 32], dtype=np.uint64)).astype(np.uint64)
    a = words[..., 0::2].reshape(U, nb * 2)[:, :n_try]
    b = words[..., 1::2].reshape(U, nb * 2)[:, :n_try]
    p = ((a * np.uint64(N)) >> np.uint64(32)).astype(np.int64)
    return np.where((b >> np.uint64(8)).astype(np.int64) < thresh[p], p, alias[p])


def sample(thresh, alias, logq, seed, offset, u_base, U, n_neg, n_try, own=None, excl=None):
    """-> (neg_pos int32 [U, n_neg] padded with -1, neg_logq fp32 [U, n_neg] padded with -inf): per row the first n_neg draws, in
    draw order and with repeats, that lie in [0, N), are not own[u] (None or -1: none) and not in excl[u] (None or U arrays)."""
    N = len(thresh)
    drawn = draws(thresh, alias, seed, offset, u_base, U, n_try)
    neg_pos = np.full((U, n_neg), -1, dtype=np.int32)
    neg_logq = np.full((U, n_neg), -np.inf, dtype=np.float32)
    for u in range(U):
        d = drawn[u]
        ok = (d >= 0) & (d < N)
        if own is not None:
            ok &= d != int(own[u])
        if excl is not None:
            ok &= ~np.isin(d, np.asarray(excl[u], dtype=np.int64))
        kept = d[ok][:n_neg]
        neg_pos[u, :len(kept)] = kept
        if logq is not None:
            neg_logq[u, :len(kept)] = np.asarray(logq, dtype=np.float32)[kept]
    return neg_pos, neg_logq


def realised_numerators(thresh, alias):
    """int64 [N]: q_i (N 2^24) = thresh_i + sum_{j: alias_j = i} (2^24 - thresh_j), exactly"""
    thresh, alias = np.asarray(thresh, dtype=np.int64), np.asarray(alias, dtype=np.int64)
    num = thresh.copy()
    np.add.at(num, alias, ONE - thresh)
    return num


def q_bound(alias):
    """|q_i - w_i / sum(w)| <= this, float64 [N].  Vose's construction splits cell j exactly between j (share p_j) and alias_j
    (share 1 - p_j); the table stores round(p_j 2^24), off by at most 1/2 in units of 2^-24 -- and what cell j's own share gains,
    alias_j's loses.  Position i is touched by its own cell and by the n_i cells whose alias it is: (1 + n_i) / 2 units, over the
    N 2^24 units of the whole table.  The float64 arithmetic of the construction adds one rounding of at most 2^-53 relative to a
    share <= N per subtraction from a large cell (n_i of them) and per scaling: (2 + n_i) 2^-52 in units of 1 / N ... of q at most
    (2 + n_i) 2^-52."""
    alias = np.asarray(alias, dtype=np.int64)
    n = np.bincount(alias, minlength=len(alias)).astype(np.float64)
    return (1.0 + n) * 0.5 / (len(alias) * float(ONE)) + (2.0 + n) * 2.0 ** -52
