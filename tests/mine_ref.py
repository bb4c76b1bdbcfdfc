"""The reference of fmx_fm_mine_negatives (include/fmx.h) for the tests: Philox4x32-10 and the draw layout in numpy, and the
selection through the entry point's own definition -- fmx_fm_topk with K = n_neg over the set of a user's drawn, non-own
candidates.  Nothing about the score is recomputed here, so the comparison with the kernel is bit for bit."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: uint32 [..., 4], key: uint32 [..., 2] (broadcast against each other) -> uint32 [..., 4]"""
    c = np.asarray(counter, dtype=np.uint64)
    k = np.asarray(key, dtype=np.uint64)
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                       # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def draws(seed, offset, u_base, U, n_draw, N):
    """The drawn positions int64 [U, n_draw]: draw j of user u is word j & 3 of the block with key (seed lo, seed hi) and
    counter (offset lo, offset hi, (u_base + u) mod 2^32, j >> 2); position = (word * N) >> 32."""
    seed, offset = int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)
    nb = (n_draw + 3) // 4
    ctr = np.zeros((U, nb, 4), dtype=np.uint64)
    ctr[..., 0] = offset & MASK
    ctr[..., 1] = offset >> 32
    ctr[..., 2] = ((int(u_base) + np.arange(U, dtype=np.uint64)) & MASK)[:, None]
    ctr[..., 3] = np.arange(nb, dtype=np.uint64)[None, :]
    words = philox4x32_10(ctr, np.array([seed & MASK, seed >> 32], dtype=np.uint64)).reshape(U, nb * 4)[:, :n_draw]
    return ((words.astype(np.uint64) * np.uint64(N)) >> np.uint64(32)).astype(np.int64)


def select(drawn, own, excl, n_neg, topk_call):
    """Per user: the distinct drawn positions ascending (so that the position tie-break survives the renumbering), without
    the own position and without the user's excluded ones; topk_call(u, positions int64 [n], K) -> (pos int [K], score
    fp32 [K]) is fmx_fm_topk over those rows of Sc / ac for user u, in the gathered numbering (-1 / -inf padded; a NaN score
    is the library's to refuse).  drawn [U, n_draw]; own [U] or None (-1: none); excl: None or U arrays.  Returns
    (neg_pos int32 [U, n_neg], neg_score fp32 [U, n_neg])."""
    U = drawn.shape[0]
    neg_pos = np.full((U, n_neg), -1, dtype=np.int32)
    neg_score = np.full((U, n_neg), -np.inf, dtype=np.float32)
    for u in range(U):
        pos = np.unique(drawn[u])
        if own is not None:
            pos = pos[pos != int(own[u])]
        if excl is not None:
            pos = pos[~np.isin(pos, np.asarray(excl[u], dtype=np.int64))]
        if len(pos) == 0:
            continue
        p, s = topk_call(u, pos, n_neg)
        p, s = np.asarray(p).reshape(-1), np.asarray(s, dtype=np.float32).reshape(-1)
        neg_pos[u] = np.where(p >= 0, pos[np.clip(p, 0, None)], -1)
        neg_score[u] = s
    return neg_pos, neg_score
