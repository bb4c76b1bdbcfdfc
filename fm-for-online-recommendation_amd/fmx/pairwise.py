"""Pairwise-ranking (BPR) training data: torch plumbing around fmx_fm_pair_* (include/fmx.h), no kernels of its own.

A batch of B pairs is [2B, F] full-width rows, row 2i the positive sample of pair i and row 2i + 1 its negative: the
positive's row with the item columns replaced.  sample_negatives draws the replacements, assemble_pairs interleaves the rows;
FMEngine.pair_step / pair_stream / pair_online_run take the result.

Hard negatives (dynamic negative sampling; Zhang et al. 2013, Rendle & Freudenthaler 2014): mine_negatives draws n_draw
candidates per positive on the device, scores them under the current FM and keeps the n_neg best (fmx_fm_mine_negatives).
HardNegatives carries the settings of that through the `negatives` argument of fit_pairs / run_pair_experiment / fit_lists.

Listwise (sampled-softmax) training (fmx_fm_list_*) takes the same positives and negatives as B lists of G = 1 + n_neg rows,
[B G, F], the positive first: assemble_lists; FMEngine.list_step / list_stream take the result.

Popularity-sampled negatives: alias_table builds Walker's alias table of a weight per candidate position on the host,
alias_sample draws from it on the device (fmx_alias_sample_negatives) and returns log Q of every draw, which the corrected list
calls (fmx_fm_list_*_q: FMEngine.list_step_q / list_stream_q) subtract from the logits.  PopularityNegatives carries the table and
its settings through the `negatives` argument.

In-batch sampled softmax (fmx_fm_inbatch_*): the positives alone, [B, F]; every row's negatives are the other rows' items.
in_batch_keys names the rows that hold the same item, which the loss leaves out of each other's softmax;
FMEngine.inbatch_step / inbatch_stream take the rows, the keys and log Q of every row's item.

The cross-batch item bank (fmx_fm_inbatch_bank_*): ItemBank keeps the items of earlier batches on the device as further
negatives of every later row; FMEngine.inbatch_bank_step / inbatch_bank_stream take it, item_keys gives the keys that hold
across batches.
"""
import ctypes as C

import torch

from . import _lib


def _item_fields(item_fields):
    fields = [int(f) for f in (item_fields if hasattr(item_fields, "__len__") else [item_fields])]
    if not fields or len(set(fields)) != len(fields):
        raise ValueError(f"item_fields {item_fields!r}: one or more distinct field indices")
    return fields


def n_pairs(idx_d):
    """-> B of the interleaved rows [2B, F] of B pairs (FMEngine's and AFMEngine's pair calls)"""
    if idx_d.dim() != 2 or idx_d.shape[0] % 2 or idx_d.shape[0] < 2:
        raise ValueError(f"pair rows must be [2B, F] with B >= 1, got {tuple(idx_d.shape)}")
    return idx_d.shape[0] // 2


def in_batch_keys(idx, item_fields):
    """Dense keys of the item columns of idx [B, F] for the in-batch loss (fmx_fm_inbatch_step's key): int32 [B] on idx's device,
    equal exactly where two rows hold the same item in every item field -- the inverse of torch.unique(dim=0) over those columns."""
    fields = _item_fields(item_fields)
    idx = torch.as_tensor(idx)
    if idx.dim() != 2:
        raise ValueError(f"in_batch_keys: rows [B, F], got {tuple(idx.shape)}")
    if not all(0 <= f < idx.shape[1] for f in fields):
        raise ValueError(f"item_fields {fields}: fields of 0..{idx.shape[1] - 1}")
    _, inverse = torch.unique(idx[:, fields], dim=0, return_inverse=True)
    return inverse.reshape(-1).to(torch.int32).contiguous()


def item_keys(idx, item_fields, field_sizes):
    """Keys of the item columns of idx [B, F] that mean the same item in EVERY batch (in_batch_keys' are dense per batch): the
    mixed-radix number of the item fields' indices over field_sizes [F], int32 [B] on idx's device.  What a keyed ItemBank needs:
    a banked item is compared with the items of later batches."""
    fields = _item_fields(item_fields)
    idx = torch.as_tensor(idx)
    if idx.dim() != 2:
        raise ValueError(f"item_keys: rows [B, F], got {tuple(idx.shape)}")
    if not all(0 <= f < idx.shape[1] for f in fields):
        raise ValueError(f"item_fields {fields}: fields of 0..{idx.shape[1] - 1}")
    total = 1
    for f in fields:
        total *= int(field_sizes[f])
    if total >= 2 ** 31:
        raise ValueError(f"item_keys: the item fields {fields} span {total} combinations, more than an int32 key holds")
    key = torch.zeros(idx.shape[0], dtype=torch.int64, device=idx.device)
    for f in fields:
        key = key * int(field_sizes[f]) + idx[:, f].long()
    return key.to(torch.int32).contiguous()


class ItemBank:
    """The cross-batch item bank of fmx_fm_inbatch_bank_* (include/fmx.h: fmx_item_bank_t): a device-resident ring of `capacity`
    slots that keeps the item-side sums (S_c, a_c) of earlier in-batch steps, which every later row takes as further negatives.
    It owns the arrays and the zeroed state (head, count).  keyed: it keeps item keys (the steps on it must pass keys that mean
    the same item in every batch: item_keys); corrected: it keeps log Q of every item (the steps must pass corr).
    The values are those of the weights when the item was pushed: they go stale as training goes on, a ring of a few batches
    bounds their age.  A captured step advances the bank on every replay; a second pass over the same data meets its own items
    as negatives unless keys mask them."""

    def __init__(self, capacity, kp, device, keyed=True, corrected=True):
        capacity, kp = int(capacity), int(kp)
        if capacity < 1 or capacity > _lib.ITEM_BANK_MAX:
            raise ValueError(f"ItemBank: capacity = {capacity} must lie in [1, {_lib.ITEM_BANK_MAX}]")
        if kp not in (4, 8, 16, 32, 64):
            raise ValueError(f"ItemBank: kp = {kp} must be the table's padded k: 4, 8, 16, 32 or 64")
        self.capacity, self.kp, self.device = capacity, kp, torch.device(device)
        self.S = torch.zeros((capacity, kp), dtype=torch.float32, device=device)
        self.a = torch.zeros(capacity, dtype=torch.float32, device=device)
        self.corr = torch.zeros(capacity, dtype=torch.float32, device=device) if corrected else None
        self.key = torch.zeros(capacity, dtype=torch.int32, device=device) if keyed else None
        self.state = torch.zeros(2, dtype=torch.int32, device=device)
        self._c = _lib.ItemBank()
        self._c.S, self._c.a, self._c.state = self.S.data_ptr(), self.a.data_ptr(), self.state.data_ptr()
        self._c.corr = None if self.corr is None else self.corr.data_ptr()
        self._c.key = None if self.key is None else self.key.data_ptr()
        self._c.capacity, self._c.kp = capacity, kp

    @property
    def keyed(self):
        return self.key is not None

    @property
    def corrected(self):
        return self.corr is not None

    def clear(self):
        """An empty bank again (the slots keep their bytes: a slot >= count is never read)"""
        self.state.zero_()

    def head(self):
        return int(self.state[0].item())

    def count(self):
        """The number of valid slots: a host read (a sync), for tests and users"""
        return int(self.state[1].item())

    def c_struct(self):
        return C.byref(self._c)


def _negatives_3d(neg_items, B, m, what="neg_items"):
    """-> [B, n_neg, m]: accepts [B, n_neg, m], [B, m] (one negative per positive) and, with one item field, [B]."""
    t = torch.as_tensor(neg_items)
    if t.dim() == 1 and m == 1:
        t = t.reshape(B, 1, 1)
    elif t.dim() == 2:
        t = t.reshape(B, 1, m)
    if t.dim() != 3 or t.shape[0] != B or t.shape[2] != m:
        raise ValueError(f"{what} of shape {tuple(t.shape)}: expected [{B}, n_neg, {m}] (or [{B}, {m}] for one negative each)")
    return t


def assemble_pairs(pos_idx, pos_xv, item_fields, neg_items, neg_xv=None):
    """The interleaved rows of B * n_neg pairs -> (idx [2 B n_neg, F] int32, xv [2 B n_neg, F] float32 or None).

    pos_idx [B, F] (pos_xv [B, F] or None: every value 1); neg_items [B, n_neg, m] holds, per positive and negative, the indices
    of the m item fields in the order of item_fields ([B, m]: one negative each).  Pair b * n_neg + j is positive b against its
    j-th negative: row 2p is the positive, row 2p + 1 the positive with the item columns replaced -- so with n_neg > 1 a positive
    is repeated once per negative.  neg_xv (same shape as neg_items) replaces the item columns' values too; by default the
    negative keeps the positive's values."""
    return _assemble(pos_idx, pos_xv, item_fields, neg_items, neg_xv, lists=False)


def assemble_lists(pos_idx, pos_xv, item_fields, neg_items, neg_xv=None):
    """The rows of B lists of G = 1 + n_neg -> (idx [B G, F] int32, xv [B G, F] float32 or None), what FMEngine.list_step takes
    (fmx_fm_list_*, the sampled-softmax loss).  The arguments, the shapes accepted and the errors are assemble_pairs'; row G b is
    positive b -- once, not once per negative -- and row G b + 1 + j the positive with the item columns replaced by its j-th
    negative."""
    return _assemble(pos_idx, pos_xv, item_fields, neg_items, neg_xv, lists=True)


def _assemble(pos_idx, pos_xv, item_fields, neg_items, neg_xv, lists):
    """pairs: [B, n_neg, (positive, negative), F]; lists: [B, (positive, negatives ...), F]; flattened over all but F"""
    fields = _item_fields(item_fields)
    pos_idx = torch.as_tensor(pos_idx)
    if pos_idx.dim() != 2:
        raise ValueError(f"pos_idx of shape {tuple(pos_idx.shape)}: expected [B, F]")
    B, F = pos_idx.shape
    if max(fields) >= F or min(fields) < 0:
        raise ValueError(f"item_fields {fields} outside the {F} columns of pos_idx")
    dev = pos_idx.device
    neg = _negatives_3d(neg_items, B, len(fields)).to(device=dev, dtype=pos_idx.dtype)
    n_neg = neg.shape[1]
    cols = torch.as_tensor(fields, dtype=torch.long, device=dev)

    def spread(t, repl):
        if lists:
            out = t.reshape(B, 1, F).expand(B, 1 + n_neg, F).clone()
            if repl is not None:
                out[:, 1:, cols] = repl
        else:
            out = t.reshape(B, 1, 1, F).expand(B, n_neg, 2, F).clone()
            if repl is not None:
                out[:, :, 1, cols] = repl
        return out.reshape(-1, F)

    rows = spread(pos_idx, neg).to(torch.int32).contiguous()
    if pos_xv is None and neg_xv is None:
        return rows, None
    xv = torch.ones((B, F), dtype=torch.float32, device=dev) if pos_xv is None else torch.as_tensor(pos_xv, dtype=torch.float32).to(dev)
    if xv.shape != (B, F):
        raise ValueError(f"pos_xv of shape {tuple(xv.shape)}: expected {(B, F)}")
    if neg_xv is not None:
        neg_xv = _negatives_3d(neg_xv, B, len(fields), "neg_xv").to(device=dev, dtype=torch.float32).expand(B, n_neg, len(fields))
    return rows, spread(xv, neg_xv).contiguous()


def sample_negatives(pos_idx, item_fields, sizes_or_candidates, n_neg=1, generator=None):
    """Uniform negative items for every positive row -> [B, n_neg, m] int64 on pos_idx's device (m = len(item_fields)).

    sizes_or_candidates: a sequence of m ints -- the vocabulary sizes of the item fields, each field drawn independently -- or a
    tensor of candidate items [N, m] ([N] with one item field), one drawn per negative.  A draw equal to the row's own positive
    item (in every item column) is redrawn, so a row never gets its own positive as a negative.  Draws are made on the
    generator's device (by default pos_idx's) and are deterministic under a seeded generator."""
    fields = _item_fields(item_fields)
    m = len(fields)
    pos_idx = torch.as_tensor(pos_idx)
    dev = pos_idx.device
    gdev = generator.device if generator is not None else dev
    B, n_neg = pos_idx.shape[0], int(n_neg)
    if n_neg < 1:
        raise ValueError("n_neg must be >= 1")
    own = pos_idx[:, fields].to(device=gdev, dtype=torch.int64).reshape(B, 1, m).expand(B, n_neg, m)
    cand = None
    if torch.is_tensor(sizes_or_candidates):
        cand = sizes_or_candidates.to(device=gdev, dtype=torch.int64).reshape(-1, m)
        n_distinct = torch.unique(cand, dim=0).shape[0]
    else:
        sizes = [int(s) for s in sizes_or_candidates]
        if len(sizes) != m or min(sizes) < 1:
            raise ValueError(f"sizes {sizes}: one positive size per item field {fields}")
        n_distinct = 1
        for s in sizes:
            n_distinct *= s
    if n_distinct < 2:
        raise ValueError("sample_negatives: fewer than two distinct items to draw from")

    def draw(n):
        if cand is not None:
            return cand[torch.randint(cand.shape[0], (n,), generator=generator, device=gdev)]
        return torch.stack([torch.randint(s, (n,), generator=generator, device=gdev) for s in sizes], dim=1)

    out = draw(B * n_neg).reshape(B, n_neg, m)
    while True:
        again = (out == own).all(dim=2)
        n = int(again.sum())
        if n == 0:
            break
        out[again] = draw(n)
    return out.to(dev)


# ---------------------------------------------------------------------------------------------------------------------------
# hard negatives: the best of n_draw drawn candidates under the current FM (include/fmx.h, fmx_fm_mine_negatives)
# ---------------------------------------------------------------------------------------------------------------------------
MINE_MAX_DRAW, MINE_MAX_NEG = 1024, 16      # the kernel's limits


class HardNegatives:
    """negatives=HardNegatives(...) of fit_pairs / run_pair_experiment: mine every positive's negatives under the current FM
    score instead of drawing them uniformly.  n_draw: candidates drawn per positive (<= 1024); exclude: per-row candidate
    positions never to return (see fmx.recommend.exclusions_csr); refresh_every: the candidates' sums are recomputed from the
    table every that many mining calls (1: always the current model's); remine_every (run_pair_experiment only): the stream
    is mined in blocks of that many positives, the candidates refreshed before each (None: once, up front).
    negatives="hard" stands for HardNegatives()."""

    def __init__(self, n_draw=32, exclude=None, refresh_every=1, remine_every=None):
        self.n_draw, self.exclude = int(n_draw), exclude
        self.refresh_every = int(refresh_every)
        self.remine_every = None if remine_every is None else int(remine_every)
        if self.n_draw < 1 or self.refresh_every < 1 or (self.remine_every is not None and self.remine_every < 1):
            raise ValueError("HardNegatives: n_draw, refresh_every and remine_every must be >= 1")


def hard_negatives(negatives):
    """The HardNegatives behind a `negatives` argument ("hard": the defaults), or None for every other value."""
    if isinstance(negatives, HardNegatives):
        return negatives
    if isinstance(negatives, str):
        if negatives != "hard":
            raise ValueError(f"negatives={negatives!r}: None (uniform), 'hard', a HardNegatives, or the negatives' item columns")
        return HardNegatives()
    return None


# ---------------------------------------------------------------------------------------------------------------------------
# popularity-sampled negatives: draws in proportion to weights from an alias table, with log Q of every draw
# (include/fmx.h, fmx_alias_sample_negatives; the corrected list loss that takes log Q: fmx_fm_list_*_q)
# ---------------------------------------------------------------------------------------------------------------------------
ALIAS_ONE = 1 << 24      # a cell's threshold is an integer in [0, 2^24]: the kernel compares the top 24 bits of a Philox word with it


def alias_table(weights):
    """Walker's alias table of non-negative weights [N] by Vose's construction in float64 -> (thresh uint32 [N] in [0, 2^24],
    alias int32 [N], q float64 [N], logq float32 [N]).  A draw picks a cell p uniformly, then p with probability
    thresh[p] / 2^24 and alias[p] otherwise, so position i is drawn with the REALISED probability
        q_i = (thresh_i + sum_{j: alias_j = i} (2^24 - thresh_j)) / (N 2^24),
    which differs from weights_i / sum(weights) by the 24-bit rounding of the thresholds; logq = log(q) of that q, not of the
    weights (-inf where q = 0).  A zero-weight position has thresh = 0 and no alias entry pointing at it: it is never drawn.
    Weights that are negative, non-finite or all zero raise ValueError."""
    import numpy as np
    w = np.asarray(torch.as_tensor(weights).detach().cpu() if torch.is_tensor(weights) else weights, dtype=np.float64).reshape(-1)
    N = w.size
    if N < 1 or not np.isfinite(w).all() or (w < 0).any() or not w.sum() > 0:
        raise ValueError("alias_table: weights must be finite, non-negative and not all zero")
    p = w * (N / w.sum())                                 # mean 1: a cell's own share of itself
    thresh = np.full(N, ALIAS_ONE, dtype=np.int64)
    alias = np.arange(N, dtype=np.int64)
    small = [i for i in range(N) if p[i] < 1.0]
    large = [i for i in range(N) if p[i] >= 1.0]
    while small and large:
        s, g = small.pop(), large[-1]
        thresh[s], alias[s] = int(round(p[s] * ALIAS_ONE)), g
        p[g] -= 1.0 - p[s]                                # the rest of cell s is g's
        if p[g] < 1.0:
            small.append(large.pop())
    for s in small:                                       # (rounding leftovers: cells of share 1 up to float64 rounding)
        if w[s] == 0:
            raise ValueError("alias_table: the weights' float64 rounding left a zero-weight cell unpaired")
    num = thresh.copy()
    np.add.at(num, alias, ALIAS_ONE - thresh)
    q = num / float(N * ALIAS_ONE)
    with np.errstate(divide="ignore"):
        logq = np.log(q).astype(np.float32)
    return thresh.astype(np.uint32), alias.astype(np.int32), q, logq


class PopularityNegatives:
    """negatives=PopularityNegatives(weights, ...) of fit_lists / run_list_experiment / fit_pairs / run_pair_experiment: every
    positive's n_neg negatives are drawn with replacement in proportion to weights ** power (fmx_alias_sample_negatives), never
    the row's own item nor an excluded position.  weights holds one entry per candidate position: the whole item field (one item
    field, candidates=None) or the rows of `candidates`.  correct=True: the list loss subtracts log Q(item) from every logit of
    the list, the positive's included (fmx_fm_list_step_q) -- without it popular items are pushed down merely for being drawn
    often; the pair loss has no correction and ignores `correct`.  exclude: per-row candidate positions never to return
    (fmx.recommend.exclusions_csr).  n_try: draws per row, default max(64, 8 n_neg); a row with fewer than n_neg eligible draws
    among them raises ValueError.  The table is built once (alias_table) and stays on the device across calls."""

    def __init__(self, weights, power=1.0, correct=True, exclude=None, n_try=None):
        w = torch.as_tensor(weights).detach().to("cpu", torch.float64).reshape(-1)
        self.power, self.correct, self.exclude = float(power), bool(correct), exclude
        self.n_try = None if n_try is None else int(n_try)
        if self.n_try is not None and self.n_try < 1:
            raise ValueError("PopularityNegatives: n_try must be >= 1")
        self.thresh, self.alias, self.q, self.logq = alias_table(w.numpy() ** self.power)
        self.N = int(w.numel())
        self._on = {}

    @classmethod
    def from_counts(cls, column, size, power=0.75, **kw):
        """The weights as the counts of an item column (torch.bincount over `size` items), under the word2vec power 0.75"""
        counts = torch.bincount(torch.as_tensor(column).reshape(-1).long().cpu(), minlength=int(size))
        if counts.numel() != int(size):
            raise ValueError(f"PopularityNegatives.from_counts: an item index beyond size = {int(size)}")
        return cls(counts, power=power, **kw)

    def tries(self, n_neg):
        return max(64, 8 * int(n_neg)) if self.n_try is None else self.n_try

    def table(self, device):
        """(thresh [N] -- the uint32 bits in an int32 tensor --, alias int32 [N], logq fp32 [N]) on `device`, copied once"""
        key = str(device)
        if key not in self._on:
            self._on[key] = tuple(torch.from_numpy(a).to(device) for a in (self.thresh.view("int32"), self.alias, self.logq))
        return self._on[key]

    def floor_logq(self):
        """log Q of a positive whose item the table never draws (q = 0, or no candidate position): log(2^-24 / N), below every
        drawable position's"""
        import math
        return math.log(1.0 / (ALIAS_ONE * self.N))

    def __getstate__(self):
        return {k: v for k, v in self.__dict__.items() if k != "_on"}

    def __setstate__(self, st):
        self.__dict__.update(st)
        self._on = {}


def popularity_negatives(negatives):
    """The PopularityNegatives behind a `negatives` argument, or None for every other value"""
    return negatives if isinstance(negatives, PopularityNegatives) else None


def alias_sample(thresh, alias, logq, n_neg, n_try, own_pos=None, seed=0, offset=0, u_base=0, excl_offsets=None, excl_pos=None,
                 U=None, stream=None, call=None):
    """The raw call of fmx_alias_sample_negatives: thresh (the uint32 bits in an int32 tensor) [N], alias int32 [N], logq fp32 [N]
    or None, own_pos int32 [U] or None, all on one device.  U: own_pos's length unless given.  call(fn, args): who makes the
    checked foreign call (FMEngine._counted; by default this function).  Returns (neg_pos int32 [U, n_neg], -1 padded; neg_logq
    fp32 [U, n_neg], -inf padded, or None without logq) on the device; no sync."""
    dev = thresh.device
    U = int(own_pos.numel() if U is None else U)
    n_neg = int(n_neg)
    if own_pos is not None and (own_pos.dtype != torch.int32 or own_pos.numel() != U or not own_pos.is_contiguous()):
        raise ValueError(f"own_pos: a contiguous int32 [U = {U}] device tensor")
    shape = (max(U, 0), max(n_neg, 0))
    neg_pos = torch.empty(shape, dtype=torch.int32, device=dev)
    neg_logq = None if logq is None else torch.empty(shape, dtype=torch.float32, device=dev)
    st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream

    def ptr(t):
        return None if t is None else t.data_ptr()

    args = (thresh.data_ptr(), alias.data_ptr(), ptr(logq), thresh.numel(), ptr(excl_offsets), ptr(excl_pos), ptr(own_pos), U, n_neg,
            int(n_try), int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), int(u_base) & 0xFFFFFFFF, neg_pos.data_ptr(),
            ptr(neg_logq), st)
    fn = _lib.load().fmx_alias_sample_negatives
    if call is None:
        _lib.check(fn(*args))
    else:
        call(fn, args)
    return neg_pos, neg_logq


def candidate_positions(items, candidates):
    """The position of each row of items [B, m] among the rows of candidates [N, m] (the lowest where a row is listed twice), -1
    where it is none -> int64 [B] on items' device.  (fmx.recommend.Candidates.positions_of answers the same question for a
    Candidates, whose construction scores every candidate row; the sampler scores nothing and has the items only.)"""
    N = candidates.shape[0]
    uniq, inv = torch.unique(torch.cat([candidates, items]), dim=0, return_inverse=True)
    first = torch.full((uniq.shape[0],), N, dtype=torch.int64, device=items.device)
    first.scatter_reduce_(0, inv[:N], torch.arange(N, dtype=torch.int64, device=items.device), reduce="amin")
    pos = first[inv[N:]]
    return torch.where(pos == N, torch.full_like(pos, -1), pos)


def fm_mine_negatives(Su, au, Sc, ac, n_draw, n_neg=1, own_pos=None, seed=0, offset=0, u_base=0, excl_offsets=None, excl_pos=None,
                      out=None, stream=None, kp=None):
    """The raw call of fmx_fm_mine_negatives: Su [U, >= kp], au [U], Sc [N, >= kp], ac [N] as fmx.recommend.fm_topk takes them;
    own_pos int32 [U] on the device or None.  Returns (neg_pos int32 [U, n_neg], neg_score fp32 [U, n_neg]) on the device."""
    U, N = Su.shape[0], Sc.shape[0]
    kp = Sc.shape[1] if kp is None else int(kp)
    n_neg = int(n_neg)
    if own_pos is not None and (own_pos.dtype != torch.int32 or own_pos.numel() != U or not own_pos.is_contiguous()):
        raise ValueError(f"own_pos: a contiguous int32 [U = {U}] device tensor")
    if out is None:
        shape = (U, max(n_neg, 0))
        out = (torch.empty(shape, dtype=torch.int32, device=Su.device), torch.empty(shape, dtype=torch.float32, device=Su.device))
    st = stream if stream is not None else torch.cuda.current_stream(Su.device).cuda_stream

    def ptr(t):
        return None if t is None else t.data_ptr()

    _lib.check(_lib.load().fmx_fm_mine_negatives(Su.data_ptr(), Su.stride(0), au.data_ptr(), U, Sc.data_ptr(), Sc.stride(0),
                                                 ac.data_ptr(), N, kp, ptr(excl_offsets), ptr(excl_pos), ptr(own_pos), int(n_draw),
                                                 n_neg, int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1),
                                                 int(u_base) & 0xFFFFFFFF, out[0].data_ptr(), out[1].data_ptr(), st))
    return out


def mine_negatives(table, cand, ctx_idx, ctx_xv, own_pos, n_draw, n_neg=1, seed=0, offset=0, u_base=0, exclude=None, hyper=None):
    """Hard negatives for every context row of ctx_idx / ctx_xv ([B, F] full width, the item columns ignored): n_draw positions
    of `cand` (a fmx.recommend.Candidates) drawn per row -- Philox4x32-10 under (seed, offset, u_base + row), see include/fmx.h
    -- scored as logit(u + c) = a_u + a_c + <S_u, S_c>, and the n_neg best kept that are neither the row's own_pos (int [B] or
    None; -1: none) nor excluded (exclude: see fmx.recommend.exclusions_csr).  One forward launch for the context side
    (side_sums over the non-item fields) and one mining launch.  Returns device tensors (neg_pos int32 [B, n_neg], -1 padded;
    neg_score fp32 [B, n_neg], -inf padded), each row by score descending, then position ascending."""
    from . import recommend
    (Su, au), off, pos = recommend._context_side(recommend.FMScorer(), table, cand, ctx_idx, ctx_xv, exclude, hyper)
    if own_pos is not None:
        own_pos = torch.as_tensor(own_pos).to(device=table.device, dtype=torch.int32).reshape(-1).contiguous()
    return fm_mine_negatives(Su, au, cand.Sc, cand.ac, n_draw, n_neg, own_pos, seed, offset, u_base, off, pos)
