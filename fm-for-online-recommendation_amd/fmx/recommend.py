"""Top-K recommendation over an FM table's candidates (include/fmx.h, fmx_fm_topk).

Split a sample's fields into context fields (user, time, ...) and item fields.  For a context u and a candidate c the logit of
the combined sample is

    logit(u + c) = a_u + a_c + <S_u, S_c>

a_u: the logit of u's context fields alone (bias included); a_c: sfirst + sbi of c's item fields alone; S_u, S_c: their sums of
V x.  Both sides are fmx_fm_forward over full-width rows in which the other side's fields carry index 0 and value 0 (a zero
value adds exact zeros to S, to sum e^2 and to the first-order sum).  What remains -- U x N kp-wide dot products and an exact
per-user top-K -- is one fmx_fm_topk call.

The DeepFM / NFM classes put a relu MLP on the bi-interaction vector.  The network does not split, its input does:
bi(u + c) = bi_u + bi_c + S_u * S_c, so each side is still computed once (side_terms) and fmx_mlp_topk runs the U x N
forwards of the network on the device, then the same exact selection (topk_network).  Networks the kernel does not take
(hidden > 256) go through mlp_topk_torch, a chunked torch statement of the same score and result order.

The attentional FM (AFMAdam) does not decompose over a masked forward: a zeroed field still adds pairs to the softmax.  Each
side instead keeps its own fields' embeddings and the softmax statistics (lin, m, Z, R) of its own pairs (afm_side,
fmx_afm_side); fmx_afm_topk computes the cross pairs of every (u, c) and combines the three groups exactly (topk_afm).

Ranking evaluation (rank, rank_network, rank_afm; fmx_fm_rank, fmx_mlp_rank, fmx_afm_rank): for held-out target positions,
the number of eligible candidates the top-K order puts in front of each -- the index the target would have in an unbounded
top-K row -- from which ranking_metrics takes hit rate, NDCG, MRR and AUC.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .engine import Hyper, _ptr, mlp_struct

CHUNK = 65536   # rows per forward launch of the side computations


def _hyper_for(table, hyper):
    return hyper if hyper is not None else Hyper(**table.ftrl)


def _as_index(a, F, device):
    """[R, F] int32 on the device; indices beyond int32 raise IndexError before the cast."""
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.int64)))
    if t.dtype in (torch.int64,) and bool(((t >= 2 ** 31) | (t < -2 ** 31)).any()):
        raise IndexError("index out of range in self")
    t = t.to(device=device, dtype=torch.int32).reshape(-1, F)
    return t.contiguous()


def _as_values(a, shape, device):
    if a is None:
        return torch.ones(shape, dtype=torch.float32, device=device)
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32)))
    t = t.to(device=device, dtype=torch.float32).reshape(shape)
    return t.contiguous()


def _masked_side(table, idx, xv, keep_fields):
    """(idx int32 [R, F], xv fp32 [R, F]) on the device with every field outside keep_fields given index 0 and value 0."""
    F, dev = table.n_fields, table.device
    idx = _as_index(idx, F, dev)
    R = idx.shape[0]
    xv = _as_values(xv, (R, F), dev)
    keep = torch.zeros(F, dtype=torch.bool, device=dev)
    keep[list(keep_fields)] = True
    idx = torch.where(keep[None, :], idx, torch.zeros_like(idx)).contiguous()
    xv = torch.where(keep[None, :], xv, torch.zeros_like(xv)).contiguous()
    return idx, xv


def _side_pass(table, idx, xv, keep_fields, hyper, outputs, after_chunk=None):
    """fmx_fm_forward over the rows of idx / xv ([R, F], full width) with every field outside keep_fields given index 0 and
    value 0, CHUNK rows per launch, writing only the FwdOut outputs named in `outputs` (S, bi [R, kp]; sfirst, sbi, logit
    [R]).  Returns those device tensors in that order; after_chunk(out, r0, B), given the dict of them, runs after the launch
    of rows r0 .. r0 + B - 1.  An index outside its field (in a kept column) raises IndexError."""
    dev, kp = table.device, table.kp
    idx, xv = _masked_side(table, idx, xv, keep_fields)
    R = idx.shape[0]
    lib, h = _lib.load(), _hyper_for(table, hyper)
    out = {n: torch.empty((R, kp) if n in ("S", "bi") else R, dtype=torch.float32, device=dev) for n in outputs}
    error = torch.zeros(1, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for r0 in range(0, R, CHUNK):
        B = min(CHUNK, R - r0)
        o = _lib.FwdOut(error=error.data_ptr(), **{n: t[r0:].data_ptr() for n, t in out.items()})
        _lib.check(lib.fmx_fm_forward(table.c_struct(), h.ref(), idx[r0:].data_ptr(), xv[r0:].data_ptr(), None, B,
                                      _lib.LOSS_NONE, 1.0, C.byref(o), stream))
        if after_chunk is not None:
            after_chunk(out, r0, B)
    if int(error.item()) != 0:
        raise IndexError("index out of range in self (flagged by the fmx kernels)")
    return tuple(out[n] for n in outputs)


def _add_first_terms(out, r0, B):
    """sfirst += sbi over rows r0 .. r0 + B - 1: side_sums' a without the bias."""
    rows = slice(r0, r0 + B)
    torch.add(out["sfirst"][rows], out["sbi"][rows], out=out["sfirst"][rows])


def side_sums(table, idx, xv, keep_fields, hyper=None, want_bias=True):
    """fmx_fm_forward over the rows of idx / xv ([R, F], full width) with every field outside keep_fields given index 0 and
    value 0.  Returns (S [R, kp], a [R]) on the device: a = the logit (bias included) when want_bias, else sfirst + sbi.
    An index outside its field (in a kept column) raises IndexError."""
    if want_bias:
        return _side_pass(table, idx, xv, keep_fields, hyper, ("S", "logit"))
    S, a, _ = _side_pass(table, idx, xv, keep_fields, hyper, ("S", "sfirst", "sbi"), _add_first_terms)
    return S, a


def side_terms(table, idx, xv, keep_fields, hyper=None):
    """As side_sums, but everything the network classes need from the one fmx_fm_forward call per chunk: returns device
    tensors (S [R, kp], bi [R, kp], sfirst [R], sbi [R], logit [R]) of the masked rows (logit = sfirst + sbi + bias)."""
    return _side_pass(table, idx, xv, keep_fields, hyper, ("S", "bi", "sfirst", "sbi", "logit"))


def network_bases(table, sfirst, sbi, logit, fm_term, context):
    """The score's base terms of one side (include/fmx.h, fmx_mlp_topk): DeepFM (fm_term = 1) a_u = logit, a_c = sfirst + sbi;
    NFM (fm_term = 0) f_u = sfirst + bias, f_c = sfirst."""
    if fm_term:
        return logit if context else sfirst + sbi
    return sfirst + table.bias_weight().reshape(-1)[0] if context else sfirst


class Candidates:
    """The candidate side of a recommendation: Sc [N, kp] and ac [N] of cand_idx's item fields ([N, F] full-width rows, the
    other columns ignored), computed on the device.  Call refresh() after the table has been trained."""

    def __init__(self, table, item_fields, cand_idx, cand_xv=None, hyper=None):
        self.table = table
        self.item_fields = sorted({int(f) for f in item_fields})
        if not self.item_fields or not all(0 <= f < table.n_fields for f in self.item_fields):
            raise ValueError(f"item_fields {list(item_fields)}: need at least one field of 0..{table.n_fields - 1}")
        self.idx = _as_index(cand_idx, table.n_fields, table.device)
        self.xv = None if cand_xv is None else _as_values(cand_xv, tuple(self.idx.shape), table.device)
        self.hyper = hyper
        self.refresh()

    @property
    def N(self):
        return self.idx.shape[0]

    def refresh(self):
        self.Sc, self.ac = side_sums(self.table, self.idx, self.xv, self.item_fields, self.hyper, want_bias=False)
        return self

    @classmethod
    def whole_field(cls, table, field, hyper=None):
        """Every row of one item field as the candidates: a position is the field's local index."""
        n = table.feature_sizes[int(field)]
        idx = torch.zeros((n, table.n_fields), dtype=torch.int32, device=table.device)
        idx[:, int(field)] = torch.arange(n, dtype=torch.int32, device=table.device)
        self = cls(table, [int(field)], idx, None, hyper=hyper)
        self._identity = True
        return self

    def positions_of(self, items, item_fields=None):
        """The candidate position of each item of items [B, m] ([B] with one item field), or -1 where the item is not a
        candidate -> int32 [B] on the device.  Columns in the order of item_fields (default: the candidates' ascending item
        fields).  An item listed at several positions gives the lowest.  The inverse index is built once per candidate set, in
        torch: one item field, a lookup table over the field's vocabulary; several, the rows' mixed-radix int64 keys sorted for
        searchsorted.  The candidates of whole_field need none: the position is the index."""
        dev = self.table.device
        fields = self.item_fields if item_fields is None else [int(f) for f in item_fields]
        if sorted(fields) != self.item_fields:
            raise ValueError(f"item_fields {fields}: these candidates hold the fields {self.item_fields}")
        m = len(fields)
        it = torch.as_tensor(items).to(device=dev, dtype=torch.int64).reshape(-1, m)
        it = it[:, [fields.index(f) for f in self.item_fields]]              # columns in ascending field order
        sizes = [self.table.feature_sizes[f] for f in self.item_fields]
        inside = torch.ones(it.shape[0], dtype=torch.bool, device=dev)
        for j, n in enumerate(sizes):
            inside &= (it[:, j] >= 0) & (it[:, j] < n)
        none = torch.full((it.shape[0],), -1, dtype=torch.int64, device=dev)
        if getattr(self, "_identity", False):
            return torch.where(inside, it[:, 0], none).to(torch.int32)
        inv = getattr(self, "_inverse", None)
        if inv is None:
            rows = self.idx[:, self.item_fields].to(torch.int64)
            where = torch.arange(self.N, dtype=torch.int64, device=dev)
            if m == 1:
                lut = torch.full((sizes[0],), self.N, dtype=torch.int64, device=dev)
                ok = (rows[:, 0] >= 0) & (rows[:, 0] < sizes[0])
                lut.scatter_reduce_(0, rows[ok, 0], where[ok], reduce="amin")
                inv = (torch.where(lut == self.N, torch.full_like(lut, -1), lut),)
            else:
                keys, order = torch.sort(self._radix_key(rows, sizes), stable=True)
                inv = (keys, where[order])
            self._inverse = inv
        it = torch.where(inside[:, None], it, torch.zeros_like(it))
        if m == 1:
            found = inv[0][it[:, 0]]
        else:
            keys, where = inv
            key = self._radix_key(it, sizes)
            at = torch.searchsorted(keys, key).clamp(max=self.N - 1)
            found = torch.where(keys[at] == key, where[at], none)
        return torch.where(inside, found, none).to(torch.int32)

    @staticmethod
    def _radix_key(rows, sizes):
        key = rows[:, 0].clone()
        for j in range(1, len(sizes)):
            key = key * sizes[j] + rows[:, j]
        return key


class NetworkCandidates(Candidates):
    """The candidate side for the DeepFM / NFM classes: Sc [N, kp], Bc [N, kp] (bi) and ac [N] (fm_term = 1: sfirst + sbi,
    0: sfirst) of cand_idx's item fields.  Call refresh() after the table has been trained."""

    def __init__(self, table, item_fields, cand_idx, cand_xv=None, fm_term=1, hyper=None):
        if fm_term not in (0, 1):
            raise ValueError(f"fm_term={fm_term}: 1 (DeepFM) or 0 (NFM)")
        self.fm_term = int(fm_term)
        super().__init__(table, item_fields, cand_idx, cand_xv, hyper)

    def refresh(self):
        S, bi, sfirst, sbi, logit = side_terms(self.table, self.idx, self.xv, self.item_fields, self.hyper)
        self.Sc, self.Bc = S, bi
        self.ac = network_bases(self.table, sfirst, sbi, logit, self.fm_term, context=False).contiguous()
        return self


def exclusions_csr(exclude, U, device):
    """exclude: None, a list of U per-user position arrays, or a tuple (offsets [U + 1], positions) in CSR form; any order,
    duplicates and positions outside the candidates allowed.  Returns device
    (offsets int32 [U + 1], positions int32) with every user's positions sorted and unique, or (None, None)."""
    if exclude is None:
        return None, None
    if isinstance(exclude, tuple):
        if len(exclude) != 2 or len(exclude[0]) != U + 1:
            raise ValueError(f"exclude as a CSR pair: (offsets [{U + 1}], positions)")
        off = np.asarray(torch.as_tensor(exclude[0]).cpu(), dtype=np.int64)
        pos = np.asarray(torch.as_tensor(exclude[1]).cpu(), dtype=np.int64)
        lists = [pos[off[u]:off[u + 1]] for u in range(U)]
    else:
        lists = [np.asarray(torch.as_tensor(e).cpu() if torch.is_tensor(e) else e, dtype=np.int64).reshape(-1) for e in exclude]
        if len(lists) != U:
            raise ValueError(f"exclude has {len(lists)} lists for {U} users")
    lists = [np.unique(p[(p >= 0) & (p < 2 ** 31 - 1)]) for p in lists]
    off = np.zeros(U + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(p) for p in lists])
    pos = np.concatenate(lists + [np.zeros(1, dtype=np.int64)]).astype(np.int32)   # never empty: a valid pointer
    return torch.from_numpy(off).to(device), torch.from_numpy(pos).to(device)


def _call_buffers(need, U, K, dev, workspace, out, stream):
    """What the raw calls share: `need` workspace bytes (a *_workspace_bytes result; a negative one raises), a workspace
    allocated when the given one is missing or short, the outputs when not given, the stream.  Returns (workspace pointer,
    workspace bytes, out, stream)."""
    need = int(need)
    _lib.check(min(need, 0))
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    if out is None:
        out = (torch.empty((U, K), dtype=torch.int32, device=dev), torch.empty((U, K), dtype=torch.float32, device=dev))
    st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
    return workspace.data_ptr(), workspace.numel() * workspace.element_size(), out, st


MLP_TOPK_MAX_HIDDEN = 256    # fmx_mlp_topk's limits (include/fmx.h); larger networks take mlp_topk_torch
MLP_TOPK_MAX_LAYERS = 8
MLP_TOPK_MAX_K = 256         # for every network


def _mlp_struct(mlp):
    params, k, hidden, n_layers = mlp
    if params.dtype != torch.float32 or not params.is_contiguous():
        raise ValueError("mlp params: a contiguous fp32 device tensor (W_l [hidden, in_l] then b_l per layer)")
    return mlp_struct(params, k, hidden, n_layers)


def mlp_kernel_takes(mlp):
    """Does fmx_mlp_topk take this network?  (Else the chunked torch path; K > 256 is refused either way.)"""
    _, k, H, L = mlp
    return 1 <= H <= MLP_TOPK_MAX_HIDDEN and 1 <= L <= MLP_TOPK_MAX_LAYERS and 1 <= k <= 64


# ---------------------------------------------------------------------------------------------------------------------------
# the attentional FM
# ---------------------------------------------------------------------------------------------------------------------------
def _afm_struct(table, afm):
    params, t = afm
    if not torch.is_tensor(params) or params.dtype != torch.float32 or not params.is_contiguous() or not params.is_cuda:
        raise ValueError("afm params: a contiguous fp32 device tensor [W (t x k) | b (t) | h (t) | p (k)]")
    t, k = int(t), table.k
    if params.numel() != t * k + 2 * t + k:
        raise ValueError(f"afm params: {params.numel()} floats, t={t} and k={k} need {t * k + 2 * t + k}")
    return _lib.Afm(params.data_ptr(), k, t)


def afm_side(table, afm, idx, xv, fields, with_bias, hyper=None):
    """fmx_afm_side over the rows of idx / xv ([R, F] full width; xv None: ones) for the ascending fields `fields`.  afm =
    (params, t) with params the flat fp32 device buffer.  Returns device tensors (E [R, n_sel, kp], stats [R, 4] = (lin, m,
    Z, R)).  An index outside its field (in a selected column) raises IndexError."""
    F, dev, kp = table.n_fields, table.device, table.kp
    fields = sorted({int(f) for f in fields})
    if not fields or not all(0 <= f < F for f in fields):
        raise ValueError(f"fields {fields}: need at least one field of 0..{F - 1}")
    a = _afm_struct(table, afm)
    idx = _as_index(idx, F, dev)
    R = idx.shape[0]
    xv = None if xv is None else _as_values(xv, (R, F), dev)
    E = torch.empty((max(R, 1), len(fields), kp), dtype=torch.float32, device=dev)
    stats = torch.empty((max(R, 1), 4), dtype=torch.float32, device=dev)
    if R == 0:
        return E[:0], stats[:0]
    error = torch.zeros(1, dtype=torch.int32, device=dev)
    sel = (C.c_int32 * len(fields))(*fields)
    lib, h = _lib.load(), _hyper_for(table, hyper)
    _lib.check(lib.fmx_afm_side(table.c_struct(), C.byref(a), h.ref(), idx.data_ptr(), _ptr(xv), R, sel, len(fields),
                                int(bool(with_bias)), E.data_ptr(), stats.data_ptr(), error.data_ptr(),
                                torch.cuda.current_stream(dev).cuda_stream))
    if int(error.item()) != 0:
        raise IndexError("index out of range in self (flagged by the fmx kernels)")
    return E, stats


class AFMCandidates(Candidates):
    """The candidate side under the AFM: Ec [N, n_item, kp] and stats_c [N, 4] of cand_idx's item fields ([N, F] full-width
    rows, the other columns ignored) under the attention parameters afm = (params, t).  The statistics depend on the attention
    parameters as well as on the table: call refresh() after either has been trained."""

    def __init__(self, table, afm, item_fields, cand_idx, cand_xv=None, hyper=None):
        self.afm = (afm[0], int(afm[1]))
        fields = sorted({int(f) for f in item_fields})
        if len(fields) >= table.n_fields:
            raise ValueError(f"item_fields {list(item_fields)} cover every field: the AFM needs at least one context field")
        super().__init__(table, item_fields, cand_idx, cand_xv, hyper)

    @property
    def t(self):
        return self.afm[1]

    def refresh(self):
        self.Ec, self.stats = afm_side(self.table, self.afm, self.idx, self.xv, self.item_fields, False, self.hyper)
        return self


# ---------------------------------------------------------------------------------------------------------------------------
# ranking evaluation: the rank of held-out targets among all candidates
# ---------------------------------------------------------------------------------------------------------------------------
RANK_MAX_T = 16    # targets per user in one fmx_*_rank call (include/fmx.h); rank / rank_network / rank_afm chunk over more


def targets_matrix(targets, U, device):
    """targets: a [U] or [U, T] array or tensor of candidate positions, or a list of U lists (ragged rows are padded with
    -1, which no call ranks).  Returns (the int32 [U, T] device matrix, T >= 1; its column chunks of at most RANK_MAX_T
    columns, contiguous).  Anything that does not have U rows raises ValueError."""
    if torch.is_tensor(targets):
        t = targets.detach().cpu().numpy()
    elif isinstance(targets, np.ndarray):
        t = targets
    else:
        rows = [np.asarray(r.cpu() if torch.is_tensor(r) else r, dtype=np.int64).reshape(-1) for r in targets]
        if len(rows) != U:
            raise ValueError(f"targets has {len(rows)} rows for {U} users")
        T = max([len(r) for r in rows] + [1])
        t = np.full((U, T), -1, dtype=np.int64)
        for u, r in enumerate(rows):
            t[u, :len(r)] = r
    t = np.asarray(t, dtype=np.int64)
    if t.ndim == 1:
        t = t[:, None]
    if t.ndim != 2 or t.shape[0] != U:
        raise ValueError(f"targets of shape {tuple(t.shape)} for {U} users: [U] or [U, T]")
    if t.shape[1] == 0:
        t = np.full((U, 1), -1, dtype=np.int64)
    t = np.where((t < 0) | (t >= 2 ** 31 - 1), -1, t).astype(np.int32)
    full = torch.from_numpy(np.ascontiguousarray(t)).to(device)
    return full, [full[:, c0:c0 + RANK_MAX_T].contiguous() for c0 in range(0, full.shape[1], RANK_MAX_T)]


def _rank_buffers(need, U, T, dev, workspace, out, stream):
    """The rank calls' buffers: the workspace and stream of _call_buffers, out = (rank int32 [U, T], score fp32 [U, T], n_cand
    int32 [U]) when not given."""
    if out is None:
        out = (torch.empty((U, T), dtype=torch.int32, device=dev), torch.empty((U, T), dtype=torch.float32, device=dev),
               torch.empty(U, dtype=torch.int32, device=dev))
    return _call_buffers(need, U, T, dev, workspace, out, stream)


def _targets_arg(targets, U):
    if targets.dtype != torch.int32 or targets.dim() != 2 or targets.shape[0] != U or not targets.is_contiguous():
        raise ValueError(f"targets: a contiguous int32 [U = {U}, T] device tensor")
    return targets.shape[1]


def _rank_key(score, pos):
    """The top-K order as one int64 per (score, position), greater = earlier: make_key of csrc/fmx_topk.hip (score descending,
    then position ascending, -0 taken as +0).  score fp32, pos integer, same shape."""
    b = (score.float() + 0.0).contiguous().view(torch.int32).long() & 0xFFFFFFFF
    o = torch.where(b >= 0x80000000, 0xFFFFFFFF - b, b + 0x80000000)           # the float bits made monotone
    return ((o - 0x80000000) << 32) + (0xFFFFFFFF - pos.long())                 # shifted into int64's signed range


def _rank_chunks(call, targets, U, device, filtered):
    """What rank, rank_network and rank_afm share after their sides: call(chunk int32 [U, <= 16], filtered) -> (rank, score,
    n_cand) over the column chunks of targets_matrix, concatenated.  `filtered` within a chunk is the call's; across chunks it
    is resolved here from the returned scores and the target positions with the same key order (_rank_key): a target's rank
    loses one for every distinct eligible target of another chunk that is ahead of it."""
    full, chunks = targets_matrix(targets, U, device)
    outs = [call(ch, filtered) for ch in chunks]
    ranks = torch.cat([o[0] for o in outs], dim=1).long()
    scores = torch.cat([o[1] for o in outs], dim=1)
    n_cand = outs[0][2].long()
    if filtered and len(chunks) > 1:
        T = full.shape[1]
        valid = ranks >= 0
        key = _rank_key(torch.where(valid, scores, torch.zeros_like(scores)), full.clamp(min=0))
        chunk_of = torch.arange(T, device=device) // RANK_MAX_T
        # first[u, t]: no earlier column lists the same position (a target listed twice was counted once as a candidate)
        eq = full[:, :, None] == full[:, None, :]
        first = ~(eq & torch.tril(torch.ones(T, T, dtype=torch.bool, device=device), -1)[None]).any(dim=2)
        same_chunk = chunk_of[None, :] == chunk_of[:, None]
        # mine[u, t, t2]: t's own chunk lists t2's position too, so the call has already left it out
        mine = torch.matmul(same_chunk.float()[None], eq.float()) > 0
        ahead = (key[:, None, :] > key[:, :, None]) & (valid & first)[:, None, :] & ~same_chunk[None] & ~mine
        ranks = torch.where(valid, ranks - ahead.sum(dim=2), ranks)
    return ranks, scores, n_cand


# ---------------------------------------------------------------------------------------------------------------------------
# the three families' scorers, and the two calls over any of them
# ---------------------------------------------------------------------------------------------------------------------------
def _raw_topk(scorer, user, cand, K, excl_offsets, excl_pos, workspace, out, stream, kp=None):
    """fmx_<family>_topk on the two sides' tensors -> (top_pos int32 [U, K], top_score fp32 [U, K]) on the device."""
    U, N, dev, ws_head, head = scorer.raw(user, cand, kp)
    lib = _lib.load()
    need = getattr(lib, f"fmx_{scorer.family}_topk_workspace_bytes")(*ws_head, U, N, K)
    ws, ws_n, out, st = _call_buffers(need, U, K, dev, workspace, out, stream)
    _lib.check(getattr(lib, f"fmx_{scorer.family}_topk")(*head, _ptr(excl_offsets), _ptr(excl_pos), K, ws, ws_n,
                                                        out[0].data_ptr(), out[1].data_ptr(), st))
    return out


def _raw_rank(scorer, user, cand, targets, filtered, excl_offsets, excl_pos, workspace, out, stream, kp=None):
    """fmx_<family>_rank: its top-K twin with targets int32 [U, T <= 16] (contiguous, on the device) and `filtered` in place of
    K.  Returns device tensors (rank int32 [U, T], -1: not eligible; score fp32 [U, T], -inf there; n_cand int32 [U])."""
    U, N, dev, ws_head, head = scorer.raw(user, cand, kp)
    T = _targets_arg(targets, U)
    lib = _lib.load()
    need = getattr(lib, f"fmx_{scorer.family}_rank_workspace_bytes")(*ws_head, U, N, T)
    ws, ws_n, out, st = _rank_buffers(need, U, T, dev, workspace, out, stream)
    _lib.check(getattr(lib, f"fmx_{scorer.family}_rank")(*head, _ptr(excl_offsets), _ptr(excl_pos), targets.data_ptr(), T,
                                                        int(bool(filtered)), ws, ws_n, out[0].data_ptr(), out[1].data_ptr(),
                                                        out[2].data_ptr(), st))
    return out


class FMScorer:
    """A family's score as the two calls need it: the check that candidates belong to it, its context side (`side`, whose first
    result has a row per context), the candidates' tensors (`cand_side`), and the foreign call's arguments (`raw`: U, N, the
    device, what its *_workspace_bytes functions take ahead of U, what its calls take up to and including kp).  This one: the
    FM, a Candidates."""
    family = "fm"

    def check(self, table, candidates):
        if candidates.table is not table:
            raise ValueError("candidates were computed for another table")

    def side(self, table, idx, xv, fields, hyper):
        return side_sums(table, idx, xv, fields, hyper)

    def cand_side(self, candidates):
        return candidates.Sc, candidates.ac

    def raw(self, user, cand, kp):
        (Su, au), (Sc, ac) = user, cand
        U, N = Su.shape[0], Sc.shape[0]
        kp = Sc.shape[1] if kp is None else int(kp)
        return U, N, Su.device, (), (Su.data_ptr(), Su.stride(0), au.data_ptr(), U, Sc.data_ptr(), Sc.stride(0), ac.data_ptr(), N, kp)

    def topk(self, user, cand, K, off, pos):
        return _raw_topk(self, user, cand, K, off, pos, None, None, None)

    def rank(self, user, cand, targets, filtered, off, pos):
        return _raw_rank(self, user, cand, targets, filtered, off, pos, None, None, None)


class NetworkScorer(FMScorer):
    """The DeepFM (fm_term = 1) / NFM (fm_term = 0) network mlp = (params, k, hidden, n_layers) on the pair's bi-interaction
    vector; a NetworkCandidates of the same fm_term.  Networks the kernels do not take go through the torch statements."""
    family = "mlp"

    def __init__(self, mlp, fm_term):
        self.mlp, self.fm_term = mlp, fm_term

    def check(self, table, candidates):
        super().check(table, candidates)
        if not isinstance(candidates, NetworkCandidates) or candidates.fm_term != int(self.fm_term):
            raise ValueError(f"candidates: a NetworkCandidates with fm_term={int(self.fm_term)}")

    def side(self, table, idx, xv, fields, hyper):
        S, bi, sfirst, sbi, logit = side_terms(table, idx, xv, fields, hyper)
        return S, bi, network_bases(table, sfirst, sbi, logit, self.fm_term, context=True).contiguous()

    def cand_side(self, candidates):
        return candidates.Sc, candidates.Bc, candidates.ac

    def raw(self, user, cand, kp):
        (Su, Bu, au), (Sc, Bc, ac) = user, cand
        U, N = Su.shape[0], Sc.shape[0]
        kp = Sc.shape[1] if kp is None else int(kp)
        if Bu.stride(0) != Su.stride(0) or Bc.stride(0) != Sc.stride(0):
            raise ValueError("Bu / Bc must share the row strides of Su / Sc")
        m = C.byref(_mlp_struct(self.mlp))
        return U, N, Su.device, (m,), (m, int(self.fm_term), Su.data_ptr(), Bu.data_ptr(), Su.stride(0), au.data_ptr(), U,
                                       Sc.data_ptr(), Bc.data_ptr(), Sc.stride(0), ac.data_ptr(), N, kp)

    def topk(self, user, cand, K, off, pos):
        if mlp_kernel_takes(self.mlp) or not 1 <= K <= MLP_TOPK_MAX_K:     # the kernel's checks raise on a bad K
            return super().topk(user, cand, K, off, pos)
        return mlp_topk_torch(self.mlp, self.fm_term, *user, *cand, K, off, pos)

    def rank(self, user, cand, targets, filtered, off, pos):
        if mlp_kernel_takes(self.mlp):
            return super().rank(user, cand, targets, filtered, off, pos)
        return mlp_rank_torch(self.mlp, self.fm_term, *user, *cand, targets, filtered, off, pos)


class AFMScorer(FMScorer):
    """The attentional FM afm = (params, t) over embeddings of size k; an AFMCandidates of the same attention parameters."""
    family = "afm"

    def __init__(self, afm, k):
        self.afm, self.k = (afm[0], int(afm[1])), int(k)

    def check(self, table, candidates):
        params, t = self.afm
        if not isinstance(candidates, AFMCandidates):
            raise ValueError("candidates: an AFMCandidates (the AFM's candidate side)")
        if candidates.table is table and (candidates.t != t or candidates.afm[0].data_ptr() != params.data_ptr()):
            raise ValueError(f"candidates were computed for another attention (t={candidates.t}; this one has t={t})")
        super().check(table, candidates)

    def side(self, table, idx, xv, fields, hyper):
        return afm_side(table, self.afm, idx, xv, fields, True, hyper)

    def cand_side(self, candidates):
        return candidates.Ec, candidates.stats

    def raw(self, user, cand, kp):
        (Eu, stats_u), (Ec, stats_c) = user, cand
        U, n_ctx, kp = Eu.shape
        N, n_item = Ec.shape[0], Ec.shape[1]
        if Ec.shape[2] != kp or not all(x.is_contiguous() for x in (Eu, stats_u, Ec, stats_c)):
            raise ValueError("Eu / Ec: contiguous [rows, fields, kp] with the same kp; stats contiguous [rows, 4]")
        a = C.byref(_lib.Afm(self.afm[0].data_ptr(), self.k, self.afm[1]))
        return U, N, Eu.device, (a, n_ctx, n_item), (a, Eu.data_ptr(), stats_u.data_ptr(), n_ctx, U, Ec.data_ptr(),
                                                     stats_c.data_ptr(), n_item, N, kp)


def _context_side(scorer, table, candidates, ctx_idx, ctx_xv, exclude, hyper):
    """What the two calls share before the foreign call: the candidates' check, the scorer's side over the fields that are not
    item fields, and the exclusions.  Returns (the side's tensors, exclusion offsets, exclusion positions)."""
    scorer.check(table, candidates)
    ctx_fields = [f for f in range(table.n_fields) if f not in candidates.item_fields]
    user = scorer.side(table, ctx_idx, ctx_xv, ctx_fields, hyper if hyper is not None else candidates.hyper)
    off, pos = exclusions_csr(exclude, user[0].shape[0], table.device)
    return user, off, pos


def scorer_topk(scorer, table, ctx_idx, ctx_xv, candidates, K, exclude=None, hyper=None):
    """Top-K candidates for every context row of ctx_idx / ctx_xv ([U, F] full width, the item columns ignored) under the
    scorer's family.  Returns device tensors (positions int64 [U, K], -1 padded; scores fp32 [U, K], -inf padded), each row by
    score descending, then position ascending.  exclude: see exclusions_csr."""
    user, off, pos = _context_side(scorer, table, candidates, ctx_idx, ctx_xv, exclude, hyper)
    top_pos, top_score = scorer.topk(user, scorer.cand_side(candidates), int(K), off, pos)
    return top_pos.long(), top_score


def scorer_rank(scorer, table, ctx_idx, ctx_xv, candidates, targets, exclude=None, hyper=None, filtered=False):
    """The rank of the target positions among all N candidates for every context row: the number of eligible candidates (not
    NaN, not excluded) that scorer_topk's order puts in front of the target, i.e. its 0-based index in an unbounded top-K row.
    targets: see targets_matrix (positions in the sense of the top-K results).  filtered: the user's other targets are not
    counted (leave-n-out evaluation).  Returns device tensors (ranks int64 [U, T], -1: no eligible target; scores fp32 [U, T],
    -inf there; n_cand int64 [U]).  More than 16 targets per user run as several calls; `filtered` across them is resolved on the
    host side of the call (see _rank_chunks) from the returned scores and positions with the same key order."""
    user, off, pos = _context_side(scorer, table, candidates, ctx_idx, ctx_xv, exclude, hyper)
    cand = scorer.cand_side(candidates)
    return _rank_chunks(lambda tg, f: scorer.rank(user, cand, tg, f, off, pos), targets, user[0].shape[0], table.device, filtered)


# ---- the public forms, per family.  The raw calls take device tensors: Su / Bu [U, >= kp] and Sc / Bc [N, >= kp] fp32 (row
# strides multiples of 4 and shared within a side, 16-byte aligned; kp defaults to Sc's width), au [U], ac [N]; mlp = (params, k,
# hidden, n_layers) and afm = (params, t) with params the flat fp32 device buffer, k the embedding size; Eu [U, n_ctx, kp],
# stats_u [U, 4], Ec [N, n_item, kp], stats_c [N, 4] contiguous (afm_side's outputs).  They return as _raw_topk / _raw_rank.
def fm_topk(Su, au, Sc, ac, K, excl_offsets=None, excl_pos=None, workspace=None, out=None, stream=None, kp=None):
    """The raw call of fmx_fm_topk -> (top_pos int32 [U, K], top_score fp32 [U, K]) on the device."""
    return _raw_topk(FMScorer(), (Su, au), (Sc, ac), K, excl_offsets, excl_pos, workspace, out, stream, kp)


def fm_rank(Su, au, Sc, ac, targets, filtered=False, excl_offsets=None, excl_pos=None, workspace=None, out=None, stream=None,
            kp=None):
    """The raw call of fmx_fm_rank: fm_topk's arguments with targets int32 [U, T <= 16] in place of K; returns as _raw_rank."""
    return _raw_rank(FMScorer(), (Su, au), (Sc, ac), targets, filtered, excl_offsets, excl_pos, workspace, out, stream, kp)


def mlp_topk(mlp, fm_term, Su, Bu, au, Sc, Bc, ac, K, excl_offsets=None, excl_pos=None, workspace=None, out=None, stream=None,
             kp=None):
    """The raw call of fmx_mlp_topk; returns as fm_topk."""
    return _raw_topk(NetworkScorer(mlp, fm_term), (Su, Bu, au), (Sc, Bc, ac), K, excl_offsets, excl_pos, workspace, out, stream, kp)


def mlp_rank(mlp, fm_term, Su, Bu, au, Sc, Bc, ac, targets, filtered=False, excl_offsets=None, excl_pos=None, workspace=None,
             out=None, stream=None, kp=None):
    """The raw call of fmx_mlp_rank: mlp_topk's arguments with targets int32 [U, T <= 16] in place of K; returns as fm_rank."""
    return _raw_rank(NetworkScorer(mlp, fm_term), (Su, Bu, au), (Sc, Bc, ac), targets, filtered, excl_offsets, excl_pos, workspace,
                     out, stream, kp)


def afm_topk(afm, k, Eu, stats_u, Ec, stats_c, K, excl_offsets=None, excl_pos=None, workspace=None, out=None, stream=None):
    """The raw call of fmx_afm_topk; returns as fm_topk."""
    return _raw_topk(AFMScorer(afm, k), (Eu, stats_u), (Ec, stats_c), K, excl_offsets, excl_pos, workspace, out, stream)


def afm_rank(afm, k, Eu, stats_u, Ec, stats_c, targets, filtered=False, excl_offsets=None, excl_pos=None, workspace=None,
             out=None, stream=None):
    """The raw call of fmx_afm_rank: afm_topk's arguments with targets int32 [U, T <= 16] in place of K; returns as fm_rank."""
    return _raw_rank(AFMScorer(afm, k), (Eu, stats_u), (Ec, stats_c), targets, filtered, excl_offsets, excl_pos, workspace, out, stream)


# The calls on a table: the FM's logit of the combined sample; topk_network / rank_network the DeepFM / NFM score (the logit of
# the combined sample for the Adam classes, the logit whose sigmoid forward() returns for the ONN classes); topk_afm / rank_afm
# the AFM's exact logit.  They return as scorer_topk / scorer_rank.
def topk(table, ctx_idx, ctx_xv, candidates, K, exclude=None, hyper=None):
    """scorer_topk under the FM's logit; candidates: a Candidates of the same table."""
    return scorer_topk(FMScorer(), table, ctx_idx, ctx_xv, candidates, K, exclude, hyper)


def rank(table, ctx_idx, ctx_xv, candidates, targets, exclude=None, hyper=None, filtered=False):
    """scorer_rank under the FM's logit and topk's order."""
    return scorer_rank(FMScorer(), table, ctx_idx, ctx_xv, candidates, targets, exclude, hyper, filtered)


def topk_network(table, mlp, fm_term, ctx_idx, ctx_xv, candidates, K, exclude=None, hyper=None):
    """scorer_topk under the DeepFM (fm_term = 1) / NFM (fm_term = 0) network mlp = (params, k, hidden, n_layers);
    candidates: a NetworkCandidates of the same table and fm_term."""
    return scorer_topk(NetworkScorer(mlp, fm_term), table, ctx_idx, ctx_xv, candidates, K, exclude, hyper)


def rank_network(table, mlp, fm_term, ctx_idx, ctx_xv, candidates, targets, exclude=None, hyper=None, filtered=False):
    """scorer_rank under the network's score and topk_network's order; networks fmx_mlp_rank does not take (hidden > 256) go
    through mlp_rank_torch."""
    return scorer_rank(NetworkScorer(mlp, fm_term), table, ctx_idx, ctx_xv, candidates, targets, exclude, hyper, filtered)


def topk_afm(table, afm, ctx_idx, ctx_xv, candidates, K, exclude=None, hyper=None):
    """scorer_topk under the AFM afm = (params, t): the exact logit of the combined sample; candidates: an AFMCandidates of
    the same table and attention parameters."""
    return scorer_topk(AFMScorer(afm, table.k), table, ctx_idx, ctx_xv, candidates, K, exclude, hyper)


def rank_afm(table, afm, ctx_idx, ctx_xv, candidates, targets, exclude=None, hyper=None, filtered=False):
    """scorer_rank under the AFM's logit and topk_afm's order."""
    return scorer_rank(AFMScorer(afm, table.k), table, ctx_idx, ctx_xv, candidates, targets, exclude, hyper, filtered)


# ---- the network's score as chunked torch: the path of networks the kernels do not take (hidden > 256), and the baseline of
# tools/mlp_topk_times.py and tools/rank_times.py
def _mlp_torch_blocks(mlp, fm_term, Su, Bu, au, Sc, Bc, ac, excl_offsets, excl_pos, kp, max_elems):
    """fmx_mlp_topk's score (up to fp32 summation order) by blocks of users: yields (u0, u1, score fp32 [u1 - u0, N] with -0 as
    +0, eligible bool [u1 - u0, N]: not NaN and not excluded)."""
    params, k, H, L = mlp
    U, N, dev = Su.shape[0], Sc.shape[0], Su.device
    kp = Sc.shape[1] if kp is None else int(kp)
    Ws, off = [], 0
    for l in range(L):
        n_in = k if l == 0 else H
        Ws.append((params[off:off + H * n_in].view(H, n_in), params[off + H * n_in:off + H * n_in + H]))
        off += H * n_in + H
    Sck, Bck = Sc[:, :k], Bc[:, :k]
    ub = max(1, min(U, max_elems // max(1, N * max(H, k))))
    cb = max(1, min(N, max_elems // max(1, ub * max(H, k))))
    offs = None if excl_offsets is None else excl_offsets.long().cpu()
    for u0 in range(0, U, ub):
        u1 = min(U, u0 + ub)
        with torch.no_grad():
            score = torch.empty((u1 - u0, N), dtype=torch.float32, device=dev)
            for c0 in range(0, N, cb):
                c1 = min(N, c0 + cb)
                x = (Bu[u0:u1, None, :k] + Bck[None, c0:c1]) + Su[u0:u1, None, :k] * Sck[None, c0:c1]
                for W, b in Ws:
                    x = torch.relu(torch.nn.functional.linear(x, W, b))
                base = au[u0:u1, None] + ac[None, c0:c1]
                if fm_term:
                    base = base + Su[u0:u1, :kp] @ Sc[c0:c1, :kp].T
                score[:, c0:c1] = base + x.sum(-1)
            score = score + 0.0                              # -0 -> +0
            ok = ~torch.isnan(score)
            if offs is not None:
                for u in range(u0, u1):
                    p = excl_pos[int(offs[u]):int(offs[u + 1])].long()
                    ok[u - u0, p[(p >= 0) & (p < N)]] = False
        yield u0, u1, score, ok


def mlp_topk_torch(mlp, fm_term, Su, Bu, au, Sc, Bc, ac, K, excl_offsets=None, excl_pos=None, kp=None, max_elems=1 << 25):
    """The same score (up to fp32 summation order) and the same result order as fmx_mlp_topk: for a block of users, every
    candidate's network output, then a stable sort on (score descending, position ascending); NaN and excluded candidates are
    never returned, rows are padded with -1 / -inf, -0 is returned as +0."""
    U, dev = Su.shape[0], Su.device
    top_pos = torch.full((U, K), -1, dtype=torch.int32, device=dev)
    top_score = torch.full((U, K), float("-inf"), dtype=torch.float32, device=dev)
    for u0, u1, score, ok in _mlp_torch_blocks(mlp, fm_term, Su, Bu, au, Sc, Bc, ac, excl_offsets, excl_pos, kp, max_elems):
        score = torch.where(ok, score, torch.full_like(score, float("-inf")))
        s1, i1 = torch.sort(score, dim=1, descending=True, stable=True)
        ok1 = torch.gather(ok, 1, i1)
        _, i2 = torch.sort(ok1.to(torch.int8), dim=1, descending=True, stable=True)
        idx = torch.gather(i1, 1, i2)[:, :K]
        sc = torch.gather(s1, 1, i2)[:, :K]
        valid = torch.gather(ok1, 1, i2)[:, :K]
        n = idx.shape[1]
        top_pos[u0:u1, :n] = torch.where(valid, idx, torch.full_like(idx, -1)).to(torch.int32)
        top_score[u0:u1, :n] = torch.where(valid, sc, torch.full_like(sc, float("-inf")))
    return top_pos, top_score


def mlp_rank_torch(mlp, fm_term, Su, Bu, au, Sc, Bc, ac, targets, filtered=False, excl_offsets=None, excl_pos=None, kp=None,
                   max_elems=1 << 25):
    """fmx_mlp_rank's definition on the same statement of the score: for a block of users the eligible candidates, and for each
    target the number of them with a greater (score, position) key.  targets: int32 [U, T], any T.  Returns as fm_rank."""
    U, N, dev = Su.shape[0], Sc.shape[0], Su.device
    T = targets.shape[1]
    rank = torch.full((U, T), -1, dtype=torch.int32, device=dev)
    score_out = torch.full((U, T), float("-inf"), dtype=torch.float32, device=dev)
    n_cand = torch.zeros(U, dtype=torch.int32, device=dev)
    positions = torch.arange(N, device=dev)
    for u0, u1, score, ok in _mlp_torch_blocks(mlp, fm_term, Su, Bu, au, Sc, Bc, ac, excl_offsets, excl_pos, kp, max_elems):
        n_cand[u0:u1] = ok.sum(1).to(torch.int32)
        key = _rank_key(torch.where(ok, score, torch.zeros_like(score)), positions[None, :].expand_as(score))
        tg = targets[u0:u1].long()
        inside = (tg >= 0) & (tg < N)
        tgc = torch.where(inside, tg, torch.zeros_like(tg))
        t_ok = inside & torch.gather(ok, 1, tgc)
        t_key = torch.gather(key, 1, tgc)
        for t in range(T):
            ahead = ok & (key > t_key[:, t:t + 1])
            if filtered:                                 # the user's other eligible targets are not counted
                others = torch.zeros_like(ok)
                rows = torch.arange(u1 - u0, device=dev)[:, None].expand(-1, T)
                others[rows[t_ok], tgc[t_ok]] = True
                ahead = ahead & ~others
            rank[u0:u1, t] = torch.where(t_ok[:, t], ahead.sum(1), torch.full_like(tg[:, t], -1)).to(torch.int32)
        score_out[u0:u1] = torch.where(t_ok, torch.gather(score, 1, tgc), torch.full_like(score_out[u0:u1], float("-inf")))
    return rank, score_out, n_cand


def ranking_metrics(ranks, n_cand, ks=(1, 5, 10)):
    """Ranking metrics of rank's results; pure torch, CPU tensors welcome.  ranks [U, T] (or [U]) integer, -1 for targets that
    were not ranked; n_cand [U].  Over the valid targets (rank >= 0): hr@K = mean [r < K]; ndcg@K = mean [r < K] / log2(r + 2);
    mrr = mean 1 / (r + 1); auc = mean 1 - r / (n_cand - 1) over the targets whose user has n_cand > 1; n = their number.
    Returns a dict of Python floats (NaN where nothing is averaged) and the int n."""
    ranks = torch.as_tensor(ranks)
    if ranks.dim() == 1:
        ranks = ranks[:, None]
    n_cand = torch.as_tensor(n_cand).reshape(-1, 1).expand_as(ranks)
    valid = ranks >= 0
    r = ranks[valid].to(torch.float64)
    nc = n_cand[valid].to(torch.float64)
    n = int(r.numel())

    def mean(x):
        return float(x.sum() / x.numel()) if x.numel() else float("nan")

    out = {}
    for K in ks:
        hit = (r < K).to(torch.float64)
        out[f"hr@{int(K)}"] = mean(hit)
        out[f"ndcg@{int(K)}"] = mean(hit / torch.log2(r + 2.0))
    out["mrr"] = mean(1.0 / (r + 1.0))
    wide = nc > 1
    out["auc"] = mean(1.0 - r[wide] / (nc[wide] - 1.0))
    out["n"] = n
    return out
