"""Top-K recommendation over an FM table's candidates (include/fmx.h, fmx_fm_topk).

Split a sample's fields into context fields (user, time, ...) and item fields.  For a context u and a candidate c the logit of
the combined sample is

    logit(u + c) = a_u + a_c + <S_u, S_c>

a_u: the logit of u's context fields alone (bias included); a_c: sfirst + sbi of c's item fields alone; S_u, S_c: their sums of
V x.  Both sides are fmx_fm_forward over full-width rows in which the other side's fields carry index 0 and value 0 (a zero
value adds exact zeros to S, to sum e^2 and to the first-order sum).  What remains -- U x N kp-wide dot products and an exact
per-user top-K -- is one fmx_fm_topk call.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .engine import Hyper

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


def side_sums(table, idx, xv, keep_fields, hyper=None, want_bias=True):
    """fmx_fm_forward over the rows of idx / xv ([R, F], full width) with every field outside keep_fields given index 0 and
    value 0.  Returns (S [R, kp], a [R]) on the device: a = the logit (bias included) when want_bias, else sfirst + sbi.
    An index outside its field (in a kept column) raises IndexError."""
    F, dev, kp = table.n_fields, table.device, table.kp
    idx = _as_index(idx, F, dev)
    R = idx.shape[0]
    xv = _as_values(xv, (R, F), dev)
    keep = torch.zeros(F, dtype=torch.bool, device=dev)
    keep[list(keep_fields)] = True
    idx = torch.where(keep[None, :], idx, torch.zeros_like(idx)).contiguous()
    xv = torch.where(keep[None, :], xv, torch.zeros_like(xv)).contiguous()
    lib, h = _lib.load(), _hyper_for(table, hyper)
    S = torch.empty((R, kp), dtype=torch.float32, device=dev)
    a = torch.empty(R, dtype=torch.float32, device=dev)
    n = min(R, CHUNK)
    sfirst = torch.empty(n, dtype=torch.float32, device=dev)
    sbi = torch.empty(n, dtype=torch.float32, device=dev)
    error = torch.zeros(1, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for r0 in range(0, R, CHUNK):
        B = min(CHUNK, R - r0)
        o = _lib.FwdOut()
        o.S = S[r0:].data_ptr()
        if want_bias:
            o.logit = a[r0:].data_ptr()
        else:
            o.sfirst, o.sbi = sfirst.data_ptr(), sbi.data_ptr()
        o.error = error.data_ptr()
        _lib.check(lib.fmx_fm_forward(table.c_struct(), h.ref(), idx[r0:].data_ptr(), xv[r0:].data_ptr(), None, B,
                                      _lib.LOSS_NONE, 1.0, C.byref(o), stream))
        if not want_bias:
            torch.add(sfirst[:B], sbi[:B], out=a[r0:r0 + B])
    if int(error.item()) != 0:
        raise IndexError("index out of range in self (flagged by the fmx kernels)")
    return S, a


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


def fm_topk(Su, au, Sc, ac, K, excl_offsets=None, excl_pos=None, workspace=None, out=None, stream=None, kp=None):
    """The raw call: Su [U, >= kp], au [U], Sc [N, >= kp], ac [N] fp32 device tensors (row strides multiples of 4, 16-byte
    aligned); kp defaults to Sc's width.  Returns (top_pos int32 [U, K], top_score fp32 [U, K]) on the device."""
    U, N = Su.shape[0], Sc.shape[0]
    kp = Sc.shape[1] if kp is None else int(kp)
    lib, dev = _lib.load(), Su.device
    need = int(lib.fmx_fm_topk_workspace_bytes(U, N, K))
    _lib.check(min(need, 0))
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    if out is None:
        out = (torch.empty((U, K), dtype=torch.int32, device=dev), torch.empty((U, K), dtype=torch.float32, device=dev))
    st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
    _lib.check(lib.fmx_fm_topk(Su.data_ptr(), Su.stride(0), au.data_ptr(), U, Sc.data_ptr(), Sc.stride(0), ac.data_ptr(), N, kp,
                               None if excl_offsets is None else excl_offsets.data_ptr(),
                               None if excl_pos is None else excl_pos.data_ptr(), K, workspace.data_ptr(),
                               workspace.numel() * workspace.element_size(), out[0].data_ptr(), out[1].data_ptr(), st))
    return out


def topk(table, ctx_idx, ctx_xv, candidates, K, exclude=None, hyper=None):
    """Top-K candidates for every context row of ctx_idx / ctx_xv ([U, F] full width, the item columns ignored).  Returns
    device tensors (positions int64 [U, K], -1 padded; logits fp32 [U, K], -inf padded), each row by logit descending, then
    position ascending.  exclude: see exclusions_csr."""
    if candidates.table is not table:
        raise ValueError("candidates were computed for another table")
    ctx_fields = [f for f in range(table.n_fields) if f not in candidates.item_fields]
    Su, au = side_sums(table, ctx_idx, ctx_xv, ctx_fields, hyper if hyper is not None else candidates.hyper, want_bias=True)
    off, pos = exclusions_csr(exclude, Su.shape[0], table.device)
    top_pos, top_score = fm_topk(Su, au, candidates.Sc, candidates.ac, int(K), off, pos)
    return top_pos.long(), top_score
