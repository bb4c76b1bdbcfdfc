"""AFMEngine: workspace + launch sequencing of the attentional FM (fmx_afm_forward / fmx_afm_step / fmx_afm_step_opt /
fmx_afm_stream / fmx_afm_online_run, their pairwise-ranking forms fmx_afm_pair_* and their listwise forms fmx_afm_list_*) for one
FlatTable.

The attention parameters live in ONE flat fp32 device buffer [ W (t x k) | b (t) | h (t) | p (k) ] (include/fmx.h, fmx_afm_t);
the step returns their gradient in the same layout and leaves updating them to the caller -- or, given an AfmOpt, applies their
rule inside the gradient's reduction."""
import ctypes as C

import torch

from . import _lib
from .engine import FMEngine, MlpOpt, _list_G, _ptr
from .pairwise import n_pairs
from .table import FlatTable


def afm_param_count(k, t):
    return t * k + 2 * t + k


class AfmOpt(MlpOpt):
    """The attention parameters' optimizer state for fmx_afm_step_opt / fmx_afm_stream: fmx.MlpOpt over the flat buffer
    [W | b | h | p], with 'signadam' (p -= lr g / (|g| + eps): a fresh Adam's first step) taken beside 'sgd', 'adagrad', 'adam'.
    'signadam' and 'sgd' keep no moments: m and v stay zero."""

    RULES = ("signadam", "sgd", "adagrad", "adam")


class AFMEngine:
    def __init__(self, table: FlatTable, params, t, max_batch=4096):
        if not torch.cuda.is_available():
            raise RuntimeError("fmx needs a ROCm GPU: the hot path has no CPU implementation")
        self.lib = _lib.load()
        self.table = table
        self.device = table.device
        self.k, self.t = table.k, int(t)
        assert params.dtype == torch.float32 and params.is_contiguous() and params.numel() == afm_param_count(self.k, self.t)
        self.params = params
        self.c_afm = _lib.Afm(params.data_ptr(), self.k, self.t)
        self.grad = torch.zeros_like(params)
        self.loss_out = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.error = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.max_batch = 0
        self._alloc(max_batch)

    def _alloc(self, B):
        B = int(B)
        self.table.ensure_sort_split(B)      # large fields are cut into sort pieces when (index, sample) would not fit 32 bits
        nbytes = int(self.lib.fmx_afm_workspace_bytes(self.table.c_struct(), C.byref(self.c_afm), B))
        if nbytes < 0:
            _lib.check(nbytes)
        self.workspace = torch.zeros(nbytes // 4, dtype=torch.int32, device=self.device)
        self.logit = torch.empty(B, dtype=torch.float32, device=self.device)
        self.loss_b = torch.empty(B, dtype=torch.float32, device=self.device)
        self.max_batch = B

    def _ensure(self, B):
        # the table's sort fields may be split further for a larger batch: the workspace follows fmx_afm_workspace_bytes
        need = int(self.lib.fmx_afm_workspace_bytes(self.table.c_struct(), C.byref(self.c_afm), max(B, self.max_batch)))
        if B > self.max_batch or need > self.workspace.numel() * 4:
            self._alloc(max(B, self.max_batch))

    _stream = FMEngine._stream
    _steps, _advance, _counted = FMEngine._steps, FMEngine._advance, FMEngine._counted     # (opt, an AfmOpt, is its mlp_opt)
    to_device = FMEngine.to_device
    check_error_flag = FMEngine.check_error_flag

    def forward(self, hyper, idx_d, xv_d=None, y_d=None, loss=None, inv_b=None, stream=None):
        """-> B; logits in self.logit[:B], per-sample losses in self.loss_b[:B] when `loss` ('logits' / 'sigmoid') and y_d."""
        B = idx_d.shape[0]
        self._ensure(B)
        _lib.check(self.lib.fmx_afm_forward(self.table.c_struct(), C.byref(self.c_afm), hyper.ref(), idx_d.data_ptr(), _ptr(xv_d),
                                            _ptr(y_d), B, _lib.LOSSES[loss], 1.0 / B if inv_b is None else inv_b,
                                            self.logit.data_ptr(), self.loss_b.data_ptr(), self.error.data_ptr(),
                                            self._stream(stream)))
        return B

    def step(self, hyper, rule, idx_d, xv_d, y_d, inv_b=None, stream=None, opt=None):
        """One mini-batch step: the table updated under `rule`, the mean loss in self.loss_out[0], the attention gradient in
        self.grad (no sync here).  opt (an AfmOpt): the attention parameters take its rule in the same call (fmx_afm_step_opt)
        and its step count advances; None leaves them to the caller."""
        B = idx_d.shape[0]
        self._ensure(B)
        head = (self.table.c_struct(), hyper.ref(), _lib.RULES[rule], C.byref(self.c_afm), idx_d.data_ptr(), _ptr(xv_d),
                y_d.data_ptr(), B, 1.0 / B if inv_b is None else inv_b, self.workspace.data_ptr(), self.workspace.numel() * 4,
                self.grad.data_ptr())
        tail = (self.loss_out.data_ptr(), self.error.data_ptr(), self._stream(stream))
        if opt is None:
            self._counted(self.lib.fmx_afm_step, (*head, *tail), hyper)
        else:
            self._counted(self.lib.fmx_afm_step_opt, (*head, opt.ref(), *tail), hyper, 1, opt)

    def stream(self, hyper, rule, idx_pool, xv_pool, y_pool, B, n_steps, opt, inv_b=None, losses=None, stream=None):
        """n_steps steps over a device-resident pool in one call (fmx_afm_stream; no sync here): idx_pool [n_pool, B, F] int32,
        xv_pool the same shape in fp32 or None (ones), y_pool [n_pool, B]; step s takes batch s mod n_pool.  losses: an fp32
        device tensor of n_steps elements for the steps' mean losses, or None.  The table's step count and opt's advance by
        n_steps; self.grad holds the last step's attention gradient."""
        B, n_steps = int(B), int(n_steps)
        n_pool = idx_pool.numel() // (B * self.table.n_fields)
        assert idx_pool.dtype == torch.int32 and idx_pool.is_contiguous() and n_pool >= 1 and y_pool.numel() == n_pool * B
        assert xv_pool is None or (xv_pool.dtype == torch.float32 and xv_pool.is_contiguous() and xv_pool.numel() == idx_pool.numel())
        assert losses is None or (losses.dtype == torch.float32 and losses.numel() >= n_steps)
        self._ensure(B)
        self._counted(self.lib.fmx_afm_stream, (self.table.c_struct(), hyper.ref(), _lib.RULES[rule], C.byref(self.c_afm),
                                                idx_pool.data_ptr(), _ptr(xv_pool), y_pool.data_ptr(), n_pool, B,
                                                1.0 / B if inv_b is None else inv_b, n_steps, self.workspace.data_ptr(),
                                                self.workspace.numel() * 4, self.grad.data_ptr(), opt.ref(), _ptr(losses),
                                                self.error.data_ptr(), self._stream(stream)), hyper, n_steps, opt)

    def online_run(self, hyper, rule, idx_d, xv_d, y_d, opt, logits=None, losses=None, stream=None):
        """The online predict-then-fit loop over a device-resident stream in one call (fmx_afm_online_run; no sync here): idx_d
        [N, F] int32, xv_d the same shape in fp32 or None (ones), y_d [N].  Sample i is predicted, then fitted on: N steps of
        step(B = 1, inv_b = 1).  logits / losses: fp32 device tensors of N elements for each sample's logit BEFORE its update
        and its loss, or None.  The table's step count and opt's advance by N; self.grad holds the last sample's attention
        gradient."""
        N = int(idx_d.shape[0])
        assert idx_d.dtype == torch.int32 and idx_d.is_contiguous() and idx_d.numel() == N * self.table.n_fields
        assert y_d.dtype == torch.float32 and y_d.numel() == N
        assert xv_d is None or (xv_d.dtype == torch.float32 and xv_d.is_contiguous() and xv_d.numel() == idx_d.numel())
        for out in (logits, losses):
            assert out is None or (out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= N)
        self._ensure(1)
        self._counted(self.lib.fmx_afm_online_run, (self.table.c_struct(), hyper.ref(), _lib.RULES[rule], C.byref(self.c_afm),
                                                    idx_d.data_ptr(), _ptr(xv_d), y_d.data_ptr(), N, self.workspace.data_ptr(),
                                                    self.workspace.numel() * 4, self.grad.data_ptr(), opt.ref(), _ptr(logits),
                                                    _ptr(losses), self.error.data_ptr(), self._stream(stream)), hyper, N, opt)

    # ---- pairwise-ranking (BPR) training: rows [2P, F] from fmx.pairwise.assemble_pairs, row 2p the positive, 2p + 1 the negative ----
    def _pair_rows(self, idx_d, xv_d):
        P = n_pairs(idx_d)
        assert idx_d.dtype == torch.int32 and idx_d.is_contiguous() and idx_d.shape[1] == self.table.n_fields
        assert xv_d is None or (xv_d.dtype == torch.float32 and xv_d.is_contiguous() and xv_d.shape == idx_d.shape)
        return P

    def pair_forward(self, hyper, idx_d, xv_d=None, margin=0.0, inv_b=None, dz=None, stream=None):
        """-> P; the 2P logits in self.logit[:2P] (the bits of forward()), the pair losses in self.loss_b[0:2P:2] (the odd slots
        +0).  dz: an fp32 device tensor of 2P elements for dlogit (inv_b folded in, default 1 / P), or None."""
        P = self._pair_rows(idx_d, xv_d)
        assert dz is None or (dz.dtype == torch.float32 and dz.is_contiguous() and dz.numel() >= 2 * P)
        self._ensure(2 * P)
        _lib.check(self.lib.fmx_afm_pair_forward(self.table.c_struct(), C.byref(self.c_afm), hyper.ref(), idx_d.data_ptr(), _ptr(xv_d),
                                                 P, margin, 1.0 / P if inv_b is None else inv_b, self.logit.data_ptr(),
                                                 self.loss_b.data_ptr(), _ptr(dz), self.error.data_ptr(), self._stream(stream)))
        return P

    def pair_step(self, hyper, rule, idx_d, xv_d=None, margin=0.0, inv_b=None, stream=None, opt=None):
        """One mini-batch pair step: the table updated under `rule`, the mean pair loss in self.loss_out[0], the attention
        gradient in self.grad, the 2P logits before the update in self.logit[:2P] (no sync here).  opt (an AfmOpt): the
        attention parameters take its rule in the same call (fmx_afm_pair_step_opt) and its step count advances."""
        P = self._pair_rows(idx_d, xv_d)
        self._ensure(2 * P)
        head = (self.table.c_struct(), hyper.ref(), _lib.RULES[rule], C.byref(self.c_afm), idx_d.data_ptr(), _ptr(xv_d), P, margin,
                1.0 / P if inv_b is None else inv_b, self.workspace.data_ptr(), self.workspace.numel() * 4, self.grad.data_ptr())
        tail = (self.logit.data_ptr(), self.loss_out.data_ptr(), self.error.data_ptr(), self._stream(stream))
        if opt is None:
            self._counted(self.lib.fmx_afm_pair_step, (*head, *tail), hyper)
        else:
            self._counted(self.lib.fmx_afm_pair_step_opt, (*head, opt.ref(), *tail), hyper, 1, opt)

    def pair_stream(self, hyper, rule, idx_pool, xv_pool, P, n_steps, opt, margin=0.0, inv_b=None, losses=None, stream=None):
        """n_steps pair steps over a device-resident pool in one call (fmx_afm_pair_stream; no sync here): idx_pool
        [n_pool, 2P, F] int32, xv_pool the same shape in fp32 or None (ones); step s takes batch s mod n_pool.  losses: an fp32
        device tensor of n_steps elements, or None.  The table's step count and opt's advance by n_steps."""
        P, n_steps = int(P), int(n_steps)
        n_pool = idx_pool.numel() // (2 * P * self.table.n_fields)
        assert idx_pool.dtype == torch.int32 and idx_pool.is_contiguous() and n_pool >= 1
        assert xv_pool is None or (xv_pool.dtype == torch.float32 and xv_pool.is_contiguous() and xv_pool.numel() == idx_pool.numel())
        assert losses is None or (losses.dtype == torch.float32 and losses.numel() >= n_steps)
        self._ensure(2 * P)
        self._counted(self.lib.fmx_afm_pair_stream, (self.table.c_struct(), hyper.ref(), _lib.RULES[rule], C.byref(self.c_afm),
                                                     idx_pool.data_ptr(), _ptr(xv_pool), n_pool, P, margin,
                                                     1.0 / P if inv_b is None else inv_b, n_steps, self.workspace.data_ptr(),
                                                     self.workspace.numel() * 4, self.grad.data_ptr(), opt.ref(), _ptr(losses),
                                                     self.error.data_ptr(), self._stream(stream)), hyper, n_steps, opt)

    def pair_online_run(self, hyper, rule, idx_d, xv_d, opt, margin=0.0, logits=None, losses=None, stream=None):
        """The online protocol for pairs in one call (fmx_afm_pair_online_run; no sync here): every pair of idx_d [2N, F] is
        predicted, then fitted on alone -- N steps of pair_step(P = 1, inv_b = 1).  logits: an fp32 device tensor of 2N elements
        for each pair's two logits BEFORE its update; losses: N elements; or None.  The table's step count and opt's advance
        by N."""
        N = self._pair_rows(idx_d, xv_d)
        assert logits is None or (logits.dtype == torch.float32 and logits.is_contiguous() and logits.numel() >= 2 * N)
        assert losses is None or (losses.dtype == torch.float32 and losses.is_contiguous() and losses.numel() >= N)
        self._ensure(2)
        self._counted(self.lib.fmx_afm_pair_online_run, (self.table.c_struct(), hyper.ref(), _lib.RULES[rule], C.byref(self.c_afm),
                                                         idx_d.data_ptr(), _ptr(xv_d), N, margin, self.workspace.data_ptr(),
                                                         self.workspace.numel() * 4, self.grad.data_ptr(), opt.ref(), _ptr(logits),
                                                         _ptr(losses), self.error.data_ptr(), self._stream(stream)), hyper, N, opt)

    # ---- listwise (sampled-softmax) training: rows [B G, F] from fmx.pairwise.assemble_lists, row G i the positive of list i ----
    def _list_rows(self, idx_d, xv_d, G, ws_lists=None):
        """-> B for the rows [B G, F] of B lists; grows the buffers, and keeps the list steps' own workspace, self._list_ws, sized
        through fmx_afm_list_workspace_bytes for ws_lists lists (default B): the AFM step's workspace and the scratch behind it
        that the bias rule of a list step runs on."""
        G = _list_G(G)
        assert idx_d.dtype == torch.int32 and idx_d.is_contiguous() and idx_d.dim() == 2 and idx_d.shape[1] == self.table.n_fields
        assert xv_d is None or (xv_d.dtype == torch.float32 and xv_d.is_contiguous() and xv_d.shape == idx_d.shape)
        rows = idx_d.shape[0]
        if rows < G or rows % G:
            raise ValueError(f"list rows must be [B G, F] with B >= 1 and G = {G}, got {rows} rows")
        B = rows // G
        n = B if ws_lists is None else int(ws_lists)
        self._ensure(n * G)
        need = int(self.lib.fmx_afm_list_workspace_bytes(self.table.c_struct(), C.byref(self.c_afm), n, G))
        if need < 0:
            _lib.check(need)
        ws = getattr(self, "_list_ws", None)
        if ws is None or need > ws.numel() * 4:
            self._list_ws = torch.zeros(need // 4, dtype=torch.int32, device=self.device)
        return B

    def list_forward(self, hyper, idx_d, G, xv_d=None, inv_b=None, dz=None, stream=None):
        """-> B; the B G logits in self.logit[:B G] (the bits of forward()), the list losses in self.loss_b[0:B G:G] (the
        negatives' slots +0).  dz: an fp32 device tensor of B G elements for dlogit (inv_b folded in, default 1 / B), or None."""
        B = self._list_rows(idx_d, xv_d, G)
        assert dz is None or (dz.dtype == torch.float32 and dz.is_contiguous() and dz.numel() >= B * G)
        _lib.check(self.lib.fmx_afm_list_forward(self.table.c_struct(), C.byref(self.c_afm), hyper.ref(), idx_d.data_ptr(), _ptr(xv_d),
                                                 B, int(G), 1.0 / B if inv_b is None else inv_b, self.logit.data_ptr(),
                                                 self.loss_b.data_ptr(), _ptr(dz), self.error.data_ptr(), self._stream(stream)))
        return B

    def list_step(self, hyper, rule, idx_d, G, xv_d=None, inv_b=None, stream=None, opt=None):
        """One mini-batch list step: the table updated under `rule` (its bias untouched), the mean list loss in self.loss_out[0],
        the attention gradient in self.grad, the B G logits before the update in self.logit[:B G] (no sync here).  opt (an
        AfmOpt): the attention parameters take its rule in the same call (fmx_afm_list_step_opt) and its step count advances."""
        B = self._list_rows(idx_d, xv_d, G)
        head = (self.table.c_struct(), hyper.ref(), _lib.RULES[rule], C.byref(self.c_afm), idx_d.data_ptr(), _ptr(xv_d), B, int(G),
                1.0 / B if inv_b is None else inv_b, self._list_ws.data_ptr(), self._list_ws.numel() * 4, self.grad.data_ptr())
        tail = (self.logit.data_ptr(), self.loss_out.data_ptr(), self.error.data_ptr(), self._stream(stream))
        if opt is None:
            self._counted(self.lib.fmx_afm_list_step, (*head, *tail), hyper)
        else:
            self._counted(self.lib.fmx_afm_list_step_opt, (*head, opt.ref(), *tail), hyper, 1, opt)

    def list_stream(self, hyper, rule, idx_pool, xv_pool, B, G, n_steps, opt, inv_b=None, losses=None, stream=None):
        """n_steps list steps over a device-resident pool in one call (fmx_afm_list_stream; no sync here): idx_pool
        [n_pool, B G, F] int32, xv_pool the same shape in fp32 or None (ones); step s takes batch s mod n_pool.  losses: an fp32
        device tensor of n_steps elements, or None.  The table's step count and opt's advance by n_steps."""
        B, G, n_steps = int(B), _list_G(G), int(n_steps)
        n_pool = idx_pool.numel() // (B * G * self.table.n_fields)
        assert n_pool >= 1 and idx_pool.numel() == n_pool * B * G * self.table.n_fields
        assert xv_pool is None or (xv_pool.dtype == torch.float32 and xv_pool.is_contiguous() and xv_pool.numel() == idx_pool.numel())
        assert losses is None or (losses.dtype == torch.float32 and losses.numel() >= n_steps)
        first = idx_pool.reshape(n_pool, B * G, self.table.n_fields)[0]
        self._list_rows(first, None, G)
        self._counted(self.lib.fmx_afm_list_stream, (self.table.c_struct(), hyper.ref(), _lib.RULES[rule], C.byref(self.c_afm),
                                                     idx_pool.data_ptr(), _ptr(xv_pool), n_pool, B, G,
                                                     1.0 / B if inv_b is None else inv_b, n_steps, self._list_ws.data_ptr(),
                                                     self._list_ws.numel() * 4, self.grad.data_ptr(), opt.ref(), _ptr(losses),
                                                     self.error.data_ptr(), self._stream(stream)), hyper, n_steps, opt)

    def list_online_run(self, hyper, rule, idx_d, G, xv_d, opt, logits=None, losses=None, stream=None):
        """The online protocol for lists in one call (fmx_afm_list_online_run; no sync here): every list of idx_d [N G, F] is
        predicted, then fitted on alone -- N steps of list_step(B = 1, inv_b = 1), queued.  logits: an fp32 device tensor of N G
        elements for each list's logits BEFORE its update; losses: N elements; or None.  The table's step count and opt's
        advance by N."""
        N = self._list_rows(idx_d, xv_d, G, ws_lists=1)
        assert logits is None or (logits.dtype == torch.float32 and logits.is_contiguous() and logits.numel() >= N * G)
        assert losses is None or (losses.dtype == torch.float32 and losses.is_contiguous() and losses.numel() >= N)
        self._counted(self.lib.fmx_afm_list_online_run, (self.table.c_struct(), hyper.ref(), _lib.RULES[rule], C.byref(self.c_afm),
                                                         idx_d.data_ptr(), _ptr(xv_d), N, int(G), self._list_ws.data_ptr(),
                                                         self._list_ws.numel() * 4, self.grad.data_ptr(), opt.ref(), _ptr(logits),
                                                         _ptr(losses), self.error.data_ptr(), self._stream(stream)), hyper, N, opt)

    def pair_online_form(self, attn_rule):
        """-> (tile buffers, moments in LDS) of the form pair_online_run takes for this table under the attention rule
        `attn_rule` (a name of AfmOpt.RULES): tile buffers > 0 is the one-workgroup kernel, 0 the queued pair steps
        (fmx_afm_pair_online_form; no device call)."""
        mom = C.c_int32(0)
        nb = self.lib.fmx_afm_pair_online_form(self.table.c_struct(), C.byref(self.c_afm), _lib.RULES[attn_rule], C.byref(mom))
        if nb < 0:
            _lib.check(nb)
        return nb, bool(mom.value)
