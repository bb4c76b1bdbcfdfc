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

    # ---- the nine training calls: step / stream / online_run under BCE on y, their pair_ forms and their list_ forms ----
    def _check(self, idx, xv, rows, y=None, outs=()):
        """The validation behind the nine: idx int32, contiguous, `rows` rows of F indices (a pool: the rows of all its batches);
        xv None or fp32, contiguous, an element per index; y None or fp32, an element per row; outs: (tensor or None, the
        elements it must hold) for every fp32 output the call fills."""
        assert idx.dtype == torch.int32 and idx.is_contiguous() and idx.numel() == rows * self.table.n_fields
        assert xv is None or (xv.dtype == torch.float32 and xv.is_contiguous() and xv.numel() == idx.numel())
        assert y is None or (y.dtype == torch.float32 and y.numel() == rows)
        for out, n in outs:
            assert out is None or (out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= n)

    def _call(self, kind, form, hyper, rule, idx, xv, y, dims, outs, opt, n=1, stream=None):
        """One checked call of fmx_afm_<kind><form> that takes n steps -- for a step given an AfmOpt, its _opt form.  kind: ""
        (BCE: y is passed), "pair_" or "list_" (the list steps' own workspace, self._list_ws).  dims: the call's counts and
        scalars between the inputs and the workspace; outs: its output pointers behind the attention gradient (and opt)."""
        name = f"fmx_afm_{kind}{form}" + ("_opt" if form == "step" and opt is not None else "")
        ws = self._list_ws if kind == "list_" else self.workspace
        args = (self.table.c_struct(), hyper.ref(), _lib.RULES[rule], C.byref(self.c_afm), idx.data_ptr(), _ptr(xv),
                *(() if kind else (y.data_ptr(),)), *dims, ws.data_ptr(), ws.numel() * 4, self.grad.data_ptr(),
                *(() if opt is None else (opt.ref(),)), *outs, self.error.data_ptr(), self._stream(stream))
        self._counted(getattr(self.lib, name), args, hyper, n, opt)

    def step(self, hyper, rule, idx_d, xv_d, y_d, inv_b=None, stream=None, opt=None):
        """One mini-batch step: the table updated under `rule`, the mean loss in self.loss_out[0], the attention gradient in
        self.grad (no sync here).  opt (an AfmOpt): the attention parameters take its rule in the same call (fmx_afm_step_opt)
        and its step count advances; None leaves them to the caller."""
        B = idx_d.shape[0]
        self._check(idx_d, xv_d, B, y_d)
        self._ensure(B)
        self._call("", "step", hyper, rule, idx_d, xv_d, y_d, (B, 1.0 / B if inv_b is None else inv_b), (self.loss_out.data_ptr(),),
                   opt, 1, stream)

    def stream(self, hyper, rule, idx_pool, xv_pool, y_pool, B, n_steps, opt, inv_b=None, losses=None, stream=None):
        """n_steps steps over a device-resident pool in one call (fmx_afm_stream; no sync here): idx_pool [n_pool, B, F] int32,
        xv_pool the same shape in fp32 or None (ones), y_pool [n_pool, B]; step s takes batch s mod n_pool.  losses: an fp32
        device tensor of n_steps elements for the steps' mean losses, or None.  The table's step count and opt's advance by
        n_steps; self.grad holds the last step's attention gradient."""
        B, n_steps = int(B), int(n_steps)
        n_pool = idx_pool.numel() // (B * self.table.n_fields)
        assert n_pool >= 1
        self._check(idx_pool, xv_pool, n_pool * B, y_pool, ((losses, n_steps),))
        self._ensure(B)
        self._call("", "stream", hyper, rule, idx_pool, xv_pool, y_pool, (n_pool, B, 1.0 / B if inv_b is None else inv_b, n_steps),
                   (_ptr(losses),), opt, n_steps, stream)

    def online_run(self, hyper, rule, idx_d, xv_d, y_d, opt, logits=None, losses=None, stream=None):
        """The online predict-then-fit loop over a device-resident stream in one call (fmx_afm_online_run; no sync here): idx_d
        [N, F] int32, xv_d the same shape in fp32 or None (ones), y_d [N].  Sample i is predicted, then fitted on: N steps of
        step(B = 1, inv_b = 1).  logits / losses: fp32 device tensors of N elements for each sample's logit BEFORE its update
        and its loss, or None.  The table's step count and opt's advance by N; self.grad holds the last sample's attention
        gradient."""
        N = int(idx_d.shape[0])
        self._check(idx_d, xv_d, N, y_d, ((logits, N), (losses, N)))
        self._ensure(1)
        self._call("", "online_run", hyper, rule, idx_d, xv_d, y_d, (N,), (_ptr(logits), _ptr(losses)), opt, N, stream)

    # ---- pairwise-ranking (BPR) training: rows [2P, F] from fmx.pairwise.assemble_pairs, row 2p the positive, 2p + 1 the negative ----
    def _pair_rows(self, idx_d, xv_d, outs=lambda P: ()):
        P = n_pairs(idx_d)
        self._check(idx_d, xv_d, 2 * P, outs=outs(P))
        return P

    def pair_forward(self, hyper, idx_d, xv_d=None, margin=0.0, inv_b=None, dz=None, stream=None):
        """-> P; the 2P logits in self.logit[:2P] (the bits of forward()), the pair losses in self.loss_b[0:2P:2] (the odd slots
        +0).  dz: an fp32 device tensor of 2P elements for dlogit (inv_b folded in, default 1 / P), or None."""
        P = self._pair_rows(idx_d, xv_d, lambda P: ((dz, 2 * P),))
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
        self._call("pair_", "step", hyper, rule, idx_d, xv_d, None, (P, margin, 1.0 / P if inv_b is None else inv_b),
                   (self.logit.data_ptr(), self.loss_out.data_ptr()), opt, 1, stream)

    def pair_stream(self, hyper, rule, idx_pool, xv_pool, P, n_steps, opt, margin=0.0, inv_b=None, losses=None, stream=None):
        """n_steps pair steps over a device-resident pool in one call (fmx_afm_pair_stream; no sync here): idx_pool
        [n_pool, 2P, F] int32, xv_pool the same shape in fp32 or None (ones); step s takes batch s mod n_pool.  losses: an fp32
        device tensor of n_steps elements, or None.  The table's step count and opt's advance by n_steps."""
        P, n_steps = int(P), int(n_steps)
        n_pool = idx_pool.numel() // (2 * P * self.table.n_fields)
        assert n_pool >= 1
        self._check(idx_pool, xv_pool, n_pool * 2 * P, outs=((losses, n_steps),))
        self._ensure(2 * P)
        self._call("pair_", "stream", hyper, rule, idx_pool, xv_pool, None,
                   (n_pool, P, margin, 1.0 / P if inv_b is None else inv_b, n_steps), (_ptr(losses),), opt, n_steps, stream)

    def pair_online_run(self, hyper, rule, idx_d, xv_d, opt, margin=0.0, logits=None, losses=None, stream=None):
        """The online protocol for pairs in one call (fmx_afm_pair_online_run; no sync here): every pair of idx_d [2N, F] is
        predicted, then fitted on alone -- N steps of pair_step(P = 1, inv_b = 1).  logits: an fp32 device tensor of 2N elements
        for each pair's two logits BEFORE its update; losses: N elements; or None.  The table's step count and opt's advance
        by N."""
        N = self._pair_rows(idx_d, xv_d, lambda N: ((logits, 2 * N), (losses, N)))
        self._ensure(2)
        self._call("pair_", "online_run", hyper, rule, idx_d, xv_d, None, (N, margin), (_ptr(logits), _ptr(losses)), opt, N, stream)

    # ---- listwise (sampled-softmax) training: rows [B G, F] from fmx.pairwise.assemble_lists, row G i the positive of list i ----
    def _list_rows(self, idx_d, xv_d, G, ws_lists=None, outs=lambda B: ()):
        """-> B for the rows [B G, F] of B lists; grows the buffers, and keeps the list steps' own workspace, self._list_ws, sized
        through fmx_afm_list_workspace_bytes for ws_lists lists (default B): the AFM step's workspace and the scratch behind it
        that the bias rule of a list step runs on.  outs(B): the outputs _check looks at."""
        G = _list_G(G)
        assert idx_d.dim() == 2
        rows = idx_d.shape[0]
        if rows < G or rows % G:
            raise ValueError(f"list rows must be [B G, F] with B >= 1 and G = {G}, got {rows} rows")
        B = rows // G
        self._check(idx_d, xv_d, rows, outs=outs(B))
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
        B = self._list_rows(idx_d, xv_d, G, outs=lambda B: ((dz, B * int(G)),))
        _lib.check(self.lib.fmx_afm_list_forward(self.table.c_struct(), C.byref(self.c_afm), hyper.ref(), idx_d.data_ptr(), _ptr(xv_d),
                                                 B, int(G), 1.0 / B if inv_b is None else inv_b, self.logit.data_ptr(),
                                                 self.loss_b.data_ptr(), _ptr(dz), self.error.data_ptr(), self._stream(stream)))
        return B

    def list_step(self, hyper, rule, idx_d, G, xv_d=None, inv_b=None, stream=None, opt=None):
        """One mini-batch list step: the table updated under `rule` (its bias untouched), the mean list loss in self.loss_out[0],
        the attention gradient in self.grad, the B G logits before the update in self.logit[:B G] (no sync here).  opt (an
        AfmOpt): the attention parameters take its rule in the same call (fmx_afm_list_step_opt) and its step count advances."""
        B = self._list_rows(idx_d, xv_d, G)
        self._call("list_", "step", hyper, rule, idx_d, xv_d, None, (B, int(G), 1.0 / B if inv_b is None else inv_b),
                   (self.logit.data_ptr(), self.loss_out.data_ptr()), opt, 1, stream)

    def list_stream(self, hyper, rule, idx_pool, xv_pool, B, G, n_steps, opt, inv_b=None, losses=None, stream=None):
        """n_steps list steps over a device-resident pool in one call (fmx_afm_list_stream; no sync here): idx_pool
        [n_pool, B G, F] int32, xv_pool the same shape in fp32 or None (ones); step s takes batch s mod n_pool.  losses: an fp32
        device tensor of n_steps elements, or None.  The table's step count and opt's advance by n_steps."""
        B, G, n_steps = int(B), _list_G(G), int(n_steps)
        n_pool = idx_pool.numel() // (B * G * self.table.n_fields)
        assert n_pool >= 1
        self._check(idx_pool, xv_pool, n_pool * B * G, outs=((losses, n_steps),))
        self._list_rows(idx_pool.reshape(n_pool, B * G, self.table.n_fields)[0], None, G)
        self._call("list_", "stream", hyper, rule, idx_pool, xv_pool, None, (n_pool, B, G, 1.0 / B if inv_b is None else inv_b, n_steps),
                   (_ptr(losses),), opt, n_steps, stream)

    def list_online_run(self, hyper, rule, idx_d, G, xv_d, opt, logits=None, losses=None, stream=None):
        """The online protocol for lists in one call (fmx_afm_list_online_run; no sync here): every list of idx_d [N G, F] is
        predicted, then fitted on alone -- N steps of list_step(B = 1, inv_b = 1), queued.  logits: an fp32 device tensor of N G
        elements for each list's logits BEFORE its update; losses: N elements; or None.  The table's step count and opt's
        advance by N."""
        N = self._list_rows(idx_d, xv_d, G, 1, lambda N: ((logits, N * int(G)), (losses, N)))
        self._call("list_", "online_run", hyper, rule, idx_d, xv_d, None, (N, int(G)), (_ptr(logits), _ptr(losses)), opt, N, stream)

    def pair_online_form(self, attn_rule):
        """-> (tile buffers, moments in LDS) of the form pair_online_run takes for this table under the attention rule
        `attn_rule` (a name of AfmOpt.RULES): tile buffers > 0 is the one-workgroup kernel, 0 the queued pair steps
        (fmx_afm_pair_online_form; no device call)."""
        mom = C.c_int32(0)
        nb = self.lib.fmx_afm_pair_online_form(self.table.c_struct(), C.byref(self.c_afm), _lib.RULES[attn_rule], C.byref(mom))
        if nb < 0:
            _lib.check(nb)
        return nb, bool(mom.value)
