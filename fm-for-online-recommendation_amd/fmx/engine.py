"""FMEngine: workspace + launch sequencing for one FlatTable (sort -> forward -> update on the current stream)."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .pairwise import n_pairs
from .table import FlatTable

class Hyper:
    """Update-rule hyper-parameters (include/fmx.h fmx_hyper_t)."""

    def __init__(self, lr=0.01, eps=1e-8, alpha=0.05, beta=1.0, l1=0.0, l2=0.0, beta1=0.9, beta2=0.999, step=0):
        self.c = _lib.Hyper(lr, eps, alpha, beta, l1, l2, beta1, beta2, int(step), 0)

    def ref(self):
        return C.byref(self.c)


def normalize_inputs(Xi, Xv, n_fields, feature_sizes=None):
    """The reference's input convention (reference fm_adam.py:35-36): nested lists (or arrays), a single sample may
    be 1-D.  Returns (idx int32 [B,F] numpy, xv float32 [B,F] numpy or None when every value is exactly 1).
    Out-of-range indices raise IndexError like nn.Embedding does."""
    idx = np.asarray(Xi, dtype=np.int64).reshape(-1, n_fields)
    xv = np.asarray(Xv, dtype=np.float32).reshape(-1, n_fields)
    if idx.shape != xv.shape:
        raise ValueError(f"Xi {idx.shape} and Xv {xv.shape} disagree")
    if feature_sizes is not None:
        sizes = np.asarray(feature_sizes, dtype=np.int64)[None, :]
        if (idx < 0).any() or (idx >= sizes).any():
            raise IndexError("index out of range in self")
    if np.all(xv == 1.0):
        xv = None
    return idx.astype(np.int32), xv


def _ptr(t):
    return None if t is None else t.data_ptr()


def _loss_cap(loss_out, n_steps):
    """loss_out (a contiguous device tensor with an element per step, or None) against the steps a call is asked for"""
    if loss_out is not None and (loss_out.numel() < n_steps or not loss_out.is_contiguous()):
        raise ValueError(f"loss_out holds {loss_out.numel()} steps, {n_steps} asked for")


def _list_G(G):
    G = int(G)
    if not 2 <= G <= _lib.LIST_MAX_G:
        raise ValueError(f"G = {G}: a list is one positive and 1 to {_lib.LIST_MAX_G - 1} negatives")
    return G


def mlp_struct(params, k, hidden, n_layers):
    """The fmx_mlp_t of a network whose flat fp32 device buffer `params` holds W_l [hidden, in_l] then b_l per layer."""
    return _lib.Mlp(params.data_ptr(), int(n_layers), int(k), int(hidden), 0)


class MlpOpt:
    """The network's optimizer state for fmx_mlp_section_opt / fmx_deepfm_stream_opt (include/fmx.h fmx_mlp_opt_t): the flat
    fp32 device tensors m, v (the layout of the flat parameter buffer; adagrad keeps its sum of squares in v), the
    hyper-parameters and the count of steps taken.  FMEngine advances `step` after each call, as it does FlatTable.step.
    rule: 'adam' (torch.optim.Adam), 'adagrad' (torch.optim.Adagrad) or 'sgd'."""

    RULES = ("sgd", "adagrad", "adam")

    def __init__(self, n_params, rule, lr=0.01, eps=None, beta1=0.9, beta2=0.999, device=None, step=0):
        if rule not in self.RULES:
            raise ValueError(f"MlpOpt: rule {rule!r} is not one of {self.RULES}")
        eps = (1e-10 if rule == "adagrad" else 1e-8) if eps is None else eps
        self.rule, self.step = rule, int(step)
        self.m = torch.zeros(int(n_params), dtype=torch.float32, device=device)
        self.v = torch.zeros_like(self.m)
        self.c = _lib.MlpOpt(self.m.data_ptr(), self.v.data_ptr(), lr, eps, beta1, beta2, _lib.RULES[rule], self.step)

    def ref(self):
        self.c.step = self.step
        return C.byref(self.c)

    def state_dict(self):
        return {"m": self.m.detach().cpu().clone(), "v": self.v.detach().cpu().clone(), "step": self.step}

    def load_state_dict(self, st):
        self.m.copy_(torch.as_tensor(st["m"], dtype=torch.float32))
        self.v.copy_(torch.as_tensor(st["v"], dtype=torch.float32))
        self.step = int(st["step"])


class HandOffTimeout(RuntimeError):
    """Device error word 2 (k_fm_update: a crossing run's row update was skipped): an in-launch hand-off ran into its spin
    bound.  Never observed; the table must be considered corrupt."""

    def __init__(self, code):
        super().__init__(f"fmx: in-launch hand-off timed out (device error word {code}); the table is not the exact result")
        self.code = code


class FMEngine:
    def __init__(self, table: FlatTable, max_batch=4096):
        if not torch.cuda.is_available():
            raise RuntimeError("fmx needs a ROCm GPU: the hot path has no CPU implementation")
        self.lib = _lib.load()
        self.table = table
        self.device = table.device
        self.max_batch = 0
        self._alloc(max_batch)

    def _alloc(self, B):
        B = int(B)
        t, dev = self.table, self.device
        t.ensure_sort_split(B)                       # large fields are cut into sort pieces when (index, sample) would not fit 32 bits
        Bp = self.lib.fmx_sorted_width(B)
        f32 = dict(dtype=torch.float32, device=dev)
        nbytes = int(self.lib.fmx_workspace_bytes(t.c_struct(), B))
        if nbytes < 0:
            _lib.check(nbytes)
        self.workspace = torch.zeros(nbytes // 4, dtype=torch.int32, device=dev)
        nsf = t.n_fields if t._sort_split is None else t._sort_split[1].numel()
        self.sorted = self.workspace[:nsf * Bp].view(nsf, Bp)     # the occurrence lists (uint32 bits), one per sort field
        self.S = torch.empty((B, t.kp), **f32)
        self.bi = torch.empty((B, t.kp), **f32)
        self.first = torch.empty((B, t.n_fields), **f32)
        self.sfirst = torch.empty(B, **f32)
        self.sbi = torch.empty(B, **f32)
        self.logit = torch.empty(B, **f32)
        self.loss_b = torch.empty(B, **f32)
        self.dz = torch.empty(B, **f32)
        self.loss_out = torch.zeros(1, **f32)
        self.error = torch.zeros(1, dtype=torch.int32, device=dev)
        self.max_batch = B

    def _steps(self, hyper):
        """A moments-layout table counts its steps (the adam rule's t - 1): the call's first step is hyper's `step`; after the
        call the table's count advances by the steps it took (_advance).  Other layouts: nothing to count."""
        if self.table.layout == "moments":
            hyper.c.step = self.table.step

    def _advance(self, n):
        if self.table.layout == "moments":
            self.table.step += int(n)

    def _counted(self, fn, args, hyper=None, n=1, mlp_opt=None):
        """One checked foreign call fn(*args) that takes n steps.  hyper (the one among args, when the call counts the table's
        steps): _steps before it, _advance(n) behind it.  mlp_opt (an MlpOpt among args, or None): its struct takes its count
        before the call and the count advances by n behind it."""
        if hyper is not None:
            self._steps(hyper)
        if mlp_opt is not None:
            mlp_opt.c.step = mlp_opt.step
        _lib.check(fn(*args))
        if hyper is not None:
            self._advance(n)
        if mlp_opt is not None:
            mlp_opt.step += n

    def _bound_run(self, fn, fixed, tail, hyper, loss_out, keep, mlp_opt=None):
        """-> run(n_steps) of a prepare_*: _counted with everything bound -- the cap check, the counters and ONE foreign call
        fn(*fixed, n_steps, *tail).  The bound structs are hyper's and mlp_opt's own: a second call continues both counts.
        `keep`: what the pointers in fixed / tail refer to, kept alive with the closure."""
        assert loss_out is None or loss_out.is_contiguous()
        check, steps, advance = _lib.check, self._steps, self._advance
        cap = None if loss_out is None else loss_out.numel()

        def run(n_steps):
            if cap is not None and n_steps > cap:
                _loss_cap(loss_out, n_steps)
            steps(hyper)
            if mlp_opt is not None:
                mlp_opt.c.step = mlp_opt.step
            check(fn(*fixed, n_steps, *tail))
            advance(n_steps)
            if mlp_opt is not None:
                mlp_opt.step += n_steps
        run.keep = keep
        return run

    def _ws_bytes(self):
        return self.workspace.numel() * self.workspace.element_size()

    def _ensure(self, B):
        if B > self.max_batch:
            self._alloc(B)

    def _stream(self, stream=None):
        """The HIP stream handle a launch goes to: `stream` (an int handle or a torch stream) when the caller already has
        it -- torch.cuda.current_stream() costs several microseconds per call -- else torch's current stream."""
        if stream is None:
            raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)   # the handle itself: ~0.3 us against ~3 for the Stream object
            if raw is not None and self.device.index is not None:
                return raw(self.device.index)
            return torch.cuda.current_stream(self.device).cuda_stream
        return stream if isinstance(stream, int) else stream.cuda_stream

    def _fwd_out(self, want_first=True, want_bi=True):
        o = _lib.FwdOut()
        o.S, o.sfirst, o.sbi, o.logit = self.S.data_ptr(), self.sfirst.data_ptr(), self.sbi.data_ptr(), self.logit.data_ptr()
        o.bi = self.bi.data_ptr() if want_bi else None
        o.first = self.first.data_ptr() if want_first else None
        o.loss, o.dz, o.error = self.loss_b.data_ptr(), self.dz.data_ptr(), self.error.data_ptr()
        return o

    # ---- device inputs ----
    def to_device(self, idx, xv=None, y=None):
        dev = self.device
        idx_d = torch.as_tensor(idx, dtype=torch.int32).to(dev).contiguous()
        xv_d = None if xv is None else torch.as_tensor(xv, dtype=torch.float32).to(dev).contiguous()
        y_d = None if y is None else torch.as_tensor(np.asarray(y, dtype=np.float32)).reshape(-1).to(dev).contiguous()
        return idx_d, xv_d, y_d

    # ---- kernels ----
    def forward(self, hyper, idx_d, xv_d=None, y_d=None, loss=None, inv_b=None, want_first=True, want_bi=True, records=None,
                stream=None):
        """records: optional [B, ld] fp32 tensor (ld >= kp + 2, multiple of 4): S, dz and loss are written as fields of one
        per-sample record (S = rec[:kp], dz = rec[kp], loss = rec[kp + 1]) instead of the engine's dense buffers."""
        B = idx_d.shape[0]
        self._ensure(B)
        key = (want_first, want_bi, None if records is None else (records.data_ptr(), records.shape[1]), self.S.data_ptr())
        cached = getattr(self, "_fwd_cache", None)
        if cached is None or cached[0] != key:     # the output struct only changes with the buffers it points at
            out = self._fwd_out(want_first, want_bi)
            if records is not None:
                kp, ld = self.table.kp, records.shape[1]
                assert ld >= kp + 2 and ld % 4 == 0 and records.is_contiguous()
                base = records.data_ptr()
                out.S, out.dz, out.loss, out.sample_ld = base, base + 4 * kp, base + 4 * (kp + 1), ld
            self._fwd_cache = cached = (key, out)
        if records is not None:
            assert records.shape[0] >= B
        inv_b = 1.0 / B if inv_b is None else inv_b
        _lib.check(self.lib.fmx_fm_forward(self.table.c_struct(), hyper.ref(), idx_d.data_ptr(), _ptr(xv_d), _ptr(y_d), B,
                                           _lib.LOSSES[loss], inv_b, C.byref(cached[1]), self._stream(stream)))
        return B

    def new_workspace(self, B):
        """A further (zero-filled) per-step workspace for batches up to B: a caller that sorts several batches ahead keeps
        one per batch in flight and passes it to sort() / update()."""
        nbytes = int(self.lib.fmx_workspace_bytes(self.table.c_struct(), B))
        return torch.zeros(nbytes // 4, dtype=torch.int32, device=self.device)

    def sort(self, idx_d, workspace=None, stream=None):
        B = idx_d.shape[0]
        self._ensure(B)
        ws = self.workspace if workspace is None else workspace
        _lib.check(self.lib.fmx_sort_occurrences(self.table.c_struct(), idx_d.data_ptr(), B, ws.data_ptr(), ws.numel() * ws.element_size(),
                                                 self.error.data_ptr(), self._stream(stream)))

    def update(self, hyper, rule, B, xv_d, dz_first, dz_bi=None, gbi=None, inv_b=None, with_loss=True, S=None, loss_b=None,
               records=None, fm_term=True, workspace=None, stream=None):
        """Row-reduced backward + fused update for the batch whose occurrences self.sort() just listed.
        S / loss_b default to the buffers the last forward() filled (a data-parallel caller passes gathered ones, or
        `records` [B, ld] as written by forward(records=...): then dz_first = dz_bi = the records' dz field)."""
        inv_b = 1.0 / B if inv_b is None else inv_b
        ld = 0
        if records is not None:
            kp, ld = self.table.kp, records.shape[1]
            base = records.data_ptr()
            S_p, dzf_p, loss_p = base, base + 4 * kp, base + 4 * (kp + 1)
            dzb_p = dzf_p if fm_term else None
        else:
            S = self.S if S is None else S
            loss_b = self.loss_b if loss_b is None else loss_b
            S_p, dzf_p, dzb_p, loss_p = S.data_ptr(), dz_first.data_ptr(), _ptr(dz_bi), loss_b.data_ptr()
        ws = self.workspace if workspace is None else workspace
        self._counted(self.lib.fmx_fm_update, (self.table.c_struct(), hyper.ref(), _lib.RULES[rule], ws.data_ptr(), ws.numel() * ws.element_size(),
                                               _ptr(xv_d), S_p, dzf_p, dzb_p, _ptr(gbi), B, ld, loss_p if with_loss else None, inv_b,
                                               self.loss_out.data_ptr() if with_loss else None, self._stream(stream)), hyper)

    def step(self, hyper, rule, loss, idx_d, xv_d, y_d, inv_b=None):
        """One pure-FM mini-batch step; the mean loss lands in self.loss_out[0] (no sync here)."""
        B = idx_d.shape[0]
        self._ensure(B)
        cached = getattr(self, "_step_out", None)
        if cached is None or cached[0] != self.S.data_ptr():       # the output struct only changes with the buffers it points at
            self._step_out = cached = (self.S.data_ptr(), self._fwd_out(want_first=False, want_bi=False))
        self._counted(self.lib.fmx_fm_step, (self.table.c_struct(), hyper.ref(), _lib.RULES[rule], _lib.LOSSES[loss], idx_d.data_ptr(),
                                             _ptr(xv_d), y_d.data_ptr(), B, 1.0 / B if inv_b is None else inv_b, self.workspace.data_ptr(),
                                             self._ws_bytes(), C.byref(cached[1]), self.loss_out.data_ptr(), self._stream()), hyper)

    def stream(self, hyper, rule, loss, idx_pool, y_pool, n_steps, loss_out=None, timed=False):
        """The online loop over a resident pool of batches (fmx_fm_stream).  Returns per-launch ms [sort, forward, update, empty event pair] when timed (the measuring mode repeats launches: see fmx.h)."""
        n_pool, B, F = idx_pool.shape
        assert F == self.table.n_fields and y_pool.shape == (n_pool, B)
        self._ensure(B)
        out = self._fwd_out(want_first=False, want_bi=False)
        ms = (C.c_float * 4)() if timed else None
        self._counted(self.lib.fmx_fm_stream, (self.table.c_struct(), hyper.ref(), _lib.RULES[rule], _lib.LOSSES[loss], idx_pool.data_ptr(),
                                               y_pool.data_ptr(), n_pool, B, 1.0 / B, n_steps, self.workspace.data_ptr(), self._ws_bytes(),
                                               C.byref(out), _ptr(loss_out), ms, self._stream()), hyper, n_steps)
        return None if ms is None else [float(v) for v in ms]

    def prepare_stream(self, hyper, rule, loss, idx_pool, y_pool, loss_out=None, stream=None):
        """-> run(n_steps): the online loop of stream() with every argument but the step count bound once (the structs, the
        device pointers and the HIP stream handle: `stream`, a torch stream or an int handle, else the stream current NOW).
        A call is then one foreign call -- what stream() spends in Python before it (building the output struct, looking up
        the current stream: tens of microseconds) is as long as two steps of the loop.  The caller keeps idx_pool, y_pool and
        loss_out alive and does not grow the engine between prepare and run."""
        n_pool, B, F = idx_pool.shape
        assert F == self.table.n_fields and y_pool.shape == (n_pool, B)
        self._ensure(B)
        out = self._fwd_out(want_first=False, want_bi=False)
        fixed = (self.table.c_struct(), hyper.ref(), _lib.RULES[rule], _lib.LOSSES[loss], idx_pool.data_ptr(), y_pool.data_ptr(),
                 n_pool, B, 1.0 / B)
        tail = (self.workspace.data_ptr(), self._ws_bytes(), C.byref(out), _ptr(loss_out), None, self._stream(stream))
        return self._bound_run(self.lib.fmx_fm_stream, fixed, tail, hyper, loss_out, (out, hyper, idx_pool, y_pool, loss_out, self.workspace))

    def prepare_deepfm_stream(self, hyper, rule, loss, params, grads, k, hidden, n_layers, lr_mlp, idx_pool, y_pool, loss_out=None,
                              stream=None, fm_term=True, mlp_opt=None):
        """-> run(n_steps): the mini-batch DeepFM loop over a resident pool (fmx_deepfm_stream), every argument but the step count
        bound once; per step forward, MLP section (SGD of the MLP applied in it: lr_mlp), table update, all issued from one call
        (fm_term=False: NFM -- the network's base is first-order + bias; weights-layout tables).
        `params` / `grads`: the flat MLP buffers (W_l then b_l per layer).  The caller keeps the tensors alive and does not grow
        the engine between prepare and run.
        mlp_opt (an MlpOpt): fmx_deepfm_stream_opt instead -- the network under mlp_opt's rule (lr_mlp is not read), the tables
        under any rule, the adaptive ones on a moments table included (NFM then takes weights or moments tables); a run advances
        the table's and mlp_opt's step counts by its steps."""
        n_pool, B, F = idx_pool.shape
        assert F == self.table.n_fields and y_pool.shape == (n_pool, B)
        self._ensure(B)
        out = self._fwd_out(want_first=False, want_bi=True)
        m = self._mlp_struct(params, k, hidden, n_layers)
        self._mlp_big_buffers(m, k, hidden, n_layers, B)
        fixed = (self.table.c_struct(), hyper.ref(), _lib.RULES[rule], C.byref(m), _lib.LOSSES[loss], int(bool(fm_term)), idx_pool.data_ptr(), y_pool.data_ptr(),
                 n_pool, B, 1.0 / B)
        keep = (out, m, hyper, mlp_opt, params, grads, idx_pool, y_pool, loss_out, self.workspace, self._mlp_ws, self._mlp_dz, self._mlp_gbi)
        ws = (self.workspace.data_ptr(), self._ws_bytes(), self._mlp_ws.data_ptr())
        bufs = (C.byref(out), self._mlp_dz.data_ptr(), self._mlp_gbi.data_ptr(), grads.data_ptr())
        if mlp_opt is not None:
            tail = (*ws, self._mlp_ws.numel() * 4, *bufs, mlp_opt.ref(), _ptr(loss_out), self._stream(stream))
            return self._bound_run(self.lib.fmx_deepfm_stream_opt, fixed, tail, hyper, loss_out, keep, mlp_opt)
        # (this path's tables are in the weights or the FTRL layout: the counters of _bound_run have nothing to count)
        return self._bound_run(self.lib.fmx_deepfm_stream, fixed, (*ws, *bufs, lr_mlp, _ptr(loss_out), self._stream(stream)), hyper, loss_out, keep)

    def prepare_deepfm_pair_stream(self, hyper, rule, params, grads, k, hidden, n_layers, lr_mlp, idx_pool, margin=0.0, loss_out=None,
                                   stream=None, fm_term=True, mlp_opt=None):
        """-> run(n_steps): prepare_deepfm_stream under the pair loss (fmx_deepfm_pair_stream) over a resident pool idx_pool
        [n_pool, 2 B_pairs, F], row 2i the positive of pair i and row 2i + 1 its negative; no labels.  mlp_opt None: the network
        under SGD by lr_mlp; an MlpOpt: its rule (lr_mlp is not read).  A run advances the table's step count (moments tables) and
        mlp_opt's by its steps.  The caller keeps the tensors alive and does not grow the engine between prepare and run."""
        n_pool, B2, F = idx_pool.shape
        assert F == self.table.n_fields and B2 % 2 == 0 and B2 >= 2 and idx_pool.is_contiguous()
        B = B2 // 2
        self._ensure(B2)
        out = self._fwd_out(want_first=False, want_bi=True)
        m = self._mlp_struct(params, k, hidden, n_layers)
        self._mlp_big_buffers(m, k, hidden, n_layers, B2)
        fixed = (self.table.c_struct(), hyper.ref(), _lib.RULES[rule], C.byref(m), int(bool(fm_term)), idx_pool.data_ptr(), n_pool, B,
                 float(margin), 1.0 / B)
        tail = (self.workspace.data_ptr(), self._ws_bytes(), self._mlp_ws.data_ptr(), self._mlp_ws.numel() * 4, C.byref(out),
                self._mlp_dz.data_ptr(), self._mlp_gbi.data_ptr(), grads.data_ptr(), float(lr_mlp),
                None if mlp_opt is None else mlp_opt.ref(), _ptr(loss_out), self._stream(stream))
        keep = (out, m, hyper, mlp_opt, params, grads, idx_pool, loss_out, self.workspace, self._mlp_ws, self._mlp_dz, self._mlp_gbi)
        return self._bound_run(self.lib.fmx_deepfm_pair_stream, fixed, tail, hyper, loss_out, keep, mlp_opt)

    def prepare_deepfm_list_stream(self, hyper, rule, params, grads, k, hidden, n_layers, lr_mlp, idx_pool, G, corr_pool=None,
                                   loss_out=None, stream=None, fm_term=True, mlp_opt=None):
        """-> run(n_steps): prepare_deepfm_stream under the list loss (fmx_deepfm_list_stream) over a resident pool idx_pool
        [n_pool, B_lists G, F], row G i the positive of list i, then its G - 1 negatives; no labels.  corr_pool (fp32
        [n_pool, B_lists G], log Q of every row's item) or None.  mlp_opt None: the network under SGD by lr_mlp; an MlpOpt: its
        rule (lr_mlp is not read).  The table workspace is the list steps' own (self._list_ws: the step workspace and the bias
        scratch behind it); the table's bias does not move.  A run advances the table's step count (moments tables) and
        mlp_opt's by its steps.  The caller keeps the tensors alive and does not grow the engine between prepare and run."""
        n_pool, rows, F = idx_pool.shape
        assert F == self.table.n_fields and idx_pool.is_contiguous()
        G = _list_G(G)
        B = self._n_lists(rows, G)
        out = self._fwd_out(want_first=False, want_bi=True)
        m = self._mlp_struct(params, k, hidden, n_layers)
        self._mlp_big_buffers(m, k, hidden, n_layers, rows)
        fixed = (self.table.c_struct(), hyper.ref(), _lib.RULES[rule], C.byref(m), int(bool(fm_term)), idx_pool.data_ptr(), n_pool, B, G,
                 None if corr_pool is None else self._corr(corr_pool, (n_pool, rows)), 1.0 / B)
        tail = (self._list_ws.data_ptr(), self._list_ws.numel() * 4, self._mlp_ws.data_ptr(), self._mlp_ws.numel() * 4, C.byref(out),
                self._mlp_dz.data_ptr(), self._mlp_gbi.data_ptr(), grads.data_ptr(), float(lr_mlp),
                None if mlp_opt is None else mlp_opt.ref(), _ptr(loss_out), self._stream(stream))
        keep = (out, m, hyper, mlp_opt, params, grads, idx_pool, corr_pool, loss_out, self._list_ws, self._mlp_ws, self._mlp_dz, self._mlp_gbi)
        return self._bound_run(self.lib.fmx_deepfm_list_stream, fixed, tail, hyper, loss_out, keep, mlp_opt)

    # ---- the small fused MLP (online steps of DeepFM / NFM / ONN); shapes beyond its limits raise FmxError(UNSUPPORTED) ----
    MLP_MAX_B, MLP_MAX_W, MLP_MAX_L = 16, 64, 8

    @staticmethod
    def mlp_fits(B, k, hidden, n_layers, mode):
        ok = B <= 16 and hidden <= 64 and 1 <= n_layers <= 8
        if mode == "fit":
            return ok and k <= 63
        if mode == "hedge":
            return ok and k + n_layers <= 64
        return ok and k <= 64

    _mlp_struct = staticmethod(mlp_struct)

    def mlp_forward(self, params, k, hidden, n_layers, base, B, want_layers):
        out = torch.empty(B, dtype=torch.float32, device=self.device)
        layers = torch.empty((n_layers, B), dtype=torch.float32, device=self.device) if want_layers else None
        m = self._mlp_struct(params, k, hidden, n_layers)
        _lib.check(self.lib.fmx_mlp_forward(C.byref(m), self.bi.data_ptr(), self.table.kp, base.data_ptr(), B, out.data_ptr(),
                                            _ptr(layers), self._stream()))
        return out, layers

    def mlp_fit(self, params, k, hidden, n_layers, hyper, rule, loss, base, y_d, B, inv_b=None, mlp_opt=None):
        """-> (dz [B], gbi [B, kp]) for self.update(); the hidden layers in `params` are updated in place.
        mlp_opt (an MlpOpt): fmx_mlp_fit_opt instead -- the hidden layers under mlp_opt's rule (`rule` and hyper's lr / eps are
        not read); mlp_opt.step advances by one."""
        dz = torch.empty(B, dtype=torch.float32, device=self.device)
        gbi = torch.empty((B, self.table.kp), dtype=torch.float32, device=self.device)
        m = self._mlp_struct(params, k, hidden, n_layers)
        args = (_lib.LOSSES[loss], self.bi.data_ptr(), self.table.kp, base.data_ptr(), y_d.data_ptr(), B, 1.0 / B if inv_b is None else inv_b,
                dz.data_ptr(), gbi.data_ptr(), self.loss_out.data_ptr())
        if mlp_opt is None:
            self._counted(self.lib.fmx_mlp_fit, (C.byref(m), hyper.ref(), _lib.RULES[rule], *args, self._stream()))
        else:
            self._counted(self.lib.fmx_mlp_fit_opt, (C.byref(m), hyper.ref(), *args, mlp_opt.ref(), self._stream()), mlp_opt=mlp_opt)
        return dz, gbi

    def mlp_pair_fit(self, params, k, hidden, n_layers, hyper, rule, base, B_pairs, margin=0.0, inv_b=None, mlp_opt=None,
                     want_logit=False):
        """mlp_fit under the pair loss (fmx_mlp_pair_fit) on self.bi's first 2 B_pairs rows, row 2i the positive of pair i and
        row 2i + 1 its negative; no labels.  -> (dz [2 B_pairs] with dz[2i + 1] = -dz[2i], gbi [2 B_pairs, kp], logit [2 B_pairs]
        or None) for self.update(); the mean pair loss lands in self.loss_out[0]; the hidden layers in `params` are updated in
        place under `rule`, or under mlp_opt's rule (an MlpOpt: `rule` and hyper are not read, mlp_opt.step advances by one)."""
        B2 = 2 * int(B_pairs)
        dz = torch.empty(B2, dtype=torch.float32, device=self.device)
        gbi = torch.empty((B2, self.table.kp), dtype=torch.float32, device=self.device)
        logit = torch.empty(B2, dtype=torch.float32, device=self.device) if want_logit else None
        m = self._mlp_struct(params, k, hidden, n_layers)
        self._counted(self.lib.fmx_mlp_pair_fit, (C.byref(m), hyper.ref(), _lib.RULES[rule], self.bi.data_ptr(), self.table.kp,
                                                  base.data_ptr(), int(B_pairs), float(margin), 1.0 / B_pairs if inv_b is None else inv_b,
                                                  _ptr(logit), dz.data_ptr(), gbi.data_ptr(), self.loss_out.data_ptr(),
                                                  None if mlp_opt is None else mlp_opt.ref(), self._stream()), mlp_opt=mlp_opt)
        return dz, gbi, logit

    def mlp_list_fit(self, params, k, hidden, n_layers, hyper, rule, base, B_lists, G, inv_b=None, corr=None, mlp_opt=None,
                     want_logit=False, want_rank=False):
        """mlp_fit under the list loss (fmx_mlp_list_fit) on self.bi's first B_lists G rows (at most 16), row G i the positive of
        list i, then its G - 1 negatives; no labels.  corr (fp32 [B_lists G], log Q of every row's item) or None: the softmax runs
        on logit - corr.  -> (dz [B_lists G], gbi [B_lists G, kp], logit [B_lists G] or None: the UNCORRECTED logits, rank uint8
        [B_lists] or None: the negatives of list i whose logit is >= its positive's) for self.list_sort_update(); the mean list
        loss lands in self.loss_out[0]; the hidden layers in `params` are updated in place under `rule`, or under mlp_opt's rule
        (an MlpOpt: `rule` and hyper are not read, mlp_opt.step advances by one)."""
        B_lists, G = int(B_lists), _list_G(G)
        rows = B_lists * G
        dz = torch.empty(rows, dtype=torch.float32, device=self.device)
        gbi = torch.empty((rows, self.table.kp), dtype=torch.float32, device=self.device)
        logit = torch.empty(rows, dtype=torch.float32, device=self.device) if want_logit else None
        rank = torch.empty(B_lists, dtype=torch.uint8, device=self.device) if want_rank else None
        m = self._mlp_struct(params, k, hidden, n_layers)
        self._counted(self.lib.fmx_mlp_list_fit, (C.byref(m), hyper.ref(), _lib.RULES[rule], self.bi.data_ptr(), self.table.kp,
                                                  base.data_ptr(), None if corr is None else self._corr(corr, (rows,)), B_lists, G,
                                                  1.0 / B_lists if inv_b is None else inv_b, _ptr(logit), dz.data_ptr(), gbi.data_ptr(),
                                                  self.loss_out.data_ptr(), _ptr(rank), None if mlp_opt is None else mlp_opt.ref(),
                                                  self._stream()), mlp_opt=mlp_opt)
        return dz, gbi, logit, rank

    def mlp_hedge_fit(self, params, k, hidden, n_layers, lr, hedge_b, hedge_s, alpha, base, y_d, B):
        m = self._mlp_struct(params, k, hidden, n_layers)
        _lib.check(self.lib.fmx_mlp_hedge_fit(C.byref(m), lr, hedge_b, hedge_s, alpha.data_ptr(), self.bi.data_ptr(),
                                              self.table.kp, base.data_ptr(), y_d.data_ptr(), B, None, self._stream()))

    def online_run(self, hyper, rule, loss, idx_d, xv_d, y_d, want_loss=False):
        """The reference's online protocol for pure FM on N device-resident samples (fmx_fm_online_run): per sample
        predict, then fit on that sample.  -> (pred uint8 [N], loss [N] or None)."""
        N = idx_d.shape[0]
        pred = torch.empty(N, dtype=torch.uint8, device=self.device)
        loss_b = torch.empty(N, dtype=torch.float32, device=self.device) if want_loss else None
        self._counted(self.lib.fmx_fm_online_run, (self.table.c_struct(), hyper.ref(), _lib.RULES[rule], _lib.LOSSES[loss], idx_d.data_ptr(),
                                                   _ptr(xv_d), y_d.data_ptr(), N, pred.data_ptr(), _ptr(loss_b), self.error.data_ptr(),
                                                   self._stream()), hyper, N)
        return pred, loss_b

    # ---- pairwise-ranking (BPR) training: idx_d [2B, F], row 2i the positive of pair i, row 2i + 1 the negative (fmx/pairwise.py) ----
    _n_pairs = staticmethod(n_pairs)

    def pair_forward(self, hyper, idx_d, xv_d=None, margin=0.0, inv_b=None, want_first=False, want_bi=False, stream=None):
        """fmx_fm_pair_forward on B pairs: S / sfirst / sbi / logit of the 2B rows, and the pair loss and its dlogit in
        self.loss_b / self.dz (loss_b[2i] = loss_i, loss_b[2i + 1] = 0, dz[2i + 1] = -dz[2i]).  -> B"""
        B = self._n_pairs(idx_d)
        self._ensure(2 * B)
        out = self._fwd_out(want_first, want_bi)
        _lib.check(self.lib.fmx_fm_pair_forward(self.table.c_struct(), hyper.ref(), idx_d.data_ptr(), _ptr(xv_d), B, float(margin),
                                                1.0 / B if inv_b is None else inv_b, C.byref(out), self._stream(stream)))
        return B

    def pair_step(self, hyper, rule, idx_d, xv_d=None, margin=0.0, inv_b=None):
        """One pair step on B pairs (fmx_fm_pair_step); the mean pair loss lands in self.loss_out[0] (no sync here)."""
        B = self._n_pairs(idx_d)
        self._ensure(2 * B)
        cached = getattr(self, "_step_out", None)
        if cached is None or cached[0] != self.S.data_ptr():
            self._step_out = cached = (self.S.data_ptr(), self._fwd_out(want_first=False, want_bi=False))
        self._counted(self.lib.fmx_fm_pair_step, (self.table.c_struct(), hyper.ref(), _lib.RULES[rule], idx_d.data_ptr(), _ptr(xv_d), B,
                                                  float(margin), 1.0 / B if inv_b is None else inv_b, self.workspace.data_ptr(),
                                                  self._ws_bytes(), C.byref(cached[1]), self.loss_out.data_ptr(), self._stream()), hyper)

    def pair_stream(self, hyper, rule, idx_pool, n_steps, margin=0.0, loss_out=None):
        """n_steps pair steps over a resident pool idx_pool [n_pool, 2B, F] (fmx_fm_pair_stream); loss_out [n_steps] or None."""
        n_pool, B2, F = idx_pool.shape
        assert F == self.table.n_fields and B2 % 2 == 0 and idx_pool.is_contiguous()
        _loss_cap(loss_out, n_steps)
        B = B2 // 2
        self._ensure(B2)
        out = self._fwd_out(want_first=False, want_bi=False)
        self._counted(self.lib.fmx_fm_pair_stream, (self.table.c_struct(), hyper.ref(), _lib.RULES[rule], idx_pool.data_ptr(), n_pool, B,
                                                    float(margin), 1.0 / B, int(n_steps), self.workspace.data_ptr(), self._ws_bytes(),
                                                    C.byref(out), _ptr(loss_out), self._stream()), hyper, n_steps)

    # ---- listwise (sampled-softmax) training: idx_d [B G, F], row G i the positive of list i, then its G - 1 negatives ----
    def _n_lists(self, rows, G):
        """-> B for B G rows; grows the buffers, and keeps the list steps' own workspace, self._list_ws, sized through
        fmx_fm_list_workspace_bytes (the step workspace and the scratch behind it that the bias rule of a list step runs on).
        The other calls' workspace and the buffers' allocation are left as they are."""
        G = _list_G(G)
        if rows < G or rows % G:
            raise ValueError(f"list rows must be [B G, F] with B >= 1 and G = {G}, got {rows} rows")
        self._ensure(rows)
        need = int(self.lib.fmx_fm_list_workspace_bytes(self.table.c_struct(), rows // G, G))
        if need < 0:
            _lib.check(need)
        ws = getattr(self, "_list_ws", None)
        if ws is None or need > ws.numel() * 4:
            self._list_ws = torch.zeros(need // 4, dtype=torch.int32, device=self.device)     # (zero-filled once, as the header asks)
        return rows // G

    @staticmethod
    def _corr(corr, shape):
        """The corrections of the corrected list calls (fmx_fm_list_*_q): one fp32 per row, contiguous, on the device"""
        if corr.dtype != torch.float32 or tuple(corr.shape) != tuple(shape) or not corr.is_contiguous():
            raise ValueError(f"corr: a contiguous float32 tensor of shape {tuple(shape)}, got {corr.dtype} {tuple(corr.shape)}")
        return corr.data_ptr()

    def list_forward(self, hyper, idx_d, G, xv_d=None, inv_b=None, want_first=False, want_bi=False, stream=None):
        """fmx_fm_list_forward on B lists of G rows: S / sfirst / sbi / logit of the B G rows, and the softmax cross-entropy of
        every list against its first row and its dlogit in self.loss_b / self.dz (loss_b[G i] = loss_i, 0 in the negatives'
        slots).  -> B"""
        return self._list_forward(hyper, idx_d, G, xv_d, None, inv_b, want_first, want_bi, stream)

    def list_forward_q(self, hyper, idx_d, G, corr, xv_d=None, inv_b=None, want_first=False, want_bi=False, stream=None):
        """fmx_fm_list_forward_q: list_forward with the softmax taken over logit - corr (corr fp32 [B G], log Q of every row's
        item); self.logit and the sums stay the uncorrected forward's.  -> B"""
        return self._list_forward(hyper, idx_d, G, xv_d, corr, inv_b, want_first, want_bi, stream)

    def _list_forward(self, hyper, idx_d, G, xv_d, corr, inv_b, want_first, want_bi, stream):
        if idx_d.dim() != 2:
            raise ValueError(f"list rows must be [B G, F], got {tuple(idx_d.shape)}")
        B = self._n_lists(idx_d.shape[0], G)
        out = self._fwd_out(want_first, want_bi)
        fn, q = (self.lib.fmx_fm_list_forward, ()) if corr is None else (self.lib.fmx_fm_list_forward_q, (self._corr(corr, idx_d.shape[:1]),))
        _lib.check(fn(self.table.c_struct(), hyper.ref(), idx_d.data_ptr(), _ptr(xv_d), *q, B, int(G),
                      1.0 / B if inv_b is None else inv_b, C.byref(out), self._stream(stream)))
        return B

    def list_step(self, hyper, rule, idx_d, G, xv_d=None, inv_b=None):
        """One list step on B lists of G rows (fmx_fm_list_step); the mean list loss lands in self.loss_out[0] (no sync here).
        The table's bias is not touched."""
        self._list_step(hyper, rule, idx_d, G, xv_d, None, inv_b)

    def list_step_q(self, hyper, rule, idx_d, G, corr, xv_d=None, inv_b=None):
        """fmx_fm_list_step_q: list_step under the log-Q corrected loss (corr fp32 [B G], see list_forward_q)."""
        self._list_step(hyper, rule, idx_d, G, xv_d, corr, inv_b)

    def _list_step(self, hyper, rule, idx_d, G, xv_d, corr, inv_b):
        if idx_d.dim() != 2:
            raise ValueError(f"list rows must be [B G, F], got {tuple(idx_d.shape)}")
        B = self._n_lists(idx_d.shape[0], G)
        out = self._fwd_out(want_first=False, want_bi=False)
        fn, q = (self.lib.fmx_fm_list_step, ()) if corr is None else (self.lib.fmx_fm_list_step_q, (self._corr(corr, idx_d.shape[:1]),))
        self._counted(fn, (self.table.c_struct(), hyper.ref(), _lib.RULES[rule], idx_d.data_ptr(), _ptr(xv_d), *q, B, int(G),
                           1.0 / B if inv_b is None else inv_b, self._list_ws.data_ptr(), self._list_ws.numel() * 4, C.byref(out),
                           self.loss_out.data_ptr(), self._stream()), hyper)

    def list_stream(self, hyper, rule, idx_pool, G, n_steps, loss_out=None):
        """n_steps list steps over a resident pool idx_pool [n_pool, B G, F] (fmx_fm_list_stream); loss_out [n_steps] or None."""
        self._list_stream(hyper, rule, idx_pool, G, None, n_steps, loss_out)

    def list_stream_q(self, hyper, rule, idx_pool, G, corr_pool, n_steps, loss_out=None):
        """fmx_fm_list_stream_q: list_stream under the corrected loss, corr_pool fp32 [n_pool, B G] beside idx_pool."""
        self._list_stream(hyper, rule, idx_pool, G, corr_pool, n_steps, loss_out)

    def _list_stream(self, hyper, rule, idx_pool, G, corr_pool, n_steps, loss_out):
        n_pool, rows, F = idx_pool.shape
        assert F == self.table.n_fields and idx_pool.is_contiguous()
        _loss_cap(loss_out, n_steps)
        B = self._n_lists(rows, G)
        out = self._fwd_out(want_first=False, want_bi=False)
        fn, q = ((self.lib.fmx_fm_list_stream, ()) if corr_pool is None
                 else (self.lib.fmx_fm_list_stream_q, (self._corr(corr_pool, idx_pool.shape[:2]),)))
        self._counted(fn, (self.table.c_struct(), hyper.ref(), _lib.RULES[rule], idx_pool.data_ptr(), *q, n_pool, B, int(G), 1.0 / B,
                           int(n_steps), self._list_ws.data_ptr(), self._list_ws.numel() * 4, C.byref(out), _ptr(loss_out),
                           self._stream()), hyper, n_steps)

    # ---- in-batch sampled softmax: idx_d [B, F], every row's negatives are the other rows' items (fmx_fm_inbatch_*) ----
    def _inbatch(self, B, item_fields, bank=None):
        """-> (the item fields as the C calls take them: a host int32 array, its length); grows the buffers and keeps the in-batch
        steps' own workspace, self._inbatch_ws, sized through fmx_fm_inbatch_workspace_bytes (with a bank:
        fmx_fm_inbatch_bank_workspace_bytes, which is never smaller)."""
        fields = [int(f) for f in item_fields]
        self._ensure(B)
        if bank is None:
            need = int(self.lib.fmx_fm_inbatch_workspace_bytes(self.table.c_struct(), int(B), len(fields)))
        else:
            need = int(self.lib.fmx_fm_inbatch_bank_workspace_bytes(self.table.c_struct(), int(B), int(bank.capacity), len(fields)))
        if need < 0:
            _lib.check(need)
        ws = getattr(self, "_inbatch_ws", None)
        if ws is None or need > ws.numel() * 4:
            self._inbatch_ws = torch.zeros(need // 4, dtype=torch.int32, device=self.device)     # (zero-filled once, as the header asks)
        return (C.c_int32 * len(fields))(*fields), len(fields)

    @staticmethod
    def _keys(key, shape):
        if key.dtype != torch.int32 or tuple(key.shape) != tuple(shape) or not key.is_contiguous():
            raise ValueError(f"key: a contiguous int32 tensor of shape {tuple(shape)}, got {key.dtype} {tuple(key.shape)}")
        return key.data_ptr()

    def _inbatch_out(self):
        o = _lib.FwdOut()
        o.loss, o.error = self.loss_b.data_ptr(), self.error.data_ptr()
        return o

    def inbatch_step(self, hyper, rule, idx_d, item_fields, xv_d=None, corr=None, key=None, inv_b=None):
        """One in-batch step on the B rows of idx_d [B, F] (fmx_fm_inbatch_step): the softmax of every row's own item against the
        other rows' items; corr fp32 [B] (log Q of every row's item) or None, key int32 [B] (equal keys: the same item, left out
        of each other's softmax) or None.  The mean loss lands in self.loss_out[0], the rows' losses in self.loss_b (no sync
        here).  The table's bias is not touched."""
        if idx_d.dim() != 2 or idx_d.shape[1] != self.table.n_fields:
            raise ValueError(f"in-batch rows must be [B, {self.table.n_fields}], got {tuple(idx_d.shape)}")
        B = idx_d.shape[0]
        fields, n = self._inbatch(B, item_fields)
        out = self._inbatch_out()
        self._counted(self.lib.fmx_fm_inbatch_step,
                      (self.table.c_struct(), hyper.ref(), _lib.RULES[rule], idx_d.data_ptr(), _ptr(xv_d), fields, n,
                       None if corr is None else self._corr(corr, (B,)), None if key is None else self._keys(key, (B,)), B,
                       1.0 / B if inv_b is None else inv_b, self._inbatch_ws.data_ptr(), self._inbatch_ws.numel() * 4, C.byref(out),
                       self.loss_out.data_ptr(), self._stream()), hyper)

    def inbatch_stream(self, hyper, rule, idx_pool, item_fields, n_steps, corr_pool=None, key_pool=None, loss_out=None):
        """n_steps in-batch steps over a resident pool idx_pool [n_pool, B, F] (fmx_fm_inbatch_stream) with corr_pool fp32 /
        key_pool int32 [n_pool, B] or None; loss_out [n_steps] or None."""
        n_pool, B, F = idx_pool.shape
        assert F == self.table.n_fields and idx_pool.is_contiguous()
        _loss_cap(loss_out, n_steps)
        fields, n = self._inbatch(B, item_fields)
        out = self._inbatch_out()
        self._counted(self.lib.fmx_fm_inbatch_stream,
                      (self.table.c_struct(), hyper.ref(), _lib.RULES[rule], idx_pool.data_ptr(), fields, n,
                       None if corr_pool is None else self._corr(corr_pool, (n_pool, B)),
                       None if key_pool is None else self._keys(key_pool, (n_pool, B)), n_pool, B, 1.0 / B, int(n_steps),
                       self._inbatch_ws.data_ptr(), self._inbatch_ws.numel() * 4, C.byref(out), _ptr(loss_out), self._stream()),
                      hyper, n_steps)

    def inbatch_bank_step(self, hyper, rule, idx_d, item_fields, bank, xv_d=None, corr=None, key=None, inv_b=None):
        """inbatch_step with a fmx.pairwise.ItemBank (fmx_fm_inbatch_bank_step): the bank's items are further negatives of every
        row, and the step's own items are pushed into it behind the update.  corr / key are given exactly when the bank keeps
        them (the C call refuses a mismatch); the keys must mean the same item in every batch (fmx.pairwise.item_keys)."""
        if idx_d.dim() != 2 or idx_d.shape[1] != self.table.n_fields:
            raise ValueError(f"in-batch rows must be [B, {self.table.n_fields}], got {tuple(idx_d.shape)}")
        B = idx_d.shape[0]
        fields, n = self._inbatch(B, item_fields, bank)
        out = self._inbatch_out()
        self._counted(self.lib.fmx_fm_inbatch_bank_step,
                      (self.table.c_struct(), hyper.ref(), _lib.RULES[rule], idx_d.data_ptr(), _ptr(xv_d), fields, n,
                       None if corr is None else self._corr(corr, (B,)), None if key is None else self._keys(key, (B,)),
                       bank.c_struct(), B, 1.0 / B if inv_b is None else inv_b, self._inbatch_ws.data_ptr(),
                       self._inbatch_ws.numel() * 4, C.byref(out), self.loss_out.data_ptr(), self._stream()), hyper)

    def inbatch_bank_stream(self, hyper, rule, idx_pool, item_fields, n_steps, bank, corr_pool=None, key_pool=None, loss_out=None):
        """inbatch_stream with a fmx.pairwise.ItemBank (fmx_fm_inbatch_bank_stream): every step reads the bank and pushes its
        items."""
        n_pool, B, F = idx_pool.shape
        assert F == self.table.n_fields and idx_pool.is_contiguous()
        _loss_cap(loss_out, n_steps)
        fields, n = self._inbatch(B, item_fields, bank)
        out = self._inbatch_out()
        self._counted(self.lib.fmx_fm_inbatch_bank_stream,
                      (self.table.c_struct(), hyper.ref(), _lib.RULES[rule], idx_pool.data_ptr(), fields, n,
                       None if corr_pool is None else self._corr(corr_pool, (n_pool, B)),
                       None if key_pool is None else self._keys(key_pool, (n_pool, B)), bank.c_struct(), n_pool, B, 1.0 / B,
                       int(n_steps), self._inbatch_ws.data_ptr(), self._inbatch_ws.numel() * 4, C.byref(out), _ptr(loss_out),
                       self._stream()), hyper, n_steps)

    def alias_sample(self, thresh, alias, logq, n_neg, n_try, own_pos=None, seed=0, offset=0, u_base=0, excl_offsets=None,
                     excl_pos=None, U=None):
        """fmx_alias_sample_negatives on this engine's stream: n_neg popularity-sampled negatives per row from the alias table
        (thresh uint32 bits in an int32 tensor [N], alias int32 [N], logq fp32 [N] or None; fmx.pairwise.alias_table) ->
        (neg_pos int32 [U, n_neg], -1 padded; neg_logq fp32 [U, n_neg], -inf padded, or None without logq).  U: own_pos's length
        unless given.  No sync."""
        from . import pairwise
        return pairwise.alias_sample(thresh, alias, logq, n_neg, n_try, own_pos, seed, offset, u_base, excl_offsets, excl_pos, U,
                                     stream=self._stream(), call=self._counted)

    def pair_online_run(self, hyper, rule, idx_d, xv_d=None, margin=0.0, want_logit=False, want_loss=False):
        """The online protocol on N device-resident pairs (fmx_fm_pair_online_run): per pair predict (z_pos > z_neg), then one
        pair step on that pair.  -> (pred uint8 [N], logit [2N] or None, loss [N] or None)."""
        N = self._n_pairs(idx_d)
        pred = torch.empty(N, dtype=torch.uint8, device=self.device)
        logit = torch.empty(2 * N, dtype=torch.float32, device=self.device) if want_logit else None
        loss_b = torch.empty(N, dtype=torch.float32, device=self.device) if want_loss else None
        self._counted(self.lib.fmx_fm_pair_online_run, (self.table.c_struct(), hyper.ref(), _lib.RULES[rule], idx_d.data_ptr(), _ptr(xv_d),
                                                        N, float(margin), pred.data_ptr(), _ptr(logit), _ptr(loss_b),
                                                        self.error.data_ptr(), self._stream()), hyper, N)
        return pred, logit, loss_b

    def list_online_run(self, hyper, rule, idx_d, G, xv_d=None, want_logit=False, want_loss=False):
        """The online protocol on N device-resident lists of G rows (fmx_fm_list_online_run): per list the positive's rank among
        its negatives (0: first), then one list step on that list.  -> (rank uint8 [N], logit [N G] or None, loss [N] or None);
        no sync.  The table's step count advances by N."""
        G = _list_G(G)
        if idx_d.dim() != 2 or idx_d.shape[0] % G:
            raise ValueError(f"list rows must be [N G, F] with G = {G}, got {tuple(idx_d.shape)}")
        N = idx_d.shape[0] // G
        rank = torch.empty(N, dtype=torch.uint8, device=self.device)
        logit = torch.empty(N * G, dtype=torch.float32, device=self.device) if want_logit else None
        loss_b = torch.empty(N, dtype=torch.float32, device=self.device) if want_loss else None
        self._counted(self.lib.fmx_fm_list_online_run, (self.table.c_struct(), hyper.ref(), _lib.RULES[rule], idx_d.data_ptr(), _ptr(xv_d),
                                                        N, G, rank.data_ptr(), _ptr(logit), _ptr(loss_b), self.error.data_ptr(),
                                                        self._stream()), hyper, N)
        return rank, logit, loss_b

    def list_online_run_fits(self, F, kp):
        """Does fmx_fm_list_online_run take this table?  fmx_fm_online_run's field limit, plain fields, and no sort split (the
        order of a list step's additions follows positions counted per sort piece)."""
        t = self.table
        return self.online_run_fits(F, kp) and not t.mapped and t._sort_split is None

    def online_run_mlp(self, hyper, rule, loss, params, k, hidden, n_layers, hedge, fm_term, hedge_b, hedge_s, alpha,
                       idx_d, xv_d, y_d, mlp_opt=None):
        """The online protocol for the classes with an MLP (fmx_online_run_mlp) -> forward() value per sample [N].
        mlp_opt (an MlpOpt; fit mode only): fmx_online_run_mlp_opt instead -- the network under mlp_opt's rule, the tables under
        any rule, the adaptive ones on a moments table included; the call advances mlp_opt.step and, on a moments table, the
        table's step count by N."""
        N = idx_d.shape[0]
        self._ensure(1)
        out = self._fwd_out(want_first=False, want_bi=True)
        m = self._mlp_struct(params, k, hidden, n_layers)
        pred = torch.empty(N, dtype=torch.float32, device=self.device)
        if getattr(self, "_online_scratch", None) is None:
            self._online_scratch = torch.zeros(self.table.kp + 8, dtype=torch.float32, device=self.device)
        head = (self.table.c_struct(), hyper.ref(), _lib.RULES[rule], _lib.LOSSES[loss], C.byref(m))
        tail = (idx_d.data_ptr(), _ptr(xv_d), y_d.data_ptr(), N, self.workspace.data_ptr(), self._ws_bytes(), C.byref(out),
                self._online_scratch.data_ptr(), pred.data_ptr())
        if mlp_opt is not None:
            if hedge:
                raise ValueError("online_run_mlp: mlp_opt is for the fit mode (Hedge has a rule of its own)")
            self._counted(self.lib.fmx_online_run_mlp_opt, (*head, 1 if fm_term else 0, *tail, mlp_opt.ref(), self._stream()), hyper, N, mlp_opt)
        else:       # (tables in the weights or the FTRL layout: no step count)
            self._counted(self.lib.fmx_online_run_mlp, (*head, 1 if hedge else 0, 1 if fm_term else 0, hedge_b, hedge_s, _ptr(alpha), *tail,
                                                        self._stream()))
        return pred

    def online_run_mlp_pair(self, hyper, rule, params, k, hidden, n_layers, fm_term, idx_d, xv_d=None, margin=0.0, mlp_opt=None,
                            want_logit=False, want_loss=False):
        """The online protocol on N device-resident pairs through the whole network of DeepFM / NFM (fmx_online_run_mlp_pair):
        idx_d [2N, F], row 2i the positive of pair i and row 2i + 1 its negative; per pair predict (z_pos > z_neg), then one pair
        step on that pair.  -> (pred uint8 [N], logit [2N] or None, loss [N] or None).  mlp_opt None: the network under `rule`
        ('signadam' / 'sgd'); an MlpOpt: its rule, and the tables under any rule.  The call advances the table's step count (on
        a moments table) and mlp_opt.step by N."""
        N = self._n_pairs(idx_d)
        self._ensure(2)
        out = self._fwd_out(want_first=False, want_bi=True)
        m = self._mlp_struct(params, k, hidden, n_layers)
        pred = torch.empty(N, dtype=torch.uint8, device=self.device)
        logit = torch.empty(2 * N, dtype=torch.float32, device=self.device) if want_logit else None
        loss_b = torch.empty(N, dtype=torch.float32, device=self.device) if want_loss else None
        if getattr(self, "_pair_online_scratch", None) is None:
            self._pair_online_scratch = torch.zeros(2 * self.table.kp + 8, dtype=torch.float32, device=self.device)
        self._counted(self.lib.fmx_online_run_mlp_pair, (self.table.c_struct(), hyper.ref(), _lib.RULES[rule], C.byref(m),
                                                         1 if fm_term else 0, idx_d.data_ptr(), _ptr(xv_d), N, float(margin),
                                                         self.workspace.data_ptr(), self._ws_bytes(), C.byref(out),
                                                         self._pair_online_scratch.data_ptr(), pred.data_ptr(), _ptr(logit), _ptr(loss_b),
                                                         None if mlp_opt is None else mlp_opt.ref(), self._stream()), hyper, N, mlp_opt)
        return pred, logit, loss_b

    def online_run_mlp_list(self, hyper, rule, params, k, hidden, n_layers, fm_term, idx_d, G, xv_d=None, corr=None, mlp_opt=None,
                            want_logit=False, want_loss=False):
        """The online protocol on N device-resident lists of G rows through the whole network of DeepFM / NFM
        (fmx_online_run_mlp_list): idx_d [N G, F], row G i the positive of list i, then its G - 1 negatives; per list the
        positive's rank among that step's own uncorrected logits (0: first), then one list step of tables and network on that
        list.  corr (fp32 [N G], log Q of every row's item) or None.  -> (rank uint8 [N], logit [N G] or None, loss [N] or None);
        no sync.  One workgroup walks the stream at G <= 8 (and a network of at most 8,192 parameters); longer lists are queued
        launches -- the same bits.  mlp_opt None: the network under `rule` ('signadam' / 'sgd'); an MlpOpt: its rule, and the tables under any
        rule.  The call advances the table's step count (on a moments table) and mlp_opt.step by N; the bias does not move."""
        G = _list_G(G)
        if idx_d.dim() != 2 or idx_d.shape[0] % G:
            raise ValueError(f"list rows must be [N G, F] with G = {G}, got {tuple(idx_d.shape)}")
        N = idx_d.shape[0] // G
        self._n_lists(G, G)         # the buffers of one list, and the list steps' own workspace
        out = self._fwd_out(want_first=False, want_bi=True)
        m = self._mlp_struct(params, k, hidden, n_layers)
        rank = torch.empty(N, dtype=torch.uint8, device=self.device)
        logit = torch.empty(N * G, dtype=torch.float32, device=self.device) if want_logit else None
        loss_b = torch.empty(N, dtype=torch.float32, device=self.device) if want_loss else None
        if getattr(self, "_list_online_scratch", None) is None:     # dz [16], then gbi [16, kp]: every G
            self._list_online_scratch = torch.zeros(16 + 16 * self.table.kp, dtype=torch.float32, device=self.device)
        self._counted(self.lib.fmx_online_run_mlp_list, (self.table.c_struct(), hyper.ref(), _lib.RULES[rule], C.byref(m),
                                                         1 if fm_term else 0, idx_d.data_ptr(), _ptr(xv_d),
                                                         None if corr is None else self._corr(corr, (N * G,)), N, G,
                                                         self._list_ws.data_ptr(), self._list_ws.numel() * 4, C.byref(out),
                                                         self._list_online_scratch.data_ptr(), rank.data_ptr(), _ptr(logit), _ptr(loss_b),
                                                         None if mlp_opt is None else mlp_opt.ref(), self._stream()), hyper, N, mlp_opt)
        return rank, logit, loss_b

    @staticmethod
    def online_run_fits(n_fields, kp):
        return n_fields <= 4 * (64 // (kp // 4))

    def _mlp_big_buffers(self, m, k, hidden, n_layers, B):
        key = (k, hidden, n_layers, B)
        if getattr(self, "_mlp_ws_key", None) != key:
            nbytes = int(self.lib.fmx_mlp_section_workspace_bytes(C.byref(m), B))
            if nbytes < 0:
                raise _lib.FmxError(nbytes, self.lib.fmx_last_error_string().decode())
            self._mlp_ws = torch.empty(nbytes // 4, dtype=torch.float32, device=self.device)
            self._mlp_dz = torch.empty(B, dtype=torch.float32, device=self.device)
            self._mlp_gbi = torch.empty((B, self.table.kp), dtype=torch.float32, device=self.device)
            self._mlp_loss = torch.zeros(1, dtype=torch.float32, device=self.device)
            self._mlp_logit = torch.empty(B, dtype=torch.float32, device=self.device)      # mlp_pair_section's logit_out
            self._mlp_ws_key = key

    def mlp_forward_batch(self, params, k, hidden, n_layers, bi, base, B, want_layers):
        """forward() of the MLP at mini-batch sizes (fmx_mlp_forward_batch) -> (logit [B], layers [L, B] or None)."""
        m = self._mlp_struct(params, k, hidden, n_layers)
        self._mlp_big_buffers(m, k, hidden, n_layers, B)
        out = torch.empty(B, dtype=torch.float32, device=self.device)
        layers = torch.empty((n_layers, B), dtype=torch.float32, device=self.device) if want_layers else None
        _lib.check(self.lib.fmx_mlp_forward_batch(C.byref(m), bi.data_ptr(), bi.stride(0), base.data_ptr(), B,
                                                  self._mlp_ws.data_ptr(), out.data_ptr(), _ptr(layers), self._stream()))
        return out, layers

    def mlp_hedge_section(self, params, grads, k, hidden, n_layers, lr, hedge_b, hedge_s, alpha, bi, base, y_d, B):
        """Hedge backprop at mini-batch sizes (fmx_mlp_hedge_section): hidden layers and alpha updated in place."""
        m = self._mlp_struct(params, k, hidden, n_layers)
        self._mlp_big_buffers(m, k, hidden, n_layers, B)
        _lib.check(self.lib.fmx_mlp_hedge_section(C.byref(m), lr, hedge_b, hedge_s, alpha.data_ptr(), bi.data_ptr(),
                                                  bi.stride(0), base.data_ptr(), y_d.data_ptr(), B, self._mlp_ws.data_ptr(),
                                                  grads.data_ptr(), None, self._stream()))

    def mlp_section(self, params, grads, k, hidden, n_layers, loss, bi, base, y_d, B, inv_b, lr_apply=0.0, mlp_opt=None):
        """The MLP on `bi` at mini-batch sizes (fmx_mlp_section: fp32 MFMA GEMMs): forward, loss, backward.
        -> (loss [1], dz [B], gbi [B, kp]); `grads` (flat, the layout of `params`) is filled; lr_apply != 0 also applies SGD.
        mlp_opt (an MlpOpt): fmx_mlp_section_opt instead -- the network's rule is mlp_opt's (lr_apply is not read), applied in
        the same pass; mlp_opt.step advances by one."""
        m = self._mlp_struct(params, k, hidden, n_layers)
        self._mlp_big_buffers(m, k, hidden, n_layers, B)
        head = (C.byref(m), _lib.LOSSES[loss], bi.data_ptr(), bi.stride(0), base.data_ptr(), y_d.data_ptr(), B, inv_b, self._mlp_ws.data_ptr())
        bufs = (None, self._mlp_dz.data_ptr(), self._mlp_gbi.data_ptr(), self.table.kp, grads.data_ptr())
        if mlp_opt is None:
            self._counted(self.lib.fmx_mlp_section, (*head, *bufs, lr_apply, self._mlp_loss.data_ptr(), self._stream()))
        else:
            self._counted(self.lib.fmx_mlp_section_opt, (*head, self._mlp_ws.numel() * 4, *bufs, mlp_opt.ref(), self._mlp_loss.data_ptr(),
                                                         self._stream()), mlp_opt=mlp_opt)
        return self._mlp_loss, self._mlp_dz, self._mlp_gbi

    def mlp_pair_section(self, params, grads, k, hidden, n_layers, bi, base, B_pairs, inv_b=None, margin=0.0, lr_apply=0.0,
                         mlp_opt=None):
        """mlp_section under the pair loss (fmx_mlp_pair_section): `bi` [2 B_pairs, ld] and `base` [2 B_pairs] hold row 2i = the
        positive of pair i, row 2i + 1 = its negative; no labels.  -> (loss [1] = the mean pair loss, dz [2 B_pairs] with
        dz[2i + 1] = -dz[2i], gbi [2 B_pairs, kp], logit [2 B_pairs]: the whole network's logits, fmx_mlp_section's bits).
        `grads` is filled; lr_apply != 0 also applies SGD; mlp_opt (an MlpOpt): its rule instead, and its step advances by one."""
        B_pairs = int(B_pairs)
        if B_pairs < 1 or bi.shape[0] < 2 * B_pairs or base.numel() < 2 * B_pairs:
            raise ValueError(f"mlp_pair_section: bi {tuple(bi.shape)} / base {tuple(base.shape)} do not hold 2 x {B_pairs} rows")
        m = self._mlp_struct(params, k, hidden, n_layers)
        self._mlp_big_buffers(m, k, hidden, n_layers, 2 * B_pairs)
        self._counted(self.lib.fmx_mlp_pair_section, (C.byref(m), bi.data_ptr(), bi.stride(0), base.data_ptr(), B_pairs, float(margin),
                                                      1.0 / B_pairs if inv_b is None else inv_b, self._mlp_ws.data_ptr(),
                                                      self._mlp_ws.numel() * 4, self._mlp_logit.data_ptr(), self._mlp_dz.data_ptr(),
                                                      self._mlp_gbi.data_ptr(), self.table.kp, grads.data_ptr(), lr_apply,
                                                      None if mlp_opt is None else mlp_opt.ref(), self._mlp_loss.data_ptr(),
                                                      self._stream()), mlp_opt=mlp_opt)
        return self._mlp_loss, self._mlp_dz, self._mlp_gbi, self._mlp_logit

    def mlp_list_section(self, params, grads, k, hidden, n_layers, bi, base, B_lists, G, inv_b=None, corr=None, lr_apply=0.0,
                         mlp_opt=None):
        """mlp_section under the list loss (fmx_mlp_list_section): `bi` [B_lists G, ld] and `base` [B_lists G] hold row G i = the
        positive of list i, then its G - 1 negatives; no labels.  corr (fp32 [B_lists G], log Q of every row's item) or None: the
        softmax runs on logit - corr.  -> (loss [1] = the mean list loss, dz [B_lists G], gbi [B_lists G, kp], logit [B_lists G]:
        the whole network's UNCORRECTED logits, fmx_mlp_forward_batch's bits).  `grads` is filled; lr_apply != 0 also applies SGD;
        mlp_opt (an MlpOpt): its rule instead, and its step advances by one.  The option "mlp_chain" does not reach this call."""
        B_lists, G = int(B_lists), _list_G(G)
        rows = B_lists * G
        if B_lists < 1 or bi.shape[0] < rows or base.numel() < rows:
            raise ValueError(f"mlp_list_section: bi {tuple(bi.shape)} / base {tuple(base.shape)} do not hold {B_lists} x {G} rows")
        m = self._mlp_struct(params, k, hidden, n_layers)
        self._mlp_big_buffers(m, k, hidden, n_layers, rows)
        self._counted(self.lib.fmx_mlp_list_section, (C.byref(m), bi.data_ptr(), bi.stride(0), base.data_ptr(),
                                                      None if corr is None else self._corr(corr, (rows,)), B_lists, G,
                                                      1.0 / B_lists if inv_b is None else inv_b, self._mlp_ws.data_ptr(),
                                                      self._mlp_ws.numel() * 4, self._mlp_logit.data_ptr(), self._mlp_dz.data_ptr(),
                                                      self._mlp_gbi.data_ptr(), self.table.kp, grads.data_ptr(), lr_apply,
                                                      None if mlp_opt is None else mlp_opt.ref(), self._mlp_loss.data_ptr(),
                                                      self._stream()), mlp_opt=mlp_opt)
        return self._mlp_loss, self._mlp_dz, self._mlp_gbi, self._mlp_logit

    def list_sort_update(self, hyper, rule, idx_d, G, xv_d, dz_first, dz_bi=None, gbi=None, inv_b=None, stream=None):
        """sort() and update() of a list step put together from the engine's calls (the classes' fit_lists(full=True)): both on
        the list steps' own workspace, and the update on a copy of the table struct whose bias points at the scratch behind
        that workspace -- what fmx_fm_list_step and fmx_deepfm_list_stream hand k_fm_update, so that the bias rule runs on
        scratch and the table's bias and its state stay bit-unchanged.  S is the last forward's; no loss is reduced."""
        rows = idx_d.shape[0]
        B = self._n_lists(rows, G)
        ws = self._list_ws
        self.sort(idx_d, workspace=ws, stream=stream)
        step_bytes = int(self.lib.fmx_workspace_bytes(self.table.c_struct(), rows))
        t = _lib.Table()
        C.memmove(C.byref(t), self.table.c_struct(), C.sizeof(t))
        t.bias = ws.data_ptr() + step_bytes
        self._counted(self.lib.fmx_fm_update, (C.byref(t), hyper.ref(), _lib.RULES[rule], ws.data_ptr(), ws.numel() * 4, _ptr(xv_d),
                                               self.S.data_ptr(), dz_first.data_ptr(), _ptr(dz_bi), _ptr(gbi), rows, 0, None,
                                               1.0 / B if inv_b is None else inv_b, None, self._stream(stream)), hyper)

    def check_error_flag(self):
        """The device-side error word (include/fmx.h, Conventions): 1 -> IndexError like nn.Embedding; 2 -> HandOffTimeout
        (an in-launch hand-off ran into its spin bound: the table is no longer the exact result).  Synchronises."""
        code = int(self.error.item())
        if code != 0:
            self.error.zero_()
            if code == 1:
                raise IndexError("index out of range in self (flagged by the fmx kernels)")
            raise HandOffTimeout(code)
