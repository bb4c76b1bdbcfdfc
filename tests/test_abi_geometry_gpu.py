"""Every table geometry the C ABI accepts (include/fmx.h: kp, z_offset, row_stride, `rows` aligned to 16 bytes and no more),
run on the MI355X inside guard bands (tests/abi_geometry.py).

A table's geometry changes addresses and nothing else: launch shapes and summation orders depend on B, F, kp and the sort, the
host code only copies row_stride / z_offset into the kernel arguments.  So every entry point is called twice on the same
inputs -- on a default-geometry fmx.FlatTable and on a GuardedTable holding the same live floats at another geometry -- and

  * every output is the same bits (outputs live in guarded buffers of exactly the size the header names),
  * the live floats of the guarded table are the bits of the FlatTable's rows, its bias likewise,
  * both guards, the lead, every dead float of every row, and the words behind the workspace (of exactly
    fmx_workspace_bytes / fmx_afm_workspace_bytes / fmx_mlp_section_workspace_bytes bytes) and the outputs keep their bits,
  * components k..kp stay +0 and the error word is 0.

Bit-identity compares the code with itself, so fmx_fm_step is also checked, at every geometry, against the float64 step the
suite already owns (oracle.fm_oracle.flat_fm_step_f64; test_adaptive_rules_cpu.flat_adaptive_step) with the existing floors.

Every pointer handed to a kernel lies inside an allocation this file owns, with the pattern around it: a kernel that addresses
wrongly scribbles on the test's own memory and fails an assertion.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import abi_geometry as ag
from helpers import assert_ftrl_step_within_f64, assert_within_f64
from oracle import fm_oracle as orc
from test_adaptive_rules_cpu import flat_adaptive_step
from test_adaptive_rules_gpu import HYP as ADAPTIVE_HYP, assert_step

pytestmark = pytest.mark.gpu

SIZES = [3, 9, 1000, 50000, 4, 17, 200, 31, 7, 2, 1]          # hot fields of 1, 2, 3 rows (long runs) beside a large one
K_OF = {4: 4, 8: 7, 16: 16, 32: 24, 64: 61}                   # k == kp and k < kp both occur for every layout
LAYOUTS = ("weights", "ftrl", "moments")
RULES = {"weights": ("signadam", "sgd"), "ftrl": ("ftrl",), "moments": ("adagrad", "adam")}
FTRL = dict(alpha=0.05, beta=1.0, l1=0.001, l2=0.01)
STEP0 = 5                                                     # the steps a moments table has taken: adam runs t = 6
B0 = 300


def geometry(layout, kp, name):
    """-> dict(z_offset, row_stride, lead)"""
    dzo, dstride = ag.default_geometry(layout, kp)
    if name == "min":
        zo, lead = kp + 4, 4
        stride = ag.need(layout, kp, zo)
    elif name == "padded":                                    # 16 bytes past a multiple of 8 floats
        zo, lead = dzo + 4, 0
        stride = ag.need(layout, kp, zo) + 12
    else:                                                     # "wide"
        zo, lead, stride = dzo, 4, 2 * dstride + 4
    return dict(z_offset=None if layout == "weights" else zo, row_stride=stride, lead=lead)


GEOMS = [(layout, kp, name) for layout in LAYOUTS for kp in (4, 8, 16, 32, 64) for name in ("min", "padded")]
GEOMS += [(layout, 16, "wide") for layout in LAYOUTS]
GEOM_IDS = [f"{g[0]}-kp{g[1]}-{g[2]}" for g in GEOMS]


@pytest.fixture(scope="module")
def fmx():
    import fmx as _fmx
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _fmx


# ---------------------------------------------------------------------------------------------------------------
# tables and problems
# ---------------------------------------------------------------------------------------------------------------
def hyper_of(fmx, rule):
    if rule in ("adam", "adagrad"):
        h = ADAPTIVE_HYP[rule]
        return fmx.Hyper(lr=h["lr"], eps=h["eps"], beta1=h["beta1"], beta2=h["beta2"], step=STEP0, **FTRL)
    return fmx.Hyper(lr=0.01, eps=1e-8, **FTRL)


def master_table(fmx, layout, k, sizes=SIZES, seed=0, mapped=None):
    """A default-geometry FlatTable with every live float non-trivial."""
    rng = np.random.default_rng(seed)
    kw = dict(field_cols=mapped[0], field_base=mapped[1], n_cols=mapped[2]) if mapped else {}
    t = fmx.FlatTable(sizes, k, layout=layout, ftrl=FTRL if layout == "ftrl" else None, **kw)
    R, kp, zo = t.n_rows, t.kp, t.z_offset
    V = (rng.normal(size=(R, k)) * 0.3).astype(np.float32)
    w = (rng.normal(size=R) * 0.3).astype(np.float32)
    if layout == "ftrl":
        t.load_ftrl_state(orc.ftrl_z_for_weight(V, **FTRL), rng.uniform(0.05, 0.2, size=(R, k)).astype(np.float32),
                          orc.ftrl_z_for_weight(w, **FTRL), rng.uniform(0.05, 0.2, size=R).astype(np.float32))
        t.bias[0], t.bias[1] = 0.4, 0.3
    else:
        t.rows[:, :k] = torch.from_numpy(V).cuda()
        t.rows[:, kp] = torch.from_numpy(w).cuda()
        t.bias[0] = 0.37
    if layout == "moments":
        t.rows[:, zo:zo + k] = torch.from_numpy((rng.normal(size=(R, k)) * 1e-3).astype(np.float32)).cuda()
        t.rows[:, zo + kp:zo + kp + k] = torch.from_numpy(rng.uniform(1e-7, 1e-5, size=(R, k)).astype(np.float32)).cuda()
        t.rows[:, kp + 1] = torch.from_numpy((rng.normal(size=R) * 1e-3).astype(np.float32)).cuda()
        t.rows[:, kp + 2] = torch.from_numpy(rng.uniform(1e-7, 1e-5, size=R).astype(np.float32)).cuda()
        t.bias[1], t.bias[2] = 1e-3, 2e-6
    t._make = (sizes, k, layout, kw)
    return t


def clone_flat(fmx, m):
    sizes, k, layout, kw = m._make
    t = fmx.FlatTable(sizes, k, layout=layout, ftrl=FTRL if layout == "ftrl" else None, **kw)
    t.rows.copy_(m.rows)
    t.bias.copy_(m.bias)
    return t


def guarded_of(m, geom):
    sizes, k, layout, kw = m._make
    return ag.GuardedTable(sizes, k, m.kp, layout, **geom, **kw).load_from(m)


def problem(sizes, B, seed, n_cols=None):
    """Zipf-skewed indices (long runs in the hot fields), real x in [-1, 1] with about 10 % exact zeros."""
    rng = np.random.default_rng(seed)
    idx = np.stack([np.minimum(rng.zipf(1.3, size=B) - 1, s - 1) for s in sizes], axis=1).astype(np.int32)
    x = rng.uniform(-1, 1, size=idx.shape).astype(np.float32)
    x[rng.uniform(size=x.shape) < 0.1] = 0.0
    y = (rng.uniform(size=B) < 0.3).astype(np.float32)
    return idx, x, y


def dev(a, dtype=None):
    t = torch.as_tensor(a)
    return (t if dtype is None else t.to(dtype)).cuda().contiguous()


def _p(t):
    return None if t is None else t.data_ptr()


# ---------------------------------------------------------------------------------------------------------------
# one call of an entry point on a table (FlatTable or GuardedTable): -> {name: int32 bits} of its outputs
# ---------------------------------------------------------------------------------------------------------------
class Call:
    def __init__(self, fmx, tab):
        self.fmx, self.L, self.lib, self.tab = fmx, fmx._lib, fmx._lib.load(), tab
        self.g = ag.GuardSet()
        self.err = self.g.new("error", 1, torch.int32, out=True)
        self.extra = {}

    def fwd_out(self, B, names):
        o = self.L.FwdOut()
        kp, F = self.tab.kp, self.tab.n_fields
        shapes = dict(S=(B, kp), bi=(B, kp), first=(B, F), sfirst=(B,), sbi=(B,), logit=(B,), loss=(B,), dz=(B,))
        self.bufs = {}
        for n in names:
            self.bufs[n] = self.g.new(n, shapes[n], out=True)
            setattr(o, n, self.bufs[n].ptr)
        o.error = self.err.ptr
        return o

    def workspace(self, B=None, nbytes=None, name="workspace"):
        if nbytes is None:
            nbytes = int(self.lib.fmx_workspace_bytes(self.tab.c_struct(), B))
        assert nbytes > 0, self.lib.fmx_last_error_string()
        return self.g.raw(name, nbytes)

    def ok(self, rc):
        assert rc == 0, (rc, self.lib.fmx_last_error_string().decode())

    def done(self):
        torch.cuda.synchronize()
        self.g.check()
        out = self.g.outputs()
        assert int(out["error"][0]) == 0, f"device error word {int(out['error'][0])}"
        out.update({k_: ag.bits(v) for k_, v in self.extra.items()})
        return out


def run_forward(fmx, tab, P, with_x, loss):
    idx, x, y = P
    c = Call(fmx, tab)
    B = idx.shape[0]
    o = c.fwd_out(B, ("S", "bi", "first", "sfirst", "sbi", "logit", "loss", "dz"))
    idx_d, x_d, y_d = dev(idx), dev(x) if with_x else None, dev(y)
    torch.cuda.synchronize()
    c.ok(c.lib.fmx_fm_forward(tab.c_struct(), hyper_of(fmx, None).ref(), idx_d.data_ptr(), _p(x_d), y_d.data_ptr(), B, c.L.LOSSES[loss],
                              1.0 / B, C.byref(o), None))
    return c.done()


def run_part_finish(fmx, tab, P, with_x=True):
    idx, x, y = P
    c = Call(fmx, tab)
    B, kp = idx.shape[0], tab.kp
    rec = 2 * kp + 4
    parts = c.g.new("parts", (B, rec), out=True)
    o = c.fwd_out(B, ("S", "bi", "sfirst", "sbi", "logit", "loss", "dz"))
    idx_d, x_d, y_d = dev(idx), dev(x) if with_x else None, dev(y)
    h = hyper_of(fmx, None)
    torch.cuda.synchronize()
    c.ok(c.lib.fmx_fm_forward_partial(tab.c_struct(), idx_d.data_ptr(), _p(x_d), B, 1, 1, B, parts.ptr, c.err.ptr, None))
    c.ok(c.lib.fmx_fm_forward_finish(h.ref(), tab.bias.data_ptr(), ag.LAYOUT_IDS[tab.layout], kp, parts.ptr, B * rec, 1, y_d.data_ptr(), B,
                                     c.L.LOSSES["logits"], 1.0 / B, C.byref(o), None))
    return c.done()


def run_step(fmx, tab, P, rule, loss="logits", with_x=True):
    idx, x, y = P
    c = Call(fmx, tab)
    B = idx.shape[0]
    o = c.fwd_out(B, ("S", "loss", "dz"))
    ws = c.workspace(B)
    loss_out = c.g.new("loss_out", 1, out=True)
    idx_d, x_d, y_d = dev(idx), dev(x) if with_x else None, dev(y)
    torch.cuda.synchronize()
    c.ok(c.lib.fmx_fm_step(tab.c_struct(), hyper_of(fmx, rule).ref(), c.L.RULES[rule], c.L.LOSSES[loss], idx_d.data_ptr(), _p(x_d),
                           y_d.data_ptr(), B, 1.0 / B, ws.ptr, ws.nbytes, C.byref(o), loss_out.ptr, None))
    return c.done()


def run_stream(fmx, tab, pool, rule):
    c = Call(fmx, tab)
    n_pool, B = len(pool), pool[0][0].shape[0]
    o = c.fwd_out(B, ("S", "loss", "dz"))
    ws = c.workspace(B)
    loss_out = c.g.new("loss_out", n_pool, out=True)
    idx_d, y_d = dev(np.stack([p[0] for p in pool])), dev(np.stack([p[2] for p in pool]))
    torch.cuda.synchronize()
    c.ok(c.lib.fmx_fm_stream(tab.c_struct(), hyper_of(fmx, rule).ref(), c.L.RULES[rule], c.L.LOSSES["logits"], idx_d.data_ptr(),
                             y_d.data_ptr(), n_pool, B, 1.0 / B, n_pool, ws.ptr, ws.nbytes, C.byref(o), loss_out.ptr, None, None))
    return c.done()


def run_update(fmx, tab, P, rule, occ):
    """fmx_sort_occurrences + fmx_fm_forward + fmx_fm_update with a network gradient g_bi (occ=False) or fmx_fm_update_occ with
    explicit per-occurrence gradients (occ=True)."""
    idx, x, y = P
    c = Call(fmx, tab)
    B, kp, k, F = idx.shape[0], tab.kp, tab.k, tab.n_fields
    o = c.fwd_out(B, ("S", "loss", "dz"))
    ws = c.workspace(B)
    loss_out = c.g.new("loss_out", 1, out=True)
    rng = np.random.default_rng(B + kp)
    idx_d, x_d, y_d = dev(idx), dev(x), dev(y)
    h = hyper_of(fmx, rule)
    t = tab.c_struct()
    torch.cuda.synchronize()
    c.ok(c.lib.fmx_sort_occurrences(t, idx_d.data_ptr(), B, ws.ptr, ws.nbytes, c.err.ptr, None))
    c.ok(c.lib.fmx_fm_forward(t, h.ref(), idx_d.data_ptr(), x_d.data_ptr(), y_d.data_ptr(), B, c.L.LOSSES["logits"], 1.0 / B,
                              C.byref(o), None))
    S, lb, dz = c.bufs["S"], c.bufs["loss"], c.bufs["dz"]
    if occ:
        E = np.zeros((B, F, kp), np.float32)
        E[:, :, :k] = rng.normal(size=(B, F, k)) * 1e-3          # (components k..kp carry no gradient: they stay zero)
        E_g = c.g.new("occ_grad", (B, F * kp), src=E.reshape(B, F * kp))
        c.ok(c.lib.fmx_fm_update_occ(t, h.ref(), c.L.RULES[rule], ws.ptr, ws.nbytes, x_d.data_ptr(), dz.ptr, E_g.ptr, F * kp, B, lb.ptr,
                                     1.0 / B, loss_out.ptr, None))
    else:
        gbi = c.g.new("gbi", (B, kp), src=rng.normal(size=(B, kp)).astype(np.float32) * 1e-3)
        c.ok(c.lib.fmx_fm_update(t, h.ref(), c.L.RULES[rule], ws.ptr, ws.nbytes, x_d.data_ptr(), S.ptr, dz.ptr, dz.ptr, gbi.ptr, B, 0,
                                 lb.ptr, 1.0 / B, loss_out.ptr, None))
    return c.done()


def run_online(fmx, tab, P, rule, loss="logits"):
    idx, x, y = P
    c = Call(fmx, tab)
    N = idx.shape[0]
    pred = c.g.new("pred", N, torch.uint8, out=True)
    lo = c.g.new("loss", N, out=True)
    idx_d, x_d, y_d = dev(idx), dev(x), dev(y)
    torch.cuda.synchronize()
    c.ok(c.lib.fmx_fm_online_run(tab.c_struct(), hyper_of(fmx, rule).ref(), c.L.RULES[rule], c.L.LOSSES[loss], idx_d.data_ptr(),
                                 x_d.data_ptr(), y_d.data_ptr(), N, pred.ptr, lo.ptr, c.err.ptr, None))
    return c.done()


def mlp_params(k, hidden, layers, seed):
    rng = np.random.default_rng(seed)
    n = sum(hidden * (k if l == 0 else hidden) + hidden for l in range(layers))
    return (rng.normal(size=n) * 0.2).astype(np.float32)


def run_online_mlp(fmx, tab, P, rule, hedge, fm_term, hidden=8, layers=2):
    idx, x, y = P
    c = Call(fmx, tab)
    N, kp, k = idx.shape[0], tab.kp, tab.k
    p0 = mlp_params(k, hidden, layers, 3)
    params = c.g.new("params", len(p0), out=True, src=p0)
    m = c.L.Mlp(params.ptr, layers, k, hidden, 0)
    alpha = c.g.new("alpha", layers, out=True, src=np.full(layers, 1.0 / layers, np.float32))
    o = c.L.FwdOut()
    for n, shape in (("S", (1, kp)), ("bi", (1, kp)), ("sfirst", (1,)), ("logit", (1,))):
        setattr(o, n, c.g.new(n, shape, out=True).ptr)
    o.error = c.err.ptr
    ws = c.workspace(1)
    scratch = c.g.new("scratch", kp + 8, out=True)
    pred = c.g.new("pred", N, out=True)
    idx_d, x_d, y_d = dev(idx), dev(x), dev(y)
    torch.cuda.synchronize()
    c.ok(c.lib.fmx_online_run_mlp(tab.c_struct(), hyper_of(fmx, None).ref(), c.L.RULES[rule], c.L.LOSSES["logits"], C.byref(m),
                                  1 if hedge else 0, 1 if fm_term else 0, 0.99, 0.2, alpha.ptr, idx_d.data_ptr(), x_d.data_ptr(),
                                  y_d.data_ptr(), N, ws.ptr, ws.nbytes, C.byref(o), scratch.ptr, pred.ptr, None))
    return c.done()


def run_deepfm_stream(fmx, tab, pool, rule, fm_term, hidden=32, layers=2):
    c = Call(fmx, tab)
    n_pool, B, kp, k = len(pool), pool[0][0].shape[0], tab.kp, tab.k
    p0 = mlp_params(k, hidden, layers, 4)
    params = c.g.new("params", len(p0), out=True, src=p0)
    grads = c.g.new("grads", len(p0), out=True)
    m = c.L.Mlp(params.ptr, layers, k, hidden, 0)
    o = c.fwd_out(B, ("S", "bi", "sfirst", "logit"))
    ws = c.workspace(B)
    mlp_bytes = int(c.lib.fmx_mlp_section_workspace_bytes(C.byref(m), B))
    mlp_ws = c.workspace(nbytes=mlp_bytes, name="mlp_workspace")
    dz, gbi = c.g.new("dz", B, out=True), c.g.new("gbi", (B, kp), out=True)
    loss_out = c.g.new("loss_out", n_pool, out=True)
    idx_d, y_d = dev(np.stack([p[0] for p in pool])), dev(np.stack([p[2] for p in pool]))
    torch.cuda.synchronize()
    c.ok(c.lib.fmx_deepfm_stream(tab.c_struct(), hyper_of(fmx, rule).ref(), c.L.RULES[rule], C.byref(m), c.L.LOSSES["logits"],
                                 1 if fm_term else 0, idx_d.data_ptr(), y_d.data_ptr(), n_pool, B, 1.0 / B, n_pool, ws.ptr, ws.nbytes,
                                 mlp_ws.ptr, C.byref(o), dz.ptr, gbi.ptr, grads.ptr, 0.01, loss_out.ptr, None))
    return c.done()


def afm_params(k, t, seed=6):
    return (np.random.default_rng(seed).normal(size=t * k + 2 * t + k) * 0.3).astype(np.float32)


def run_afm(fmx, tab, P, what, rule=None, t=8):
    idx, x, y = P
    c = Call(fmx, tab)
    B, kp, k, F = idx.shape[0], tab.kp, tab.k, tab.n_fields
    p0 = afm_params(k, t)
    params = c.g.new("params", len(p0), out=True, src=p0)
    afm = c.L.Afm(params.ptr, k, t)
    idx_d, x_d, y_d = dev(idx), dev(x), dev(y)
    h = hyper_of(fmx, rule)
    tc = tab.c_struct()
    if what == "forward":
        logit, loss = c.g.new("logit", B, out=True), c.g.new("loss", B, out=True)
        torch.cuda.synchronize()
        c.ok(c.lib.fmx_afm_forward(tc, C.byref(afm), h.ref(), idx_d.data_ptr(), x_d.data_ptr(), y_d.data_ptr(), B, c.L.LOSSES["logits"],
                                   1.0 / B, logit.ptr, loss.ptr, c.err.ptr, None))
    elif what == "step":
        nbytes = int(c.lib.fmx_afm_workspace_bytes(tc, C.byref(afm), B))
        ws = c.workspace(nbytes=nbytes)
        grad, loss_out = c.g.new("attn_grad", len(p0), out=True), c.g.new("loss_out", 1, out=True)
        torch.cuda.synchronize()
        c.ok(c.lib.fmx_afm_step(tc, h.ref(), c.L.RULES[rule], C.byref(afm), idx_d.data_ptr(), x_d.data_ptr(), y_d.data_ptr(), B, 1.0 / B,
                                ws.ptr, ws.nbytes, grad.ptr, loss_out.ptr, c.err.ptr, None))
    else:
        sel = [0, 2, 3, 5, F - 1]
        fields = (C.c_int32 * len(sel))(*sel)
        E, stats = c.g.new("E", (B, len(sel), kp), out=True), c.g.new("stats", (B, 4), out=True)
        torch.cuda.synchronize()
        c.ok(c.lib.fmx_afm_side(tc, C.byref(afm), h.ref(), idx_d.data_ptr(), x_d.data_ptr(), B, fields, len(sel), 1, E.ptr, stats.ptr,
                                c.err.ptr, None))
    return c.done()


def run_owner_step(fmx, tab, P, rule):
    """fmx_owner_prefetch + fmx_owner_step with one rank: nothing is exchanged, the receive buffers are the send buffers."""
    idx, _, y = P
    c = Call(fmx, tab)
    B, kp = idx.shape[0], tab.kp
    ws = c.workspace(B)
    send = c.g.new("parts", (B, 2 * kp + 4), out=True)
    rec = c.g.new("rec", (B, kp + 4), out=True)
    loss_out = c.g.new("loss_out", 1, out=True)
    bufs = c.L.OwnerBufs(send.ptr, send.ptr, rec.ptr, rec.ptr)
    idx_d, y_d = dev(idx), dev(y)
    comm = C.c_void_p()
    c.ok(c.lib.fmx_comm_create(None, 0, 1, None, 0, C.byref(comm)))
    try:
        torch.cuda.synchronize()
        tc = tab.c_struct()
        c.ok(c.lib.fmx_owner_prefetch(comm, tc, idx_d.data_ptr(), B, 0, None, ws.ptr, ws.nbytes, c.err.ptr, None))
        c.ok(c.lib.fmx_owner_step(comm, tc, hyper_of(fmx, rule).ref(), c.L.RULES[rule], c.L.LOSSES["logits"], idx_d.data_ptr(),
                                  y_d.data_ptr(), B, 0, ws.ptr, ws.nbytes, C.byref(bufs), loss_out.ptr, c.err.ptr, None))
        return c.done()
    finally:
        torch.cuda.synchronize()
        c.lib.fmx_comm_destroy(comm)


# ---------------------------------------------------------------------------------------------------------------
# the comparison
# ---------------------------------------------------------------------------------------------------------------
def both(fmx, master, geom, run, what):
    """run(table) on a default-geometry copy of `master` and on a guarded table at `geom` holding the same live floats.
    -> (the FlatTable after the call, the guarded table after the call, the outputs)."""
    flat, gt = clone_flat(fmx, master), guarded_of(master, geom)
    a, b = run(flat), run(gt)
    assert a.keys() == b.keys()
    for name in a:
        np.testing.assert_array_equal(b[name], a[name], err_msg=f"{what}: output {name} differs from the default geometry's")
    gt.assert_live_equals(flat, what)
    gt.assert_dead_untouched(what)
    gt.assert_zero_components(what)
    return flat, gt, a


def f32(bits_):
    return np.ascontiguousarray(bits_).view(np.float32)


def state_of(layout, k, kp, rows, bias):
    """The oracle's state names from rows in the DEFAULT geometry (float32 [R, stride]) and the bias."""
    zo, _ = ag.default_geometry(layout, kp)
    d = np.float64
    if layout == "weights":
        return dict(V=rows[:, :k].copy(), w=rows[:, kp].copy(), bias=np.float32(bias[0]))
    if layout == "ftrl":
        return dict(zV=rows[:, zo:zo + k].copy(), nV=rows[:, zo + kp:zo + kp + k].copy(), zw=rows[:, kp + 1].copy(),
                    nw=rows[:, kp + 2].copy(), zb=np.float32(bias[0]), nb=np.float32(bias[1]))
    return dict(V=rows[:, :k].astype(d), w=rows[:, kp].astype(d), bias=d(bias[0]), mV=rows[:, zo:zo + k].astype(d),
                vV=rows[:, zo + kp:zo + kp + k].astype(d), mw=rows[:, kp + 1].astype(d), vw=rows[:, kp + 2].astype(d),
                mb=d(bias[1]), vb=d(bias[2]))


def anchor_step_f64(master, gt, out, P, rule, what):
    """The guarded table after fmx_fm_step against the float64 step from the master's state, with the suite's floors."""
    idx, x, y = P
    layout, k, kp = master.layout, master.k, master.kp
    offs = master.offsets_host
    rows = idx.astype(np.int64) + offs[:-1][None, :]
    before = state_of(layout, k, kp, master.rows.cpu().numpy(), master.bias.cpu().numpy())
    after = state_of(layout, k, kp, f32(gt.live()), gt.bias.cpu().numpy())
    loss = float(f32(out["loss_out"])[0])
    if layout == "moments":
        h = ADAPTIVE_HYP[rule]
        ref, urows, ex = flat_adaptive_step(before, rows, x, y, "logits", rule, h, STEP0 + 1)
        assert_step(before, after, ref, urows, ex, rule, h, STEP0 + 1, what=what)
        return
    if layout == "ftrl":
        ref = orc.flat_fm_step_f64(before, rows, x, y, "logits", "ftrl", FTRL)
        assert_within_f64(loss, ref["loss"], ref["floor"]["loss"], f"{what}: loss")
        assert_ftrl_step_within_f64(after, ref, what=f"{what}: ", before=before)
        return
    ref = orc.flat_fm_step_f64(before, rows, x, y, "logits", rule, dict(lr=0.01))
    u, new, fl = ref["urows"], ref["new"], ref["floor"]
    assert_within_f64(loss, ref["loss"], fl["loss"], f"{what}: loss")
    assert_within_f64(after["V"][u], new["V"][u], fl["V"], f"{what}: V")
    assert_within_f64(after["w"][u], new["w"][u], fl["w"], f"{what}: w")
    assert_within_f64(after["bias"], new["bias"], fl["bias"], f"{what}: bias")
    mask = np.ones(len(before["w"]), bool)
    mask[u] = False
    np.testing.assert_array_equal(after["V"][mask], before["V"][mask], err_msg=f"{what}: untouched rows moved")
    np.testing.assert_array_equal(after["w"][mask], before["w"][mask], err_msg=f"{what}: untouched rows moved")


# ---------------------------------------------------------------------------------------------------------------
# the tests
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,kp,name", GEOMS, ids=GEOM_IDS)
def test_every_entry_point_at_this_geometry(fmx, layout, kp, name):
    k = K_OF[kp]
    geom = geometry(layout, kp, name)
    gt0 = ag.GuardedTable([1], k, kp, layout, **geom)
    assert int(fmx._lib.load().fmx_workspace_bytes(gt0.c_struct(), B0)) > 0, "check_table refuses a geometry the header allows"
    if geom["lead"]:
        assert gt0.rows.data_ptr() % 32 == 16
    master = master_table(fmx, layout, k, seed=kp)
    P = problem(SIZES, B0, seed=100 + kp)
    tag = f"{layout} kp={kp} {name}"
    for with_x in (True, False):
        for loss in ("logits", "sigmoid"):
            both(fmx, master, geom, lambda t: run_forward(fmx, t, P, with_x, loss), f"{tag}: fmx_fm_forward x={with_x} {loss}")
    both(fmx, master, geom, lambda t: run_part_finish(fmx, t, P), f"{tag}: fmx_fm_forward_partial + _finish")
    for rule in RULES[layout]:
        _, gt, out = both(fmx, master, geom, lambda t: run_step(fmx, t, P, rule), f"{tag}: fmx_fm_step {rule}")
        anchor_step_f64(master, gt, out, P, rule, f"{tag}: fmx_fm_step {rule} vs float64")
        both(fmx, master, geom, lambda t: run_online(fmx, t, tuple(a[:64] for a in P), rule), f"{tag}: fmx_fm_online_run {rule}")
    both(fmx, master, geom, lambda t: run_step(fmx, t, P, RULES[layout][0], loss="sigmoid", with_x=False), f"{tag}: fmx_fm_step sigmoid, x = 1")
    pool = [problem(SIZES, B0, seed=200 + kp + j) for j in range(3)]
    both(fmx, master, geom, lambda t: run_stream(fmx, t, pool, RULES[layout][-1]), f"{tag}: fmx_fm_stream")
    both(fmx, master, geom, lambda t: run_update(fmx, t, P, RULES[layout][0], occ=False), f"{tag}: fmx_fm_update with g_bi")
    both(fmx, master, geom, lambda t: run_update(fmx, t, P, RULES[layout][-1], occ=True), f"{tag}: fmx_fm_update_occ")
    P64 = tuple(a[:64] for a in P)
    both(fmx, master, geom, lambda t: run_online_mlp(fmx, t, P64, "signadam", hedge=True, fm_term=True), f"{tag}: fmx_online_run_mlp Hedge")
    if layout == "weights":       # the fit mode takes SIGNADAM / SGD, i.e. weights-layout tables (FTRL / MOMENTS: refused on the host)
        both(fmx, master, geom, lambda t: run_online_mlp(fmx, t, P64, "signadam", hedge=False, fm_term=True), f"{tag}: fmx_online_run_mlp fit")
        both(fmx, master, geom, lambda t: run_online_mlp(fmx, t, P64, "sgd", hedge=False, fm_term=False), f"{tag}: fmx_online_run_mlp fit, NFM")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("B", [1, 4096])
def test_batch_sizes_at_the_minimum_geometry(fmx, layout, B):
    kp, k = 16, 16
    geom = geometry(layout, kp, "min")
    master = master_table(fmx, layout, k, seed=B)
    P = problem(SIZES, B, seed=300 + B)
    tag = f"{layout} kp=16 min B={B}"
    both(fmx, master, geom, lambda t: run_forward(fmx, t, P, True, "logits"), f"{tag}: fmx_fm_forward")
    both(fmx, master, geom, lambda t: run_part_finish(fmx, t, P), f"{tag}: fmx_fm_forward_partial + _finish")
    for rule in RULES[layout]:
        _, gt, out = both(fmx, master, geom, lambda t: run_step(fmx, t, P, rule), f"{tag}: fmx_fm_step {rule}")
        anchor_step_f64(master, gt, out, P, rule, f"{tag}: fmx_fm_step {rule} vs float64")
    both(fmx, master, geom, lambda t: run_update(fmx, t, P, RULES[layout][0], occ=False), f"{tag}: fmx_fm_update with g_bi")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("option,value,B", [("inline_fixup", 0, B0), ("sort_chunked", 2, 4096), ("online_persistent", 0, 64)])
def test_labelled_switches_at_the_minimum_geometry(fmx, layout, option, value, B):
    """The second-launch fix-up (k_fm_fixup), the chunked sort and the per-sample launches of fmx_online_run_mlp also address
    the table through a non-default geometry.  The switches change how the same bits are computed (include/fmx.h): the
    outputs equal the default switches' too."""
    lib = fmx._lib.load()
    kp, k = 16, 16
    geom = geometry(layout, kp, "min")
    master = master_table(fmx, layout, k, seed=7)
    P = problem(SIZES, B, seed=400 + B)
    tag = f"{layout} kp=16 min {option}={value}"
    if option == "online_persistent":
        runs = [lambda t: run_online_mlp(fmx, t, P, "signadam", hedge=True, fm_term=True)]
        if layout == "weights":
            runs.append(lambda t: run_online_mlp(fmx, t, P, "sgd", hedge=False, fm_term=True))
    else:
        runs = [lambda t, r=r: run_step(fmx, t, P, r) for r in RULES[layout]]
        runs.append(lambda t: run_update(fmx, t, P, RULES[layout][0], occ=False))
        runs.append(lambda t: run_update(fmx, t, P, RULES[layout][-1], occ=True))
    for i, run in enumerate(runs):
        _, _, want = both(fmx, master, geom, run, f"{tag}: call {i}, default switches")
        prev = lib.fmx_set_option(option.encode(), value)
        assert prev >= 0
        try:
            _, _, got = both(fmx, master, geom, run, f"{tag}: call {i}")
        finally:
            lib.fmx_set_option(option.encode(), prev)
        for name in want:
            if name not in ("S", "bi", "sfirst", "logit", "scratch"):      # (per-sample launches leave the last sample's forward there)
                np.testing.assert_array_equal(got[name], want[name], err_msg=f"{tag}: {name} depends on the switch")


@pytest.mark.parametrize("name", ["min", "padded"])
@pytest.mark.parametrize("layout,rule,fm_term", [("weights", "signadam", True), ("weights", "sgd", False), ("ftrl", "ftrl", True)])
def test_deepfm_stream_rider(fmx, layout, rule, fm_term, name):
    """fmx_deepfm_stream (k_fm_update_rider: the MLP's reduction inside the table update's launch).  mlp_workspace has no byte
    count in the ABI: it is given exactly fmx_mlp_section_workspace_bytes, with the pattern behind it."""
    kp, k = 16, 16
    geom = geometry(layout, kp, name)
    master = master_table(fmx, layout, k, seed=11)
    pool = [problem(SIZES, B0, seed=500 + j) for j in range(3)]
    both(fmx, master, geom, lambda t: run_deepfm_stream(fmx, t, pool, rule, fm_term), f"{layout} kp=16 {name}: fmx_deepfm_stream {rule}")


@pytest.mark.parametrize("name", ["min", "padded"])
@pytest.mark.parametrize("kp", [16, 8])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_afm_entry_points(fmx, layout, kp, name):
    k = K_OF[kp]
    geom = geometry(layout, kp, name)
    master = master_table(fmx, layout, k, seed=13 + kp)
    P = problem(SIZES, B0, seed=600 + kp)
    tag = f"{layout} kp={kp} {name}"
    both(fmx, master, geom, lambda t: run_afm(fmx, t, P, "forward"), f"{tag}: fmx_afm_forward")
    both(fmx, master, geom, lambda t: run_afm(fmx, t, P, "side"), f"{tag}: fmx_afm_side")
    for rule in RULES[layout]:
        both(fmx, master, geom, lambda t: run_afm(fmx, t, P, "step", rule), f"{tag}: fmx_afm_step {rule}")


@pytest.mark.parametrize("name", ["min", "padded"])
@pytest.mark.parametrize("layout,rule", [("weights", "sgd"), ("weights", "signadam"), ("ftrl", "ftrl")])
def test_mapped_table_with_an_empty_trailing_field(fmx, layout, rule, name):
    """Fields as pieces of index columns: two columns split in two pieces, the last field EMPTY.  The forward's branch-free
    gather reads (and drops) the row at n_rows for it: here that is the first guard row, inside the test's own buffer."""
    kp, k = 16, 16
    col_sizes = [50, 3000, 7, 120, 999, 16]
    cols, base, sizes = [], [], []
    for c_, n in enumerate(col_sizes):
        if c_ in (1, 4):
            cols += [c_, c_]
            base += [0, n // 2]
            sizes += [n // 2, n - n // 2]
        else:
            cols.append(c_)
            base.append(0)
            sizes.append(n)
    cols.append(0), base.append(0), sizes.append(0)                   # the empty trailing field
    master = master_table(fmx, layout, k, sizes=sizes, seed=17, mapped=(cols, base, len(col_sizes)))
    assert master.offsets_host[-1] == master.offsets_host[-2] == master.n_rows
    geom = geometry(layout, kp, name)
    P = problem(col_sizes, B0, seed=700)
    tag = f"mapped {layout} kp=16 {name}"
    both(fmx, master, geom, lambda t: run_forward(fmx, t, P, True, "logits"), f"{tag}: fmx_fm_forward")
    both(fmx, master, geom, lambda t: run_forward(fmx, t, P, False, "sigmoid"), f"{tag}: fmx_fm_forward x = 1")
    both(fmx, master, geom, lambda t: run_part_finish(fmx, t, P), f"{tag}: fmx_fm_forward_partial + _finish")
    both(fmx, master, geom, lambda t: run_step(fmx, t, P, rule), f"{tag}: fmx_fm_step {rule}")
    both(fmx, master, geom, lambda t: run_owner_step(fmx, t, P, rule), f"{tag}: fmx_owner_step {rule}")
