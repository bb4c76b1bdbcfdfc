"""k_fm_forward with the loss epilogues of a workgroup's samples evaluated together (by its first wave, on adjacent lanes), through
the C ABI.

Every case compares every output two ways:

  * bit for bit against fmx_fm_forward_partial at ONE block followed by fmx_fm_forward_finish: kernels of their own (one sample
    per wave / per lane group) that add in the same tree.  fmx_fm_forward_partial takes at most four fields per lane group
    (F <= 4 * 64 / (kp / 4)); beyond that -- (kp, F) = (32, 39 ... 70), (64, 39 ... 70): the generic field loop
    -- it refuses, there is no second path with the same tree, and the case is pinned by the oracle alone;
  * against oracle.fm_oracle (flat_forward, loss_value, dloss_dlogit) at the tolerances of tests/test_kernels_gpu.py's forward
    tests: 1e-5 relative plus their floors.  One floor is derived here instead of copied: sfirst sums F terms, and two fp32
    orders of one sum differ by at most 2 (F - 1) 2^-24 sum|t| (each within (F - 1) 2^-24 sum|t| of the exact sum), which at
    70 fields is above the 1e-6 that suits test_kernels_gpu's 11 fields.  The epilogue is compared with the oracle's fp32
    evaluation at the kernel's own logit, as there; its floors of 1e-7 / 1e-9 suit 37 samples with small logits, and over
    thousands of samples the two fp32 evaluations themselves differ by more: the loss adds three terms of magnitude <= |z|
    (two roundings of <= 2^-24 |z| on each side: 4 * 2^-24 |z|), and dz subtracts the label from a sigmoid that each side has
    within 2 ulp of 1 (4 * 2^-24 / B).  These are added to the floors; the bit-for-bit comparison is the sharp one.

B walks through the group boundaries (a group is the 1, 2 or 4 samples of a workgroup: B = 1, 2, 3, 5, 63, 4095, 4097 end in a
partial group whose absent samples' waves run along to the barrier and must store nothing); the
outputs live in buffers filled with a NaN pattern, with pattern-filled bands around them (tests/abi_geometry.py), so a store of
an absent sample, or a sample that is not stored, is seen.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import abi_geometry as ag
from oracle import fm_oracle as orc

pytestmark = pytest.mark.gpu

HYP = dict(lr=0.01, eps=1e-8, alpha=0.05, beta=1.0, l1=0.001, l2=0.01)
FTRL = {k: HYP[k] for k in ("alpha", "beta", "l1", "l2")}
BATCHES = [1, 2, 3, 5, 63, 64, 4095, 4096, 4097]
KPS = [4, 8, 16, 32, 64]
FIELDS = [1, 10, 39, 48, 49, 70]
LAYOUTS = ["weights", "ftrl", "moments"]
LOSS_KINDS = ["logits", "sigmoid", None]
OUTS = ("S", "bi", "first", "sfirst", "sbi", "logit", "loss", "dz")


@pytest.fixture(scope="module")
def fmx():
    import fmx as _fmx
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _fmx


def _sizes(F, kp):
    rng = np.random.default_rng(F * 100 + kp)
    return [int(v) for v in rng.integers(1, 3000, size=F)]


def _table(fmx, sizes, k, layout, seed):
    rng = np.random.default_rng(seed)
    t = fmx.FlatTable(sizes, k, layout=layout, ftrl=FTRL if layout == "ftrl" else None)
    R = t.n_rows
    V = (rng.normal(size=(R, k)) * 0.3).astype(np.float32)
    w = (rng.normal(size=R) * 0.3).astype(np.float32)
    t.rows[:, :k] = torch.from_numpy(V).cuda()
    t.rows[:, t.kp] = torch.from_numpy(w).cuda()
    if layout == "ftrl":
        t.bias[0], t.bias[1] = 0.4, 0.3          # (z, n): the bias weight goes through ftrl_w
        bias = orc.ftrl_weight(np.float32(0.4), np.float32(0.3), **FTRL)
    else:
        t.bias[0] = 0.37
        bias = np.float32(0.37)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return t, dict(V=V, w=w, bias=np.float32(bias), offs=offs)


def _problem(sizes, B, real_x, seed):
    rng = np.random.default_rng(seed)
    idx = np.stack([rng.integers(0, s, size=B) for s in sizes], axis=1).astype(np.int32)
    xv = rng.uniform(-1, 1, size=idx.shape).astype(np.float32) if real_x else None
    y = (rng.uniform(size=B) < 0.3).astype(np.float32)
    return idx, xv, y


class Outputs:
    """The forward's output buffers, each a pattern-filled body between pattern-filled bands; `absent` names pointers left null.
    sample_ld > 0: S, dz and loss share records of sample_ld floats (S at 0, dz at kp, loss at kp + 1), as the step lays them out."""

    def __init__(self, fmx, B, F, kp, sample_ld=0, absent=()):
        self.B, self.F, self.kp, self.ld = B, F, kp, sample_ld
        shapes = dict(S=(B, kp), bi=(B, kp), first=(B, F), sfirst=(B,), sbi=(B,), logit=(B,), loss=(B,), dz=(B,))
        self.g, self.absent = {}, set(absent)
        self.out = fmx._lib.FwdOut()
        self.err = ag.Guarded(4, torch.int32, name="error")
        self.out.error = self.err.ptr
        if sample_ld > 0:
            self.rec = ag.Guarded(4 * B * sample_ld, name="records", shape=(B, sample_ld))
            self.rec.t.view(torch.int32).fill_(ag.PATTERN)
        for n in OUTS:
            if n in self.absent:
                continue
            if sample_ld > 0 and n in ("S", "dz", "loss"):
                setattr(self.out, n, self.rec.ptr + 4 * {"S": 0, "dz": kp, "loss": kp + 1}[n])
                continue
            g = self.g[n] = ag.Guarded(4 * int(np.prod(shapes[n])), name=n, shape=shapes[n])
            g.t.view(torch.int32).fill_(ag.PATTERN)
            setattr(self.out, n, g.ptr)
        self.out.sample_ld = sample_ld

    def bits(self):
        """{name: int32 bits [B, ...]} of what was asked for; checks the bands and, with records, the floats between the outputs."""
        self.err.check()
        r = {n: ag.bits(g.t) for n, g in self.g.items()}
        for g in self.g.values():
            g.check()
        if self.ld > 0:
            self.rec.check()
            rec = ag.bits(self.rec.t)
            kp = self.kp
            live = np.zeros(self.ld, dtype=bool)
            for n, (o, w) in dict(S=(0, kp), dz=(kp, 1), loss=(kp + 1, 1)).items():
                if n not in self.absent:
                    r[n] = rec[:, o:o + w].reshape((self.B, kp) if n == "S" else (self.B,))
                    live[o:o + w] = True
            assert (rec[:, ~live] == ag.PATTERN).all(), "floats of the records that belong to no output were written"
        return r

    def error(self):
        return int(self.err.t.item())


def _dev(a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _run_forward(fmx, t, idx_d, xv_d, y_d, B, loss, o):
    hyper = fmx.Hyper(**HYP)
    fmx._lib.check(fmx._lib.load().fmx_fm_forward(t.c_struct(), hyper.ref(), _ptr(idx_d), _ptr(xv_d), _ptr(y_d), B,
                                                  fmx._lib.LOSSES[loss], 1.0 / B, C.byref(o.out), None))
    torch.cuda.synchronize()


def _part_finish_supported(kp, F):
    return F <= 4 * (64 // (kp // 4))


def _run_part_finish(fmx, t, idx_d, xv_d, y_d, B, loss, o):
    """The same outputs by fmx_fm_forward_partial (one block) + fmx_fm_forward_finish; they do not produce `first`."""
    lib, hyper = fmx._lib.load(), fmx.Hyper(**HYP)
    rec = 2 * t.kp + 4
    parts = torch.zeros((B, rec), dtype=torch.float32, device="cuda")
    fmx._lib.check(lib.fmx_fm_forward_partial(t.c_struct(), _ptr(idx_d), _ptr(xv_d), B, 1, 1, B, parts.data_ptr(), o.err.ptr, None))
    layout = fmx._lib.LAYOUT_FTRL if t.layout == "ftrl" else fmx._lib.LAYOUT_WEIGHTS   # (a moments table is read as a weights one)
    fmx._lib.check(lib.fmx_fm_forward_finish(hyper.ref(), t.bias.data_ptr(), layout, t.kp, parts.data_ptr(), B * rec, 1,
                                             _ptr(y_d), B, fmx._lib.LOSSES[loss], 1.0 / B, C.byref(o.out), None))
    torch.cuda.synchronize()


def _f32(b):
    return np.ascontiguousarray(b).view(np.float32)


def close(a, b, rtol, floor, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, what
    err = np.abs(a - b)
    tol = rtol * np.abs(b) + floor
    assert (err <= tol).all(), f"{what}: max err {err.max():.3e} (tol there {tol.flat[err.argmax()]:.3e}), n_bad {(err > tol).sum()}"


def _check_oracle(got, ref_tab, idx, xv, y, B, k, loss, ok=None):
    """got: {name: bits}; ok [B, F] bool: the indices inside their fields (the others contribute nothing)."""
    F = idx.shape[1]
    x = xv if xv is not None else np.ones(idx.shape, dtype=np.float32)
    rows = idx.astype(np.int64)
    if ok is not None:
        x = np.where(ok, x, np.float32(0)).astype(np.float32)
        rows = np.where(ok, rows, 0)
    rows = rows + ref_tab["offs"][:-1][None, :]
    ref = orc.flat_forward(ref_tab["V"], ref_tab["w"], ref_tab["bias"], rows, x)
    smax = max(float(np.abs(ref["S"]).max()), 1e-30)
    t_abs = float(np.abs(ref["first"]).sum(axis=1).max())
    floors = dict(S=1e-6 * smax, bi=2e-6 * smax * smax, first=1e-8, sfirst=1e-6 + 2 * (F - 1) * 2.0 ** -24 * t_abs,
                  sbi=4e-6 * smax * smax * k, logit=4e-6 * smax * smax * k + 2 * (F - 1) * 2.0 ** -24 * t_abs)
    for n, floor in floors.items():
        if n in got:
            v = _f32(got[n])
            if n in ("S", "bi"):
                assert (v[:, k:] == 0).all(), f"{n}: pad components"
                v = v[:, :k]
            close(v, ref[n], 1e-6 if n == "first" else 1e-5, floor, n)
    if loss is not None and "logit" in got:
        z = _f32(got["logit"])          # the epilogue itself: the oracle evaluated at the kernel's own logit
        if "loss" in got:
            close(_f32(got["loss"]), orc.loss_value(z, y, loss), 1e-5, 1e-7 + 4 * 2.0 ** -24 * np.abs(z.astype(np.float64)), "loss")
        if "dz" in got:
            close(_f32(got["dz"]), orc.dloss_dlogit(z, y, loss, 1.0 / B), 1e-5, 1e-9 + 4 * 2.0 ** -24 / B, "dz")


def _case(fmx, t, ref_tab, idx, xv, y, loss, sample_ld=0, absent=(), expect_error=0, ok=None):
    B, F = idx.shape
    idx_d, xv_d, y_d = _dev(idx, torch.int32), _dev(xv, torch.float32), _dev(y, torch.float32)
    o = Outputs(fmx, B, F, t.kp, sample_ld, absent)
    _run_forward(fmx, t, idx_d, xv_d, y_d, B, loss, o)
    assert o.error() == expect_error
    got = o.bits()
    written = [n for n in OUTS if n not in absent and not (loss is None and n in ("loss", "dz"))]
    for n in written:
        assert (got[n] != ag.PATTERN).all(), f"{n}: samples without a result"
    for n in ("loss", "dz"):
        if loss is None and n in got:
            assert (got[n] == ag.PATTERN).all(), f"{n} written without a loss"
    if _part_finish_supported(t.kp, F):
        r = Outputs(fmx, B, F, t.kp, sample_ld, tuple(absent) + ("first",))
        _run_part_finish(fmx, t, idx_d, xv_d, y_d, B, loss, r)
        assert r.error() == expect_error
        ref = r.bits()
        for n in written:
            if n != "first":
                assert np.array_equal(got[n], ref[n]), f"{n}: k_fm_forward and part + finish differ (B={B}, loss={loss})"
    _check_oracle({n: got[n] for n in written}, ref_tab, idx, xv, y, B, t.k, loss, ok)


@pytest.mark.parametrize("F", FIELDS)
@pytest.mark.parametrize("kp", KPS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_forward_every_batch_tail(fmx, layout, kp, F):
    sizes = _sizes(F, kp)
    t, ref_tab = _table(fmx, sizes, kp, layout, seed=F + kp)
    for B in BATCHES:
        for real_x in (False, True):
            idx, xv, y = _problem(sizes, B, real_x, seed=B * 7 + F + real_x)
            for loss in LOSS_KINDS:
                _case(fmx, t, ref_tab, idx, xv, y, loss)


@pytest.mark.parametrize("null", OUTS)
@pytest.mark.parametrize("kp,F", [(16, 39), (4, 70), (64, 10), (32, 49)])
def test_each_output_pointer_null_in_turn(fmx, kp, F, null):
    sizes = _sizes(F, kp)
    t, ref_tab = _table(fmx, sizes, kp, "ftrl", seed=3)
    for B in (5, 4097):
        idx, xv, y = _problem(sizes, B, False, seed=B)
        _case(fmx, t, ref_tab, idx, xv, y, "logits", absent=(null,))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kp,F", [(16, 39), (8, 48), (4, 1), (64, 70)])
def test_sample_records(fmx, kp, F, layout):
    """sample_ld > 0: S, dz and loss of a sample inside one record, as the step's update reads them."""
    sizes = _sizes(F, kp)
    t, ref_tab = _table(fmx, sizes, kp, layout, seed=4)
    ld = kp + 4
    for B in (3, 63, 4097):
        for real_x in (False, True):
            idx, xv, y = _problem(sizes, B, real_x, seed=B + 1)
            for loss in LOSS_KINDS:
                _case(fmx, t, ref_tab, idx, xv, y, loss, sample_ld=ld)


@pytest.mark.parametrize("real_x", [False, True])
@pytest.mark.parametrize("kp,F", [(16, 39), (4, 70), (8, 10), (64, 13), (32, 48)])
@pytest.mark.parametrize("B", [1, 3, 5, 63, 4095, 4097])
def test_out_of_range_index_in_the_last_partial_group(fmx, B, kp, F, real_x):
    """One index past its field in the batch's last sample, which sits in a partial group: the error word is raised exactly as
    by the one-sample paths, the field contributes nothing, every other sample is untouched by it."""
    sizes = _sizes(F, kp)
    t, ref_tab = _table(fmx, sizes, kp, "ftrl", seed=6)
    idx, xv, y = _problem(sizes, B, real_x, seed=B + kp)
    f = F // 2
    idx[B - 1, f] = sizes[f] + 7
    ok = np.ones(idx.shape, dtype=bool)
    ok[B - 1, f] = False
    _case(fmx, t, ref_tab, idx, xv, y, "logits", expect_error=1, ok=ok)
    idx[B - 1, f] = 0                               # and the word stays clear without it
    _case(fmx, t, ref_tab, idx, xv, y, "logits", expect_error=0)
