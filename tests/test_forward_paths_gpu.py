"""k_fm_forward against the owner-mode pair k_fm_forward_part + k_fm_forward_finish at ONE block, bit for bit: both evaluate the
same sum tree (include/fmx.h, "the forward pass split over field owners"), so S, the logit, its parts, the loss and dlogit agree
exactly.  Covers field counts that are not a multiple of the lane groups, one and two field windows, with and without values,
every row width, fields that are pieces of index columns, and indices outside their field."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HYP = dict(lr=0.01, eps=1e-8, alpha=0.05, beta=1.0, l1=0.001, l2=0.01)
FTRL = {k: HYP[k] for k in ("alpha", "beta", "l1", "l2")}


@pytest.fixture(scope="module")
def fmx():
    import fmx as _fmx
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _fmx


def _setup(fmx, sizes, k, layout, seed, mapped=None):
    rng = np.random.default_rng(seed)
    kw = {}
    if mapped is not None:
        kw = dict(field_cols=mapped[0], field_base=mapped[1], n_cols=mapped[2])
    t = fmx.FlatTable(sizes, k, layout=layout, ftrl=FTRL if layout == "ftrl" else None, **kw)
    R = t.n_rows
    t.rows[:, :k] = torch.from_numpy((rng.normal(size=(R, k)) * 0.3).astype(np.float32)).cuda()
    t.rows[:, t.kp] = torch.from_numpy((rng.normal(size=R) * 0.3).astype(np.float32)).cuda()
    if layout == "ftrl":
        t.bias[0], t.bias[1] = 0.4, 0.3          # (z, n): the bias weight goes through ftrl_w
    else:
        t.bias[0] = 0.37
    return t, rng


def _compare(fmx, t, idx, xv, y, expect_error):
    B = idx.shape[0]
    kp = t.kp
    hyper = fmx.Hyper(**HYP)
    eng = fmx.FMEngine(t, max_batch=B)
    idx_d, xv_d, y_d = eng.to_device(idx, xv, y)
    eng.error.zero_()
    eng.forward(hyper, idx_d, xv_d, y_d, loss="logits", want_first=False, want_bi=False)
    torch.cuda.synchronize()
    assert int(eng.error.item()) == expect_error
    got = {n: getattr(eng, n)[:B].clone() for n in ("S", "sfirst", "sbi", "logit", "loss_b", "dz")}

    lib = eng.lib
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    rec = 2 * kp + 4
    parts = torch.zeros((B, rec), dtype=torch.float32, device="cuda")
    fmx._lib.check(lib.fmx_fm_forward_partial(t.c_struct(), idx_d.data_ptr(), None if xv_d is None else xv_d.data_ptr(), B, 1, 1,
                                              B, parts.data_ptr(), err.data_ptr(), None))
    ref = {n: torch.full_like(v, float("nan")) for n, v in got.items()}
    out = fmx._lib.FwdOut()
    out.S, out.sfirst, out.sbi, out.logit = (ref[n].data_ptr() for n in ("S", "sfirst", "sbi", "logit"))
    out.loss, out.dz, out.error = ref["loss_b"].data_ptr(), ref["dz"].data_ptr(), err.data_ptr()
    layout = fmx._lib.LAYOUT_WEIGHTS if t.layout == "weights" else fmx._lib.LAYOUT_FTRL
    fmx._lib.check(lib.fmx_fm_forward_finish(hyper.ref(), t.bias.data_ptr(), layout, kp, parts.data_ptr(), B * rec, 1, y_d.data_ptr(),
                                             B, fmx._lib.LOSSES["logits"], 1.0 / B, C.byref(out), None))
    torch.cuda.synchronize()
    assert int(err.item()) == expect_error
    for n in got:
        a, b = got[n].cpu().numpy(), ref[n].cpu().numpy()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{n}: forward and part + finish differ"
    assert np.isfinite(got["loss_b"].cpu().numpy()).all()


def _problem(rng, sizes, B, real_x, bad):
    idx = np.stack([rng.integers(0, s, size=B) for s in sizes], axis=1).astype(np.int32)
    if bad:                                          # indices just past the field and far past it
        idx[3, 1] = sizes[1]
        idx[B - 1, len(sizes) - 1] = sizes[-1] + 1000
    xv = rng.uniform(-1, 1, size=idx.shape).astype(np.float32) if real_x else None
    y = (rng.uniform(size=B) < 0.3).astype(np.float32)
    return idx, xv, y


# (k, fields): fields not a multiple of the lane groups 64 / (k / 4); k = 4 at 70 fields takes two windows of 64 fields
GEOMETRIES = [(4, 39), (4, 70), (8, 39), (16, 39), (16, 13), (32, 23), (64, 13)]


@pytest.mark.parametrize("k,F", GEOMETRIES)
@pytest.mark.parametrize("layout", ["weights", "ftrl"])
@pytest.mark.parametrize("real_x", [False, True])
def test_forward_matches_part_finish(fmx, k, F, layout, real_x):
    rng0 = np.random.default_rng(F * 100 + k)
    sizes = [int(v) for v in rng0.integers(1, 3000, size=F)]
    t, rng = _setup(fmx, sizes, k, layout, seed=F + k)
    idx, xv, y = _problem(rng, sizes, 301, real_x, bad=False)
    _compare(fmx, t, idx, xv, y, expect_error=0)


@pytest.mark.parametrize("k,F", [(4, 70), (16, 39), (64, 13)])
@pytest.mark.parametrize("real_x", [False, True])
def test_out_of_range_index_raises_error_word(fmx, k, F, real_x):
    sizes = [7 + 3 * f for f in range(F)]
    t, rng = _setup(fmx, sizes, k, "ftrl", seed=5)
    idx, xv, y = _problem(rng, sizes, 257, real_x, bad=True)
    _compare(fmx, t, idx, xv, y, expect_error=1)


@pytest.mark.parametrize("k", [4, 16, 64])
@pytest.mark.parametrize("real_x", [False, True])
def test_mapped_fields_match_part_finish(fmx, k, real_x):
    # 9 index columns, two of them split into two pieces: 11 fields; an index outside a piece belongs to the other one
    n_cols = 9
    col_sizes = [50, 3000, 7, 120, 999, 16, 2, 400, 65]
    cols, base, sizes = [], [], []
    for c, n in enumerate(col_sizes):
        if c in (1, 4):
            cols += [c, c]
            base += [0, n // 2]
            sizes += [n // 2, n - n // 2]
        else:
            cols.append(c)
            base.append(0)
            sizes.append(n)
    t, rng = _setup(fmx, sizes, k, "weights", seed=11 + k, mapped=(cols, base, n_cols))
    B = 300
    idx = np.stack([rng.integers(0, n, size=B) for n in col_sizes], axis=1).astype(np.int32)
    idx[0, 0] = col_sizes[0] + 5                     # outside every piece of its column: no contribution, no error
    xv = rng.uniform(-1, 1, size=idx.shape).astype(np.float32) if real_x else None
    y = (rng.uniform(size=B) < 0.3).astype(np.float32)
    _compare(fmx, t, idx, xv, y, expect_error=0)
