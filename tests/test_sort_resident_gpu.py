"""The resident-capped form of the online loop's side-stream group sort (fmx_set_option("sort_resident", R)) on the MI355X,
through the C ABI.

From a call's third group on, fmx_fm_stream / fmx_deepfm_stream sort a group of batches with min(units, R) workgroups (rounded
up to a multiple of 8, one per CU at the most), each walking several (batch, sort field) units, instead of one workgroup per
unit.  The lists are integer sorts of unique composites, so which workgroup sorts a unit must not be visible anywhere: table
rows, bias, per-step losses and the error word of a stream are compared BIT FOR BIT with the same stream under
sort_resident = 0 and with the same steps taken one by one (fmx_fm_step).

R = 1, 3, 8: one workgroup per XCD walks all of its units (3: not a multiple of 8); 24: three per XCD; 1000: more than there are
units.  B = 512 is the smallest batch that takes the side stream, 600 pads the lists to 1,024.  41 steps are groups of 4, 16,
16 and 5: two capped launches, the second partial, then a call boundary; the pool sizes 5 and 7 are coprime to the group size,
so a unit that was skipped would leave ANOTHER batch's list in the ring.  Every case runs two calls on one workspace."""
import numpy as np
import pytest
import torch

from update_forms import same          # bit for bit, the words as integers

pytestmark = pytest.mark.gpu

# a one-row field, an empty one, fields of at most 511 rows (one counting pass) and larger ones (the bitonic network)
SIZES = [1, 300, 5000, 0, 511, 512, 40000, 7, 64, 2000, 100, 130000]
MAPPED = dict(field_cols=list(range(len(SIZES))), field_base=[0] * len(SIZES), n_cols=len(SIZES))  # (empty fields need a mapped table)
PLAIN_SIZES = [3, 9000, 50, 700, 20000, 5, 600, 2]
HYP = dict(lr=0.01, eps=1e-8, alpha=0.05, beta=1.0, l1=0.001, l2=0.01)
LAYOUT = {"ftrl": "ftrl", "sgd": "weights"}
N_STEPS, N_CALLS = 41, 2


@pytest.fixture(scope="module")
def fmx():
    import fmx as _fmx
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _fmx


class resident:
    """sort_resident = R for a block; back to -1, the library's default, on the way out."""

    def __init__(self, lib, R):
        self.lib, self.R = lib, R

    def __enter__(self):
        self.lib.fmx_set_option(b"sort_resident", self.R)

    def __exit__(self, *exc):
        self.lib.fmx_set_option(b"sort_resident", -1)


def indices(sizes, shape, seed):
    rng = np.random.default_rng(seed)
    cols = [np.minimum(rng.zipf(1.3, size=shape) - 1, max(int(s), 1) - 1) if f % 2 else rng.integers(0, max(int(s), 1), size=shape)
            for f, s in enumerate(sizes)]
    return np.stack(cols, axis=-1).astype(np.int32)


def make_table(fmx, sizes, k, rule, **kw):
    t = fmx.FlatTable(sizes, k, layout=LAYOUT[rule], ftrl=HYP, **kw)
    gen = torch.Generator(device="cuda").manual_seed(7)
    V0 = torch.randn((t.n_rows, k), device="cuda", generator=gen) * 0.1
    w0 = torch.randn(t.n_rows, device="cuda", generator=gen) * 0.1
    t.rows[:, :k] = V0
    t.rows[:, t.kp] = w0
    if rule == "ftrl":
        t.rows[:, t.z_offset:t.z_offset + k] = fmx.table.ftrl_z_for_weight_torch(V0, t.ftrl)
        t.bias[0] = -0.4
    else:
        t.bias[0] = 0.37
    return t


def pool(sizes, n_pool, B, seed):
    idx = torch.from_numpy(indices(sizes, (n_pool, B), seed)).cuda()
    y = torch.from_numpy((np.random.default_rng(seed + 1).uniform(size=(n_pool, B)) < 0.3).astype(np.float32)).cuda()
    return idx, y


def run_stream(fmx, R, sizes, k, rule, idx, y, table_kw=None, cap=None):
    """N_CALLS calls of N_STEPS steps of fmx_fm_stream on one engine under sort_resident = R."""
    with resident(fmx._lib.load(), R):
        t = make_table(fmx, sizes, k, rule, **(table_kw or {}))
        t.sort_cap_override = cap
        eng = fmx.FMEngine(t, max_batch=idx.shape[1])
        hyp = fmx.Hyper(**HYP)
        loss = torch.zeros(N_CALLS * N_STEPS, device="cuda")
        for c in range(N_CALLS):
            eng.stream(hyp, rule, "logits", idx, y, N_STEPS, loss[c * N_STEPS:(c + 1) * N_STEPS])
        torch.cuda.synchronize()
        return dict(rows=t.rows.clone(), bias=t.bias.clone(), loss=loss, error=eng.error.clone())


def run_steps(fmx, sizes, k, rule, idx, y, table_kw=None):
    """The same steps one by one (fmx_fm_step: no group sort at all)."""
    t = make_table(fmx, sizes, k, rule, **(table_kw or {}))
    eng = fmx.FMEngine(t, max_batch=idx.shape[1])
    hyp = fmx.Hyper(**HYP)
    loss = torch.zeros(N_CALLS * N_STEPS, device="cuda")
    for c in range(N_CALLS):
        for s in range(N_STEPS):
            j = s % idx.shape[0]
            eng.step(hyp, rule, "logits", idx[j], None, y[j])
            loss[c * N_STEPS + s] = eng.loss_out[0]
    torch.cuda.synchronize()
    return dict(rows=t.rows.clone(), bias=t.bias.clone(), loss=loss, error=eng.error.clone())


_REFS = {}


def references(fmx, B, k, rule, n_pool):
    """(pool, the stream under sort_resident = 0, the single steps) of a shape: computed once, shared by the caps."""
    key = (B, k, rule, n_pool)
    if key not in _REFS:
        idx, y = pool(SIZES, n_pool, B, seed=B + k + n_pool)
        ref = run_stream(fmx, 0, SIZES, k, rule, idx, y, MAPPED)
        steps = run_steps(fmx, SIZES, k, rule, idx, y, MAPPED)
        same(steps, ref, f"uncapped stream against its single steps {key}")
        assert int(ref["error"].item()) == 0
        assert bool(torch.isfinite(ref["loss"]).all()) and bool(torch.isfinite(ref["rows"]).all())
        assert not torch.equal(ref["rows"], make_table(fmx, SIZES, k, rule, **MAPPED).rows)   # the steps did train the table
        _REFS[key] = (idx, y, ref)
    return _REFS[key]


@pytest.mark.parametrize("n_pool", [5, 7])
@pytest.mark.parametrize("rule", ["ftrl", "sgd"])
@pytest.mark.parametrize("k", [4, 16])
@pytest.mark.parametrize("B", [512, 600])
@pytest.mark.parametrize("R", [1, 3, 8, 24, 1000])
def test_capped_stream_gives_identical_bits(fmx, R, B, k, rule, n_pool):
    idx, y, ref = references(fmx, B, k, rule, n_pool)
    got = run_stream(fmx, R, SIZES, k, rule, idx, y, MAPPED)
    same(got, ref, f"sort_resident = {R}, B = {B}, k = {k}, {rule}, n_pool = {n_pool}")


def test_default_cap_gives_identical_bits(fmx):
    idx, y, ref = references(fmx, 600, 16, "ftrl", 5)
    same(run_stream(fmx, -1, SIZES, 16, "ftrl", idx, y, MAPPED), ref, "sort_resident = -1")


def test_sort_pieces(fmx):
    """Large fields cut into sort pieces (ensure_sort_split): 1 + 9 + 1 + 1 + 20 + 1 + 1 + 1 = 35 sort fields of 8 index columns."""
    idx, y = pool(PLAIN_SIZES, 5, 512, seed=11)
    ref = run_stream(fmx, 0, PLAIN_SIZES, 16, "ftrl", idx, y, cap=1000)
    assert int(ref["error"].item()) == 0
    for R in (8, 24):
        same(run_stream(fmx, R, PLAIN_SIZES, 16, "ftrl", idx, y, cap=1000), ref, f"sort pieces, sort_resident = {R}")


def test_deepfm_stream(fmx):
    """fmx_deepfm_stream runs the same loop: rows, bias, network and losses bit for bit."""
    lib = fmx._lib.load()
    k, H, L, B, n_pool = 16, 32, 2, 512, 5
    idx, y = pool(PLAIN_SIZES, n_pool, B, seed=3)
    n_params = H * k + H + H * H + H
    results = []
    for R in (0, 8):
        with resident(lib, R):
            t = make_table(fmx, PLAIN_SIZES, k, "ftrl")
            eng = fmx.FMEngine(t, max_batch=B)
            params = (torch.randn(n_params, generator=torch.Generator().manual_seed(1)) * (1.0 / np.sqrt(H))).cuda()
            grads = torch.zeros_like(params)
            loss = torch.zeros(N_STEPS, device="cuda")
            run = eng.prepare_deepfm_stream(fmx.Hyper(**HYP), "ftrl", "sigmoid", params, grads, k, H, L, 0.05, idx, y, loss_out=loss)
            run(N_STEPS)
            torch.cuda.synchronize()
            results.append(dict(rows=t.rows.clone(), bias=t.bias.clone(), loss=loss, params=params, error=eng.error.clone()))
    assert int(results[0]["error"].item()) == 0
    same(results[1], results[0], "fmx_deepfm_stream")


@pytest.mark.parametrize("fields", [(0, 4), (7,)], ids=["second_iteration", "last_iteration"])
def test_bad_index_is_flagged(fmx, fields):
    """An index outside its field, in a unit a workgroup reaches in its second and in its last loop iteration, raises error
    word 1 and the stream is the one sort_resident = 0 gives.  Under R = 8 the third group (steps 20 .. 35, 16 batches) is
    walked by ONE workgroup per XCD: XCD 0's takes (first field, batch 0), (first field, batch 8), ..., (last field, batch 8) --
    the first field being field 4, the largest, where the table's row counts are known, else field 0; the last, field 7, is the
    smallest either way.  Batch 8 of that group is step 28."""
    n_pool = N_STEPS                                      # step 28 is the pool's batch 28 and no other step of a call
    idx, y = pool(PLAIN_SIZES, n_pool, 512, seed=5)
    for f in fields:
        idx[28, 100 + f, f] = PLAIN_SIZES[f] + 5
    ref = run_stream(fmx, 0, PLAIN_SIZES, 16, "ftrl", idx, y)
    got = run_stream(fmx, 8, PLAIN_SIZES, 16, "ftrl", idx, y)
    assert int(ref["error"].item()) == 1 and int(got["error"].item()) == 1
    same(got, ref, f"bad index in fields {fields}")


def test_option_round_trip(fmx):
    lib = fmx._lib.load()
    assert lib.fmx_set_option(b"sort_resident", 24) == -1      # the default
    assert lib.fmx_set_option(b"sort_resident", 0) == 24
    assert lib.fmx_set_option(b"sort_resident", -7) == 0       # any negative value: the default again
    assert lib.fmx_set_option(b"sort_resident", -1) == -1
