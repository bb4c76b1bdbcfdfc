"""The dispatch order of k_fm_update's tiles (fmx_set_option("upd_order", v)) on the MI355X, through the C ABI.

The order in which the grid takes the sort fields -- 0: index order, 1: ascending row count (the default), 2: descending, the
adversarial order with every closing tile as late as possible -- is not visible in any result: table rows, bias and per-step
losses are compared BIT FOR BIT across the three orders and against the second-launch form (inline_fixup = 0, k_fm_fixup), and
the error word stays 0 (2 would be a hand-off wait that ran into its bound).  Every instantiation of update_body is covered:
k_fm_update (fmx_fm_step, fmx_fm_stream), k_fm_update_rider (fmx_deepfm_stream) and k_fm_update_occ (fmx_fm_update_occ).

Table: row counts [1, 3, 70, 5000, 2, 200000, 64, 65] -- a one-row field (one run through every tile of its list), fields of
exactly 64 and 65 rows, and fields with next to no crossing run.  Batches of 64 (one tile per field), 100 and 257 (a ragged last
tile), 1000 (16 tiles per field)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 70, 5000, 2, 200000, 64, 65]
HYP = dict(lr=0.01, eps=1e-8, alpha=0.05, beta=1.0, l1=0.001, l2=0.01)
LAYOUT = {"ftrl": "ftrl", "sgd": "weights", "adam": "moments"}
N_STEPS = 30
# (upd_order, inline_fixup): the three orders in the one-launch form, and the second-launch form as the parent's yardstick
CONFIGS = [(0, 1), (1, 1), (2, 1), (0, 0)]


@pytest.fixture(scope="module")
def fmx():
    import fmx as _fmx
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _fmx


class options:
    """fmx_set_option for a block, restored on the way out."""

    def __init__(self, lib, **kw):
        self.lib, self.kw, self.old = lib, kw, {}

    def __enter__(self):
        for name, v in self.kw.items():
            self.old[name] = self.lib.fmx_set_option(name.encode(), v)
            assert self.old[name] >= 0, name

    def __exit__(self, *exc):
        for name, v in self.old.items():
            self.lib.fmx_set_option(name.encode(), v)


def indices(sizes, shape, zipf, seed):
    rng = np.random.default_rng(seed)
    cols = []
    for s in sizes:
        s = max(int(s), 1)                 # (an empty field of a mapped table: every index lies outside it)
        col = np.minimum(rng.zipf(1.3, size=shape) - 1, s - 1) if zipf else rng.integers(0, s, size=shape)
        cols.append(col)
    return np.stack(cols, axis=-1).astype(np.int32)


def make_table(fmx, sizes, k, rule, **kw):
    """A seeded table in the rule's layout: the same bits for the same arguments."""
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


def snap(**tensors):
    """Copies that stay on the device: the tables are compared there."""
    return {name: v.detach().clone() for name, v in tensors.items()}


def same(results, what):
    ref = results[0]
    for cfg, r in zip(CONFIGS[1:], results[1:]):
        for name in ref:
            # bit for bit: the float32 words as integers (a NaN would differ from itself otherwise)
            a, b = r[name].contiguous().view(torch.int32), ref[name].contiguous().view(torch.int32)
            assert torch.equal(a, b), f"{what}: {name} under (upd_order, inline_fixup) = {cfg}: {int((a != b).sum())} words differ"
    assert bool(torch.isfinite(ref["loss"]).all()) and bool(torch.isfinite(ref["rows"]).all()), what


def steps_and_stream(fmx, sizes, k, rule, B, zipf, table_kw=None, cap=None, n_sort_fields=None):
    """30 steps of fmx_fm_step (feature values != 1) and then 30 of fmx_fm_stream on the same table, under every configuration."""
    lib = fmx._lib.load()
    n_pool = 3
    idx = indices(sizes, (n_pool, B), zipf, seed=B + k)
    rng = np.random.default_rng(B)
    x = rng.uniform(-1, 1, size=(n_pool, B, len(sizes))).astype(np.float32)
    y = (rng.uniform(size=(n_pool, B)) < 0.3).astype(np.float32)
    results = []
    for order, inline in CONFIGS:
        with options(lib, upd_order=order, inline_fixup=inline):
            t = make_table(fmx, sizes, k, rule, **(table_kw or {}))
            t.sort_cap_override = cap
            eng = fmx.FMEngine(t, max_batch=B)
            if n_sort_fields is not None:
                assert t._sort_split[1].numel() == n_sort_fields
            hyp = fmx.Hyper(**HYP)
            idx_d, x_d, y_d = torch.from_numpy(idx).cuda(), torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
            loss = torch.zeros(2 * N_STEPS, device="cuda")
            for s in range(N_STEPS):
                eng.step(hyp, rule, "logits", idx_d[s % n_pool], x_d[s % n_pool], y_d[s % n_pool])
                loss[s] = eng.loss_out[0]
            eng.stream(hyp, rule, "logits", idx_d, y_d, N_STEPS, loss[N_STEPS:])
            torch.cuda.synchronize()
            assert int(eng.error.item()) == 0, f"error word {int(eng.error.item())} under (upd_order, inline_fixup) = {(order, inline)}"
            results.append(snap(rows=t.rows, bias=t.bias, loss=loss))
    same(results, f"{rule} k={k} B={B} zipf={zipf}")
    return results[0]


@pytest.mark.parametrize("zipf", [False, True], ids=["uniform", "zipf"])
@pytest.mark.parametrize("B", [64, 100, 257, 1000])
@pytest.mark.parametrize("k", [4, 16, 64])
@pytest.mark.parametrize("rule", ["ftrl", "sgd", "adam"])
def test_orders_and_second_launch_give_identical_bits(fmx, rule, k, B, zipf):
    before = make_table(fmx, SIZES, k, rule).rows
    after = steps_and_stream(fmx, SIZES, k, rule, B, zipf)
    assert not torch.equal(after["rows"], before)                    # the steps did train the table


def test_empty_fields(fmx):
    """A table whose fields are pieces of index columns may hold empty fields: 0 rows, first in the ascending order, no
    occurrence in any list."""
    sizes = [5, 0, 300, 0, 7000, 64, 0]
    kw = dict(field_cols=list(range(len(sizes))), field_base=[0] * len(sizes), n_cols=len(sizes))
    for rule in ("ftrl", "sgd"):
        steps_and_stream(fmx, sizes, 16, rule, 257, True, table_kw=kw)


@pytest.mark.parametrize("cap,n_sort_fields", [(2500, 1 + 1 + 1 + 2 + 1 + 80 + 1 + 1), (1000, 1 + 1 + 1 + 5 + 1 + 200 + 1 + 1)])
def test_sort_pieces(fmx, cap, n_sort_fields):
    """Large fields cut into sort pieces: every piece is a sort field with a place of its own in the order -- 88 sort fields --
    and a table of more sort fields than the launch carries by value (211 > 128) is updated in index order under every option."""
    steps_and_stream(fmx, SIZES, 16, "ftrl", 257, False, cap=cap, n_sort_fields=n_sort_fields)


def test_rider_form(fmx):
    """k_fm_update_rider (fmx_deepfm_stream: the MLP's gradient reduction rides behind the update's blocks) at B = 64 with a
    16-32-32 network: rows, bias, network and losses bit for bit under every order."""
    lib = fmx._lib.load()
    k, H, L, B, n_pool = 16, 32, 2, 64, 3
    idx = torch.from_numpy(indices(SIZES, (n_pool, B), True, seed=3)).cuda()
    y = torch.from_numpy((np.random.default_rng(4).uniform(size=(n_pool, B)) < 0.3).astype(np.float32)).cuda()
    n_params = H * k + H + H * H + H
    results = []
    for order, inline in CONFIGS:
        with options(lib, upd_order=order, inline_fixup=inline):
            t = make_table(fmx, SIZES, k, "ftrl")
            eng = fmx.FMEngine(t, max_batch=B)
            params = (torch.randn(n_params, generator=torch.Generator().manual_seed(1)) * (1.0 / np.sqrt(H))).cuda()
            grads = torch.zeros_like(params)
            loss = torch.zeros(N_STEPS, device="cuda")
            run = eng.prepare_deepfm_stream(fmx.Hyper(**HYP), "ftrl", "sigmoid", params, grads, k, H, L, 0.05, idx, y, loss_out=loss)
            run(N_STEPS)
            torch.cuda.synchronize()
            assert int(eng.error.item()) == 0
            results.append(snap(rows=t.rows, bias=t.bias, loss=loss, params=params))
    same(results, "fmx_deepfm_stream")


def test_update_occ(fmx):
    """k_fm_update_occ (fmx_fm_update_occ: explicit per-occurrence gradients) behind a sort and a forward of the same batch."""
    lib = fmx._lib.load()
    k, B, F = 16, 257, len(SIZES)
    idx = indices(SIZES, (B,), True, seed=5)
    rng = np.random.default_rng(6)
    y = (rng.uniform(size=B) < 0.3).astype(np.float32)
    results = []
    for order, inline in CONFIGS:
        with options(lib, upd_order=order, inline_fixup=inline):
            t = make_table(fmx, SIZES, k, "sgd")
            eng = fmx.FMEngine(t, max_batch=B)
            hyp = fmx.Hyper(**HYP)
            idx_d, _, y_d = eng.to_device(idx, None, y)
            E = np.zeros((B, F, t.kp), np.float32)
            E[:, :, :k] = np.random.default_rng(8).normal(size=(B, F, k)) * 1e-3
            E_d = torch.from_numpy(E.reshape(B, F * t.kp)).cuda()
            loss = torch.zeros(5, device="cuda")
            for s in range(5):
                eng.sort(idx_d)
                eng.forward(hyp, idx_d, None, y_d, loss="logits", want_first=False, want_bi=False)
                rc = lib.fmx_fm_update_occ(t.c_struct(), hyp.ref(), fmx._lib.RULES["sgd"], eng.workspace.data_ptr(), eng._ws_bytes(), None,
                                           eng.dz.data_ptr(), E_d.data_ptr(), F * t.kp, B, eng.loss_b.data_ptr(), 1.0 / B,
                                           eng.loss_out.data_ptr(), None)
                assert rc == 0, lib.fmx_last_error_string().decode()
                loss[s] = eng.loss_out[0]
            torch.cuda.synchronize()
            assert int(eng.error.item()) == 0
            results.append(snap(rows=t.rows, bias=t.bias, loss=loss))
    same(results, "fmx_fm_update_occ")


def test_option_round_trip(fmx):
    lib = fmx._lib.load()
    assert lib.fmx_set_option(b"upd_order", 2) == 1          # the default
    assert lib.fmx_set_option(b"upd_order", 1) == 2
