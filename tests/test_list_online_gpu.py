"""The FM's online list loop on the device: fmx_fm_list_online_run against N calls of fmx_fm_list_step on one list each, bit for
bit, and FMAdam.run_list_experiment against the loop of forward_fm + fit_lists.

The data are made so that the ORDER in which the table update adds a run's terms is exercised (a run: the occurrences of a field
that name the same row).  Fields 0, 1 are the context every row of a list shares (runs of G); field 2 gives the first three rows
of a list the rows 0, 1, 2 and every other row the row 3 -- three smaller rows in front of a run of G - 3; field 3 is an item
field of 3 rows, so negatives collide in runs that start anywhere; field 4 an item field of 40 rows; the fields behind them
(4 rows each) are drawn per row.  On the sorted list of a field, EPG = kp / 4 consecutive positions are a lane group:
run_geometry() finds, on the host, how many lane groups the longest-spanning run of the inputs covers and whether a run starts
off a group's first position, and the tests assert both where the shape allows them (a start off a multiple of EPG needs
EPG > 1: kp >= 8).  N <= 24 lists per case."""

import numpy as np
import pytest
import torch

from abi_geometry import PATTERN, Guarded
from test_kernels_gpu import HYP
from test_pair_gpu import RULES, build_table, clone_table, dev, same_bits

pytestmark = pytest.mark.gpu

N_LISTS = 24
FIELDS = {4: 70, 6: 40, 16: 39, 64: 14}      # k -> fields: 2, 2, 3 and 4 passes of a wave's lane groups (kp = 4, 8, 16, 64)


@pytest.fixture(scope="module")
def fmx():
    import fmx as _fmx
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _fmx


def make_sizes(F):
    return [7, 5, 4, 3, 40] + [4] * (F - 5)


def make_lists(sizes, N, G, seed, real_x):
    """-> (rows int32 [N G, F] local indices, x float32 [N G, F] or None), see the module's docstring"""
    rng = np.random.default_rng(seed)
    F = len(sizes)
    rows = np.stack([rng.integers(0, s, size=(N, G)) for s in sizes], axis=2)
    rows[:, :, :2] = rows[:, :1, :2]                                   # the shared context
    rows[:, :, 2] = np.minimum(np.arange(G), 3)[None, :]               # rows 0, 1, 2, then a run of row 3
    x = None
    if real_x:
        x = rng.uniform(0.5, 1.5, size=(N, G, F)).astype(np.float32)
        x[:, :, :2] = x[:, :1, :2]
        x = x.reshape(N * G, F)
    return rows.reshape(N * G, F).astype(np.int32), x


def run_geometry(rows, sizes, G, epg):
    """-> (the most lane groups one run spans, does a run start off a multiple of epg) over every list and field: a field's valid
    occurrences sorted by (row, list position), a run's first position = the occurrences with a smaller row."""
    most, off = 1, False
    for lst in rows.reshape(-1, G, rows.shape[1]):
        for f, size in enumerate(sizes):
            col = lst[:, f]
            col = col[(col >= 0) & (col < size)]
            for r in np.unique(col):
                a, L = int((col < r).sum()), int((col == r).sum())
                most = max(most, (a + L - 1) // epg - a // epg + 1)
                off = off or (L > 1 and a % epg != 0)
    return most, off


def put_the_best_row_first(eng, hyp, rows, x, G, lists):
    """In the first `lists` lists, the row the untrained table scores highest becomes the positive (so some positive ranks first);
    a list's rows stay the same set, so its runs stay what they were up to the order inside them."""
    idx_d, xv_d = dev(eng, rows, x)
    eng.forward(hyp, idx_d, xv_d)
    z = eng.logit[:rows.shape[0]].cpu().numpy().reshape(-1, G)
    for i in range(lists):
        j = int(np.argmax(z[i]))
        for a in (rows,) if x is None else (rows, x):
            a[[G * i, G * i + j]] = a[[G * i + j, G * i]]


def step_loop(fmx, eng, rule, idx_d, xv_d, G, N):
    """N calls of fmx_fm_list_step on one list each -> (logits [N G], losses [N]) of the steps' own forwards"""
    h, logits, losses = fmx.Hyper(**HYP), [], []
    for i in range(N):
        xi = None if xv_d is None else xv_d[G * i:G * (i + 1)]
        eng.list_step(h, rule, idx_d[G * i:G * (i + 1)], G, xi, inv_b=1.0)
        logits.append(eng.logit[:G].clone())
        losses.append(eng.loss_out.clone())
    return torch.cat(logits), torch.cat(losses)


def check_case(fmx, rule, k, G, F, N=N_LISTS):
    sizes = make_sizes(F)
    for real_x in (True, False):
        what = f"{rule} k={k} G={G} F={F} x={real_x}"
        t1, _ = build_table(fmx, sizes, k, RULES[rule])
        t2 = clone_table(fmx, t1)
        e1, e2 = fmx.FMEngine(t1, max_batch=N * G), fmx.FMEngine(t2, max_batch=16)
        assert e1.list_online_run_fits(F, t1.kp), what
        rows, x = make_lists(sizes, N, G, seed=100 * G + k, real_x=real_x)
        put_the_best_row_first(e1, fmx.Hyper(**HYP), rows, x, G, lists=4)
        # the inputs exercise the order of a run's additions (a condition on the data, checked here on the host)
        epg = t1.kp // 4
        most, off = run_geometry(rows, sizes, G, epg)
        if G >= 3 and epg == 1 or G == 16 and epg <= 4:
            assert most >= 3, (what, most)
        if G >= 5 and epg > 1:
            assert off, what
        idx_d, xv_d = dev(e1, rows, x)
        bias0, step0 = t1.bias.clone(), t1.step
        rank, logit, loss = e1.list_online_run(fmx.Hyper(**HYP), rule, idx_d, G, xv_d, want_logit=True, want_loss=True)
        logits2, losses2 = step_loop(fmx, e2, rule, idx_d, xv_d, G, N)
        torch.cuda.synchronize()
        e1.check_error_flag()
        e2.check_error_flag()
        same_bits(t1.rows, t2.rows, what + " rows")
        same_bits(t1.bias, t2.bias, what + " bias")
        same_bits(t1.bias, bias0, what + " bias unchanged")
        assert t1.step == t2.step == (step0 + N if RULES[rule] == "moments" else step0), what
        same_bits(logit, logits2, what + " logit_out")
        same_bits(loss, losses2, what + " loss_out")
        z = logits2.reshape(N, G)
        want_rank = (z[:, 1:] >= z[:, :1]).sum(dim=1).to(torch.uint8)
        assert torch.equal(rank.cpu(), want_rank.cpu()), what
        assert 0 < int((rank == 0).sum()) < N, (what, rank.tolist())


# ---- 1. the online loop is N steps of one list ----
@pytest.mark.parametrize("G", [2, 3, 5, 8, 16])
@pytest.mark.parametrize("rule", list(RULES))
def test_online_run_is_single_list_steps_rules(fmx, rule, G):
    check_case(fmx, rule, 16, G, 5 if G == 2 else FIELDS[16])


@pytest.mark.parametrize("G", [3, 8, 16])
@pytest.mark.parametrize("k", [4, 6, 16, 64])
@pytest.mark.parametrize("rule", ["signadam", "ftrl"])
def test_online_run_is_single_list_steps_widths(fmx, rule, k, G):
    check_case(fmx, rule, k, G, FIELDS[k])


def test_the_inputs_reach_three_lane_groups_and_odd_starts():
    """What the grid above relies on, stated once for kp = 4 and kp = 16 on the host: a run over at least three lane groups, and
    (where a lane group holds more than one position) a run that starts off a group's first position."""
    for k, epg in ((4, 1), (16, 4)):
        rows, _ = make_lists(make_sizes(FIELDS[k]), N_LISTS, 16, seed=1600 + k, real_x=False)
        most, off = run_geometry(rows, make_sizes(FIELDS[k]), 16, epg)
        assert most >= 3 and (off or epg == 1), (k, most, off)
    rows, _ = make_lists(make_sizes(FIELDS[4]), N_LISTS, 3, seed=304, real_x=False)
    assert run_geometry(rows, make_sizes(FIELDS[4]), 3, 1)[0] >= 3


# ---- 2. the bias ----
@pytest.mark.parametrize("rule", list(RULES))
def test_bias_and_its_state_stay_bit_unchanged(fmx, rule):
    sizes, G, N = make_sizes(5), 4, 12
    t, _ = build_table(fmx, sizes, 16, RULES[rule])
    eng = fmx.FMEngine(t, max_batch=N * G)
    rows, x = make_lists(sizes, N, G, seed=5, real_x=True)
    idx_d, xv_d = dev(eng, rows, x)
    bias0, rows0 = t.bias.clone(), t.rows.clone()
    eng.list_online_run(fmx.Hyper(**HYP), rule, idx_d, G, xv_d)
    torch.cuda.synchronize()
    eng.check_error_flag()
    same_bits(t.bias, bias0, rule + " bias")
    assert not torch.equal(t.rows, rows0)                               # ... while the rows moved


# ---- 3. an out-of-range index ----
def test_online_run_flags_and_drops_an_out_of_range_index(fmx):
    sizes, G, N, k = make_sizes(5), 4, 8, 16
    t1, _ = build_table(fmx, sizes, k, "weights")
    t2 = clone_table(fmx, t1)
    e1, e2 = fmx.FMEngine(t1, max_batch=N * G), fmx.FMEngine(t2, max_batch=16)
    rows, _ = make_lists(sizes, N, G, seed=6, real_x=False)
    rows[G * 3 + 2, 4] = sizes[4] + 3                                   # a negative of list 3
    idx_d, _ = dev(e1, rows, None)
    rank, logit, _ = e1.list_online_run(fmx.Hyper(**HYP), "signadam", idx_d, G, None, want_logit=True)
    torch.cuda.synchronize()
    assert int(e1.error.item()) == 1
    with pytest.raises(IndexError):
        e1.check_error_flag()
    logits2, _ = step_loop(fmx, e2, "signadam", idx_d, None, G, N)     # the steps drop the same occurrence
    torch.cuda.synchronize()
    with pytest.raises(IndexError):
        e2.check_error_flag()
    same_bits(t1.rows, t2.rows, "rows")
    same_bits(logit, logits2, "logit_out")
    wide = fmx.FlatTable([7] * 70, 16)
    e3 = fmx.FMEngine(wide, max_batch=4)
    with pytest.raises(fmx._lib.FmxError) as ei:
        e3.list_online_run(fmx.Hyper(**HYP), "sgd", torch.zeros((4, 70), dtype=torch.int32, device="cuda"), 2)
    assert ei.value.code == fmx._lib.ERR_UNSUPPORTED and not e3.list_online_run_fits(70, 16)


# ---- 4. guard bands, null optional outputs; 5. determinism ----
def test_guard_bands_null_outputs_and_determinism(fmx):
    L, lib = fmx._lib, fmx._lib.load()
    sizes, G, N, k = make_sizes(FIELDS[16]), 5, 8, 16
    rows, x = make_lists(sizes, N, G, seed=7, real_x=True)
    tables = []
    for with_outputs in (True, True, False):
        t, _ = build_table(fmx, sizes, k, "ftrl")
        eng = fmx.FMEngine(t, max_batch=N * G)
        idx_d, xv_d = dev(eng, rows, x)
        bufs = dict(rank=Guarded(N, torch.uint8, name="rank_out"), logit=Guarded(N * G * 4, name="logit_out"),
                    loss=Guarded(N * 4, name="loss_out"), error=Guarded(4, torch.int32, name="error"))
        hyp = fmx.Hyper(**HYP)
        rc = lib.fmx_fm_list_online_run(t.c_struct(), hyp.ref(), L.RULE_FTRL, idx_d.data_ptr(), xv_d.data_ptr(), N, G,
                                        bufs["rank"].ptr, bufs["logit"].ptr if with_outputs else None,
                                        bufs["loss"].ptr if with_outputs else None, bufs["error"].ptr, None)
        assert rc == L.OK, lib.fmx_last_error_string()
        torch.cuda.synchronize()
        for b in bufs.values():
            b.check()
        assert int(bufs["error"].t.item()) == 0
        if with_outputs:
            assert (bufs["logit"].t.view(torch.int32) != PATTERN).all() and (bufs["loss"].t > 0).all()
        else:
            assert not bufs["logit"].t.any() and not bufs["loss"].t.any()            # untouched
        tables.append((t, bufs))
    (ta, ba), (tb, bb), (tc, bc) = tables
    same_bits(ta.rows, tb.rows, "two calls from the same state: rows")
    same_bits(ba["logit"].t, bb["logit"].t, "logit_out")
    same_bits(ba["loss"].t, bb["loss"].t, "loss_out")
    assert torch.equal(ba["rank"].t, bb["rank"].t) and torch.equal(ba["rank"].t, bc["rank"].t)
    same_bits(ta.rows, tc.rows, "without the optional outputs: rows")


# ---- 6. the class ----
SMALL = [7, 5, 11, 3, 6]
ITEM = [2, 3]


def new_model(rule, k=10, seed=21):
    from models.models_online_deep.fm_adam import FMAdam
    torch.manual_seed(seed)
    return FMAdam(SMALL, embedding_size=k, n=0.01, update_rule=rule)


def class_data(N, n_neg, seed=4):
    rng = np.random.default_rng(seed)
    Xi = np.stack([rng.integers(0, s, N) for s in SMALL], axis=1).astype(np.int64)
    Xv = rng.uniform(0.5, 1.5, (N, len(SMALL))).astype(np.float32)
    neg = np.stack([rng.integers(0, SMALL[f], (N, n_neg)) for f in ITEM], axis=2).astype(np.int64)
    return Xi, Xv, neg


def host_loop(fmx, m, Xi, Xv, neg):
    """forward_fm + fit_lists, one list at a time -> the number of positives that rank first"""
    correct = 0
    for i in range(len(Xi)):
        rows, xv = fmx.pairwise.assemble_lists(torch.from_numpy(Xi[i:i + 1]), torch.from_numpy(Xv[i:i + 1]), ITEM, torch.from_numpy(neg[i:i + 1]))
        z = m.forward_fm(rows.numpy(), xv.numpy())
        correct += int(int((z[1:] >= z[0]).sum()) == 0)
        m.fit_lists(Xi[i:i + 1], Xv[i:i + 1], ITEM, negatives=neg[i:i + 1])
    return correct


@pytest.mark.parametrize("rule", ["signadam", "adam"])
def test_run_list_experiment_is_the_host_loop(fmx, rule):
    N, n_neg = 40, 4
    Xi, Xv, neg = class_data(N, n_neg, seed=8)
    a, b, c = new_model(rule), new_model(rule), new_model(rule)
    assert a._device_loop_ok() and a._engine.list_online_run_fits(a.field_size, a._table.kp)
    secs, acc, checkpoints, counts = a.run_list_experiment(Xi, Xv, ITEM, negatives=neg)
    correct = host_loop(fmx, b, Xi, Xv, neg)
    torch.cuda.synchronize()
    same_bits(a._table.rows, b._table.rows, "rows")
    same_bits(a._table.bias, b._table.bias, "bias")
    assert counts == {"correct": correct, "wrong": N - correct} and a._table.step == b._table.step
    assert 0 < correct < N
    assert acc == checkpoints[-1] == pytest.approx(100.0 * correct / N) and len(checkpoints) == 2 and secs > 0
    # the same call where the device loop is not taken: the loop over fit_lists inside run_list_experiment
    c.device_online_loop = False
    _, acc_c, cp_c, counts_c = c.run_list_experiment(Xi, Xv, ITEM, negatives=neg)
    same_bits(a._table.rows, c._table.rows, "rows (host loop)")
    same_bits(a._table.bias, c._table.bias, "bias (host loop)")
    assert counts_c == counts and cp_c == checkpoints and acc_c == acc and c._table.step == a._table.step
    # a table whose sort fields are split takes the host loop too, and agrees with forward_fm + fit_lists on such a table
    d, e = new_model(rule), new_model(rule)
    for m in (d, e):
        m._table.sort_cap_override = 4
        m._table.ensure_sort_split(m._engine.max_batch)
        assert m._table._sort_split is not None and m._device_loop_ok()
        assert not m._engine.list_online_run_fits(m.field_size, m._table.kp)
    _, _, _, counts_d = d.run_list_experiment(Xi, Xv, ITEM, negatives=neg)
    correct_e = host_loop(fmx, e, Xi, Xv, neg)
    torch.cuda.synchronize()
    same_bits(d._table.rows, e._table.rows, "rows (split table)")
    assert counts_d == {"correct": correct_e, "wrong": N - correct_e}
    with pytest.raises(IndexError):
        a.run_list_experiment(Xi, Xv, ITEM, negatives=neg + 100)


def test_run_list_experiment_uniform_and_hard_negatives_are_reproducible(fmx):
    N = 40
    Xi, Xv, _ = class_data(N, 1, seed=9)
    Xv[:, ITEM[0]] = 1.0                       # (the mined candidates are scored with value 1 in the item column)
    hard = lambda: fmx.pairwise.HardNegatives(n_draw=8, remine_every=16)
    for negatives, item in ((None, ITEM), ("hard", [ITEM[0]])):
        out = []
        for seed in (5, 5, 6):
            m = new_model("signadam")
            g = torch.Generator(device="cuda").manual_seed(seed)
            res = m.run_list_experiment(Xi, Xv, item, negatives=hard() if negatives else None, n_neg=3, generator=g)
            torch.cuda.synchronize()
            assert res[3]["correct"] + res[3]["wrong"] == N
            if negatives:
                assert m._mining_offset == 3                               # blocks of 16, 16 and 8 positives
            out.append((m, res))
        same_bits(out[0][0]._table.rows, out[1][0]._table.rows, f"{negatives}: the same seed")
        assert out[0][1][1:] == out[1][1][1:]
        assert not torch.equal(out[0][0]._table.rows, out[2][0]._table.rows), f"{negatives}: another seed"
