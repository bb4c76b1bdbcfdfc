"""The two forms of the table update on the MI355X, through the C ABI: runs that cross a 64-entry tile are finished inside the
launch (fmx_set_option("inline_fixup", 1), the default) or by a second launch, k_fm_fixup ("inline_fixup", 0 -- and every stream
that is being captured).  csrc/fmx_update.hip promises the same bits from both, so every case here runs the same steps twice from
the same state and compares table rows, bias, per-step losses, network / attention parameters and the error word BIT FOR BIT, and
asserts that the steps moved the table.  Where a float64 statement of the step exists the result is also held to it, with that
statement's own tolerance (1e-5 relative plus the fp32 floor it derives), under both forms.

The inputs come from update_forms.py, and test_update_forms_cpu.py shows on numpy's sort what they reach.  From B = 4161 on a
one-row field's head tile has 65 or more tiles behind it (the second iteration of k_fm_fixup's walk over the meta words; 192 at
12,289, 511 at 32,768) -- re-asserted here on the lists the device's sort left; every B > 4096 runs k_fm_fixup's extra workgroup
and the slices of the bias / loss reduction; 4097 leaves a last slice of one sample and lists that are half padding; the field of
64 occurrences per row ends every run on a tile's last entry.

What each test instantiates with INL = false (update_body / k_fm_fixup; slices = red_slices(B)):
  test_pointwise_*                      k_fm_update<LPR 1 | 4 | 16, WEIGHTS sgd / signadam | FTRL | MOMENTS adam / adagrad, HAS_GBI 0>,
                                        k_fm_fixup of the same; 2 slices (4097, 5000, 8192), 4 (12,289: LPR 4), 8 (32,768: LPR 2)
  test_pair_and_list_*                  the same kernels under fmx_fm_pair_step / _list_step / _list_step_q, LPR 4, FTRL and sgd, 2 slices
  test_network_gradient_*               HAS_GBI 1, LPR 4, sgd and FTRL, 1 slice (300) and 2 (4097)
  test_rider_fallback_*                 HAS_GBI 1 behind mlp_launch_reduce (no k_fm_update_rider), LPR 4, FTRL and MOMENTS adam, 1 slice
  test_occurrence_gradient_*            k_fm_update_occ<LPR 2, sgd | FTRL, INL false>, 1 slice (130) and 2 (4097 / 4098 / 4100)
  test_strided_records_*                sample_ld = kp + 4, LPR 4, FTRL, 2 slices
  test_mapped_table_and_sort_pieces_*   cols != null (a mapped table with an empty field; sort pieces of at most 1,000 rows), LPR 4, FTRL, 2 slices
  test_dispatch_orders_*                ordered = 0 and 1 (upd_order 0, 1, 2), LPR 4, FTRL, 2 slices
  test_queued_online_loop_*             HAS_GBI 1 at B = 1 (fmx_online_run_mlp's per-sample launches), LPR 4, signadam

A head's walk never ends on LEAD_NONE: a tile is open only when the next one starts with its last key, so every head has m >= 1 and
"the head's own trail record only" cannot occur -- a run that ends on a tile's last entry leaves trail = 0 and k_fm_fixup's wave
of that tile returns (the 64-per-row field: no record is handed over at all when B is a multiple of 64).

The tests can fail: with k_fm_fixup changed to stop a walk that reached its second iteration one tile early, [ftrl-16-5000] of
test_pointwise_forms_give_identical_bits differs in 21,713 words ([ftrl-16-4097], whose longest walk is 64 tiles, passes); with
its extra workgroup skipping the last slice, [ftrl-16-4097] differs and test_pointwise_within_float64[ftrl-4097-0] misses the
float64 step (form 1 passes)."""
import numpy as np
import pytest
import torch

import update_forms as uf
from helpers import assert_ftrl_step_within_f64, assert_within_f64
from list_f64 import list_step_f64
from listq_f64 import listq_step_f64
from oracle import fm_oracle as orc
from pair_f64 import pair_step_f64
from test_adaptive_rules_cpu import flat_adaptive_step
from test_adaptive_rules_gpu import HYP as AHYP, assert_step, moments_table, state_of
from test_kernels_gpu import HYP, check_weights_after, close, ftrl_state, ftrl_table, make_problem, weights_table
from test_pair_gpu import build_table

pytestmark = pytest.mark.gpu

LAYOUT = {"sgd": "weights", "signadam": "weights", "ftrl": "ftrl", "adam": "moments", "adagrad": "moments"}
RULES = list(LAYOUT)
FTRL_H = {kk: HYP[kk] for kk in ("alpha", "beta", "l1", "l2")}
N_STEPS = 3
FORMS = (0, 1)          # inline_fixup: 0 the second launch, 1 the in-launch hand-off


@pytest.fixture(scope="module")
def fmx():
    import fmx as _fmx
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _fmx


def hyper_for(fmx, rule):
    if LAYOUT[rule] == "moments":
        h = AHYP[rule]
        return fmx.Hyper(lr=h["lr"], eps=h["eps"], beta1=h["beta1"], beta2=h["beta2"])
    return fmx.Hyper(**HYP)


def problem(sizes, k, B, seed, real_x, kinds=None):
    """test_kernels_gpu.make_problem's weights, labels and feature values around the generator's indices."""
    pr = make_problem(sizes, k, B, seed, real_x=real_x)
    pr["idx"] = uf.indices(sizes, B, seed, kinds)
    pr["rows"] = pr["idx"].astype(np.int64) + pr["offs"][:-1][None, :]
    return pr


def table_for(fmx, rule, sizes, k, pr, **kw):
    if LAYOUT[rule] == "weights":
        return weights_table(fmx, sizes, k, pr)
    if LAYOUT[rule] == "ftrl":
        return ftrl_table(fmx, sizes, k, ftrl_state(pr, HYP))
    return moments_table(fmx, sizes, k, seed=7)


def snap(t, eng, losses, **more):
    out = dict(rows=t.rows.clone(), bias=t.bias.clone(), loss=torch.stack([l.reshape(()) for l in losses]),
               error=eng.error.clone())
    out.update({kk: v.clone() for kk, v in more.items()})
    return out


def both_forms(fmx, run, what, moved=True):
    """run() under inline_fixup = 0 and 1 -> the two snapshots, compared bit for bit; the error word 0; the table trained."""
    lib = fmx._lib.load()
    res = []
    for form in FORMS:
        with uf.option(lib, "inline_fixup", form):
            res.append(run())
            torch.cuda.synchronize()
    for r in res:
        assert int(r["error"].item()) == 0, f"{what}: error word {int(r['error'].item())}"
        assert bool(torch.isfinite(r["loss"]).all()) and bool(torch.isfinite(r["rows"]).all()), what
    uf.same(res[1], res[0], what + ": in-launch hand-off against the second launch")
    if moved:
        assert not torch.equal(res[0]["rows"], res[0]["rows0"]), what + ": the steps did not move the table"
    return res


def assert_long_heads(eng, B, what):
    """On the lists the device's sort left: a head tile with 65 or more tiles behind it (B >= 4161)."""
    best = max(r["max_m"] for r in uf.heads_on_device(eng, B))
    assert best >= (65 if B >= 4161 else (B + 63) // 64 - 1), f"{what}: the longest hand-over spans {best} tiles"
    return best


# ---------------------------------------------------------------------------------------------------------------
# pointwise steps, every layout
# ---------------------------------------------------------------------------------------------------------------
def pointwise_case(fmx, rule, k, B, F=8, kinds=None, n_steps=N_STEPS):
    sizes = uf.field_sizes(B, F, kinds)
    real_x = (RULES.index(rule) + k // 4 + B) % 2 == 1
    pr = problem(sizes, k, B, seed=B + k, real_x=real_x, kinds=kinds)
    hyp = hyper_for(fmx, rule)
    what = f"{rule} k={k} B={B} x={real_x}"
    seen = {}

    def run():
        t = table_for(fmx, rule, sizes, k, pr)
        rows0 = t.rows.clone()
        eng = fmx.FMEngine(t, max_batch=B)
        assert t._sort_split is None
        idx_d, xv_d, y_d = eng.to_device(pr["idx"], pr["x"], pr["y"])
        losses = []
        for _ in range(n_steps):
            eng.step(hyp, rule, "logits", idx_d, xv_d, y_d)
            losses.append(eng.loss_out.clone())
        seen["m"] = assert_long_heads(eng, B, what)
        return snap(t, eng, losses, rows0=rows0)

    both_forms(fmx, run, what)
    return seen["m"]


@pytest.mark.parametrize("B", [4097, 5000, 8192])
@pytest.mark.parametrize("k", [4, 16, 64])
@pytest.mark.parametrize("rule", RULES)
def test_pointwise_forms_give_identical_bits(fmx, rule, k, B):
    """LPR 1, 4 and 16 lanes per row; two slices of the batch (one sample in the second at 4097); feature values for half."""
    pointwise_case(fmx, rule, k, B, F=6 if k == 64 else 8)


@pytest.mark.parametrize("rule", ["ftrl", "adam"])
def test_pointwise_forms_four_slices_and_192_tiles(fmx, rule):
    assert pointwise_case(fmx, rule, 16, 12289, F=6) >= 129


@pytest.mark.parametrize("rule", ["ftrl", "adam"])
def test_pointwise_forms_at_the_largest_batch(fmx, rule):
    """32,768 samples: eight slices, 512 tiles per field, the one-row field's head adds 511 records in eight iterations."""
    assert pointwise_case(fmx, rule, 8, 32768, kinds=("one", "tiles", "uniform")) == 511


_F64 = {}


def f64_case(rule, B):
    """(sizes, problem, float64 reference of the FIRST step) of a shape: computed once, shared by the two forms."""
    key = (rule, B)
    if key not in _F64:
        k = 16
        sizes = uf.field_sizes(B, 6)
        pr = problem(sizes, k, B, seed=3 * B + 1, real_x=(B == 5000))
        x = pr["x"] if pr["x"] is not None else np.ones(pr["idx"].shape, np.float32)
        ref = None
        if rule == "ftrl":
            ref = orc.flat_fm_step_f64(ftrl_state(pr, HYP), pr["rows"], x, pr["y"], "logits", "ftrl", FTRL_H)
        elif rule == "sgd":
            state = dict(V=pr["V"].copy(), w=pr["w"].copy(), bias=np.float32(pr["bias"]))
            ref = (state, orc.flat_fm_step(state, pr["rows"], x, pr["y"], "logits", "sgd", dict(lr=HYP["lr"])))
        _F64[key] = (sizes, pr, x, ref)
    return _F64[key]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("B", [4097, 5000, 12289])
@pytest.mark.parametrize("rule", ["ftrl", "sgd", "adam", "adagrad"])
def test_pointwise_within_float64(fmx, rule, B, form):
    """Ragged batches above one slice against the float64 statement of the step, under both forms: a last slice of 1, 904 and 1
    samples, lists of 8,192 and 16,384 entries that are up to half padding.  ftrl: oracle.flat_fm_step_f64 and its floors; sgd:
    the oracle's step and check_weights_after's bound; adam / adagrad: test_adaptive_rules' float64 statement, two steps."""
    k = 16
    sizes, pr, x, ref = f64_case(rule, B)
    with uf.option(fmx._lib.load(), "inline_fixup", form):
        t = table_for(fmx, rule, sizes, k, pr)
        eng = fmx.FMEngine(t, max_batch=B)
        idx_d, xv_d, y_d = eng.to_device(pr["idx"], pr["x"], pr["y"])
        hyp = hyper_for(fmx, rule)
        what = f"{rule} B={B} inline_fixup={form}"
        if LAYOUT[rule] == "moments":
            for s in (1, 2):
                before = state_of(t)
                eng.step(hyp, rule, "logits", idx_d, xv_d, y_d)
                torch.cuda.synchronize()
                want, urows, ex = flat_adaptive_step(before, pr["rows"], x, pr["y"], "logits", rule, AHYP[rule], s)
                assert_step(before, state_of(t), want, urows, ex, rule, AHYP[rule], s, what=f"{what} step {s}")
            eng.check_error_flag()
            return
        eng.step(hyp, rule, "logits", idx_d, xv_d, y_d)
        torch.cuda.synchronize()
        eng.check_error_flag()
        loss = float(eng.loss_out.item())
    if rule == "ftrl":
        st0 = ftrl_state(pr, HYP)
        assert_within_f64(loss, ref["loss"], ref["floor"]["loss"], what + " loss")
        zV, nV, zw, nw = [a.numpy() for a in t.export_ftrl_state()]
        assert_ftrl_step_within_f64(dict(zV=zV, nV=nV, zw=zw, nw=nw, zb=t.bias[0].item(), nb=t.bias[1].item()), ref, what + " ",
                                    before=st0)
        return
    state, out = ref
    close(loss, out["loss"], 1e-5, 1e-7, what + " mean loss")
    check_weights_after(pr, t, state, out, "sgd", k)


# ---------------------------------------------------------------------------------------------------------------
# pair and list objectives: full-width lists of more than 4,096 rows
# ---------------------------------------------------------------------------------------------------------------
def objective_inputs(rows_n, seed):
    sizes = uf.field_sizes(rows_n, 6)
    idx = uf.indices(sizes, rows_n, seed)
    x = np.random.default_rng(seed + 1).uniform(0.5, 1.5, size=idx.shape).astype(np.float32)
    corr = np.random.default_rng(seed + 2).uniform(-8.0, 0.0, rows_n).astype(np.float32)
    return sizes, idx, x, corr


def objective_step(eng, hyp, entry, rule, idx_d, xv_d, corr_d, G):
    if entry == "pair":
        eng.pair_step(hyp, rule, idx_d, xv_d, margin=0.1)
    elif entry == "list":
        eng.list_step(hyp, rule, idx_d, G, xv_d)
    else:
        eng.list_step_q(hyp, rule, idx_d, G, corr_d, xv_d)


OBJECTIVES = [("pair", 2 * 2049, 2), ("pair", 2 * 2500, 2), ("list", 5 * 820, 5), ("listq", 5 * 820, 5)]


@pytest.mark.parametrize("rule", ["ftrl", "sgd"])
@pytest.mark.parametrize("entry,rows_n,G", OBJECTIVES)
def test_pair_and_list_forms_give_identical_bits(fmx, entry, rows_n, G, rule):
    """fmx_fm_pair_step at 2,049 and 2,500 pairs, fmx_fm_list_step / _q at 820 lists of 5: 4,098 / 5,000 / 4,100 rows."""
    k = 16
    sizes, idx, x, corr = objective_inputs(rows_n, seed=rows_n)
    hyp = fmx.Hyper(**HYP)
    what = f"{entry} {rule} rows={rows_n}"

    def run():
        t, _ = build_table(fmx, sizes, k, LAYOUT[rule], seed=7)
        rows0 = t.rows.clone()
        eng = fmx.FMEngine(t, max_batch=rows_n)
        idx_d, xv_d, _ = eng.to_device(idx, x)
        corr_d = torch.from_numpy(corr).cuda()
        losses = []
        for _ in range(N_STEPS):
            objective_step(eng, hyp, entry, rule, idx_d, xv_d, corr_d, G)
            losses.append(eng.loss_out.clone())
        if entry == "pair":                              # (the list steps sort into a workspace of their own)
            assert_long_heads(eng, rows_n, what)
        return snap(t, eng, losses, rows0=rows0)

    both_forms(fmx, run, what)


@pytest.mark.parametrize("entry,rows_n,G,rule", [("pair",2 * 2049, 2, "ftrl"), ("list", 5 * 820, 5, "sgd"), ("listq", 5 * 820, 5, "ftrl")])
def test_pair_and_list_second_launch_within_float64(fmx, entry, rows_n, G, rule):
    """One step of each objective in the two-launch form against pair_f64 / list_f64 / listq_f64 and their floors."""
    k = 16
    sizes, idx, x, corr = objective_inputs(rows_n, seed=rows_n)
    with uf.option(fmx._lib.load(), "inline_fixup", 0):
        t, pr = build_table(fmx, sizes, k, LAYOUT[rule], seed=7)
        eng = fmx.FMEngine(t, max_batch=rows_n)
        idx_d, xv_d, _ = eng.to_device(idx, x)
        objective_step(eng, fmx.Hyper(**HYP), entry, rule, idx_d, xv_d, torch.from_numpy(corr).cuda(), G)
        torch.cuda.synchronize()
        eng.check_error_flag()
    grows = idx.astype(np.int64) + np.asarray(t.offsets_host[:-1], np.int64)[None, :]
    st0 = pr["ftrl_state"] if rule == "ftrl" else dict(V=pr["V"], w=pr["w"], bias=pr["bias"])
    h = FTRL_H if rule == "ftrl" else dict(lr=HYP["lr"])
    n = rows_n // G
    if entry == "pair":
        ref = pair_step_f64(st0, grows, x, 0.1, rule, h, inv_b=1.0 / n)
    elif entry == "list":
        ref = list_step_f64(st0, grows, x, G, rule, h, inv_b=1.0 / n)
    else:
        ref = listq_step_f64(st0, grows, x, G, corr, rule, h, inv_b=1.0 / n)
    assert_within_f64(float(eng.loss_out.item()), ref["loss"], ref["floor"]["loss"], f"{entry} loss")
    if rule == "ftrl":
        zV, nV, zw, nw = [a.numpy() for a in t.export_ftrl_state()]
        assert_ftrl_step_within_f64(dict(zV=zV, nV=nV, zw=zw, nw=nw, zb=t.bias[0].item(), nb=t.bias[1].item()), ref, entry + " ",
                                    before=st0)
        return
    u, new, fl = ref["urows"], ref["new"], ref["floor"]
    got = dict(V=t.rows[:, :k].cpu().numpy(), w=t.rows[:, t.kp].cpu().numpy())
    for kk in ("V", "w"):
        b0 = np.asarray(st0[kk], np.float64)[u]
        assert_within_f64(got[kk][u], new[kk][u], fl[kk], f"{entry} {kk}")
        assert_within_f64(got[kk][u].astype(np.float64) - b0, new[kk][u] - b0, fl[kk], f"{entry} {kk} (the step)")
        mask = np.ones(len(got[kk]), bool)
        mask[u] = False
        np.testing.assert_array_equal(got[kk][mask], st0[kk][mask], err_msg=kk + " untouched rows")
        assert np.abs(new[kk][u] - b0).max() > 0


# ---------------------------------------------------------------------------------------------------------------
# the network gradient (HAS_GBI), strided records, mapped tables and sort pieces, the dispatch order
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [300, 4097])
@pytest.mark.parametrize("rule", ["sgd", "ftrl"])
def test_network_gradient_forms_give_identical_bits(fmx, rule, B):
    """fmx_fm_update with gbi (G[b, d] = dz_bi[b] + gbi[b, d], a first-order coefficient of its own), as the DeepFM / NFM callers
    issue it: sort, forward, update."""
    k = 16
    sizes = uf.field_sizes(B, 6)
    pr = problem(sizes, k, B, seed=21 + B, real_x=True)
    rng = np.random.default_rng(4)
    dz_first = torch.from_numpy((rng.normal(size=B) * 0.1).astype(np.float32)).cuda()
    dz_bi = torch.from_numpy((rng.normal(size=B) * 0.1).astype(np.float32)).cuda()
    hyp = fmx.Hyper(**HYP)

    def run():
        t = table_for(fmx, rule, sizes, k, pr)
        rows0 = t.rows.clone()
        eng = fmx.FMEngine(t, max_batch=B)
        gbi = torch.zeros((B, t.kp), device="cuda")
        gbi[:, :k] = torch.from_numpy((np.random.default_rng(5).normal(size=(B, k)) * 0.1).astype(np.float32)).cuda()
        idx_d, xv_d, y_d = eng.to_device(pr["idx"], pr["x"], pr["y"])
        losses = []
        for s in range(N_STEPS):
            eng.sort(idx_d)
            eng.forward(hyp, idx_d, xv_d, y_d, loss="logits")
            eng.update(hyp, rule, B, xv_d, dz_first, dz_bi if s != 1 else None, gbi)
            losses.append(eng.loss_out.clone())
        return snap(t, eng, losses, rows0=rows0)

    both_forms(fmx, run, f"network gradient {rule} B={B}")


def test_strided_records_forms_give_identical_bits(fmx):
    """The owner step's records (sample_ld > 0): S, dlogit and loss are fields of one record of kp + 4 floats per sample."""
    rule, k, B = "ftrl", 16, 4097
    sizes = uf.field_sizes(B, 6)
    pr = problem(sizes, k, B, seed=9, real_x=False)
    hyp = fmx.Hyper(**HYP)

    def run():
        t = table_for(fmx, rule, sizes, k, pr)
        rows0 = t.rows.clone()
        eng = fmx.FMEngine(t, max_batch=B)
        rec = torch.zeros((B, t.kp + 4), device="cuda")
        idx_d, _, y_d = eng.to_device(pr["idx"], None, pr["y"])
        losses = []
        for _ in range(N_STEPS):
            eng.sort(idx_d)
            eng.forward(hyp, idx_d, None, y_d, loss="logits", records=rec, want_first=False, want_bi=False)
            eng.update(hyp, rule, B, None, None, records=rec)
            losses.append(eng.loss_out.clone())
        return snap(t, eng, losses, rows0=rows0, records=rec)

    strided = both_forms(fmx, run, "strided records")[0]

    def plain():
        t = table_for(fmx, rule, sizes, k, pr)
        eng = fmx.FMEngine(t, max_batch=B)
        idx_d, _, y_d = eng.to_device(pr["idx"], None, pr["y"])
        losses = []
        for _ in range(N_STEPS):
            eng.step(hyp, rule, "logits", idx_d, None, y_d)
            losses.append(eng.loss_out.clone())
        torch.cuda.synchronize()
        return snap(t, eng, losses)

    ref = plain()                                      # the records hold what the dense buffers hold: the plain step's bits
    uf.same({kk: strided[kk] for kk in ref}, ref, "strided records against fmx_fm_step")


MAPPED_B = 4161


@pytest.mark.parametrize("kind", ["mapped", "pieces"])
def test_mapped_table_and_sort_pieces_forms_give_identical_bits(fmx, kind):
    """cols != null in the update: a mapped table (field_cols / field_base) with an empty field, and a plain one whose large
    field is cut into sort pieces of at most 1,000 rows."""
    rule, k, B = "ftrl", 16, MAPPED_B
    sizes = uf.field_sizes(B, 6)
    idx = uf.indices(sizes, B, seed=2)
    kw = {}
    if kind == "mapped":
        sizes = sizes[:3] + [0] + sizes[3:]
        idx = np.concatenate([idx[:, :3], np.zeros((B, 1), np.int32), idx[:, 3:]], axis=1)
        kw = dict(field_cols=list(range(len(sizes))), field_base=[0] * len(sizes), n_cols=len(sizes))
    y = (np.random.default_rng(3).uniform(size=B) < 0.3).astype(np.float32)
    hyp = fmx.Hyper(**HYP)

    def run():
        t = fmx.FlatTable(sizes, k, layout="ftrl", ftrl=HYP, **kw)
        gen = torch.Generator(device="cuda").manual_seed(7)
        V0 = torch.randn((t.n_rows, k), device="cuda", generator=gen) * 0.1
        t.rows[:, :k] = V0
        t.rows[:, t.kp] = torch.randn(t.n_rows, device="cuda", generator=gen) * 0.1
        t.rows[:, t.z_offset:t.z_offset + k] = fmx.table.ftrl_z_for_weight_torch(V0, t.ftrl)
        t.bias[0] = -0.4
        if kind == "pieces":
            t.sort_cap_override = 1000
        rows0 = t.rows.clone()
        eng = fmx.FMEngine(t, max_batch=B)
        assert (t._sort_split is not None) == (kind == "pieces")
        idx_d, _, y_d = eng.to_device(idx, None, y)
        losses = []
        for _ in range(N_STEPS):
            eng.step(hyp, rule, "logits", idx_d, None, y_d)
            losses.append(eng.loss_out.clone())
        assert_long_heads(eng, B, kind)
        return snap(t, eng, losses, rows0=rows0)

    both_forms(fmx, run, kind)


def test_dispatch_orders_and_forms_give_identical_bits(fmx):
    """upd_order 0 (index order), 1 (ascending row count) and 2 (descending) under both forms: six runs, one result."""
    rule, k, B = "ftrl", 16, 4161
    sizes = uf.field_sizes(B, 8)
    pr = problem(sizes, k, B, seed=6, real_x=True)
    hyp = fmx.Hyper(**HYP)
    lib = fmx._lib.load()
    res = {}
    for order in (0, 1, 2):
        for form in FORMS:
            with uf.option(lib, "upd_order", order), uf.option(lib, "inline_fixup", form):
                t = table_for(fmx, rule, sizes, k, pr)
                rows0 = t.rows.clone()
                eng = fmx.FMEngine(t, max_batch=B)
                idx_d, xv_d, y_d = eng.to_device(pr["idx"], pr["x"], pr["y"])
                losses = []
                for _ in range(N_STEPS):
                    eng.step(hyp, rule, "logits", idx_d, xv_d, y_d)
                    losses.append(eng.loss_out.clone())
                torch.cuda.synchronize()
                res[(order, form)] = snap(t, eng, losses)
    ref = res[(0, 0)]
    assert int(ref["error"].item()) == 0 and not torch.equal(ref["rows"], rows0)
    for cfg, r in res.items():
        uf.same(r, ref, f"(upd_order, inline_fixup) = {cfg}")


# ---------------------------------------------------------------------------------------------------------------
# the rider's fallback: the MLP's gradient reduction as a launch of its own in front of the update
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["deepfm_stream", "deepfm_stream_opt", "deepfm_pair_stream"])
def test_rider_fallback_gives_identical_bits(fmx, entry):
    """fmx_deepfm_stream / _opt / _pair_stream: with the hand-off the reduction rides in the update's launch
    (k_fm_update_rider); without it update_impl issues mlp_launch_reduce first and the two-launch update behind it."""
    k, H, L, B, n_pool, n_steps = 16, 32, 2, 512, 3, 9
    rule = "adam" if entry == "deepfm_stream_opt" else "ftrl"
    sizes = uf.field_sizes(B, 6)
    idx = np.stack([uf.indices(sizes, B, seed=30 + j) for j in range(n_pool)])
    y = (np.random.default_rng(8).uniform(size=(n_pool, B)) < 0.3).astype(np.float32)
    pr = problem(sizes, k, B, seed=12, real_x=False)
    n_params = H * k + H + H * H + H

    def run():
        t = table_for(fmx, rule, sizes, k, pr)
        rows0 = t.rows.clone()
        eng = fmx.FMEngine(t, max_batch=B)
        params = (torch.randn(n_params, generator=torch.Generator().manual_seed(1)) * (1.0 / np.sqrt(H))).cuda()
        params0 = params.clone()
        grads = torch.zeros_like(params)
        loss = torch.zeros(n_steps, device="cuda")
        idx_d, y_d = torch.from_numpy(idx).cuda(), torch.from_numpy(y).cuda()
        hyp = hyper_for(fmx, rule)
        more = {}
        if entry == "deepfm_stream":
            go = eng.prepare_deepfm_stream(hyp, rule, "sigmoid", params, grads, k, H, L, 0.05, idx_d, y_d, loss_out=loss)
        elif entry == "deepfm_stream_opt":
            opt = fmx.MlpOpt(n_params, "adam", lr=0.01, device="cuda")
            go = eng.prepare_deepfm_stream(hyp, rule, "sigmoid", params, grads, k, H, L, 0.0, idx_d, y_d, loss_out=loss, mlp_opt=opt)
            more = dict(opt_m=opt.m, opt_v=opt.v)
        else:
            go = eng.prepare_deepfm_pair_stream(hyp, rule, params, grads, k, H, L, 0.05, idx_d, margin=0.1, loss_out=loss)
        go(n_steps)
        torch.cuda.synchronize()
        assert not torch.equal(params, params0), "the network did not train"
        return dict(rows=t.rows.clone(), bias=t.bias.clone(), loss=loss, error=eng.error.clone(), params=params, rows0=rows0,
                    **{kk: v.clone() for kk, v in more.items()})

    both_forms(fmx, run, entry)


# ---------------------------------------------------------------------------------------------------------------
# occurrence gradients: every AFM step
# ---------------------------------------------------------------------------------------------------------------
AFM_ENTRIES = [("step", "sgd"), ("step", "ftrl"), ("step_opt", "sgd"), ("pair_step", "ftrl"), ("list_step", "sgd")]


@pytest.mark.parametrize("B", [130, 4097])
@pytest.mark.parametrize("entry,rule", AFM_ENTRIES)
def test_occurrence_gradient_forms_give_identical_bits(fmx, entry, rule, B):
    """k_fm_update_occ<..., INL = false>: fmx_afm_step, _step_opt (adam on the attention parameters), _pair_step, _list_step
    (G = 5) at F = 6, k = 8, t = 8; the pair and list forms round B to whole pairs / lists (130 / 4,098 and 130 / 4,100 rows)."""
    import test_afm_gpu as ta
    from fmx.afm import AfmOpt, afm_param_count
    k, tt, G = 8, 8, 5
    rows_n = {"pair_step": B + B % 2, "list_step": (B + G - 1) // G * G}.get(entry, B)
    sizes = uf.field_sizes(rows_n, 6)
    idx = uf.indices(sizes, rows_n, seed=B)
    rng = np.random.default_rng(B + 1)
    xv = rng.uniform(0.2, 1.8, size=idx.shape).astype(np.float32)
    y = (rng.uniform(size=rows_n) < 0.4).astype(np.float32)
    hyp_kw = dict(ta.HYP, lr=0.01)

    def run():
        tb, params, _ = ta.make(sizes, k, tt, layout=LAYOUT[rule], seed=3)
        rows0 = tb.rows.clone()
        eng = ta.engine(tb, params, tt, rows_n)
        idx_d, xv_d, y_d = eng.to_device(idx, xv, y)
        hyp = fmx.Hyper(**hyp_kw)
        opt = AfmOpt(afm_param_count(k, tt), "adam", lr=0.01, device="cuda") if entry == "step_opt" else None
        losses = []
        for _ in range(N_STEPS):
            if entry in ("step", "step_opt"):
                eng.step(hyp, rule, idx_d, xv_d, y_d, opt=opt)
            elif entry == "pair_step":
                eng.pair_step(hyp, rule, idx_d, xv_d, margin=0.1)
            else:
                eng.list_step(hyp, rule, idx_d, G, xv_d)
            losses.append(eng.loss_out.clone())
        torch.cuda.synchronize()
        more = dict(opt_m=opt.m, opt_v=opt.v) if opt is not None else {}
        return snap(tb, eng, losses, rows0=rows0, grad=eng.grad, params=params, **more)

    res = both_forms(fmx, run, f"afm {entry} {rule} rows={rows_n}")
    assert bool(res[0]["grad"].abs().max() > 0)


def test_occurrence_gradient_second_launch_within_float64(fmx):
    """fmx_afm_step in the two-launch form against afm_f64: 130 samples, a one-row field and two hot rows whose runs cross the tiles."""
    import test_afm_gpu as ta
    with uf.option(fmx._lib.load(), "inline_fixup", 0):
        ta._step_and_check("sgd", [2, 1, 50, 3, 20011, 3000], 8, 8, 130, hot=True, seed=5)


# ---------------------------------------------------------------------------------------------------------------
# the queued online form, the option
# ---------------------------------------------------------------------------------------------------------------
def test_queued_online_loop_forms_give_identical_bits(fmx):
    """fmx_online_run_mlp with online_persistent = 0: per-sample launches of the forward, the network, the sort and the update
    with the network's gradient, 40 samples."""
    import test_mlp_small_gpu as tm
    lib = fmx._lib.load()
    sizes = [7 + (3 * f) % 23 for f in range(8)]
    Xi, Xv, Y = tm.samples(sizes, 40, seed=4)
    res = []
    for form in FORMS:
        with uf.option(lib, "online_persistent", 0), uf.option(lib, "inline_fixup", form):
            m = tm.make_model("DeepFMAdam", sizes, 16, 32, 2, "signadam", seed=11)
            sd0 = tm.sd_np(m)
            pred = tm.online(m, Xi, Xv, Y)
            res.append((pred, tm.sd_np(m)))
    np.testing.assert_array_equal(res[0][0].view(np.int32), res[1][0].view(np.int32), err_msg="predictions")
    for kk in res[0][1]:
        a, b = np.ascontiguousarray(res[0][1][kk]), np.ascontiguousarray(res[1][1][kk])
        assert a.tobytes() == b.tobytes(), kk
    assert not np.array_equal(res[0][1]["hidden_layers.0.weight"], sd0["hidden_layers.0.weight"])


def test_option_round_trip(fmx):
    lib = fmx._lib.load()
    assert lib.fmx_set_option(b"inline_fixup", 0) == 1         # the default: the in-launch hand-off
    assert lib.fmx_set_option(b"inline_fixup", 1) == 0
    assert lib.fmx_set_option(b"inline_fixup", 1) == 1
    assert lib.fmx_set_option(b"no_such_option", 1) == fmx._lib.ERR_ARG
