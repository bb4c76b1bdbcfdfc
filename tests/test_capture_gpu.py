"""include/fmx.h: "calls are safe to capture into a hipGraph ...; a capturing stream takes the paths without in-launch hand-offs".
Pinned here for the entry points that run on ONE stream, each at one shape.

The pattern: a stream of its own and static input tensors; one eager warm-up call of the same entry point (the library raises
kernel attributes and learns a table's row counts at first use, never while capturing); ONE call captured with
torch.cuda.graph(g, stream=s); six replays, the next batch copied into the static tensors on that stream before each and the loss
read behind it.  Rows, bias, losses and parameters are compared BIT FOR BIT with the same six calls issued eagerly on a twin table
-- in the default one-launch form, which test_update_forms_gpu.py shows to give the bits of the two-launch form a capture takes.
The error word stays 0, and one eager step behind the replays matches its twin: the capture leaves the stream usable.

Not captured, on purpose: fmx_fm_stream, fmx_deepfm_stream* and every *_stream / *_online_run entry (cross-stream events; the
header excludes the first), anything that would give the graph parallel branches, more than one stream, threads, and
FMX_RULE_ADAM (its step constants are computed on the host per call: a replay would reuse the captured step's)."""
import numpy as np
import pytest
import torch

import update_forms as uf
from test_kernels_gpu import HYP
from test_update_forms_gpu import LAYOUT, hyper_for, problem, table_for

pytestmark = pytest.mark.gpu

N_REPLAYS = 6


@pytest.fixture(scope="module")
def fmx():
    import fmx as _fmx
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _fmx


class Side:
    """One side of a comparison: a table, its engine, static inputs, and the one call that reads them."""

    def __init__(self, table, eng, statics, call, outputs):
        self.table, self.eng, self.statics, self.call, self.outputs = table, eng, statics, call, outputs
        self.rows0, self.bias0 = table.rows.clone(), table.bias.clone()

    def load(self, batch):
        for dst, src in zip(self.statics, batch):
            dst.copy_(src, non_blocking=True)

    def restore(self):
        self.table.rows.copy_(self.rows0)
        self.table.bias.copy_(self.bias0)

    def snap(self, losses):
        out = dict(rows=self.table.rows.clone(), bias=self.table.bias.clone(), loss=torch.stack(losses), error=self.eng.error.clone())
        out.update({kk: v.clone() for kk, v in self.outputs().items()})
        return out


def replayed_against_eager(make_side, batches, what, warm_other=False):
    """make_side() -> Side; batches: N_REPLAYS + 1 tuples of device tensors shaped like the statics (the last for the eager step
    behind the replays).  warm_other: the warm-up call goes to a table of its own, so the captured call meets a table the
    library has not seen (no cached dispatch order: the capture takes index order)."""
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        a, b = make_side(), make_side()
        warm = make_side() if warm_other else a
        warm.load(batches[0])
        warm.call()                                       # eager: attributes raised, side state created, the table's order learnt
        a.restore()
        a.load(batches[0])
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        a.call()
    got, want = [], []
    with torch.cuda.stream(s):
        for i in range(N_REPLAYS):
            a.load(batches[i])
            g.replay()
            got.append(a.eng.loss_out.reshape(()).clone())
        for i in range(N_REPLAYS):
            b.load(batches[i])
            b.call()
            want.append(b.eng.loss_out.reshape(()).clone())
        ra, rb = a.snap(got), b.snap(want)
        # the stream after the capture: one eager call on each side
        for side in (a, b):
            side.load(batches[N_REPLAYS])
            side.call()
        ta, tb = a.snap([a.eng.loss_out.reshape(()).clone()]), b.snap([b.eng.loss_out.reshape(()).clone()])
    s.synchronize()
    assert int(ra["error"].item()) == 0 and int(rb["error"].item()) == 0, what
    assert bool(torch.isfinite(rb["loss"]).all()) and not torch.equal(rb["rows"], b.rows0), what + ": the eager twin did not train"
    uf.same(ra, rb, what + ": six replays against six eager calls")
    uf.same(ta, tb, what + ": the eager call behind the replays")
    assert len({float(v) for v in rb["loss"]}) > 1, what + ": the batches must differ"
    return ra


def pointwise_batches(sizes, B, real_x, n=N_REPLAYS + 1):
    out = []
    for j in range(n):
        rng = np.random.default_rng(100 + j)
        idx = torch.from_numpy(uf.indices(sizes, B, seed=50 + j)).cuda()
        x = torch.from_numpy(rng.uniform(0.5, 1.5, size=(B, len(sizes))).astype(np.float32)).cuda()
        y = torch.from_numpy((rng.uniform(size=B) < 0.3).astype(np.float32)).cuda()
        out.append((idx, x, y) if real_x else (idx, y))
    return out


def fm_side(fmx, rule, sizes, k, B, real_x, step):
    """step(eng, hyp, idx, xv, y): the captured call."""
    pr = problem(sizes, k, B, seed=1, real_x=False)

    def make():
        t = table_for(fmx, rule, sizes, k, pr)
        eng = fmx.FMEngine(t, max_batch=B)
        hyp = hyper_for(fmx, rule)
        idx = torch.zeros((B, len(sizes)), dtype=torch.int32, device="cuda")
        xv = torch.ones((B, len(sizes)), device="cuda") if real_x else None
        y = torch.zeros(B, device="cuda")
        statics = (idx, xv, y) if real_x else (idx, y)
        return Side(t, eng, statics, lambda: step(eng, hyp, idx, xv, y), dict)
    return make


@pytest.mark.parametrize("rule,B,warm_other", [("ftrl", 700, False), ("ftrl", 700, True), ("sgd", 700, False), ("adagrad", 700, False),
                                               ("ftrl", 4161, False)])
def test_fm_step_replays(fmx, rule, B, warm_other):
    """fmx_fm_step.  B = 700: eleven tiles per field, runs that cross them; with the warm-up on the same table (update_order
    finds its entry) and on another (the look-up is skipped while capturing: index order).  B = 4161: two slices, k_fm_fixup's
    extra workgroup, 65 tiles handed over in two iterations, and the chunked sort, all inside the graph."""
    sizes, real_x = uf.field_sizes(B, 6), rule == "sgd"
    make = fm_side(fmx, rule, sizes, 16, B, real_x, lambda eng, hyp, idx, xv, y: eng.step(hyp, rule, "logits", idx, xv, y))
    replayed_against_eager(make, pointwise_batches(sizes, B, real_x), f"fmx_fm_step {rule} B={B} warm_other={warm_other}", warm_other)


@pytest.mark.parametrize("entry", ["pair", "list"])
def test_pair_and_list_step_replay(fmx, entry):
    """fmx_fm_pair_step (350 pairs) and fmx_fm_list_step (140 lists of 5) on 700 rows, ftrl."""
    rows_n, G = 700, 5
    sizes = uf.field_sizes(rows_n, 6)

    def step(eng, hyp, idx, xv, y):
        if entry == "pair":
            eng.pair_step(hyp, "ftrl", idx, xv, margin=0.1)
        else:
            eng.list_step(hyp, "ftrl", idx, G, xv)
    make = fm_side(fmx, "ftrl", sizes, 16, rows_n, True, step)
    replayed_against_eager(make, pointwise_batches(sizes, rows_n, True), f"fmx_fm_{entry}_step")


def test_afm_step_replays(fmx):
    """fmx_afm_step (sgd): the forward, the attention's backward and k_fm_update_occ + k_fm_fixup in one graph; the attention
    gradient compared as well."""
    import test_afm_gpu as ta
    k, tt, B = 8, 8, 300
    sizes = uf.field_sizes(B, 6)

    def make():
        tb, params, _ = ta.make(sizes, k, tt, layout="weights", seed=3)
        eng = ta.engine(tb, params, tt, B)
        hyp = fmx.Hyper(**dict(ta.HYP, lr=0.01))
        idx = torch.zeros((B, len(sizes)), dtype=torch.int32, device="cuda")
        xv = torch.ones((B, len(sizes)), device="cuda")
        y = torch.zeros(B, device="cuda")
        return Side(tb, eng, (idx, xv, y), lambda: eng.step(hyp, "sgd", idx, xv, y), lambda: dict(grad=eng.grad, params=params))
    ra = replayed_against_eager(make, pointwise_batches(sizes, B, True), "fmx_afm_step")
    assert bool(ra["grad"].abs().max() > 0)


def test_update_with_network_gradient_replays(fmx):
    """fmx_sort_occurrences + fmx_fm_forward + fmx_fm_update with gbi captured together (HAS_GBI, the two-launch form)."""
    rule, k, B = "ftrl", 16, 700
    sizes = uf.field_sizes(B, 6)
    pr = problem(sizes, k, B, seed=1, real_x=False)
    rng = np.random.default_rng(4)
    dz_first = torch.from_numpy((rng.normal(size=B) * 0.1).astype(np.float32)).cuda()
    dz_bi = torch.from_numpy((rng.normal(size=B) * 0.1).astype(np.float32)).cuda()

    def make():
        t = table_for(fmx, rule, sizes, k, pr)
        eng = fmx.FMEngine(t, max_batch=B)
        hyp = fmx.Hyper(**HYP)
        gbi = torch.zeros((B, t.kp), device="cuda")
        gbi[:, :k] = torch.from_numpy((np.random.default_rng(5).normal(size=(B, k)) * 0.1).astype(np.float32)).cuda()
        idx = torch.zeros((B, len(sizes)), dtype=torch.int32, device="cuda")
        xv = torch.ones((B, len(sizes)), device="cuda")
        y = torch.zeros(B, device="cuda")

        def call():
            eng.sort(idx)
            eng.forward(hyp, idx, xv, y, loss="logits")
            eng.update(hyp, rule, B, xv, dz_first, dz_bi, gbi)
        return Side(t, eng, (idx, xv, y), call, dict)
    replayed_against_eager(make, pointwise_batches(sizes, B, True), "sort + forward + update with gbi")


@pytest.mark.parametrize("entry", ["topk", "rank"])
def test_topk_and_rank_replay(fmx, entry):
    """fmx_fm_topk / fmx_fm_rank, which the header names as safe under capture: two replays on new user sides, the bits of the
    eager call."""
    from fmx import recommend as rec
    U, N, kp, K, T = 9, 3000, 16, 10, 3
    gen = torch.Generator(device="cuda").manual_seed(3)
    rnd = lambda *shape: torch.randn(shape, device="cuda", generator=gen)
    Sc, ac = rnd(N, kp), rnd(N)
    users = [(rnd(U, kp), rnd(U)) for _ in range(3)]
    targets = torch.randint(0, N, (U, T), generator=torch.Generator().manual_seed(1)).to(torch.int32).cuda()
    lib = fmx._lib.load()
    need = int(lib.fmx_fm_topk_workspace_bytes(U, N, K) if entry == "topk" else lib.fmx_fm_rank_workspace_bytes(U, N, T))
    assert need >= 0

    def buffers():
        ws = torch.zeros(max(need, 16), dtype=torch.uint8, device="cuda")
        if entry == "topk":
            return ws, (torch.zeros((U, K), dtype=torch.int32, device="cuda"), torch.zeros((U, K), device="cuda"))
        return ws, (torch.zeros((U, T), dtype=torch.int32, device="cuda"), torch.zeros((U, T), device="cuda"),
                    torch.zeros(U, dtype=torch.int32, device="cuda"))

    def call(Su, au, ws, out, st):
        if entry == "topk":
            rec.fm_topk(Su, au, Sc, ac, K, workspace=ws, out=out, stream=st)
        else:
            rec.fm_rank(Su, au, Sc, ac, targets, workspace=ws, out=out, stream=st)

    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        Su, au = users[0][0].clone(), users[0][1].clone()
        ws, out = buffers()
        call(Su, au, ws, out, s.cuda_stream)                  # the eager warm-up
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call(Su, au, ws, out, s.cuda_stream)
    with torch.cuda.stream(s):
        for u, a in users[1:]:
            Su.copy_(u)
            au.copy_(a)
            g.replay()
            got = [o.clone() for o in out]
            ws2, want = buffers()
            call(u, a, ws2, want, s.cuda_stream)
            s.synchronize()
            uf.same({str(i): o for i, o in enumerate(got)}, {str(i): o for i, o in enumerate(want)}, f"fmx_fm_{entry} replayed")
            assert bool((want[0] >= 0).any())
