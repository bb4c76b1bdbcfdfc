"""In-batch sampled-softmax training of the FM on the device (fmx_fm_inbatch_*, include/fmx.h).

Shapes.  Tables of 154 and 125 rows: F = 5 with the item fields (2, 4), every value 1, and F = 3 with the item field (1) and
non-unit values.  B in {1, 2, 3, 63, 64, 65, 255, 256, 257}: around the 64-row tile of the scans and around one, two and four
tiles; one B just above the first j-split threshold as fmx_fm_inbatch_splits reports it; and the ragged B = 1003 (16 tiles, 16
ranges of 63 rows, the last of 58).  k = 3 (kp = 4, one padded column), 16 and 64: R = 8, 2 and 1 rows of the uniform side at a
time.  The vocabularies are small, so contexts and items repeat at every B >= 4.

Checks: the scores against fmx_fm_topk's bit for bit; loss, gSu, gSc, gac, occ_grad and the table after a step under sgd and ftrl
against tests/inbatch_f64.py within its floors (1e-5 |ref| + the fp32 floor, test_list_gpu's tolerance); the step against the
composition of public calls bit for bit under every rule; the stream against its steps; guard bands; graph capture; the class."""
import ctypes as C

import numpy as np
import pytest
import torch

from abi_geometry import PATTERN, Guarded
from helpers import assert_ftrl_step_within_f64
from inbatch_f64 import inbatch_step_f64
from test_kernels_gpu import HYP
from test_list_gpu import new_model, within
from test_pair_gpu import RULES, build_table, clone_table, same_bits

pytestmark = pytest.mark.gpu

SHAPES = {"F5": ([50, 30, 40, 9, 25], [2, 4], False), "F3": ([60, 20, 45], [1], True)}
BS = [1, 2, 3, 63, 64, 65, 255, 256, 257]
RAGGED = 1003
KS = [3, 16, 64]


@pytest.fixture(scope="module")
def fmx():
    import fmx as _fmx
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _fmx


def first_split_B(fmx):
    """The smallest B whose sums are cut into two ranges, read from the library's geometry"""
    lib = fmx._lib.load()
    B = 1
    while lib.fmx_fm_inbatch_splits(B, 16) == 1:
        B += 1
    assert B > 1 and lib.fmx_fm_inbatch_splits(B - 1, 16) == 1
    return B


def all_Bs(fmx):
    return sorted(set(BS + [first_split_B(fmx), RAGGED]))


def make_batch(shape, B, seed):
    """-> (rows int32 [B, F] local indices, x float32 [B, F] or None, item fields): rows 1 and 3 share their context, rows 2 and 5
    their item; the small vocabularies repeat both at larger B anyway."""
    sizes, item, real_x = SHAPES[shape]
    rng = np.random.default_rng(seed)
    F = len(sizes)
    rows = np.stack([rng.integers(0, s, size=B) for s in sizes], axis=1)
    ctx = [f for f in range(F) if f not in item]
    if B > 3:
        rows[3, ctx] = rows[1, ctx]
    if B > 5:
        rows[5, item] = rows[2, item]
    x = rng.uniform(0.5, 1.5, size=(B, F)).astype(np.float32) if real_x else None
    return rows.astype(np.int32), x, item


def zipf_logq(fmx, rows, item, sizes):
    """log q of every row's item under a Zipf popularity over the first item field's vocabulary"""
    N = sizes[item[0]]
    logq = fmx.pairwise.alias_table(1.0 / np.arange(1, N + 1, dtype=np.float64) ** 1.1)[3]
    return logq[rows[:, item[0]]].astype(np.float32)


def variants(fmx, shape, rows, item, B):
    """(name, key, corr) as numpy / None: keys null, in_batch_keys, all equal; corr null, +0, Zipf log q"""
    sizes = SHAPES[shape][0]
    keys = fmx.pairwise.in_batch_keys(torch.from_numpy(rows), item).numpy()
    return [("free", None, None), ("keys+zipf", keys, zipf_logq(fmx, rows, item, sizes)), ("zipf", None, zipf_logq(fmx, rows, item, sizes)),
            ("keys+zero", keys, np.zeros(B, np.float32)), ("one key", np.zeros(B, np.int32), None)]


class Call:
    """One batch on the device and the public calls on it (the composition the header states for fmx_fm_inbatch_step), every output
    in a guarded buffer."""

    def __init__(self, fmx, t, rows, x, item, key=None, corr=None, inv_b=None):
        self.fmx, self.L, self.lib, self.t = fmx, fmx._lib, fmx._lib.load(), t
        L, lib = self.L, self.lib
        self.B, self.F, self.kp, self.item = rows.shape[0], t.n_fields, t.kp, list(item)
        B, F, kp = self.B, self.F, self.kp
        self.inv_b = 1.0 / B if inv_b is None else inv_b
        self.idx = torch.from_numpy(np.ascontiguousarray(rows, np.int32)).cuda()
        self.xv = None if x is None else torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
        self.key = None if key is None else torch.from_numpy(np.ascontiguousarray(key, np.int32)).cuda()
        self.corr = None if corr is None else torch.from_numpy(np.ascontiguousarray(corr, np.float32)).cuda()
        self.fields = (C.c_int32 * len(item))(*item)
        self.step_bytes = int(lib.fmx_workspace_bytes(t.c_struct(), B))
        self.lse_bytes = int(lib.fmx_fm_inbatch_lse_bytes(B, kp))
        g = lambda name, n, dt=torch.float32: Guarded(n * 4, dt, name=name)  # noqa: E731
        self.bufs = dict(Su=g("Su", B * kp), au=g("au", B), Sc=g("Sc", B * kp), sfirst=g("sfirst", B), sbi=g("sbi", B), loss=g("loss", B),
                         gSu=g("gSu", B * kp), gSc=g("gSc", B * kp), gac=g("gac", B), occ=g("occ_grad", B * F * kp),
                         lse=Guarded(self.lse_bytes, torch.int32, name="lse"), ws=Guarded(self.step_bytes + 16, torch.int32, name="workspace"),
                         loss_out=g("loss_out", 1), error=g("error", 1, torch.int32))
        for name in ("loss", "gSu", "gSc", "gac", "occ"):
            self.bufs[name].t.view(torch.int32).fill_(PATTERN)
        self.st = torch.cuda.current_stream().cuda_stream

    def p(self, name):
        return self.bufs[name].ptr

    @staticmethod
    def ptr(t):
        return None if t is None else t.data_ptr()

    def sides(self, hyp):
        """The two masked forwards: S_u, a_u = logit; S_c, a_c = sfirst + sbi (one torch addition)"""
        L, lib, t, B = self.L, self.lib, self.t, self.B
        keep = torch.zeros(self.F, dtype=torch.bool, device="cuda")
        keep[self.item] = True
        xv = torch.ones((B, self.F), device="cuda") if self.xv is None else self.xv
        zi, zx = torch.zeros_like(self.idx), torch.zeros_like(xv)
        self.idx_u, self.xv_u = torch.where(keep[None, :], zi, self.idx).contiguous(), torch.where(keep[None, :], zx, xv).contiguous()
        self.idx_c, self.xv_c = torch.where(keep[None, :], self.idx, zi).contiguous(), torch.where(keep[None, :], xv, zx).contiguous()
        ou, oc = L.FwdOut(), L.FwdOut()
        ou.S, ou.logit, ou.error = self.p("Su"), self.p("au"), self.p("error")
        oc.S, oc.sfirst, oc.sbi, oc.error = self.p("Sc"), self.p("sfirst"), self.p("sbi"), self.p("error")
        L.check(lib.fmx_fm_forward(t.c_struct(), hyp.ref(), self.idx_u.data_ptr(), self.xv_u.data_ptr(), None, B, L.LOSS_NONE, 1.0,
                                   C.byref(ou), self.st))
        L.check(lib.fmx_fm_forward(t.c_struct(), hyp.ref(), self.idx_c.data_ptr(), self.xv_c.data_ptr(), None, B, L.LOSS_NONE, 1.0,
                                   C.byref(oc), self.st))
        self.ac = torch.add(self.bufs["sfirst"].t, self.bufs["sbi"].t)

    def forward(self, score_out=None):
        kp, B = self.kp, self.B
        self.L.check(self.lib.fmx_fm_inbatch_forward(self.p("Su"), kp, self.p("au"), self.p("Sc"), kp, self.ac.data_ptr(), B, kp,
                                                     self.ptr(self.corr), self.ptr(self.key), self.inv_b, self.p("lse"), self.lse_bytes,
                                                     self.p("loss"), self.ptr(score_out), self.st))

    def backward(self):
        kp, B = self.kp, self.B
        self.L.check(self.lib.fmx_fm_inbatch_backward(self.p("Su"), kp, self.p("au"), self.p("Sc"), kp, self.ac.data_ptr(), B, kp,
                                                      self.ptr(self.corr), self.ptr(self.key), self.inv_b, self.p("lse"), self.lse_bytes,
                                                      self.p("gSu"), self.p("gSc"), self.p("gac"), self.st))

    def occ_grad(self):
        kp, B, F = self.kp, self.B, self.F
        self.L.check(self.lib.fmx_fm_inbatch_occ_grad(self.t.c_struct(), self.idx.data_ptr(), self.ptr(self.xv), self.fields, len(self.item),
                                                      self.p("gSu"), self.p("gSc"), self.p("gac"), self.p("Sc"), kp, B, self.p("occ"), F * kp,
                                                      self.st))

    def compose(self, hyp, rule):
        """The whole composition, the table updated -> the outputs as numpy"""
        L, lib, t, B, F, kp = self.L, self.lib, self.t, self.B, self.F, self.kp
        hyp.c.step = t.step
        L.check(lib.fmx_sort_occurrences(t.c_struct(), self.idx.data_ptr(), B, self.p("ws"), self.step_bytes, self.p("error"), self.st))
        self.sides(hyp)
        self.forward()
        self.backward()
        self.occ_grad()
        tu = L.Table.from_buffer_copy(t._cstruct)
        tu.bias = self.p("ws") + self.step_bytes                                 # the bias rule runs on the scratch behind the workspace
        L.check(lib.fmx_fm_update_occ(C.byref(tu), hyp.ref(), L.RULES[rule], self.p("ws"), self.step_bytes, self.xv_c.data_ptr(),
                                      self.p("gac"), self.p("occ"), F * kp, B, self.p("loss"), self.inv_b, self.p("loss_out"), self.st))
        if t.layout == "moments":
            t.step += 1
        torch.cuda.synchronize()
        self.check()
        assert int(self.bufs["error"].t.item()) == 0
        return self.numpy()

    def check(self):
        for g in self.bufs.values():
            g.check()

    def numpy(self):
        B, F, kp = self.B, self.F, self.kp
        shapes = dict(Su=(B, kp), Sc=(B, kp), gSu=(B, kp), gSc=(B, kp), occ=(B, F, kp))
        out = {n: self.bufs[n].t.cpu().numpy().reshape(shapes.get(n, (-1,))) for n in ("Su", "au", "Sc", "loss", "gSu", "gSc", "gac", "occ",
                                                                                         "loss_out")}
        out["ac"] = self.ac.cpu().numpy()
        return out


def reference(t, pr, rows, x, item, rule, key, corr, kp):
    grows = rows.astype(np.int64) + np.asarray(t.offsets_host[:-1], np.int64)[None, :]
    xx = x if x is not None else np.ones(rows.shape, np.float32)
    if rule == "ftrl":
        h = dict(alpha=HYP["alpha"], beta=HYP["beta"], l1=HYP["l1"], l2=HYP["l2"])
        return inbatch_step_f64(pr["ftrl_state"], grows, xx, item, "ftrl", h, corr=corr, key=key, kp=kp)
    return inbatch_step_f64(dict(V=pr["V"], w=pr["w"], bias=pr["bias"]), grows, xx, item, "sgd", dict(lr=HYP["lr"]), corr=corr, key=key, kp=kp)


def engine_step(fmx, t, rule, rows, x, item, key, corr, hyp=None):
    """fmx_fm_inbatch_step through the engine -> (engine, its hyper)"""
    B = rows.shape[0]
    eng = fmx.FMEngine(t, max_batch=B)
    hyp = fmx.Hyper(**HYP) if hyp is None else hyp
    idx_d, xv_d, _ = eng.to_device(rows, x)
    eng.inbatch_step(hyp, rule, idx_d, item, xv_d, corr=None if corr is None else torch.from_numpy(corr).cuda(),
                     key=None if key is None else torch.from_numpy(key).cuda())
    torch.cuda.synchronize()
    eng.check_error_flag()
    return eng


def check_table_within(t, pr, ref, rule, k, what):
    if rule == "ftrl":
        zV, nV, zw, nw = [a.numpy() for a in t.export_ftrl_state()]
        assert_ftrl_step_within_f64(dict(zV=zV, nV=nV, zw=zw, nw=nw, zb=t.bias[0].item(), nb=t.bias[1].item()), ref, what=what + " ",
                                    before=pr["ftrl_state"])
        return
    u, new, fl = ref["urows"], ref["new"], ref["floor"]
    got = dict(V=t.rows[:, :k].cpu().numpy(), w=t.rows[:, t.kp].cpu().numpy())
    for kk in ("V", "w"):
        b0 = np.asarray(pr[kk], np.float64)[u]
        within(got[kk][u], new[kk][u], fl[kk], f"{what} {kk}")
        within(got[kk][u].astype(np.float64) - b0, new[kk][u] - b0, fl[kk], f"{what} {kk} (the step)")
        mask = np.ones(len(got[kk]), bool)
        mask[u] = False
        np.testing.assert_array_equal(got[kk][mask], pr[kk][mask], err_msg=kk + " untouched rows")
    assert float(t.bias[0].item()) == float(new["bias"])


def unchanged_at_one_row(t, before, rule, what):
    """B = 1: every gradient is +-0 and the weights stay bit-unchanged under sgd / signadam / ftrl.  ftrl: the state (z, n) is
    compared; the weight slots [ V | w ] are re-derived from it by every update, so they hold the kernel's own derivation of
    the same state from the first step on."""
    if rule != "ftrl":
        same_bits(t.rows, before, what + ": B = 1 leaves the weights bit-unchanged")
        return
    kp, zo = t.kp, t.z_offset
    for lo, hi in ((kp + 1, kp + 3), (zo, zo + 2 * kp)):
        same_bits(t.rows[:, lo:hi], before[:, lo:hi], what + ": B = 1 leaves (z, n) bit-unchanged")
    torch.testing.assert_close(t.rows[:, :kp + 1], before[:, :kp + 1], rtol=1e-6, atol=1e-9)


def check_outputs_within(out, ref, k, what):
    fl = ref["floor"]
    for name in ("loss", "gSu", "gSc", "gac", "occ"):
        assert np.isfinite(out[name]).all(), f"{what} {name}"
    within(out["Su"][:, :k], ref["Su"], fl["Su"], what + " Su")
    within(out["au"], ref["au"], fl["au"], what + " au")
    within(out["Sc"][:, :k], ref["Sc"], fl["Sc"], what + " Sc")
    within(out["ac"], ref["ac"], fl["ac"], what + " ac")
    within(out["loss"], ref["loss_b"], fl["loss_b"], what + " loss")
    within(out["gSu"][:, :k], ref["gSu"], fl["gSu"], what + " gSu")
    within(out["gSc"][:, :k], ref["gSc"], fl["gSc"], what + " gSc")
    within(out["gac"], ref["gac"], fl["gac"], what + " gac")
    within(out["occ"][:, :, :k], ref["occ"], fl["occ"], what + " occ_grad")
    within(float(out["loss_out"][0]), ref["loss"], fl["loss"], what + " loss_out")
    for name in ("Su", "Sc", "gSu", "gSc"):                                     # the padded columns hold zeros
        assert not out[name][:, k:].any(), f"{what}: padded columns of {name}"
    assert not out["occ"][:, :, k:].any(), what + ": padded columns of occ_grad"


# ---- 1. the training logit is the serving score, bit for bit ----
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_scores_are_fmx_fm_topk_scores(fmx, shape, k):
    sizes = SHAPES[shape][0]
    t, _ = build_table(fmx, sizes, k, "weights", seed=7)
    hyp = fmx.Hyper(**HYP)
    for B in [b for b in all_Bs(fmx) if b <= 256]:
        rows, x, item = make_batch(shape, B, seed=5 * B + k)
        c = Call(fmx, t, rows, x, item)
        c.sides(hyp)
        score = Guarded(B * B * 4, name="score_out")
        score.t.view(torch.int32).fill_(PATTERN)
        c.forward(score_out=score.t)
        K = min(B, 256)
        top_pos, top_score = fmx.recommend.fm_topk(c.bufs["Su"].t.view(B, t.kp), c.bufs["au"].t, c.bufs["Sc"].t.view(B, t.kp), c.ac, K, kp=t.kp)
        torch.cuda.synchronize()
        c.check()
        score.check()
        got = score.t.view(B, B)
        assert (got.view(torch.int32) != PATTERN).all()
        assert (top_pos >= 0).all() and torch.equal(torch.sort(top_pos, dim=1)[0], torch.arange(B, device="cuda", dtype=torch.int32).expand(B, B))
        at = torch.gather(got, 1, top_pos.long())
        at = torch.where(at == 0, torch.zeros_like(at), at)                     # fmx_fm_topk returns a score of -0 as +0
        same_bits(at, top_score, f"{shape} k={k} B={B}: score_out against top_score")


# ---- 2. every output and the table after one step within the float64 evaluation; the step is the composition ----
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("B", BS + ["first split", RAGGED])
def test_step_within_float64(fmx, B, k):
    B = first_split_B(fmx) if B == "first split" else B
    for shape in SHAPES:
        sizes = SHAPES[shape][0]
        rows, x, item = make_batch(shape, B, seed=31 * B + k)
        picked = variants(fmx, shape, rows, item, B)
        picked = picked if B <= 65 else picked[:2] + picked[4:]                 # (the larger batches: three of the five variants)
        for vi, (name, key, corr) in enumerate(picked):
            for rule in (("sgd", "ftrl") if vi < 2 else (("sgd", "ftrl")[vi % 2],)):   # (the first two variants: both rules)
                what = f"{shape} k={k} B={B} {name} {rule}"
                t, pr = build_table(fmx, sizes, k, RULES[rule], seed=7)
                twin = clone_table(fmx, t)
                bias0 = t.bias.clone()
                out = Call(fmx, t, rows, x, item, key, corr).compose(fmx.Hyper(**HYP), rule)
                ref = reference(t, pr, rows, x, item, rule, key, corr, t.kp)
                check_outputs_within(out, ref, k, what)
                check_table_within(t, pr, ref, rule, k, what)
                same_bits(t.bias, bias0, what + " bias")
                if name == "one key":                                           # only the diagonal is eligible
                    assert not out["loss"].any() and not out["loss_out"].any(), what
                    for g in ("gSu", "gSc", "gac", "occ"):
                        assert not out[g].any(), f"{what}: {g} must be +-0"
                if B == 1:
                    assert not out["loss"].any() and not out["occ"].any(), what
                    unchanged_at_one_row(t, twin.rows, rule, what)
                eng = engine_step(fmx, twin, rule, rows, x, item, key, corr)
                same_bits(twin.rows, t.rows, what + ": the step's rows against the composition's")
                same_bits(twin.bias, bias0, what + ": the step's bias")
                same_bits(eng.loss_out, torch.from_numpy(out["loss_out"]), what + " loss_out")
                same_bits(eng.loss_b[:B], torch.from_numpy(out["loss"]), what + " loss_b")


# ---- 3. corr of +0 is the null-corr call; two runs give the same bits ----
@pytest.mark.parametrize("B", [3, 65, 257])
def test_zero_corr_is_no_corr_and_runs_repeat(fmx, B):
    shape, k = "F3", 16
    sizes = SHAPES[shape][0]
    rows, x, item = make_batch(shape, B, seed=B)
    keys = variants(fmx, shape, rows, item, B)[1][1]
    outs = []
    for corr in (None, np.zeros(B, np.float32), None):
        t, _ = build_table(fmx, sizes, k, "moments", seed=7)
        o = Call(fmx, t, rows, x, item, keys, corr).compose(fmx.Hyper(**HYP), "adam")
        o["rows"] = t.rows.cpu().numpy()
        outs.append(o)
    for name in outs[0]:
        same_bits(torch.from_numpy(outs[1][name]), torch.from_numpy(outs[0][name]), f"B={B} {name}: corr +0 against null")
        same_bits(torch.from_numpy(outs[2][name]), torch.from_numpy(outs[0][name]), f"B={B} {name}: run to run")


# ---- 4. the step is the composition of public calls under every rule; the bias and its state never move ----
@pytest.mark.parametrize("rule", list(RULES))
@pytest.mark.parametrize("k", [3, 16])
def test_step_is_the_composition_under_every_rule(fmx, rule, k):
    for shape in SHAPES:
        sizes = SHAPES[shape][0]
        for B in (1, 3, first_split_B(fmx), 257):
            rows, x, item = make_batch(shape, B, seed=7 * B + k)
            _, key, corr = variants(fmx, shape, rows, item, B)[1]
            what = f"{shape} k={k} B={B} {rule}"
            t, _ = build_table(fmx, sizes, k, RULES[rule], seed=7)
            twin = clone_table(fmx, t)
            before = t.rows.clone()
            bias0 = t.bias.clone()
            out = Call(fmx, t, rows, x, item, key, corr).compose(fmx.Hyper(**HYP), rule)
            eng = engine_step(fmx, twin, rule, rows, x, item, key, corr)
            same_bits(twin.rows, t.rows, what + " rows, first-order weights and moments")
            same_bits(eng.loss_out, torch.from_numpy(out["loss_out"]), what + " loss_out")
            same_bits(t.bias, bias0, what + ": the composition's bias")
            same_bits(twin.bias, bias0, what + ": the step's bias and its state")
            assert twin.step == t.step
            if B > 1:
                assert not torch.equal(t.rows, before), what + ": nothing trained"
            elif rule in ("sgd", "signadam", "ftrl"):
                unchanged_at_one_row(t, before, rule, what)
            # a touched context row's first-order weight under a +0 gradient: unchanged, but under adam (ftrl: its z and n; the
            # weight slot is re-derived from them by every update)
            if rule != "adam":
                ctx = [f for f in range(len(sizes)) if f not in item]
                grow = (rows[:, ctx].astype(np.int64) + np.asarray(t.offsets_host[:-1], np.int64)[ctx][None, :]).reshape(-1)
                grow = torch.from_numpy(np.unique(grow)).cuda()
                cols = [t.kp + 1, t.kp + 2] if rule == "ftrl" else [t.kp]
                same_bits(t.rows[grow][:, cols], before[grow][:, cols], what + ": context first-order weights")


# ---- 5. the stream is its steps ----
@pytest.mark.parametrize("rule", ["signadam", "ftrl", "adam"])
def test_stream_is_its_steps(fmx, rule):
    shape, k, B, n_pool = "F5", 16, 130, 3
    sizes, item, _ = SHAPES[shape]
    pool = [make_batch(shape, B, seed=40 + j)[0] for j in range(n_pool)]
    keys = [fmx.pairwise.in_batch_keys(torch.from_numpy(r), item).numpy() for r in pool]
    corrs = [zipf_logq(fmx, r, item, sizes) for r in pool]
    idx_pool = torch.from_numpy(np.stack(pool)).cuda().contiguous()
    key_pool = torch.from_numpy(np.stack(keys)).cuda().contiguous()
    corr_pool = torch.from_numpy(np.stack(corrs)).cuda().contiguous()
    t1, _ = build_table(fmx, sizes, k, RULES[rule], seed=7)
    t2, t3 = clone_table(fmx, t1), clone_table(fmx, t1)
    bias0 = t1.bias.clone()
    e1, e2, e3 = (fmx.FMEngine(t, max_batch=B) for t in (t1, t2, t3))
    h1, h2, h3 = (fmx.Hyper(**HYP) for _ in range(3))
    l1, l3 = torch.zeros(5, device="cuda"), torch.zeros(5, device="cuda")
    e1.inbatch_stream(h1, rule, idx_pool, item, 3, corr_pool, key_pool, loss_out=l1[:3])
    # (the second call starts at the pool's batch 0 again: its steps are steps 0 and 1 of the pool)
    e1.inbatch_stream(h1, rule, idx_pool, item, 2, corr_pool, key_pool, loss_out=l1[3:])
    want = []
    for s in (0, 1, 2, 0, 1):
        e2.inbatch_step(h2, rule, idx_pool[s], item, None, corr=corr_pool[s], key=key_pool[s])
        want.append(e2.loss_out.reshape(()).clone())
    e3.inbatch_stream(h3, rule, idx_pool, item, 3, corr_pool, key_pool, loss_out=l3[:3])
    e3.inbatch_stream(h3, rule, idx_pool, item, 2, corr_pool, key_pool, loss_out=l3[3:])
    torch.cuda.synchronize()
    for e in (e1, e2, e3):
        e.check_error_flag()
    same_bits(t1.rows, t2.rows, f"{rule}: the stream's rows against five steps")
    same_bits(l1, torch.stack(want), f"{rule}: the stream's losses")
    same_bits(t3.rows, t1.rows, f"{rule}: run to run")
    same_bits(l3, l1, f"{rule}: run to run, losses")
    for t in (t1, t2):
        same_bits(t.bias, bias0, f"{rule}: bias")
    assert t1.step == t2.step and (t1.step == 8 if rule == "adam" else True)
    assert bool(torch.isfinite(l1).all()) and float(l1[0]) > 0


# ---- 6. scores that span about +-60 ----
@pytest.mark.parametrize("k", [3, 16])
def test_scores_sixty_apart(fmx, k):
    shape, B = "F5", first_split_B(fmx)
    sizes = SHAPES[shape][0]
    rows, x, item = make_batch(shape, B, seed=12)
    _, key, corr = variants(fmx, shape, rows, item, B)[1]
    for rule in ("sgd", "ftrl"):
        t, pr = build_table(fmx, sizes, k, RULES[rule], seed=7)
        V0 = pr["V"].copy()

        def load_V(V):
            """the table and the reference's state with second-order weights V (ftrl: the z that gives them at n = 0)"""
            if rule == "sgd":
                pr["V"] = V
                t.rows[:, :k] = torch.from_numpy(V).cuda()
                return
            from oracle.fm_oracle import ftrl_z_for_weight
            st = pr["ftrl_state"]
            h = dict(alpha=HYP["alpha"], beta=HYP["beta"], l1=HYP["l1"], l2=HYP["l2"])
            st["zV"], st["nV"] = ftrl_z_for_weight(V, **h), np.zeros_like(st["nV"])
            t.load_ftrl_state(st["zV"], st["nV"], st["zw"], st["nw"])
        load_V(V0)
        base = reference(t, pr, rows, x, item, rule, key, corr, t.kp)
        load_V((V0 * np.sqrt(60.0 / np.abs(base["score"]).max())).astype(np.float32))     # the second-order terms grow with the square
        ref = reference(t, pr, rows, x, item, rule, key, corr, t.kp)
        span = ref["score"].max() - ref["score"].min()
        print(f"k={k} {rule}: scores in [{ref['score'].min():.1f}, {ref['score'].max():.1f}]")
        assert 30.0 < np.abs(ref["score"]).max() < 120.0 and span > 40.0
        what = f"k={k} {rule} scores +-60"
        out = Call(fmx, t, rows, x, item, key, corr).compose(fmx.Hyper(**HYP), rule)
        check_outputs_within(out, ref, k, what)
        check_table_within(t, pr, ref, rule, k, what)


# ---- 7. nothing is written around the step's workspace, its outputs, or the raw calls' buffers (Call.check, every test above) ----
@pytest.mark.parametrize("rule", ["signadam", "ftrl", "adam"])
@pytest.mark.parametrize("B", [3, 65, 257])
def test_guard_bands_of_the_step(fmx, rule, B):
    L = fmx._lib
    lib = L.load()
    shape, k = "F3", 10
    sizes = SHAPES[shape][0]
    rows, x, item = make_batch(shape, B, seed=9)
    _, key, corr = variants(fmx, shape, rows, item, B)[1]
    t, _ = build_table(fmx, sizes, k, RULES[rule])
    idx_d, xv_d = torch.from_numpy(rows).cuda(), torch.from_numpy(x).cuda()
    key_d, corr_d = torch.from_numpy(key).cuda(), torch.from_numpy(corr).cuda()
    need = int(lib.fmx_fm_inbatch_workspace_bytes(t.c_struct(), B, len(item)))
    bufs = dict(ws=Guarded(need, torch.int32, name="workspace"), loss=Guarded(B * 4, name="loss"), loss_out=Guarded(4, name="loss_out"),
                error=Guarded(4, torch.int32, name="error"))
    bufs["loss"].t.view(torch.int32).fill_(PATTERN)
    out = L.FwdOut()
    out.loss, out.error = bufs["loss"].ptr, bufs["error"].ptr
    hyp = fmx.Hyper(**HYP)
    hyp.c.step = t.step
    fields = (C.c_int32 * len(item))(*item)
    st = torch.cuda.current_stream().cuda_stream
    bias0 = t.bias.clone()
    args = (t.c_struct(), hyp.ref(), L.RULES[rule], idx_d.data_ptr(), xv_d.data_ptr(), fields, len(item), corr_d.data_ptr(), key_d.data_ptr(), B,
            1.0 / B, bufs["ws"].ptr)
    L.check(lib.fmx_fm_inbatch_step(*args, need, C.byref(out), bufs["loss_out"].ptr, st))
    torch.cuda.synchronize()
    for g in bufs.values():
        g.check()
    assert int(bufs["error"].t.item()) == 0
    assert np.isfinite(bufs["loss_out"].t.cpu().numpy()).all() and float(bufs["loss_out"].t.item()) > 0
    assert (bufs["loss"].t.view(torch.int32) != PATTERN).all()
    same_bits(t.bias, bias0, "bias")
    assert lib.fmx_fm_inbatch_step(*args, need - 1, C.byref(out), bufs["loss_out"].ptr, st) == L.ERR_SHAPE
    # fwd may be null: the losses stay in the workspace
    L.check(lib.fmx_fm_inbatch_step(*args, need, None, bufs["loss_out"].ptr, st))
    torch.cuda.synchronize()
    for g in bufs.values():
        g.check()


# ---- 8. one captured step, replayed four times on new batches, against four eager steps on a twin ----
def test_a_captured_step_replays(fmx):
    import update_forms as uf
    shape, k, B, rule, n = "F5", 16, 257, "ftrl", 4
    sizes, item, _ = SHAPES[shape]
    batches = []
    for j in range(n + 1):
        rows = make_batch(shape, B, seed=70 + j)[0]
        batches.append((torch.from_numpy(rows).cuda(), fmx.pairwise.in_batch_keys(torch.from_numpy(rows), item).cuda(),
                        torch.from_numpy(zipf_logq(fmx, rows, item, sizes)).cuda()))
    t0, _ = build_table(fmx, sizes, k, RULES[rule], seed=7)

    class Side:
        def __init__(self):
            self.t = clone_table(fmx, t0)
            self.eng = fmx.FMEngine(self.t, max_batch=B)
            self.hyp = fmx.Hyper(**HYP)
            self.statics = (torch.zeros((B, len(sizes)), dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda"),
                            torch.zeros(B, device="cuda"))

        def load(self, batch):
            for dst, src in zip(self.statics, batch):
                dst.copy_(src, non_blocking=True)

        def call(self):
            idx, key, corr = self.statics
            self.eng.inbatch_step(self.hyp, rule, idx, item, None, corr=corr, key=key)

        def snap(self, losses):
            return dict(rows=self.t.rows.clone(), bias=self.t.bias.clone(), loss=torch.stack(losses), error=self.eng.error.clone())

    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        a, b = Side(), Side()
        a.load(batches[0])
        a.call()                                            # eager: the workspace allocated, the table's order learnt
        a.t.rows.copy_(t0.rows)
        a.t.bias.copy_(t0.bias)
        a.load(batches[0])
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        a.call()
    got, want = [], []
    with torch.cuda.stream(s):
        for i in range(n):
            a.load(batches[i])
            g.replay()
            got.append(a.eng.loss_out.reshape(()).clone())
        for i in range(n):
            b.load(batches[i])
            b.call()
            want.append(b.eng.loss_out.reshape(()).clone())
        ra, rb = a.snap(got), b.snap(want)
        for side in (a, b):                                 # the stream after the capture: one eager call on each side
            side.load(batches[n])
            side.call()
        ta, tb = a.snap([a.eng.loss_out.reshape(()).clone()]), b.snap([b.eng.loss_out.reshape(()).clone()])
    s.synchronize()
    assert int(ra["error"].item()) == 0 and int(rb["error"].item()) == 0
    assert bool(torch.isfinite(rb["loss"]).all()) and not torch.equal(rb["rows"], t0.rows)
    uf.same(ra, rb, "four replays against four eager steps")
    uf.same(ta, tb, "the eager step behind the replays")
    assert len({float(v) for v in rb["loss"]}) > 1


# ---- 9. the class ----
def test_fit_in_batch_is_the_engine_call(fmx):
    shape, B = "F3", 65
    sizes, item, _ = SHAPES[shape]
    rows, x, _ = make_batch(shape, B, seed=4)
    log_q = zipf_logq(fmx, rows, item, sizes)
    idx, xv = torch.from_numpy(rows).cuda(), torch.from_numpy(x).cuda()
    keys = fmx.pairwise.in_batch_keys(idx, item)
    assert len(set(keys.tolist())) < B                                           # some rows do share their item
    for kw, eng_kw in ((dict(log_q=log_q), dict(corr=torch.from_numpy(log_q).cuda(), key=keys)),
                       (dict(), dict(key=keys)),
                       (dict(log_q=log_q, mask_duplicates=False), dict(corr=torch.from_numpy(log_q).cuda(), key=None))):
        a, b = new_model("signadam", sizes), new_model("signadam", sizes)
        same_bits(a._table.rows, b._table.rows, "the same seed gives the same model")
        bias0 = b._table.bias.clone()
        la = a.fit_in_batch(rows, x, item, **kw)
        b._engine.inbatch_step(b._hyper, "signadam", idx, item, xv, **eng_kw)
        torch.cuda.synchronize()
        same_bits(a._table.rows, b._table.rows, f"{sorted(kw)} rows")
        same_bits(a._table.bias, bias0, "bias untouched")
        same_bits(la.reshape(1), b._engine.loss_out, "loss")
        assert float(la) > 0
    masked, free = new_model("signadam", sizes), new_model("signadam", sizes)
    masked.fit_in_batch(rows, x, item)
    free.fit_in_batch(rows, x, item, mask_duplicates=False)
    assert not torch.equal(masked._table.rows, free._table.rows)
    with pytest.raises(ValueError, match="log_q"):
        masked.fit_in_batch(rows, x, item, log_q=log_q[:-1])
    with pytest.raises(IndexError):
        masked.fit_in_batch(rows + 1000, x, item)
    # adam counts its steps
    m = new_model("adam", sizes)
    for _ in range(3):
        m.fit_in_batch(rows, x, item, log_q=log_q)
    assert m._table.step == 3


def test_popularity_negatives_as_log_q(fmx):
    shape, B = "F3", 33
    sizes, item, _ = SHAPES[shape]
    rows, x, _ = make_batch(shape, B, seed=6)
    N = sizes[item[0]]
    weights = 1.0 / np.arange(1, N + 1) ** 1.1
    weights[3] = 0.0                                                            # an item the table never draws takes the floor
    rows[0, item[0]] = 3
    pop = fmx.pairwise.PopularityNegatives(weights)
    a, b = new_model("signadam", sizes), new_model("signadam", sizes)
    cands = fmx.recommend.Candidates.whole_field(a._table, item[0], hyper=a._hyper)
    want = np.maximum(pop.logq[rows[:, item[0]]], np.float32(pop.floor_logq())).astype(np.float32)
    assert np.isfinite(want).all() and want[0] == np.float32(pop.floor_logq())
    la = a.fit_in_batch(rows, x, item, log_q=pop, candidates=cands)
    lb = b.fit_in_batch(rows, x, item, log_q=want)
    torch.cuda.synchronize()
    same_bits(a._table.rows, b._table.rows, "PopularityNegatives as log_q gathers the items' log q")
    same_bits(la.reshape(1), lb.reshape(1), "loss")
    with pytest.raises(ValueError, match="candidates"):
        a.fit_in_batch(rows, x, item, log_q=pop)
    with pytest.raises(ValueError, match="weights"):
        a.fit_in_batch(rows, x, item, log_q=fmx.pairwise.PopularityNegatives(weights[:-1]), candidates=cands)


def test_sixty_steps_learn_a_planted_model(fmx):
    """Context c's item is planted[c]: sixty in-batch steps lower the loss and raise the hit rate of the planted item over the
    untrained model"""
    sizes, item, B = [20, 6, 20], [2], 64
    rng = np.random.default_rng(1)
    planted = rng.permutation(sizes[2])

    def batch():
        c = rng.integers(0, sizes[0], size=B)
        return np.stack([c, rng.integers(0, sizes[1], size=B), planted[c]], axis=1).astype(np.int32)
    m = new_model("signadam", sizes)
    held = batch()
    before = m.evaluate_ranking(held, None, item, held[:, 2])
    losses = [float(m.fit_in_batch(batch(), None, item)) for _ in range(60)]
    after = m.evaluate_ranking(held, None, item, held[:, 2])
    print("before", before, "after", after, "loss", losses[0], "->", losses[-1])
    assert np.isfinite(losses).all() and np.mean(losses[-5:]) < np.mean(losses[:5])
    assert after["n"] == before["n"] == B
    assert after["hr@1"] > before["hr@1"] and after["hr@5"] > before["hr@5"] and after["mrr"] > before["mrr"]
