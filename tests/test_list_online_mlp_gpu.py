"""The one-workgroup list step of DeepFM / NFM (fmx_mlp_list_fit: k_mlp_small_list) and the online list loop on top of it
(fmx_online_run_mlp_list: k_online_mlp_list walking the stream, or the queued per-list launches), on the MI355X; and
run_list_experiment(full=True) of the classes with list_loop_on_device = True.

Bit-level: corr None == a corr of zeros; at G = 2 the two dz are exact negatives; the outputs do not depend on the rule; the
one-workgroup form == the queued form == the per-list sequence from outside (fmx_fm_forward at B = G, the NFM base add,
fmx_mlp_list_fit at B_lists = 1, fmx_sort_occurrences, fmx_fm_update on the list steps' copy of the table, both step counts
advanced by the engine) in rows (moments included), bias words, params, m, v, rank_out, logit_out and loss_out; halves == whole;
guard bands.
Against float64 (tests/list_fit_f64.py), with the bounds test_pair_online_mlp_gpu.py applies to fmx_mlp_pair_fit, restated:
* logit, loss, dz, gbi with test_mlp_gpu.close: 2e-5 of the tensor's largest magnitude; the loss, a scalar that log(s) leaves
  near 0 for a list its positive wins, also takes list_fit_f64's loss_floor, (G + 2) 2^-24 per list and the logits' noise (derived
  there from the formula, not from the kernel: at loss 1.3e-3 the kernel's 4.3e-8 is the rounding of s = 1.0013);
* the SGD step of every parameter tensor against -lr times the float64 gradient: 2e-5 of the tensor's largest gradient + 4 gnoise,
  plus one rounding of the parameter, 2^-23 |p|;
* rank equal wherever no comparison is closer than four times the logits' fp32 noise.
A list's dz: with u = 2^-24, dz_j = fl(fl(e_j / s) inv_b) carries 2 u |dz_j|, the sum neg of the G - 1 negatives' e_j (G - 2
additions) carries (G - 2) u neg, and dz_0 = -fl(fl(neg / s) inv_b) another 2 u |dz_0|: the exact sum of a list's dz is at most
(G + 2) u |dz_0| from zero.
Every test runs its kernels once and compares."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from abi_geometry import Guarded
from list_fit_f64 import list_fit_f64
from test_adaptive_rules_gpu import MIXED_SIZES, problem
from test_deep_adaptive_gpu import n_params
from test_kernels_gpu import HYP
from test_list_mlp_gpu import class_data, model_words, new_model
from test_mlp_gpu import close, live_units
from test_online_adaptive_gpu import NET_STEP0, T_STEP0, persistent, setup
from test_pair_gpu import build_table, same_bits

pytestmark = pytest.mark.gpu

SIZES = MIXED_SIZES[:-1]          # ten fields, none with a single row
ITEM = (2, 3)                     # the item columns (1000 and 50000 rows, zipf-drawn: the same rows again and again)
U32 = 2.0 ** -24
LR = 0.05
FIT_SHAPES = [(1, 2), (1, 16), (2, 8), (5, 3), (3, 3), (8, 2)]                      # B_lists, G
FIT_NETS = [(10, 16, 10, 5), (4, 4, 4, 1), (4, 4, 4, 8), (10, 16, 60, 3), (20, 32, 10, 5)]     # k, kp, hidden, layers: 5 x 10, 1 x 4, 8 x 4, 3 x 60, kp 32


@pytest.fixture(scope="module")
def fmx():
    import fmx as _fmx
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _fmx


def stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------------------------
# 1: fmx_mlp_list_fit alone
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fit_problem(Bl, G, k, kp, H, L):
    """-> (params, bi [Bl G, kp], base [Bl G], corr [Bl G]) as CPU tensors: no unit dead for every row (live_units)"""
    rows = Bl * G
    g = torch.Generator().manual_seed(1000 * Bl + 10 * G + H + L + k)
    params = torch.randn(n_params(k, H, L), generator=g) * (1.0 / np.sqrt(H))
    bi = torch.zeros(rows, kp)
    bi[:, :k] = torch.randn(rows, k, generator=g) * 0.5
    params = torch.from_numpy(live_units(params.numpy(), k, H, L, bi[:, :k].numpy()))
    base = torch.randn(rows, generator=g) * 0.3
    corr = torch.log(torch.rand(rows, generator=g) * 0.999 + 1e-3)
    return params, bi, base, corr


@functools.lru_cache(maxsize=None)
def fit_reference(Bl, G, k, kp, H, L, corrected):
    """the float64 reference of a case: computed once, shared by the tests, never written to"""
    params, bi, base, corr = fit_problem(Bl, G, k, kp, H, L)
    return list_fit_f64(params.numpy(), k, H, L, bi[:, :k].numpy(), base.numpy(), G, 1.0 / Bl, corr.numpy() if corrected else None)


class ListFit:
    """fmx_mlp_list_fit on one case's device buffers; run() starts from the case's parameters every time"""

    def __init__(self, fmx, Bl, G, k, kp, H, L):
        self.fmx, self.lib = fmx, fmx._lib.load()
        self.Bl, self.G, self.k, self.kp, self.H, self.L = Bl, G, k, kp, H, L
        params, bi, base, corr = fit_problem(Bl, G, k, kp, H, L)
        self.p0, self.bi, self.base, self.corr = params.cuda(), bi.cuda(), base.cuda(), corr.cuda()
        self.params = self.p0.clone()
        self.m = fmx._lib.Mlp(self.params.data_ptr(), L, k, H, 0)
        rows, f = Bl * G, dict(device="cuda")
        self.dz, self.logit = torch.empty(rows, **f), torch.empty(rows, **f)
        self.gbi, self.loss = torch.empty((rows, kp), **f), torch.zeros(1, **f)
        self.rank = torch.empty(Bl, dtype=torch.uint8, **f)
        self.hyper = fmx.Hyper(lr=LR, eps=1e-8)

    def run(self, corr=None, rule="sgd", opt=None):
        self.params.copy_(self.p0)
        for t in (self.dz, self.logit, self.gbi, self.loss):
            t.fill_(float("nan"))
        self.rank.fill_(255)
        self.fmx._lib.check(self.lib.fmx_mlp_list_fit(
            C.byref(self.m), self.hyper.ref(), self.fmx._lib.RULES[rule], self.bi.data_ptr(), self.kp, self.base.data_ptr(),
            None if corr is None else corr.data_ptr(), self.Bl, self.G, 1.0 / self.Bl, self.logit.data_ptr(), self.dz.data_ptr(),
            self.gbi.data_ptr(), self.loss.data_ptr(), self.rank.data_ptr(), None if opt is None else opt.ref(), stream()))
        torch.cuda.synchronize()

    def forward_logit(self):
        """fmx_mlp_forward's out on the same bi / base and the case's parameters"""
        m0 = self.fmx._lib.Mlp(self.p0.data_ptr(), self.L, self.k, self.H, 0)      # (read only)
        out = torch.empty_like(self.logit)
        self.fmx._lib.check(self.lib.fmx_mlp_forward(C.byref(m0), self.bi.data_ptr(), self.kp, self.base.data_ptr(), self.Bl * self.G,
                                                     out.data_ptr(), None, stream()))
        torch.cuda.synchronize()
        return out

    def outputs(self):
        return [t.clone() for t in (self.dz, self.gbi, self.logit, self.loss, self.rank)]


OUT_NAMES = ("dz", "gbi", "logit", "loss", "rank")


def same_words(a, b, what):
    """same_bits, the ranks' bytes widened first"""
    same_bits(a.int() if a.dtype == torch.uint8 else a, b.int() if b.dtype == torch.uint8 else b, what)


def fit_cases():
    """every shape with every network; the nine rows of (3, 3) at L = 8 are the threads 63 .. 71 of mlp_small_body's loss site"""
    return [(Bl, G, *net) for Bl, G in FIT_SHAPES for net in FIT_NETS]


@pytest.mark.parametrize("corrected", [False, True], ids=["plain", "corr"])
@pytest.mark.parametrize("Bl,G,k,kp,H,L", fit_cases())
def test_list_fit_vs_float64_and_its_bit_statements(fmx, Bl, G, k, kp, H, L, corrected):
    s = ListFit(fmx, Bl, G, k, kp, H, L)
    what = f"B_lists={Bl} G={G} k={k} H={H} L={L} corr={corrected}"
    s.run(s.corr if corrected else None)
    got = s.outputs()
    same_bits(s.logit, s.forward_logit(), "logit_out vs fmx_mlp_forward: the uncorrected logit")
    r = fit_reference(Bl, G, k, kp, H, L, corrected)
    close(s.logit.cpu().numpy(), r["out"], "logit")
    close(s.loss.item(), r["loss"], "loss", floor=r["loss_floor"])
    print(f"{what} loss: err {abs(s.loss.item() - r['loss']):.3e}, bound {2e-5 * abs(r['loss']) + r['loss_floor']:.3e}")
    close(s.dz.cpu().numpy(), r["dz"], "dz")
    gbi = s.gbi.cpu().numpy()
    close(gbi[:, :k], r["gbi"], "gbi")
    assert (gbi[:, k:] == 0).all(), "padding columns of gbi must be zeroed"
    for name, a, b in (("logit", s.logit.cpu().numpy(), r["out"]), ("dz", s.dz.cpu().numpy(), r["dz"]), ("gbi", gbi[:, :k], r["gbi"])):
        print(f"{what} {name}: max err / (2e-5 max|ref|) = {np.abs(a - b).max() / (2e-5 * max(np.abs(b).max(), 1e-30)):.4f}")
    rank = s.rank.cpu().numpy()
    sure = ~r["ties"]
    np.testing.assert_array_equal(rank[sure], r["rank"][sure], err_msg=what + ": rank")
    z = s.logit.cpu().numpy().reshape(Bl, G)
    np.testing.assert_array_equal(rank, (z[:, 1:] >= z[:, :1]).sum(1), err_msg=what + ": rank is counted on the stored logits")
    # a list's dz: exact negatives at G = 2, within (G + 2) u |dz_0| of zero otherwise (the module docstring)
    dz = s.dz.cpu().double().numpy().reshape(Bl, G)
    assert (dz[:, 0] <= 0).all() and (dz[:, 1:] >= 0).all(), what + ": dz_0 <= 0 <= dz_j"
    if G == 2:
        same_bits(s.dz[1::2], -s.dz[0::2], what + ": dz[2i + 1] == -dz[2i]")
    assert (np.abs(dz.sum(1)) <= (G + 2) * U32 * np.abs(dz[:, 0])).all(), (what, dz.sum(1), dz[:, 0])
    # the SGD step: -lr times the float64 gradient, close_per_tensor's bound on the gradient plus one rounding of the parameter
    p0, p1 = s.p0.cpu().numpy().astype(np.float64), s.params.cpu().numpy().astype(np.float64)
    assert not np.array_equal(p0, p1), "the network did not move"
    off = 0
    for l in range(L):
        i = k if l == 0 else H
        for name, n, g_ref, g_noise in (("W", H * i, r["grads"][l][0], r["gnoise"][l][0]), ("b", H, r["grads"][l][1], r["gnoise"][l][1])):
            close(p1[off:off + n] - p0[off:off + n], -LR * g_ref.reshape(-1), f"{what}: step of {name}{l}",
                  floor=LR * 4 * g_noise.reshape(-1) + 2 * U32 * np.abs(p1[off:off + n]))
            off += n
    assert off == p0.size
    if not corrected:       # corr == nullptr and a corr of +0 agree in every bit, the parameters included
        params = s.params.clone()
        s.run(torch.zeros_like(s.corr))
        for name, a, b in zip(OUT_NAMES, got, s.outputs()):
            same_words(a, b, f"{what}: corr None vs zeros: {name}")
        same_bits(params, s.params, what + ": corr None vs zeros: params")
    else:                   # ... and the correction reaches the loss while the stored logit stays the uncorrected one
        s.run(None)
        same_bits(got[2], s.logit, what + ": logit_out does not see corr")
        assert not torch.equal(got[0], s.dz)


@pytest.mark.parametrize("Bl,G,k,kp,H,L", [(1, 16, 10, 16, 10, 5), (3, 3, 4, 4, 4, 8), (2, 8, 10, 16, 60, 3), (8, 2, 20, 32, 10, 5)])
def test_list_fit_rules(fmx, Bl, G, k, kp, H, L):
    """dz, gbi, logit, loss and rank do not depend on the rule; opt (SGD) is rule SGD at the same lr; opt->step is read only; under
    opt ADAM m and v move, under ADAGRAD m keeps its bits."""
    s = ListFit(fmx, Bl, G, k, kp, H, L)
    s.run(s.corr, rule="sgd")
    first, by_rule_sgd = s.outputs(), s.params.clone()
    s.run(s.corr, rule="signadam")
    for name, a, b in zip(OUT_NAMES, first, s.outputs()):
        same_words(a, b, f"rule signadam: {name}")
    assert not torch.equal(s.params, s.p0) and not torch.equal(s.params, by_rule_sgd)
    n = s.p0.numel()
    g = torch.Generator().manual_seed(n)
    for rule in ("sgd", "adagrad", "adam"):
        opt = fmx.MlpOpt(n, rule, lr=LR, device="cuda", step=5)
        opt.m.copy_((torch.randn(n, generator=g) * 1e-3).cuda())
        opt.v.copy_((torch.randn(n, generator=g) ** 2 * 1e-5).cuda())
        m0, v0 = opt.m.clone(), opt.v.clone()
        s.run(s.corr, rule="signadam", opt=opt)            # (`rule` is not read with opt)
        for name, a, b in zip(OUT_NAMES, first, s.outputs()):
            same_words(a, b, f"opt {rule}: {name}")
        assert opt.c.step == 5 and opt.step == 5, "opt->step is read, never written"
        if rule == "sgd":
            same_bits(s.params, by_rule_sgd, "opt (SGD) vs rule SGD at the same lr")
            same_bits(opt.m, m0, "opt (SGD): m")
            same_bits(opt.v, v0, "opt (SGD): v")
        else:
            assert not torch.equal(s.params, s.p0) and not torch.equal(opt.v, v0), rule
            if rule == "adagrad":
                same_bits(opt.m, m0, "adagrad neither loads nor stores m")
            else:
                assert not torch.equal(opt.m, m0)


# ---------------------------------------------------------------------------------------------------------------
# 2: the loop, three ways
# ---------------------------------------------------------------------------------------------------------------
RULE_PAIRS = [("signadam", None), ("sgd", None), ("adam", "adam"), ("adagrad", "adagrad")]
K_OF_KP = {4: 4, 16: 10, 32: 20, 64: 60}


def list_stream(sizes, k, N, G, seed, item=ITEM, with_x=True, with_corr=True):
    """-> (rows int32 [N G, F], x float32 [N G, F] or None, corr float32 [N G] or None).  Zipf-drawn positives (the same rows
    again and again); a list's negatives are its positive with the second item column redrawn from the same law and, in every
    other negative, the first as well: the context fields name the same row in all G positions.  List 3: its last two rows
    name the same item (G >= 3).  List 5: its first negative is its positive, x included.  List 6: its first negative differs from
    the positive in every column.  About 10 % of x is exactly 0."""
    _, idx, x, _ = problem(sizes, k, N * G, seed)
    rows = np.repeat(idx[0::G][:, None, :], G, axis=1)
    draws = idx.reshape(N, G, -1)
    rows[:, 1:, item[1]] = draws[:, 1:, item[1]]
    rows[:, 2::2, item[0]] = draws[:, 2::2, item[0]]
    x = x.reshape(N, G, -1).copy()
    if N > 6:
        rows[3, G - 1] = rows[3, G - 2]
        rows[5, 1], x[5, 1] = rows[5, 0], x[5, 0]
        rows[6, 1] = (rows[6, 0] + 1) % np.asarray(sizes, dtype=np.int32)
    rows = np.ascontiguousarray(rows.reshape(N * G, -1).astype(np.int32))
    corr = np.log(np.random.default_rng(seed).uniform(1e-3, 1.0, size=N * G)).astype(np.float32) if with_corr else None
    return rows, (np.ascontiguousarray(x.reshape(N * G, -1)) if with_x else None), corr


def assert_stream_has_the_cases(rows, sizes, N, G):
    lists = rows.reshape(N, G, -1)
    ctx = [f for f in range(len(sizes)) if f not in ITEM]
    assert (lists[:, :, ctx] == lists[:, :1, ctx]).all(1).all(1).sum() >= N - 1, "context fields shared by all G rows"
    assert len(np.unique(lists[:, 0, ITEM[1]])) < N, "zipf: rows repeat across lists"
    assert (lists[5, 1] == lists[5, 0]).all(), "a negative equal to its positive"
    assert (lists[6, 1] != lists[6, 0]).all(), "a negative that differs in every column"
    assert G < 3 or (lists[3, G - 1] == lists[3, G - 2]).all(), "two negatives naming the same item"


def snapshot(t, params, opt, outs):
    torch.cuda.synchronize()
    rank, logit, loss = outs
    s = dict(rows=t.rows.cpu().numpy().copy(), bias=t.bias.cpu().numpy().copy(), params=params.cpu().numpy().copy(),
             rank=rank.cpu().numpy().copy(), logit=logit.cpu().numpy().copy(), loss=loss.cpu().numpy().copy(),
             steps=np.array([t.step if t.layout == "moments" else -1, -1 if opt is None else opt.step]))
    if opt is not None:
        s.update(m=opt.m.cpu().numpy().copy(), v=opt.v.cpu().numpy().copy())
    return s


def assert_same(a, b, what):
    for kk in a:
        np.testing.assert_array_equal(a[kk].view(np.int32) if a[kk].dtype == np.float32 else a[kk],
                                      b[kk].view(np.int32) if b[kk].dtype == np.float32 else b[kk], err_msg=f"{what}: {kk}")


def per_list(e, t, hyp, table_rule, params, k, H, L, fm_term, idx_d, xv_d, corr_d, G, opt):
    """The N per-list sequences from outside: fmx_fm_forward (B = G, no loss), the NFM base add, fmx_mlp_list_fit (B_lists = 1,
    inv_b = 1), fmx_sort_occurrences (B = G), fmx_fm_update (B = G) on the list steps' copy of the table (list_sort_update);
    FMEngine advances the table's and the network's counts."""
    N = idx_d.shape[0] // G
    rank = torch.empty(N, dtype=torch.uint8, device="cuda")
    logit, loss = torch.empty(N * G, device="cuda"), torch.empty(N, device="cuda")
    for i in range(N):
        r = idx_d[G * i:G * (i + 1)]
        xi = None if xv_d is None else xv_d[G * i:G * (i + 1)]
        e.forward(hyp, r, xi, want_first=False, want_bi=True)
        base = (e.logit[:G] if fm_term else e.sfirst[:G] + t.bias[0]).contiguous()
        dz, gbi, z, rk = e.mlp_list_fit(params, k, H, L, hyp, table_rule if opt is None else "sgd", base, 1, G, inv_b=1.0,
                                        corr=None if corr_d is None else corr_d[G * i:G * (i + 1)], mlp_opt=opt, want_logit=True,
                                        want_rank=True)
        rank[i:i + 1] = rk
        logit[G * i:G * (i + 1)] = z
        loss[i] = e.loss_out[0]
        e.list_sort_update(hyp, table_rule, r, G, xi, dz, dz if fm_term else None, gbi, inv_b=1.0)
    return rank, logit, loss


def loop(e, hyp, table_rule, params, k, H, L, fm_term, idx_d, xv_d, corr_d, G, opt):
    return e.online_run_mlp_list(hyp, table_rule, params, k, H, L, fm_term, idx_d, G, xv_d, corr=corr_d, mlp_opt=opt, want_logit=True,
                                 want_loss=True)


def three_ways(fmx, make, table_rule, k, H, L, fm_term, rows, x, corr, G, forms=("one workgroup", "queued", "per list"), flag=False):
    """make() -> (table, engine, hyper, params, opt or None), identical every time.  -> {form: snapshot}"""
    res = {}
    for form in forms:
        t, e, hyp, params, opt = make()
        idx_d, xv_d, _ = e.to_device(rows, x)
        corr_d = None if corr is None else torch.from_numpy(corr).cuda()
        if form == "per list":
            outs = per_list(e, t, hyp, table_rule, params, k, H, L, fm_term, idx_d, xv_d, corr_d, G, opt)
        else:
            with persistent(fmx, form != "queued"):
                outs = loop(e, hyp, table_rule, params, k, H, L, fm_term, idx_d, xv_d, corr_d, G, opt)
        torch.cuda.synchronize()
        if flag:
            assert int(e.error.item()) == 1, f"{form}: the index flag was not raised"
            e.error.zero_()
        else:
            e.check_error_flag()
        res[form] = snapshot(t, params, opt, outs)
    return res


def maker(fmx, table_rule, net_rule, k, H, L, seed, sizes=SIZES):
    def make():
        t, e, hyp, params, opt = setup(fmx, table_rule, net_rule or "sgd", k, H, L, seed=seed, sizes=sizes)
        return t, e, hyp, params, (opt if net_rule else None)
    return make


def check_three(res, what):
    assert_same(res["one workgroup"], res["queued"], what + ": one workgroup vs queued launches")
    assert_same(res["one workgroup"], res["per list"], what + ": one workgroup vs per-list calls")


@pytest.mark.parametrize("kp", [16, 32])
@pytest.mark.parametrize("table_rule,net_rule", RULE_PAIRS)
@pytest.mark.parametrize("fm_term", [1, 0], ids=["deepfm", "nfm"])
@pytest.mark.parametrize("G", [2, 3, 8, 9, 16])
def test_one_workgroup_equals_queued_equals_per_list_calls(fmx, G, fm_term, table_rule, net_rule, kp):
    """G <= 8: one workgroup (k_online_mlp_list) against the queued form and the per-list calls.  G = 9 and 16 take the queued form
    whatever online_persistent says, and still equal the per-list sequence."""
    k, H, L, N = K_OF_KP[kp], 32, 2, 40
    odd = (RULE_PAIRS.index((table_rule, net_rule)) + [16, 32].index(kp) + fm_term + G) % 2 == 0
    rows, x, corr = list_stream(SIZES, k, N, G, 7100 + kp + G, with_x=odd, with_corr=not odd or G == 3)     # xv / corr given and null
    assert_stream_has_the_cases(rows, SIZES, N, G)
    assert x is None or (x == 0).any()
    make = maker(fmx, table_rule, net_rule, k, H, L, seed=kp + G)
    assert make()[0].kp == kp
    res = three_ways(fmx, make, table_rule, k, H, L, fm_term, rows, x, corr, G)
    whole = res["one workgroup"]
    moments = table_rule in ("adam", "adagrad")
    assert list(whole["steps"]) == [T_STEP0 + N if moments else -1, NET_STEP0 + N if net_rule else -1]
    check_three(res, f"G={G} kp={kp} {table_rule}/{net_rule} fm_term={fm_term}")
    z = whole["logit"].reshape(N, G)
    np.testing.assert_array_equal(whole["rank"], (z[:, 1:] >= z[:, :1]).sum(1))
    assert z[5, 1].view(np.int32) == z[5, 0].view(np.int32) and whole["rank"][5] >= 1, "the negative that is its positive ties with it"
    assert np.isfinite(whole["loss"]).all() and np.isfinite(whole["logit"]).all() and (whole["loss"] > 0).all()
    t0, _, _, p0, o0 = make()
    assert not np.array_equal(whole["params"], p0.cpu().numpy()), "the network did not move"
    if net_rule == "adagrad":
        np.testing.assert_array_equal(whole["m"], o0.m.cpu().numpy(), err_msg="adagrad neither loads nor stores m")
        assert not np.array_equal(whole["v"], o0.v.cpu().numpy())
    elif net_rule == "adam":
        assert not np.array_equal(whole["m"], o0.m.cpu().numpy()) and not np.array_equal(whole["v"], o0.v.cpu().numpy())
    # untouched rows keep their bits; the bias and its state are bit-unchanged under EVERY rule (ADAM's moments included)
    offs = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    touched = np.unique(rows.astype(np.int64) + offs[:-1][None, :])
    untouched = np.setdiff1d(np.arange(t0.n_rows), touched)
    assert untouched.size > 0
    rows0 = t0.rows.cpu().numpy()
    np.testing.assert_array_equal(whole["rows"][untouched].view(np.int32), rows0[untouched].view(np.int32))
    assert not np.array_equal(whole["rows"][touched], rows0[touched])
    np.testing.assert_array_equal(whole["bias"].view(np.int32), t0.bias.cpu().numpy().view(np.int32))


@pytest.mark.parametrize("G", [3, 8])
def test_runs_over_three_lane_groups_at_eight_waves(fmx, G):
    """kp = 4: a lane group is ONE position of a field's sorted list, so a shared context field of G >= 3 rows is a run over three
    lane groups (RunSum) in the one-workgroup form."""
    k, H, L, N = 4, 16, 2, 40
    rows, x, corr = list_stream(SIZES, k, N, G, 7200 + G)
    make = maker(fmx, "adam", "adam", k, H, L, seed=G)
    assert make()[0].kp == 4
    check_three(three_ways(fmx, make, "adam", k, H, L, 1, rows, x, corr, G), f"kp = 4, G = {G}")


# ---------------------------------------------------------------------------------------------------------------
# 3: field counts at the edges of the one-workgroup form; FTRL tables; the LDS cap
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kp,F", [(64, 4), (64, 16), (64, 17), (4, 128), (4, 129)])
@pytest.mark.parametrize("G", [3, 9])
def test_field_counts_around_the_one_workgroup_form(fmx, kp, F, G):
    """kp = 64: four rows per pass, four passes -- F = 16 is the most one wavefront holds, F = 17 takes the queued form whatever
    online_persistent says.  kp = 4: the kernel keeps the (index, value) of 128 fields; F = 129 takes the queued form.  Every
    form still equals the per-list sequence."""
    k, H, L, N = K_OF_KP[kp], 32, 2, 12 if F > 100 else 40
    sizes = [5 + i % 7 for i in range(F)]
    rows, x, corr = list_stream(sizes, k, N, G, 7300 + F, item=(F - 2, F - 1))
    make = maker(fmx, "adam", "adam", k, H, L, seed=F, sizes=sizes)
    assert make()[0].kp == kp
    check_three(three_ways(fmx, make, "adam", k, H, L, 1, rows, x, corr, G), f"kp = {kp}, F = {F}, G = {G}")


@pytest.mark.parametrize("net_rule", ["adam", "sgd"])
def test_ftrl_table_with_opt_takes_the_queued_form(fmx, net_rule):
    k, H, L, N, G = 16, 32, 2, 40, 4
    rows, x, corr = list_stream(SIZES, k, N, G, 7400)

    def make():
        t, _ = build_table(fmx, SIZES, k, "ftrl")
        e, hyp = fmx.FMEngine(t, max_batch=8), fmx.Hyper(**HYP)
        _, _, _, params, opt = setup(fmx, "sgd", net_rule, k, H, L, seed=3, sizes=SIZES)
        return t, e, hyp, params, opt
    res = three_ways(fmx, make, "ftrl", k, H, L, 1, rows, x, corr, G)
    check_three(res, "FTRL tables")
    t0 = make()[0]
    assert not np.array_equal(res["queued"]["rows"], t0.rows.cpu().numpy())
    np.testing.assert_array_equal(res["queued"]["bias"].view(np.int32), t0.bias.cpu().numpy().view(np.int32))


@pytest.mark.parametrize("net_rule", ["adam", None], ids=["moments", "no moments"])
@pytest.mark.parametrize("k,G", [(61, 3), (61, 8), (63, 3)])
def test_networks_around_the_lds_cap(fmx, k, G, net_rule):
    """H = 64, L = 2: 8,128 parameters at k = 61, the largest network of this shape under the one-workgroup form's cap of 8,192 --
    under ADAM 96 KB of parameters and moments in LDS beside the kernel's 54 KB of static arrays, at 4 and at 8 waves -- and 8,256
    at k = 63, just above it: the queued form."""
    H, L, N = 64, 2, 24
    n = n_params(k, H, L)
    assert (n <= 8192) == (k == 61) and abs(n - 8192) <= 64
    table_rule = "adam" if net_rule else "signadam"
    rows, x, corr = list_stream(SIZES, k, N, G, 7500 + k)
    check_three(three_ways(fmx, maker(fmx, table_rule, net_rule, k, H, L, seed=k), table_rule, k, H, L, 1, rows, x, corr, G),
                f"{n} parameters, G = {G}, {net_rule}")


# ---------------------------------------------------------------------------------------------------------------
# 4: halves equal the whole; guard bands; the index flag
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["one workgroup", "queued"])
def test_two_halves_equal_one_call(fmx, form):
    k, H, L, N, G = 16, 32, 2, 40, 5
    rows, x, corr = list_stream(SIZES, k, N, G, 7600)
    res = []
    for cuts in ([N], [N // 2, N - N // 2]):
        t, e, hyp, params, opt = setup(fmx, "adam", "adam", k, H, L, seed=2, sizes=SIZES)
        idx_d, xv_d, _ = e.to_device(rows, x)
        corr_d = torch.from_numpy(corr).cuda()
        outs, lo = [], 0
        with persistent(fmx, form == "one workgroup"):
            for c in cuts:
                sl = slice(G * lo, G * (lo + c))
                outs.append(loop(e, hyp, "adam", params, k, H, L, 1, idx_d[sl], xv_d[sl], corr_d[sl], G, opt))
                lo += c
                assert t.step == T_STEP0 + lo and opt.step == NET_STEP0 + lo
        e.check_error_flag()
        res.append(snapshot(t, params, opt, [torch.cat(o) for o in zip(*outs)]))
    assert_same(res[0], res[1], f"{form}: one call vs two halves")


@pytest.mark.parametrize("form", ["one workgroup", "queued"])
@pytest.mark.parametrize("fm_term,G", [(1, 3), (0, 8), (0, 16)], ids=["deepfm-3", "nfm-8", "nfm-16"])
def test_guard_bands_and_which_form_ran(fmx, form, fm_term, G):
    """Every buffer the call writes sits between NaN-patterned bands that must survive: rank_out, logit_out, loss_out, scratch,
    the fwd buffers, the workspace, params, m, v.  Which form ran: k_online_mlp_list keeps everything between the rows and its
    outputs in registers and LDS, so the one-workgroup form (G <= 8) leaves the caller's scratch and fwd buffers as they were, a
    NaN in every word, while the queued launches write them -- as does the default at G = 16, which queues."""
    L_ = fmx._lib
    lib = L_.load()
    k, H, L, N = 16, 32, 2, 24
    rows, x, corr = list_stream(SIZES, k, N, G, 7700)
    t, e, hyp, params, opt = setup(fmx, "adam", "adam", k, H, L, seed=4, sizes=SIZES)
    idx_d, xv_d, _ = e.to_device(rows, x)
    corr_d = torch.from_numpy(corr).cuda()
    kp, n = t.kp, params.numel()
    g = {name: Guarded(4 * words, name=name) for name, words in
         (("logit_out", N * G), ("loss_out", N), ("scratch", 16 + G * kp), ("S", G * kp), ("bi", G * kp), ("sfirst", G), ("logit", G),
          ("params", n), ("m", n), ("v", n))}
    g["rank_out"] = Guarded(N, dtype=torch.uint8, name="rank_out")
    g["error"] = Guarded(4, dtype=torch.int32, name="error")
    g["workspace"] = Guarded(int(lib.fmx_fm_list_workspace_bytes(t.c_struct(), 1, G)), dtype=torch.int32, name="workspace")
    g["params"].t.copy_(params)
    g["m"].t.copy_(opt.m)
    g["v"].t.copy_(opt.v)
    staging = ("scratch", "S", "bi", "sfirst", "logit")
    for name in staging:
        g[name].t.fill_(float("nan"))
    bias0 = t.bias.clone()
    out = L_.FwdOut()
    out.S, out.bi, out.sfirst, out.logit, out.error = g["S"].ptr, g["bi"].ptr, g["sfirst"].ptr, g["logit"].ptr, g["error"].ptr
    mlp = L_.Mlp(g["params"].ptr, L, k, H, 0)
    o = L_.MlpOpt(g["m"].ptr, g["v"].ptr, opt.c.lr, opt.c.eps, opt.c.beta1, opt.c.beta2, opt.c.rule, NET_STEP0)
    hyp.c.step = t.step
    with persistent(fmx, form == "one workgroup"):
        L_.check(lib.fmx_online_run_mlp_list(t.c_struct(), hyp.ref(), L_.RULES["adam"], C.byref(mlp), fm_term, idx_d.data_ptr(),
                                             xv_d.data_ptr(), corr_d.data_ptr(), N, G, g["workspace"].ptr, g["workspace"].nbytes,
                                             C.byref(out), g["scratch"].ptr, g["rank_out"].ptr, g["logit_out"].ptr, g["loss_out"].ptr,
                                             C.byref(o), stream()))
    torch.cuda.synchronize()
    for b in g.values():
        b.check()
    assert int(g["error"].t[0].item()) == 0
    assert not torch.equal(g["params"].t, params) and np.isfinite(g["loss_out"].t.cpu().numpy()).all() and np.isfinite(g["logit_out"].t.cpu().numpy()).all()
    same_bits(t.bias, bias0, "the bias and its state are read, never written")
    untouched = [bool(torch.isnan(g[name].t).all()) for name in staging]
    if form == "one workgroup" and G <= 8:
        assert all(untouched), f"k_online_mlp_list did not run: staging buffers written {dict(zip(staging, untouched))}"
    else:
        assert not any(untouched[:3]), f"the queued launches did not run: {dict(zip(staging, untouched))}"      # (dz / gbi, S, bi)


@pytest.mark.parametrize("G,where", [(4, 0), (4, 2), (9, 5)])
def test_out_of_range_index_in_one_row_of_one_list(fmx, G, where):
    """An index past its field in ONE row of one list: the existing range check catches it (the occurrence is dropped, nothing is
    read or written through it), the flag is raised in every form, and the other rows' run of the field is the per-list
    sequence's, whose sort drops the occurrence.  The rows no valid index names keep their bits (the row the bad index would
    alias among them)."""
    k, H, L, N = 16, 32, 2, 16
    rows, x, corr = list_stream(SIZES, k, N, G, 7800)
    f, i = 4, 7
    bad = G * i + where
    rows[bad, f] = SIZES[f] + 5                       # would alias row 5 of the next field
    rows[:, f + 1] = np.minimum(rows[:, f + 1], 4)    # ... which nothing else names
    make = maker(fmx, "adam", "adam", k, H, L, seed=8)
    res = three_ways(fmx, make, "adam", k, H, L, 1, rows, x, corr, G, flag=True)
    check_three(res, f"bad index in row {where} of a list of {G}")
    t0 = make()[0]
    offs = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    valid = rows.astype(np.int64) < np.asarray(SIZES)[None, :]
    touched = np.unique((rows.astype(np.int64) + offs[:-1][None, :])[valid])
    untouched = np.setdiff1d(np.arange(t0.n_rows), touched)
    assert offs[f + 1] + 5 in untouched
    np.testing.assert_array_equal(res["one workgroup"]["rows"][untouched].view(np.int32), t0.rows.cpu().numpy()[untouched].view(np.int32))
    other = offs[f] + rows[bad + (1 if where == 0 else -1), f]      # another row of that list: its row of the field moved
    assert not np.array_equal(res["one workgroup"]["rows"][other], t0.rows.cpu().numpy()[other])


# ---------------------------------------------------------------------------------------------------------------
# 5: the classes
# ---------------------------------------------------------------------------------------------------------------
def by_hand_loop(m, rows, xv, G, corr=None):
    """run_list_experiment(full=True)'s device loop restated with the engine's per-list sequence -> the lists ranked first"""
    rank, _, _ = per_list(m._engine, m._table, m._hyper, m.update_rule, m._mlp_flat, m.embedding_size, m.neuron_per_hidden_layer,
                          m.num_hidden_layers, m._fm_term_in_forward, rows.contiguous(), None if xv is None else xv.contiguous(),
                          corr, G, m._mlp_fused)
    return int((rank == 0).sum().item())


@pytest.mark.parametrize("cls,rule", [("DeepFMAdam", "signadam"), ("NFMAdam", "adam")])
def test_run_list_experiment_on_the_device_is_the_per_list_sequence(fmx, cls, rule):
    N, n_neg = 30, 4
    Xi, Xv, item, neg = class_data(N, n_neg, seed=8)
    a, b = new_model(cls, rule), new_model(cls, rule)
    assert a.list_loop_on_device is False
    a.list_loop_on_device = True
    assert a._list_device_loop_ok()
    secs, acc, checkpoints, counts = a.run_list_experiment(Xi, Xv, item, negatives=neg, full=True)
    rows, xv = fmx.pairwise.assemble_lists(torch.from_numpy(Xi).cuda(), torch.from_numpy(Xv).cuda(), item, torch.from_numpy(neg).cuda())
    correct = by_hand_loop(b, rows, xv, 1 + n_neg)
    torch.cuda.synchronize()
    for (name, wa), (_, wb) in zip(model_words(a), model_words(b)):
        same_bits(wa, wb, f"{cls} {rule}: {name}")
    assert counts == {"correct": correct, "wrong": N - correct} and a._table.step == b._table.step
    assert a._mlp_fused is None or a._mlp_fused.step == b._mlp_fused.step == N
    assert acc == checkpoints[-1] == pytest.approx(100.0 * correct / N) and len(checkpoints) == 2 and secs > 0


@pytest.mark.parametrize("cls,rule", [("DeepFMAdam", "signadam"), ("NFMAdam", "adam")])
def test_with_the_attribute_false_the_host_loop_runs(fmx, cls, rule):
    """Counted, not timed: the default takes one fmx_mlp_list_section per list and never the device loop; with the attribute set
    it is the other way round."""
    N, n_neg = 6, 3
    Xi, Xv, item, neg = class_data(N, n_neg, seed=9)
    for on in (False, True):
        m = new_model(cls, rule)
        m.list_loop_on_device = on
        e, count = m._engine, {"section": 0, "loop": 0}
        section, run = e.mlp_list_section, e.online_run_mlp_list

        def counted_section(*a, **kw):
            count["section"] += 1
            return section(*a, **kw)

        def counted_run(*a, **kw):
            count["loop"] += 1
            return run(*a, **kw)
        e.mlp_list_section, e.online_run_mlp_list = counted_section, counted_run
        m.run_list_experiment(Xi, Xv, item, negatives=neg, full=True)
        assert count == ({"section": 0, "loop": 1} if on else {"section": N, "loop": 0}), (on, count)


def test_popularity_negatives_on_the_device_are_the_up_front_draws(fmx):
    """PopularityNegatives(correct=True) with the device loop: ONE sampler call for all positives, its log Q the call's corr --
    the per-list sequence fed the same draws (a twin model at the same seed and draw count makes them)."""
    from fmx.pairwise import PopularityNegatives
    from test_pair_gpu import SMALL
    N, n_neg, item = 20, 3, [4]
    Xi, Xv, _, _ = class_data(N, n_neg, seed=10)
    weights = np.arange(1, SMALL[4] + 1, dtype=np.float64)
    a, b = new_model("DeepFMAdam", "signadam"), new_model("DeepFMAdam", "signadam")
    a.list_loop_on_device = True
    _, _, _, counts = a.run_list_experiment(Xi, Xv, item, negatives=PopularityNegatives(weights, correct=True), n_neg=n_neg, full=True)
    assert a._mining_offset == 1, "one draw for the whole stream"
    idx_d, xv_d, _ = b._inputs(Xi, Xv)
    negs, corr = b._sample_popular(idx_d, item, PopularityNegatives(weights, correct=True), n_neg, None, None)
    rows, xv = fmx.pairwise.assemble_lists(idx_d, xv_d, item, negs)
    correct = by_hand_loop(b, rows, xv, 1 + n_neg, corr.reshape(-1).contiguous())
    torch.cuda.synchronize()
    for (name, wa), (_, wb) in zip(model_words(a), model_words(b)):
        same_bits(wa, wb, f"popularity negatives: {name}")
    assert counts == {"correct": correct, "wrong": N - correct}
    # ... and the correction reaches the step: the same draws without it end elsewhere
    c = new_model("DeepFMAdam", "signadam")
    c.list_loop_on_device = True
    c.run_list_experiment(Xi, Xv, item, negatives=PopularityNegatives(weights, correct=False), n_neg=n_neg, full=True)
    assert not torch.equal(c._mlp_flat, a._mlp_flat)


@pytest.mark.parametrize("cls,rule", [("DeepFMAdam", "signadam"), ("NFMAdam", "adam")])
def test_the_device_loop_learns(fmx, cls, rule):
    """Thirty lists repeated over a few passes: the hit rate (the positive ranked first) of the last pass is above the first's,
    and the mean list loss below."""
    N, n_neg = 30, 4
    Xi, Xv, item, neg = class_data(N, n_neg, seed=9)
    m = new_model(cls, rule)
    rows, xv = fmx.pairwise.assemble_lists(torch.from_numpy(Xi).cuda(), torch.from_numpy(Xv).cuda(), item, torch.from_numpy(neg).cuda())
    hits, means = [], []
    for _ in range(8):
        rank, _, loss = m._engine.online_run_mlp_list(m._hyper, m.update_rule, m._mlp_flat, m.embedding_size, m.neuron_per_hidden_layer,
                                                      m.num_hidden_layers, m._fm_term_in_forward, rows.contiguous(), 1 + n_neg,
                                                      xv.contiguous(), mlp_opt=m._mlp_fused, want_loss=True)
        hits.append(int((rank == 0).sum().item()))
        means.append(float(loss.mean().item()))
    m._engine.check_error_flag()
    print("hits per pass:", hits, "mean list loss per pass:", means)
    assert hits[-1] > hits[0] and means[-1] < means[0]
