"""Listwise (sampled-softmax) training of DeepFM / NFM on the device: fmx_mlp_list_section (k_mlp_list_loss between the separate
forward and backward GEMM launches, never k_mlp_chain), fmx_deepfm_list_stream and the classes' fit_lists /
run_list_experiment(full=True).

The reference is tests/list_mlp_f64.py (float64 autograd with the rounding noise of every output); the bounds are test_mlp_gpu's
close / close_per_tensor with four times that noise as the floor, the multiplier test_pair_mlp_gpu.py uses.  A corrected case's
reference is list_mlp_f64 on base - corr, and the device's (uncorrected) logits are compared with its out + corr.

Shapes (B_lists, G, k, kp, hidden, layers): one list at hidden 1; one full workgroup of four lists at a ragged width with
kp > k; one list past a workgroup at an odd width below 64; 37 lists of 8 through five layers; the largest list; and two
chain-eligible networks (hidden 256), run under mlp_chain = 1 and 0 with every output bit-identical, since the list section
never takes the chain kernel."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from abi_geometry import Guarded
from list_mlp_f64 import list_mlp_f64
from test_deep_adaptive_gpu import NET_HYP, assert_net_step, draw_clear_of_kinks, tensors_of, unsafe_samples
from test_kernels_gpu import HYP
from test_mlp_gpu import close, close_per_tensor, live_units
from test_pair_gpu import SMALL, build_table, clone_table, same_bits

pytestmark = pytest.mark.gpu

CASES = [(1, 2, 4, 4, 1, 2), (4, 3, 10, 12, 40, 2), (5, 5, 4, 4, 33, 1), (37, 8, 16, 16, 64, 5), (3, 16, 16, 16, 64, 2),
         (9, 7, 16, 16, 256, 3), (17, 2, 64, 64, 256, 1)]
CHAIN_ELIGIBLE = CASES[5:]
WORKLOAD = (2048, 8, 16, 16, 256, 3)      # 16,384 rows: the separate GEMM launches at hidden 256 above B = 4,096
GUARD_ROWS = 5
NAN_WORD = 0x7FC00BAD      # a quiet NaN with a payload of its own


@pytest.fixture(scope="module")
def fmx():
    import fmx as _fmx
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _fmx


def n_params(k, H, L):
    return sum(H * (k if l == 0 else H) + H for l in range(L))


@functools.lru_cache(maxsize=None)
def problem(Bl, G, k, kp, H, L):
    """-> (params, bi [N, kp], base [N], corr [N]) as CPU tensors, N = Bl G: no layer dead (live_units); corr is log Q of a
    popularity between 1e-3 and 1"""
    N = Bl * G
    g = torch.Generator().manual_seed(1000 * Bl + 31 * G + H + L + k)
    params = torch.randn(n_params(k, H, L), generator=g) * (1.0 / np.sqrt(H))
    bi = torch.zeros(N, kp)
    bi[:, :k] = torch.randn(N, k, generator=g) * 0.5
    params = torch.from_numpy(live_units(params.numpy(), k, H, L, bi[:, :k].numpy()))
    if (Bl, G, k, kp, H, L) == WORKLOAD:
        # 16,384 rows x 768 units: a row or two sit within fp32 rounding of a relu kink, where the fp32 forward takes the other
        # side than float64 and the row's gbi jumps by a whole unit's path (row 9,614 of the first draw: 126 times the bound, every
        # other row at 0.03 of it) -- no statement about the kernels.  Such rows are drawn again, as test_deep_adaptive_gpu does.
        # (unsafe_samples judges row by row: after the first pass only the rows drawn again are looked at)
        rng, todo = np.random.default_rng(N), np.arange(N)
        for _ in range(200):
            todo = todo[unsafe_samples(params.numpy(), k, H, L, bi[todo, :k].numpy())]
            if not todo.size:
                break
            bi[todo, :k] = torch.from_numpy(rng.normal(size=(todo.size, k)) * 0.5).float()
        assert not todo.size, "no batch clear of the relu kinks in 200 rounds"
    base = torch.randn(N, generator=g) * 0.3
    corr = torch.log(torch.rand(N, generator=g) * 0.999 + 1e-3)
    return params, bi, base, corr


@functools.lru_cache(maxsize=None)
def reference(Bl, G, k, kp, H, L, corrected):
    """the float64 reference of a case: computed once, shared by the tests, never written to"""
    params, bi, base, corr = problem(Bl, G, k, kp, H, L)
    b64 = base.double().numpy() - (corr.double().numpy() if corrected else 0.0)
    r = list_mlp_f64(params.numpy(), k, H, L, bi[:, :k].numpy(), b64, G, 1.0 / Bl)
    for l in range(L):
        # every layer is exercised.  (A bias gradient sums a list's dz over the rows a unit is live for: at hidden = 1 with one list
        # of two rows, both on the one unit, it is dz_0 + dz_1 = exactly 0 in float64 too -- no sign of a dead layer, so W's
        # gradient decides there, as in test_pair_mlp_gpu.)
        assert np.any(r["grads"][l][0]) and (np.any(r["grads"][l][1]) or H == 1), f"layer {l} has no live unit (a dead network)"
    return r


def nan_filled(*shape):
    return torch.full(shape, NAN_WORD, dtype=torch.int32, device="cuda").view(torch.float32)


class Section:
    """fmx_mlp_list_section on one case's device buffers: dz, gbi and logit hold GUARD_ROWS rows of a NaN pattern past the
    batch, the workspace sits in a guard band"""

    def __init__(self, fmx, Bl, G, k, kp, H, L, params=None):
        self.fmx, self.lib = fmx, fmx._lib.load()
        self.Bl, self.G, self.N, self.k, self.kp, self.H, self.L = Bl, G, Bl * G, k, kp, H, L
        p, bi, base, corr = problem(Bl, G, k, kp, H, L)
        self.params = (p if params is None else params).cuda().clone()
        self.bi, self.base, self.corr = bi.cuda(), base.cuda(), corr.cuda()
        self.p0 = self.params.clone()
        self.m = fmx._lib.Mlp(self.params.data_ptr(), L, k, H, 0)
        self.ws_bytes = int(self.lib.fmx_mlp_section_workspace_bytes(C.byref(self.m), self.N))
        self.ws = Guarded(self.ws_bytes, torch.int32, name="workspace")
        self.ws.t.fill_(NAN_WORD)
        rows = self.N + GUARD_ROWS
        self.grads = torch.zeros_like(self.params)
        self.dz, self.logit, self.gbi, self.loss = nan_filled(rows), nan_filled(rows), nan_filled(rows, kp), torch.zeros(1, device="cuda")

    def run(self, corr=None, lr_apply=0.0, opt=None, chain=1, bi=None, base=None, want_logit=True):
        prev = self.lib.fmx_set_option(b"mlp_chain", chain)
        try:
            self.fmx._lib.check(self.lib.fmx_mlp_list_section(
                C.byref(self.m), (self.bi if bi is None else bi).data_ptr(), self.kp, (self.base if base is None else base).data_ptr(),
                None if corr is None else corr.data_ptr(), self.Bl, self.G, 1.0 / self.Bl, self.ws.ptr, self.ws_bytes,
                self.logit.data_ptr() if want_logit else None, self.dz.data_ptr(), self.gbi.data_ptr(), self.kp, self.grads.data_ptr(), lr_apply,
                None if opt is None else C.byref(opt), self.loss.data_ptr(), torch.cuda.current_stream().cuda_stream))
        finally:
            self.lib.fmx_set_option(b"mlp_chain", prev)
        torch.cuda.synchronize()

    def outputs(self):
        return dict(logit=self.logit.clone(), dz=self.dz.clone(), gbi=self.gbi.clone(), grads=self.grads.clone(), loss=self.loss.clone())

    def check_guards(self, what):
        self.ws.check()
        for name, t in (("dz", self.dz), ("logit", self.logit), ("gbi", self.gbi)):
            tail = t[self.N:].contiguous().view(torch.int32)
            assert bool((tail == NAN_WORD).all()), f"{what}: rows of {name} past B_lists G were written"


def same_outputs(a, b, what):
    for name in a:
        same_bits(a[name], b[name], f"{what}: {name}")


def check_vs_float64(s, r, corr, what):
    """logits, dz, gbi, the flat gradients per tensor and the loss against list_mlp_f64, and the structure of every list's dz"""
    N, k, G = s.N, s.k, s.G
    want_logit = r["out"] + (corr.double().cpu().numpy() if corr is not None else 0.0)
    close(s.logit[:N].cpu().numpy(), want_logit, what + " logit", floor=4 * r["logit_noise"])
    close(s.loss.item(), r["loss"], what + " loss")
    dz = s.dz[:N].cpu().numpy()
    close(dz, r["dz"], what + " dz", floor=4 * r["dz_noise"])
    gbi = s.gbi[:N].cpu()
    close(gbi[:, :k].numpy(), r["gbi"], what + " gbi", floor=4 * r["gbi_noise"])
    assert bool((gbi[:, k:].contiguous().view(torch.int32) == 0).all()), what + ": padding columns of gbi must be +0"
    grads = s.grads.cpu().numpy()
    close(grads, r["flat"], what + " flat gradients")
    close_per_tensor(grads, r, k, s.H, s.L, N, what + " gradients")
    d = dz.astype(np.float64).reshape(s.Bl, G)
    assert (d[:, 0] < 0).all() and (d[:, 1:] > 0).all(), what + ": dz_0 < 0 < dz_j"
    total, bound = np.abs(d.sum(1)), r["dz_noise"].reshape(s.Bl, G).sum(1)
    print(f"{what}: worst |sum_j dz_j| / sum_j dz_noise_j {float((total / bound).max()):.3f}")
    assert (total <= bound).all(), f"{what}: |sum_j dz_j| / bound {float((total / bound).max()):.3f}"


# ---- 1. the section against float64, with and without corr, SGD applied and not; the chain option does not reach it ----
@pytest.mark.parametrize("corrected", [False, True])
@pytest.mark.parametrize("Bl,G,k,kp,H,L", CASES)
def test_section_vs_float64(fmx, Bl, G, k, kp, H, L, corrected):
    s = Section(fmx, Bl, G, k, kp, H, L)
    corr = s.corr if corrected else None
    what = f"B_lists={Bl} G={G} H={H} corr={corrected}"
    s.run(corr)
    s.check_guards(what)
    check_vs_float64(s, reference(Bl, G, k, kp, H, L, corrected), corr, what)
    assert torch.equal(s.params, s.p0), "lr_apply = 0 must leave the parameters alone"
    first = s.outputs()
    # SGD applied: the same bits out, and the parameters moved by lr times those gradients
    s.grads.zero_()
    s.run(corr, lr_apply=0.25)
    s.check_guards(what + " (sgd)")
    same_outputs(first, s.outputs(), what + " two runs / lr_apply")
    np.testing.assert_array_equal((s.p0 - 0.25 * s.grads).cpu().numpy(), s.params.cpu().numpy())
    if (Bl, G, k, kp, H, L) in CHAIN_ELIGIBLE:      # a network k_mlp_chain takes: the list section does not, under either setting
        s.params.copy_(s.p0)
        s.grads.zero_()
        s.run(corr, chain=0)
        same_outputs(first, s.outputs(), what + " mlp_chain = 0 vs 1")
        s.run(corr, lr_apply=0.25, chain=0)
        np.testing.assert_array_equal((s.p0 - 0.25 * s.grads).cpu().numpy(), s.params.cpu().numpy())


# ---- 2. the bit statements ----
@pytest.mark.parametrize("Bl,G,k,kp,H,L", CASES)
def test_bit_statements(fmx, Bl, G, k, kp, H, L):
    s = Section(fmx, Bl, G, k, kp, H, L)
    what = f"B_lists={Bl} G={G} H={H}"
    s.run(None)
    plain = s.outputs()
    s.run(torch.zeros_like(s.corr))
    same_outputs(plain, s.outputs(), what + " corr = None vs corr of +0")
    s.run(s.corr)
    same_bits(plain["logit"], s.logit, what + ": the stored logit is the uncorrected one")
    assert not torch.equal(plain["dz"][:s.N], s.dz[:s.N]), "corr reaches the softmax"
    # fmx_mlp_forward_batch on the same inputs
    out = torch.empty(s.N, device="cuda")
    ws = torch.empty(s.ws_bytes // 4, device="cuda")
    fmx._lib.check(s.lib.fmx_mlp_forward_batch(C.byref(s.m), s.bi.data_ptr(), s.kp, s.base.data_ptr(), s.N, ws.data_ptr(), out.data_ptr(),
                                               None, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    same_bits(out, plain["logit"][:s.N], what + ": logit_out vs fmx_mlp_forward_batch")
    # logit_out is optional
    s.logit.view(torch.int32).fill_(NAN_WORD)
    s.run(None, want_logit=False)
    same_bits(plain["dz"], s.dz, what + ": dz without logit_out")
    assert bool((s.logit.view(torch.int32) == NAN_WORD).all())
    s.check_guards(what)


# ---- 3. the network under opt's rule: two consecutive steps against the float64 rule ----
def float64_rule_step(rule, h, t, p, m, v, g, k, H, L):
    """One float64 step of torch's own optimizer from (p, m, v, t - 1 steps taken) by the flat gradient g (the construction of
    test_deep_adaptive_gpu.torch_net_step) -> ref dict of flat p, m, v after the step"""
    pt = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in tensors_of(np.asarray(p, np.float64), k, H, L)]
    if rule == "adam":
        opt = torch.optim.Adam(pt, lr=h["lr"], betas=(h["beta1"], h["beta2"]), eps=h["eps"])
        for q, mm, vv in zip(pt, tensors_of(np.asarray(m, np.float64), k, H, L), tensors_of(np.asarray(v, np.float64), k, H, L)):
            opt.state[q] = dict(step=torch.tensor(float(t - 1)), exp_avg=torch.tensor(mm), exp_avg_sq=torch.tensor(vv))
    else:
        opt = torch.optim.Adagrad(pt, lr=h["lr"], eps=h["eps"])
        for q, vv in zip(pt, tensors_of(np.asarray(v, np.float64), k, H, L)):
            opt.state[q]["sum"] = torch.tensor(vv)
            opt.state[q]["step"] = torch.tensor(float(t - 1))
    for q, gg in zip(pt, tensors_of(np.asarray(g, np.float64), k, H, L)):
        q.grad = torch.tensor(gg)
    opt.step()
    flat = lambda ts: np.concatenate([a.detach().numpy().reshape(-1) for a in ts])
    ref = dict(p=flat(pt), m=np.asarray(m, np.float64).copy(), v=np.asarray(v, np.float64).copy())
    if rule == "adam":
        ref["m"], ref["v"] = flat([opt.state[q]["exp_avg"] for q in pt]), flat([opt.state[q]["exp_avg_sq"] for q in pt])
    else:
        ref["v"] = flat([opt.state[q]["sum"] for q in pt])
    return ref


@pytest.mark.parametrize("rule", ["adam", "adagrad"])
@pytest.mark.parametrize("Bl,G,k,kp,H,L", [CASES[1], CASES[5]])
def test_opt_two_steps_vs_float64_rule(fmx, Bl, G, k, kp, H, L, rule):
    L_ = fmx._lib
    h, N, n = NET_HYP[rule], Bl * G, n_params(k, H, L)
    rng = np.random.default_rng(Bl * 7 + H)
    s = Section(fmx, Bl, G, k, kp, H, L)
    bufs = {name: Guarded(4 * n, name=name) for name in ("m", "v")}
    for t in (1, 2):
        bi = draw_clear_of_kinks(rng, s.params.cpu().numpy(), k, H, L, N, kp)
        bi_d = torch.from_numpy(bi).cuda()
        before = {"p": s.params.cpu().numpy().astype(np.float64), "m": bufs["m"].t.cpu().numpy().astype(np.float64),
                  "v": bufs["v"].t.cpu().numpy().astype(np.float64)}
        # lr_apply = 0 on the same inputs: the bits of everything but the parameters
        s.grads.zero_()
        s.run(s.corr, bi=bi_d)
        zero = s.outputs()
        assert torch.equal(s.params, torch.from_numpy(before["p"].astype(np.float32)).cuda())
        opt = L_.MlpOpt(bufs["m"].ptr, bufs["v"].ptr, h["lr"], h["eps"], h["beta1"], h["beta2"], L_.RULES[rule], t - 1)
        s.grads.zero_()
        s.run(s.corr, lr_apply=123.0, opt=opt, bi=bi_d)
        assert opt.step == t - 1, "the step count is the caller's: never written back"
        same_outputs(zero, s.outputs(), f"{rule} step {t} vs lr_apply = 0")
        for g_ in bufs.values():
            g_.check()
        s.check_guards(f"{rule} step {t}")
        r = list_mlp_f64(before["p"], k, H, L, bi[:, :k], s.base.double().cpu().numpy() - s.corr.double().cpu().numpy(), G, 1.0 / Bl)
        assert all(np.any(a) for a in tensors_of(r["flat"], k, H, L)), "a layer without a live unit"
        ref = float64_rule_step(rule, h, t, before["p"], before["m"], before["v"], r["flat"], k, H, L)
        after = {"p": s.params.cpu().numpy().astype(np.float64), "m": bufs["m"].t.cpu().numpy().astype(np.float64),
                 "v": bufs["v"].t.cpu().numpy().astype(np.float64)}
        assert_net_step(f"{rule} B_lists={Bl} G={G} H={H} step {t}", rule, h, t, before, after, ref, r["flat"], k, H, L)


# ---- 4. one workload-shaped case: 16,384 rows through the separate GEMM launches at hidden 256 ----
def test_workload_shape_vs_float64(fmx):
    Bl, G, k, kp, H, L = WORKLOAD
    s = Section(fmx, Bl, G, k, kp, H, L)
    s.run(s.corr)
    s.check_guards("workload shape")
    check_vs_float64(s, reference(Bl, G, k, kp, H, L, True), s.corr, "workload shape")


# ---- 5. the stream is its steps ----
ITEM_FIELDS = [3, 4]
LAYOUT = {"signadam": "weights", "adam": "moments"}


def make_lists(sizes, B, G, seed, item=ITEM_FIELDS):
    """-> rows int32 [B G, F] local indices: a list's negatives are its positive with the item columns redrawn"""
    rng = np.random.default_rng(seed)
    pos = np.stack([rng.integers(0, s, size=B) for s in sizes], axis=1)
    rows = np.repeat(pos[:, None, :], G, axis=1)
    for f in item:
        rows[:, 1:, f] = rng.integers(0, sizes[f], size=(B, G - 1))
    return rows.reshape(B * G, len(sizes)).astype(np.int32)


class Trainer:
    """a table, an engine, a network and its optimizer state: one side of a stream comparison"""

    def __init__(self, fmx, t, params, net_rule, rows):
        self.t, self.e, self.h = t, fmx.FMEngine(t, max_batch=rows), fmx.Hyper(**HYP)
        self.params, self.grads = params.clone(), torch.zeros_like(params)
        self.opt = None if net_rule == "sgd" else fmx.MlpOpt(params.numel(), net_rule, lr=0.02, device="cuda", step=1)

    def words(self):
        out = [("rows", self.t.rows), ("bias", self.t.bias), ("params", self.params), ("grads", self.grads),
               ("dz", self.e._mlp_dz), ("gbi", self.e._mlp_gbi)]
        return out if self.opt is None else out + [("m", self.opt.m), ("v", self.opt.v)]


STREAM_CASES = [(Bl, G, rule, net_rule, fm_term, corrected) for Bl in (7,) for G in (4, 5) for rule, net_rule in (("signadam", "sgd"), ("adam", "adam"))
                for fm_term in (1, 0) for corrected in (False, True)] + [(128, 4, "signadam", "sgd", 1, True)]      # 512 rows: the sorts run ahead


@pytest.mark.parametrize("Bl,G,rule,net_rule,fm_term,corrected", STREAM_CASES)
def test_stream_is_its_steps(fmx, Bl, G, rule, net_rule, fm_term, corrected):
    sizes, k, H, L = SMALL, 10, 40, 2
    n_pool, n_steps, lr_mlp, rows = 2, 3, 0.05, Bl * G
    t1, _ = build_table(fmx, sizes, k, LAYOUT[rule])
    g = torch.Generator().manual_seed(H + Bl + G)
    params = (torch.randn(n_params(k, H, L), generator=g) * (0.5 / np.sqrt(H))).cuda()
    a, b = (Trainer(fmx, t, params, net_rule, rows) for t in (t1, clone_table(fmx, t1)))
    rows0, bias0 = t1.rows.clone(), t1.bias.clone()
    pool = np.stack([make_lists(sizes, Bl, G, seed=300 + j) for j in range(n_pool)])
    pool_d = torch.from_numpy(pool).cuda().contiguous()
    corr_pool = torch.log(torch.rand(n_pool, rows, generator=g) * 0.999 + 1e-3).cuda().contiguous() if corrected else None
    net = (k, H, L)
    losses_a = torch.full((n_steps,), float("nan"), device="cuda")
    a.e.prepare_deepfm_list_stream(a.h, rule, a.params, a.grads, *net, lr_mlp, pool_d, G, corr_pool=corr_pool, loss_out=losses_a,
                                   fm_term=fm_term, mlp_opt=a.opt)(n_steps)
    # the steps by the public calls: forward without a loss, the NFM base, the list section, the sort, the update on scratch's bias
    losses_b = []
    for s_ in range(n_steps):
        idx = pool_d[s_ % n_pool]
        N = b.e.forward(b.h, idx, None)
        base = b.e.logit[:N] if fm_term else (b.e.sfirst[:N] + b.t.bias[0])
        loss, dz, gbi, _ = b.e.mlp_list_section(b.params, b.grads, *net, b.e.bi[:N], base.contiguous(), Bl, G, 1.0 / Bl,
                                                corr=None if corr_pool is None else corr_pool[s_ % n_pool], lr_apply=lr_mlp, mlp_opt=b.opt)
        b.e.list_sort_update(b.h, rule, idx, G, None, dz, dz if fm_term else None, gbi, inv_b=1.0 / Bl)
        losses_b.append(loss.clone())
    torch.cuda.synchronize()
    for x in (a, b):
        x.e.check_error_flag()
    what = f"{rule}/{net_rule} fm_term={fm_term} B_lists={Bl} G={G} corr={corrected}"
    for (name, wa), (_, wb) in zip(a.words(), b.words()):
        same_bits(wa, wb, f"{what}: {name} (stream vs steps)")
    same_bits(losses_a, torch.cat(losses_b), what + ": loss_out")
    assert bool((losses_a > 0).all())
    assert not torch.equal(a.params, params), "the network moved"
    assert a.t.step == b.t.step and (a.opt is None or a.opt.step == b.opt.step == 1 + n_steps)
    # the bias and its state are bit-unchanged under every rule, and so is every row no list touches
    same_bits(a.t.bias, bias0, what + ": the bias words stay")
    touched = np.zeros(t1.rows.shape[0], bool)
    touched[np.unique(pool.reshape(-1, len(sizes)).astype(np.int64) + np.asarray(t1.offsets_host[:-1], np.int64)[None, :])] = True
    assert touched.any() and (Bl > 7 or not touched.all())      # (the 128 lists of the last case reach every row of the small table)
    keep = torch.from_numpy(~touched).cuda()
    same_bits(a.t.rows[keep], rows0[keep], what + ": rows no list touches")
    assert not torch.equal(a.t.rows[~keep], rows0[~keep]), "the touched rows moved"


# ---- 6. the classes ----
def new_model(cls, rule, k=10, H=32, L=2, seed=21, sizes=SMALL):
    from models.models_online_deep.deepfm_adam import DeepFMAdam
    from models.models_online_deep.nfm_adam import NFMAdam
    torch.manual_seed(seed)
    klass = {"DeepFMAdam": DeepFMAdam, "NFMAdam": NFMAdam}[cls]
    return klass(sizes, embedding_size=k, num_hidden_layers=L, neuron_per_hidden_layer=H, n=0.01, update_rule=rule,
                 fused_optimizer=rule in ("adam", "adagrad"))


def class_data(B, n_neg, seed=4):
    """-> (Xi [B, F], Xv [B, F], item fields, negatives [B, n_neg, 2])"""
    rng = np.random.default_rng(seed)
    Xi = np.stack([rng.integers(0, s, size=B) for s in SMALL], axis=1).astype(np.int32)
    Xv = rng.uniform(0.5, 1.5, size=Xi.shape).astype(np.float32)
    neg = np.stack([rng.integers(0, SMALL[f], size=(B, n_neg)) for f in ITEM_FIELDS], axis=2).astype(np.int64)
    return Xi, Xv, ITEM_FIELDS, neg


def model_words(m):
    out = [("rows", m._table.rows), ("bias", m._table.bias), ("mlp", m._mlp_flat)]
    return out if m._mlp_fused is None else out + [("m", m._mlp_fused.m), ("v", m._mlp_fused.v)]


def by_hand(fmx, m, rows, xv, G, corr=None):
    """fit_lists(full=True)'s engine calls"""
    e, lr, rule = m._engine, float(m.n), m.update_rule
    N = e.forward(m._hyper, rows, xv)
    B = N // G
    if getattr(m, "_mlp_gflat", None) is None:
        m._mlp_gflat = torch.zeros_like(m._mlp_flat)
    loss, dz, gbi, logit = e.mlp_list_section(m._mlp_flat, m._mlp_gflat, m.embedding_size, m.neuron_per_hidden_layer, m.num_hidden_layers,
                                              e.bi[:N], m._base_logit(N).contiguous(), B, G, 1.0 / B, corr=corr,
                                              lr_apply=lr if rule == "sgd" else 0.0, mlp_opt=m._mlp_fused)
    if rule == "signadam":
        g = m._mlp_gflat
        m._mlp_flat.sub_(lr * g / (g.abs() + 1e-8))
    e.list_sort_update(m._hyper, rule, rows, G, xv, dz, dz if m._fm_term_in_forward else None, gbi, inv_b=1.0 / B)
    return loss.clone(), logit


@pytest.mark.parametrize("rule", ["sgd", "signadam", "adam"])
@pytest.mark.parametrize("cls,k,H", [("DeepFMAdam", 10, 32), ("NFMAdam", 10, 32), ("DeepFMAdam", 16, 256)])
def test_fit_lists_full_is_the_engine_calls(fmx, cls, k, H, rule):
    B, n_neg = 33, 4
    Xi, Xv, item, neg = class_data(B, n_neg)
    a, b = new_model(cls, rule, k=k, H=H), new_model(cls, rule, k=k, H=H)
    for (name, wa), (_, wb) in zip(model_words(a), model_words(b)):
        same_bits(wa, wb, f"the same seed gives the same model: {name}")
    before = [w.clone() for _, w in model_words(a)]
    rows, xv = fmx.pairwise.assemble_lists(torch.from_numpy(Xi).cuda(), torch.from_numpy(Xv).cuda(), item, torch.from_numpy(neg).cuda())
    for step in range(2):
        la = a.fit_lists(Xi, Xv, item, negatives=neg, full=True)
        lb, _ = by_hand(fmx, b, rows, xv, 1 + n_neg)
        torch.cuda.synchronize()
        for (name, wa), (_, wb) in zip(model_words(a), model_words(b)):
            same_bits(wa, wb, f"{cls} {rule} step {step}: {name}")
        same_bits(la.reshape(1), lb, "loss")
        assert float(la) > 0
    for (name, w), w0 in zip(model_words(a), before):
        assert (name == "bias") == torch.equal(w, w0), f"{name}: everything but the bias moves"
    assert a._table.step == b._table.step and (a._mlp_fused is None or a._mlp_fused.step == b._mlp_fused.step == 2)


@pytest.mark.parametrize("correct", [True, False])
def test_fit_lists_full_takes_popularity_negatives(fmx, correct):
    from fmx.pairwise import PopularityNegatives
    B, n_neg = 9, 3
    Xi, Xv, _, _ = class_data(B, n_neg)
    item = [4]
    m = new_model("DeepFMAdam", "signadam")
    pop = PopularityNegatives(np.arange(1, SMALL[4] + 1, dtype=np.float64), correct=correct)
    bias0 = m._table.bias.clone()
    for call in range(2):
        offset = int(getattr(m, "_mining_offset", 0))
        loss = m.fit_lists(Xi, Xv, item, negatives=pop, n_neg=n_neg, full=True)
        assert np.isfinite(float(loss)) and float(loss) > 0
        assert m._mining_offset == offset + 1, "one draw per call"
    same_bits(m._table.bias, bias0, "the bias does not move")
    # the correction reaches the loss: the same draws, with and without it, give another loss
    twin = new_model("DeepFMAdam", "signadam")
    other = PopularityNegatives(np.arange(1, SMALL[4] + 1, dtype=np.float64), correct=not correct)
    assert float(twin.fit_lists(Xi, Xv, item, negatives=other, n_neg=n_neg, full=True)) != \
        float(new_model("DeepFMAdam", "signadam").fit_lists(Xi, Xv, item, negatives=pop, n_neg=n_neg, full=True))


@pytest.mark.parametrize("cls,rule", [("DeepFMAdam", "signadam"), ("NFMAdam", "adam")])
def test_run_list_experiment_full_is_its_loop(fmx, cls, rule):
    N, n_neg = 12, 4
    Xi, Xv, item, neg = class_data(N, n_neg, seed=8)
    a, b = new_model(cls, rule), new_model(cls, rule)
    secs, acc, checkpoints, counts = a.run_list_experiment(Xi, Xv, item, negatives=neg, full=True)
    correct = 0
    for i in range(N):
        b.fit_lists(Xi[i:i + 1], Xv[i:i + 1], item, negatives=neg[i:i + 1], full=True)
        z = b._engine._mlp_logit[:1 + n_neg].cpu()                # the step's own logits: the whole network's, before its update
        correct += int(not bool((z[1:] >= z[0]).any()))
    torch.cuda.synchronize()
    for (name, wa), (_, wb) in zip(model_words(a), model_words(b)):
        same_bits(wa, wb, f"{cls} {rule}: {name}")
    assert counts == {"correct": correct, "wrong": N - correct} and counts["correct"] + counts["wrong"] == 12
    assert a._table.step == b._table.step
    assert acc == checkpoints[-1] == pytest.approx(100.0 * correct / N) and len(checkpoints) == 2 and secs > 0
