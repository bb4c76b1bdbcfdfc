"""Pairwise-ranking (BPR) training of DeepFM / NFM on the device: fmx_mlp_pair_section (k_mlp_chain<true> at hidden = 256,
k_mlp_pair_loss elsewhere), fmx_deepfm_pair_stream and the classes' fit_pairs / run_pair_experiment(full=True).

Shapes (rows = 2 B_pairs).  Chain kernel: B_pairs 1 (one pair), 8 (one full slab of 16 rows), 9 (one pair past it), 17 (three
slabs, the last with one pair), at k 16 with three layers and k 64 with one; one of them again as separate launches.  GEMM
path: hidden 1, a ragged 40, an odd 33 at 74 rows (the last workgroup of k_mlp_pair_loss holds one pair of its four) and five
layers of 64."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle.fm_oracle import EPS32, K_FP32
from pair_f64 import pair_loss_f64
from pair_mlp_f64 import pair_mlp_f64
from test_kernels_gpu import HYP
from test_mlp_gpu import close, close_per_tensor, live_units
from test_pair_gpu import SHAPES, SMALL, build_table, clone_table, make_pairs, same_bits

pytestmark = pytest.mark.gpu

CHAIN = [(P, k, k, 256, L) for P in (1, 8, 9, 17) for k, L in ((16, 3), (64, 1))]
GEMM = [(1, 4, 4, 1, 2), (19, 10, 12, 40, 2), (37, 4, 4, 33, 1), (150, 16, 16, 64, 5)]
NO_CHAIN = (9, 16, 16, 256, 3)
CASES = [c + (1,) for c in CHAIN + GEMM] + [NO_CHAIN + (0,)]      # B_pairs, k, kp, hidden, layers, mlp_chain
MARGINS = [0.0, 0.1]


@pytest.fixture(scope="module")
def fmx():
    import fmx as _fmx
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _fmx


def n_params(k, H, L):
    return sum(H * (k if l == 0 else H) + H for l in range(L))


@functools.lru_cache(maxsize=None)
def problem(P, k, kp, H, L):
    """-> (params, bi [2P, kp], base [2P]) as CPU tensors: no layer dead (live_units)"""
    g = torch.Generator().manual_seed(1000 * P + H + L + k)
    params = torch.randn(n_params(k, H, L), generator=g) * (1.0 / np.sqrt(H))
    bi = torch.zeros(2 * P, kp)
    bi[:, :k] = torch.randn(2 * P, k, generator=g) * 0.5
    params = torch.from_numpy(live_units(params.numpy(), k, H, L, bi[:, :k].numpy()))
    base = torch.randn(2 * P, generator=g) * 0.3
    return params, bi, base


@functools.lru_cache(maxsize=None)
def reference(P, k, kp, H, L, margin):
    """the float64 reference of a case: computed once, shared by the tests, never written to"""
    params, bi, base = problem(P, k, kp, H, L)
    r = pair_mlp_f64(params.numpy(), k, H, L, bi[:, :k].numpy(), base.numpy(), margin, 1.0 / P)
    for l in range(L):
        # every layer is exercised.  (A bias gradient sums +g and -g over the two rows of a pair: at hidden = 1 with one pair,
        # both rows on the one unit, it is exactly 0 in float64 too -- no sign of a dead layer, so W's gradient decides there.)
        assert np.any(r["grads"][l][0]) and (np.any(r["grads"][l][1]) or H == 1), f"layer {l} has no live unit (a dead network)"
    return r


class Section:
    """fmx_mlp_pair_section on one case's device buffers"""

    def __init__(self, fmx, P, k, kp, H, L, chain=1):
        self.fmx, self.lib = fmx, fmx._lib.load()
        self.P, self.k, self.kp, self.H, self.L, self.chain = P, k, kp, H, L, chain
        params, bi, base = problem(P, k, kp, H, L)
        self.params, self.bi, self.base = params.cuda(), bi.cuda(), base.cuda()
        self.p0 = self.params.clone()
        self.m = fmx._lib.Mlp(self.params.data_ptr(), L, k, H, 0)
        self.ws = torch.empty(int(self.lib.fmx_mlp_section_workspace_bytes(C.byref(self.m), 2 * P)) // 4, device="cuda")
        f = dict(device="cuda")
        self.grads, self.dz, self.logit = torch.zeros_like(self.params), torch.empty(2 * P, **f), torch.empty(2 * P, **f)
        self.gbi, self.loss = torch.full((2 * P, kp), 7.0, **f), torch.zeros(1, **f)

    def run(self, margin, lr_apply=0.0, opt=None, base=None):
        base = self.base if base is None else base
        prev = self.lib.fmx_set_option(b"mlp_chain", self.chain)
        try:
            self.fmx._lib.check(self.lib.fmx_mlp_pair_section(
                C.byref(self.m), self.bi.data_ptr(), self.kp, base.data_ptr(), self.P, margin, 1.0 / self.P, self.ws.data_ptr(),
                self.ws.numel() * 4, self.logit.data_ptr(), self.dz.data_ptr(), self.gbi.data_ptr(), self.kp, self.grads.data_ptr(),
                lr_apply, None if opt is None else opt.ref(), self.loss.data_ptr(), torch.cuda.current_stream().cuda_stream))
        finally:
            self.lib.fmx_set_option(b"mlp_chain", prev)
        torch.cuda.synchronize()

    def pointwise_logit(self, base=None):
        """fmx_mlp_section's logit_out on the same bi / base, under arbitrary labels"""
        base = self.base if base is None else base
        y = (torch.arange(2 * self.P, device="cuda") % 3 == 0).float()
        logit, dz, gbi = torch.empty_like(self.logit), torch.empty_like(self.dz), torch.empty_like(self.gbi)
        prev = self.lib.fmx_set_option(b"mlp_chain", self.chain)
        try:
            self.fmx._lib.check(self.lib.fmx_mlp_section(
                C.byref(self.m), self.fmx._lib.LOSSES["logits"], self.bi.data_ptr(), self.kp, base.data_ptr(), y.data_ptr(), 2 * self.P,
                1.0 / self.P, self.ws.data_ptr(), logit.data_ptr(), dz.data_ptr(), gbi.data_ptr(), self.kp, torch.zeros_like(self.grads).data_ptr(),
                0.0, None, torch.cuda.current_stream().cuda_stream))
        finally:
            self.lib.fmx_set_option(b"mlp_chain", prev)
        torch.cuda.synchronize()
        return logit


def check_section_epilogue(s, margin, what):
    """test_pair_gpu.check_epilogue's bounds on the section's outputs, from the device's own logits: 1e-5 relative plus
    4 EPS32 floors; dz[2i + 1] is dz[2i] negated; loss_out against the float64 sum (the ordered sum of 2P terms may be off by
    at most 2P EPS32 times the sum of their magnitudes)."""
    P, inv_b = s.P, 1.0 / s.P
    z = s.logit.double().cpu().numpy()
    dz = s.dz.cpu()
    assert np.isfinite(z).all() and np.isfinite(dz.numpy()).all() and np.isfinite(s.gbi.cpu().numpy()).all(), what
    assert np.isfinite(s.grads.cpu().numpy()).all() and np.isfinite(s.loss.item()), what
    ref_loss, g = pair_loss_f64(z[0::2] - z[1::2], margin)
    ref_dz = g * inv_b
    err, tol = np.abs(dz[0::2].double().numpy() - ref_dz), 1e-5 * np.abs(ref_dz) + 4 * EPS32 * inv_b
    print(f"{what} dz: worst err/tol {float((err / tol).max()):.3f}")
    assert (err <= tol).all(), f"{what} dz: worst err/tol {float((err / tol).max()):.3f}"
    same_bits(dz[1::2], -dz[0::2], what + " dz[2i+1] == -dz[2i]")
    want = ref_loss.sum() * inv_b
    tol = inv_b * ((1e-5 * np.abs(ref_loss) + 4 * EPS32 * (1 + np.abs(ref_loss))).sum() + 2 * P * EPS32 * np.abs(ref_loss).sum())
    err = abs(s.loss.item() - want)
    print(f"{what} loss_out: err/tol {err / tol:.3f}")
    assert err <= tol, f"{what} loss_out {s.loss.item()} vs {want}: err/tol {err / tol:.3f}"
    return z


# ---- 1. + 2. the forward is fmx_mlp_section's; the epilogue from the device's own logits ----
@pytest.mark.parametrize("margin", MARGINS)
@pytest.mark.parametrize("P,k,kp,H,L,chain", CASES)
def test_forward_identity_and_epilogue(fmx, P, k, kp, H, L, chain, margin):
    s = Section(fmx, P, k, kp, H, L, chain)
    s.run(margin)
    same_bits(s.logit, s.pointwise_logit(), "logit_out")
    z = check_section_epilogue(s, margin, f"P={P} H={H}")
    # logit differences from -30 to 30: the positives' base moved so that d_i becomes the target
    target = np.linspace(-30.0, 30.0, P) if P > 1 else np.array([30.0])
    wide = s.base.clone()
    wide[0::2] += torch.from_numpy(target - (z[0::2] - z[1::2])).float().cuda()
    s.run(margin, base=wide)
    same_bits(s.logit, s.pointwise_logit(wide), "logit_out (wide)")
    z = check_section_epilogue(s, margin, f"P={P} H={H} wide")
    d = z[0::2] - z[1::2]
    assert P == 1 or (d.min() < -25 and d.max() > 25)
    assert torch.equal(s.params, s.p0), "lr_apply = 0 must leave the parameters alone"


# ---- 3. the backward against float64 autograd ----
@pytest.mark.parametrize("margin", MARGINS)
@pytest.mark.parametrize("P,k,kp,H,L,chain", CASES)
def test_backward_vs_autograd(fmx, P, k, kp, H, L, chain, margin):
    s = Section(fmx, P, k, kp, H, L, chain)
    s.run(margin)
    r = reference(P, k, kp, H, L, margin)
    close(s.logit.cpu().numpy(), r["out"], "logit")
    close(s.loss.item(), r["loss"], "loss")
    close(s.dz.cpu().numpy(), r["dz"], "dz")
    gbi = s.gbi.cpu().numpy()
    close(gbi[:, :k], r["gbi"], "gbi")
    assert (gbi[:, k:] == 0).all(), "padding columns of gbi must be zeroed"
    grads = s.grads.cpu().numpy()
    close(grads, r["flat"], "flat gradients")
    close_per_tensor(grads, r, k, H, L, 2 * P, "gradients")


# ---- 4. the rule application ----
@pytest.mark.parametrize("P,k,kp,H,L,chain", [CASES[2], CASES[9], CASES[-1]])
def test_rule_application(fmx, P, k, kp, H, L, chain):
    margin = 0.1
    s = Section(fmx, P, k, kp, H, L, chain)
    s.run(margin)
    first = [t.clone() for t in (s.grads, s.dz, s.gbi, s.logit, s.loss)]
    s.grads.zero_()
    s.run(margin, lr_apply=0.25)
    for name, a, b in zip(("grads", "dz", "gbi", "logit", "loss"), first, (s.grads, s.dz, s.gbi, s.logit, s.loss)):
        same_bits(a, b, f"two runs: {name}")
    np.testing.assert_array_equal((s.p0 - 0.25 * s.grads).cpu().numpy(), s.params.cpu().numpy())
    sgd_by_lr = s.params.clone()
    # opt (SGD) is lr_apply = opt->lr; opt (ADAM) leaves grads / dz / gbi as they are and moves the parameters and moments
    s.params.copy_(s.p0)
    opt = fmx.MlpOpt(s.params.numel(), "sgd", lr=0.25, device="cuda")
    s.run(margin, lr_apply=123.0, opt=opt)
    same_bits(s.params, sgd_by_lr, "opt (SGD) vs lr_apply")
    s.params.copy_(s.p0)
    opt = fmx.MlpOpt(s.params.numel(), "adam", lr=0.01, device="cuda", step=2)
    s.run(margin, opt=opt)
    for name, a, b in zip(("grads", "dz", "gbi", "logit", "loss"), first, (s.grads, s.dz, s.gbi, s.logit, s.loss)):
        same_bits(a, b, f"opt (ADAM): {name}")
    assert not torch.equal(s.params, s.p0) and bool(opt.m.abs().sum() > 0) and bool(opt.v.abs().sum() > 0)


# ---- 5. the stream is its steps ----
NETS = [(256, 1), (40, 2)]
STREAM_RULES = [("signadam", "sgd", 1), ("signadam", "sgd", 0), ("ftrl", "sgd", 1), ("adam", "adam", 1), ("adam", "adam", 0),
                ("adagrad", "adagrad", 1), ("sgd", "sgd", 0)]
LAYOUT = {"signadam": "weights", "sgd": "weights", "ftrl": "ftrl", "adagrad": "moments", "adam": "moments"}


class Trainer:
    """a table, an engine, a network and its optimizer state: one side of a stream comparison"""

    def __init__(self, fmx, t, params, net_rule, P):
        self.t, self.e, self.h = t, fmx.FMEngine(t, max_batch=2 * P), fmx.Hyper(**HYP)
        self.params, self.grads = params.clone(), torch.zeros_like(params)
        self.opt = None if net_rule == "sgd" else fmx.MlpOpt(params.numel(), net_rule, lr=0.02, device="cuda", step=1)

    def words(self):
        out = [("rows", self.t.rows), ("bias", self.t.bias), ("params", self.params), ("grads", self.grads)]
        return out if self.opt is None else out + [("m", self.opt.m), ("v", self.opt.v)]


@pytest.mark.parametrize("P", [33, 256])                        # 2P = 512: the sorts run ahead on the side stream
@pytest.mark.parametrize("H,L", NETS)
@pytest.mark.parametrize("rule,net_rule,fm_term", STREAM_RULES)
def test_stream_is_its_steps(fmx, rule, net_rule, fm_term, H, L, P):
    sizes, k = SHAPES["c"]
    n_pool, n_steps, margin, lr_mlp = 3, 5, 0.1 if P == 33 else 0.0, 0.05
    t1, _ = build_table(fmx, sizes, k, LAYOUT[rule])
    g = torch.Generator().manual_seed(H + P)
    params = (torch.randn(n_params(k, H, L), generator=g) * (0.5 / np.sqrt(H))).cuda()
    a, b, c = (Trainer(fmx, t, params, net_rule, P) for t in (t1, clone_table(fmx, t1), clone_table(fmx, t1)))
    bias0 = t1.bias.clone()
    pool = np.stack([make_pairs(sizes, P, seed=200 + j, n_item=1 + j % 2)[0] for j in range(n_pool)])
    pool_d = torch.from_numpy(pool).cuda().contiguous()
    net = (k, H, L)
    losses_a = torch.full((n_steps,), float("nan"), device="cuda")
    a.e.prepare_deepfm_pair_stream(a.h, rule, a.params, a.grads, *net, lr_mlp, pool_d, margin=margin, loss_out=losses_a,
                                   fm_term=fm_term, mlp_opt=a.opt)(n_steps)
    # the five steps by hand: forward without a loss, the NFM base, the pair section, the sort, the update
    losses_b = []
    for s_ in range(n_steps):
        idx = pool_d[s_ % n_pool]
        B2 = b.e.forward(b.h, idx, None)
        base = b.e.logit[:B2] if fm_term else (b.e.sfirst[:B2] + b.t.bias[0])
        loss, dz, gbi, _ = b.e.mlp_pair_section(b.params, b.grads, *net, b.e.bi[:B2], base.contiguous(), P, 1.0 / P, margin=margin,
                                                lr_apply=lr_mlp, mlp_opt=b.opt)
        b.e.sort(idx)
        b.e.update(b.h, rule, B2, None, dz, dz if fm_term else None, gbi, inv_b=1.0 / P, with_loss=False)
        losses_b.append(loss.clone())
    # ... and as two runs of 2 + 3 steps
    losses_c = torch.full((n_steps,), float("nan"), device="cuda")
    run = c.e.prepare_deepfm_pair_stream(c.h, rule, c.params, c.grads, *net, lr_mlp, pool_d, margin=margin, loss_out=losses_c[:2],
                                         fm_term=fm_term, mlp_opt=c.opt)
    run(2)
    # the second run starts at step 2 of the pool: the pool rotated by two batches
    rot = torch.cat([pool_d[2:], pool_d[:2]]).contiguous()
    c.e.prepare_deepfm_pair_stream(c.h, rule, c.params, c.grads, *net, lr_mlp, rot, margin=margin, loss_out=losses_c[2:],
                                   fm_term=fm_term, mlp_opt=c.opt)(3)
    torch.cuda.synchronize()
    for x in (a, b, c):
        x.e.check_error_flag()
    what = f"{rule}/{net_rule} fm_term={fm_term} {H}x{L} P={P}"
    for (name, wa), (_, wb), (_, wc) in zip(a.words(), b.words(), c.words()):
        same_bits(wa, wb, f"{what}: {name} (stream vs steps)")
        same_bits(wa, wc, f"{what}: {name} (5 vs 2 + 3)")
    same_bits(losses_a, torch.cat(losses_b), what + ": loss_out")
    same_bits(losses_a, losses_c, what + ": loss_out (2 + 3)")
    assert bool((losses_a > 0).all())
    assert not torch.equal(a.params, params), "the network moved"
    assert a.t.step == b.t.step == c.t.step == (3 + n_steps if LAYOUT[rule] == "moments" else a.t.step)
    assert a.opt is None or a.opt.step == b.opt.step == c.opt.step == 1 + n_steps
    if rule != "adam":
        same_bits(a.t.bias, bias0, what + ": the bias gradient is exactly 0, the bias words stay")


# ---- 6. the classes ----
def new_model(cls, rule, k=10, H=32, L=2, seed=21, sizes=SMALL):
    from models.models_online_deep.deepfm_adam import DeepFMAdam
    from models.models_online_deep.nfm_adam import NFMAdam
    torch.manual_seed(seed)
    klass = {"DeepFMAdam": DeepFMAdam, "NFMAdam": NFMAdam}[cls]
    return klass(sizes, embedding_size=k, num_hidden_layers=L, neuron_per_hidden_layer=H, n=0.01, update_rule=rule,
                 fused_optimizer=rule in ("adam", "adagrad"))


def class_data(B, seed=4):
    rows, x, item = make_pairs(SMALL, B, seed=seed, n_item=2, real_x=True)
    return rows[0::2].copy(), x[0::2].copy(), item, rows[1::2][:, item].copy()


def model_words(m):
    out = [("rows", m._table.rows), ("bias", m._table.bias), ("mlp", m._mlp_flat)]
    return out if m._mlp_fused is None else out + [("m", m._mlp_fused.m), ("v", m._mlp_fused.v)]


def by_hand(fmx, m, rows, xv, margin):
    """fit_pairs(full=True)'s engine calls"""
    e, P, lr, rule = m._engine, rows.shape[0] // 2, float(m.n), m.update_rule
    B2 = e.forward(m._hyper, rows, xv)
    if getattr(m, "_mlp_gflat", None) is None:
        m._mlp_gflat = torch.zeros_like(m._mlp_flat)
    loss, dz, gbi, logit = e.mlp_pair_section(m._mlp_flat, m._mlp_gflat, m.embedding_size, m.neuron_per_hidden_layer, m.num_hidden_layers,
                                              e.bi[:B2], m._base_logit(B2).contiguous(), P, 1.0 / P, margin=margin,
                                              lr_apply=lr if rule == "sgd" else 0.0, mlp_opt=m._mlp_fused)
    if rule == "signadam":
        g = m._mlp_gflat
        m._mlp_flat.sub_(lr * g / (g.abs() + 1e-8))
    e.sort(rows)
    e.update(m._hyper, rule, B2, xv, dz, dz if m._fm_term_in_forward else None, gbi, inv_b=1.0 / P, with_loss=False)
    return loss.clone(), logit


@pytest.mark.parametrize("rule", ["sgd", "signadam", "adam"])
@pytest.mark.parametrize("cls,k,H", [("DeepFMAdam", 10, 32), ("NFMAdam", 10, 32), ("DeepFMAdam", 16, 256)])
def test_fit_pairs_full_is_the_engine_calls(fmx, cls, k, H, rule):
    Xi, Xv, item, neg = class_data(33)
    a, b = new_model(cls, rule, k=k, H=H), new_model(cls, rule, k=k, H=H)
    for (name, wa), (_, wb) in zip(model_words(a), model_words(b)):
        same_bits(wa, wb, f"the same seed gives the same model: {name}")
    before = [w.clone() for _, w in model_words(a)]
    rows, xv = fmx.pairwise.assemble_pairs(torch.from_numpy(Xi).cuda(), torch.from_numpy(Xv).cuda(), item, torch.from_numpy(neg).cuda())
    for step in range(2):
        la = a.fit_pairs(Xi, Xv, item, negatives=neg, margin=0.1, full=True)
        lb, _ = by_hand(fmx, b, rows, xv, 0.1)
        torch.cuda.synchronize()
        for (name, wa), (_, wb) in zip(model_words(a), model_words(b)):
            same_bits(wa, wb, f"{cls} {rule} step {step}: {name}")
        same_bits(la.reshape(1), lb, "loss")
        assert float(la) > 0
    for (name, w), w0 in zip(model_words(a), before):
        assert not torch.equal(w, w0) or name == "bias", f"{name} did not move"
    assert a._table.step == b._table.step and (a._mlp_fused is None or a._mlp_fused.step == b._mlp_fused.step == 2)


@pytest.mark.parametrize("cls,rule", [("DeepFMAdam", "signadam"), ("NFMAdam", "adam")])
def test_run_pair_experiment_full_is_its_loop(fmx, cls, rule):
    N = 12
    Xi, Xv, item, neg = class_data(N, seed=8)
    a, b = new_model(cls, rule), new_model(cls, rule)
    secs, acc, checkpoints, counts = a.run_pair_experiment(Xi, Xv, item, negatives=neg, margin=0.0, full=True)
    correct = 0
    for i in range(N):
        b.fit_pairs(Xi[i:i + 1], Xv[i:i + 1], item, negatives=neg[i:i + 1], full=True)
        z = b._engine._mlp_logit[:2].cpu()                       # the step's own logits: the whole network's, before its update
        correct += int(z[0] > z[1])
    torch.cuda.synchronize()
    for (name, wa), (_, wb) in zip(model_words(a), model_words(b)):
        same_bits(wa, wb, f"{cls} {rule}: {name}")
    assert counts == {"correct": correct, "wrong": N - correct} and a._table.step == b._table.step
    assert acc == checkpoints[-1] == pytest.approx(100.0 * correct / N) and len(checkpoints) == 2 and secs > 0


@pytest.mark.parametrize("margin", MARGINS)
def test_whole_model_sgd_step_within_float64(fmx, margin):
    """One fit_pairs(full=True) step of DeepFMAdam under sgd against float64 autograd of tables plus network.  Every touched
    row's step is held to 1e-5 of the tensor's largest step plus a floor built term by term: tests/pair_f64.py's floors with the
    per-column G = dz + gbi in place of dz.  The noise of a logit is the FM logit's floor (pair_f64's f_logit), the network's own
    rounding (the helper's logit_noise, four standard deviations) and the floor of bi carried through |d net / d bi|; dz's
    floor is its slope times the noise of d plus 4 EPS32 inv_b; gbi's floor is four times the helper's gbi_noise, plus dz's
    FM-side floor times |d net / d bi|."""
    from pair_mlp_f64 import pair_loss_t
    P, k, H, L, lr = 33, 10, 32, 2, 0.01
    Xi, Xv, item, neg = class_data(P)
    m = new_model("DeepFMAdam", "sgd", k=k, H=H, L=L)
    t = m._table
    kp, offs = t.kp, np.asarray(t.offsets_host[:-1], np.int64)
    V0, w0 = t.rows[:, :k].cpu().numpy().copy(), t.rows[:, kp].cpu().numpy().copy()
    bias0, p0 = float(t.bias[0].item()), m._mlp_flat.cpu().numpy().copy()
    rows_t, xv_t = fmx.pairwise.assemble_pairs(torch.from_numpy(Xi), torch.from_numpy(Xv), item, torch.from_numpy(neg))
    rows, x = rows_t.numpy().astype(np.int64) + offs[None, :], xv_t.numpy().astype(np.float64)
    loss_dev = float(m.fit_pairs(Xi, Xv, item, negatives=neg, margin=margin, full=True))
    torch.cuda.synchronize()
    # ---- float64 autograd of the whole model ----
    d = torch.float64
    V, w = torch.tensor(V0, dtype=d, requires_grad=True), torch.tensor(w0, dtype=d, requires_grad=True)
    bias, p = torch.tensor(bias0, dtype=d, requires_grad=True), torch.tensor(p0, dtype=d, requires_grad=True)
    rt, xt = torch.from_numpy(rows), torch.from_numpy(x)
    e = V[rt] * xt[:, :, None]
    S, SS = e.sum(1), (e * e).sum(1)
    bi = 0.5 * (S * S - SS)
    first = w[rt] * xt
    z_fm = first.sum(1) + bi.sum(1) + bias
    h, off = bi, 0
    for l in range(L):
        i = k if l == 0 else H
        h = torch.relu(h @ p[off:off + H * i].view(H, i).t() + p[off + H * i:off + H * i + H])
        off += H * i + H
    net = h.sum(1)
    J = torch.autograd.grad(net.sum(), bi, retain_graph=True)[0].detach().numpy()        # d net_b / d bi_b
    z = z_fm + net
    inv_b = 1.0 / P
    loss = pair_loss_t(z[0::2] - z[1::2], margin).sum() * inv_b
    loss.backward()
    # ---- floors ----
    r = pair_mlp_f64(p0, k, H, L, bi.detach().numpy(), z_fm.detach().numpy(), margin, inv_b)
    en, Sn, SSn, bin_, fn = e.detach().numpy(), S.detach().numpy(), SS.detach().numpy(), bi.detach().numpy(), first.detach().numpy()
    fS = K_FP32 * np.abs(en).sum(1)
    f_bi = np.abs(Sn) * fS + K_FP32 * 0.5 * (Sn * Sn + SSn)
    f_logit = f_bi.sum(1) + K_FP32 * (np.abs(fn).sum(1) + abs(bias0)) + K_FP32 * np.abs(bin_).sum(1)
    f_z = f_logit + 4 * r["logit_noise"] + (np.abs(J) * f_bi).sum(1)
    f_d = np.repeat(f_z[0::2] + f_z[1::2], 2)
    dz = r["dz"]
    f_dz = r["hess"] * f_d + 4 * EPS32 * inv_b
    G = dz[:, None] + r["gbi"]
    f_G = f_dz[:, None] * (1 + np.abs(J)) + 4 * r["gbi_noise"] + 2 * EPS32 * np.abs(G)
    F = rows.shape[1]
    urows, inv = np.unique(rows.reshape(-1), return_inverse=True)
    inv = inv.reshape(-1)
    xe, ee = x.reshape(-1, 1), en.reshape(-1, k)
    Sb, fSb = np.repeat(Sn, F, axis=0), np.repeat(fS, F, axis=0)
    Gb, fGb = np.repeat(G, F, axis=0), np.repeat(f_G, F, axis=0)
    dzb, fdzb = np.repeat(dz, F)[:, None], np.repeat(f_dz, F)[:, None]
    fV = np.zeros((len(urows), k))
    np.add.at(fV, inv, np.abs(xe) * ((np.abs(Sb) + np.abs(ee)) * (K_FP32 * np.abs(Gb) + fGb) + np.abs(Gb) * fSb))
    fw = np.zeros(len(urows))
    np.add.at(fw, inv, (np.abs(xe) * (K_FP32 * np.abs(dzb) + fdzb))[:, 0])
    # ---- the touched rows ----
    V1, w1 = t.rows[:, :k].cpu().numpy(), t.rows[:, kp].cpu().numpy()
    for name, got, old, grad, floor in (("V", V1, V0, V.grad.numpy(), fV), ("w", w1, w0, w.grad.numpy(), fw)):
        step, want = got[urows].astype(np.float64) - old[urows], -lr * grad[urows]
        tol = 1e-5 * lr * np.abs(grad).max() + lr * floor + 2 * EPS32 * np.abs(got[urows])
        err = np.abs(step - want)
        print(f"margin {margin} {name}: worst err/tol {float((err / tol).max()):.3f}")
        assert (err <= tol).all(), f"{name}: worst err/tol {float((err / tol).max()):.3f}"
        assert np.abs(want).max() > 0
        mask = np.ones(len(got), bool)
        mask[urows] = False
        np.testing.assert_array_equal(got[mask], old[mask], err_msg=name + " untouched rows")
    assert float(t.bias[0].item()) == bias0, "the bias gradient is exactly 0"
    close(loss_dev, float(loss.detach()), "loss")
    # the network's sgd step is lr times the float64 gradient, within the section's bounds
    g_dev = (p0.astype(np.float64) - m._mlp_flat.cpu().numpy()) / lr
    flat_noise = np.concatenate([t_.reshape(-1) for pair in r["gnoise"] for t_ in pair])
    close(g_dev, p.grad.numpy(), "network step", floor=4 * flat_noise + 2 * EPS32 * np.abs(p0) / lr)
