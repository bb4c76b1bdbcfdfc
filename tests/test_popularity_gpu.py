"""Popularity-sampled negatives and the log-Q corrected list loss on the device: fmx_alias_sample_negatives against the numpy
sampler of tests/alias_ref.py (integers: bit for bit), fmx_fm_list_forward_q / _step_q / _stream_q against the uncorrected calls
at corr = 0 (bit for bit) and against tests/listq_f64.py at random corr, and the classes under PopularityNegatives.

Shapes.  The sampler: U in {1, 3, 65} (one wave, a part of a workgroup of four, seventeen workgroups), N in {2, 7, 1000}, n_neg in
{1, 4, 16}; n_try = 130 with most positions excluded puts a row's fill across 64-draw rounds.  The corrected calls: test_list_gpu's
four small fields, so rows repeat; G in {2, 3, 5, 8, 16} gives 4, 3, 5, 8, 16 waves per workgroup; B_lists in {1, 3, 5}.  The
tolerance against listq_f64 is test_list_gpu's: 1e-5 |ref| + the fp32 floor."""
import ctypes as C
import pickle

import numpy as np
import pytest
import torch

import alias_ref
from abi_geometry import PATTERN, Guarded
from helpers import assert_ftrl_step_within_f64
from listq_f64 import listq_step_f64
from test_kernels_gpu import HYP
from test_list_gpu import ITEM, SIZES, make_lists, new_model, within
from test_pair_gpu import RULES, build_table, clone_table, dev, same_bits

pytestmark = pytest.mark.gpu

GS = [2, 3, 5, 8, 16]


@pytest.fixture(scope="module")
def fmx():
    import fmx as _fmx
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _fmx


# =====================================================================================================================
# the sampler
# =====================================================================================================================
def zipf_table(fmx, N, zeros=()):
    w = 1.0 / np.arange(1, N + 1, dtype=np.float64) ** 1.1
    w[list(zeros)] = 0.0
    thresh, alias, q, logq = fmx.pairwise.alias_table(w)
    return thresh, alias, q, logq


def on_device(thresh, alias, logq):
    return (torch.from_numpy(thresh.view(np.int32).copy()).cuda(), torch.from_numpy(np.asarray(alias, np.int32).copy()).cuda(),
            torch.from_numpy(logq.copy()).cuda())


def csr(excl):
    off = np.zeros(len(excl) + 1, np.int32)
    off[1:] = np.cumsum([len(e) for e in excl])
    pos = np.concatenate([np.asarray(e, np.int64) for e in excl] + [np.zeros(1, np.int64)]).astype(np.int32)
    return torch.from_numpy(off).cuda(), torch.from_numpy(pos).cuda()


def run_sampler(fmx, table, U, n_neg, n_try, seed, offset, u_base, own=None, excl=None, with_logq=True):
    """The raw call into guarded outputs -> (neg_pos int32 [U, n_neg], neg_logq fp32 [U, n_neg] or None) as numpy"""
    L = fmx._lib
    th, al, lq = on_device(*table)
    own_d = None if own is None else torch.from_numpy(np.asarray(own, np.int32)).cuda()
    off, pos = (None, None) if excl is None else csr(excl)
    g_pos = Guarded(U * n_neg * 4, torch.int32, name="neg_pos")
    g_lq = Guarded(U * n_neg * 4, name="neg_logq")
    g_pos.t.fill_(PATTERN)
    g_lq.t.view(torch.int32).fill_(PATTERN)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    L.check(L.load().fmx_alias_sample_negatives(th.data_ptr(), al.data_ptr(), lq.data_ptr() if with_logq else None, len(table[0]),
                                                ptr(off), ptr(pos), ptr(own_d), U, n_neg, n_try, seed, offset, u_base, g_pos.ptr,
                                                g_lq.ptr if with_logq else None, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    g_pos.check()
    g_lq.check()
    got_pos = g_pos.t.cpu().numpy().reshape(U, n_neg)
    assert (got_pos != PATTERN).all()                                        # every slot was written: a position or -1
    if not with_logq:
        assert (g_lq.t.view(torch.int32) == PATTERN).all()
        return got_pos, None
    return got_pos, g_lq.t.cpu().numpy().reshape(U, n_neg)


def same_sample(got, want, what):
    np.testing.assert_array_equal(got[0], want[0], err_msg=what + " neg_pos")
    if got[1] is not None:
        np.testing.assert_array_equal(got[1].view(np.int32), want[1].view(np.int32), err_msg=what + " neg_logq")


SEED, OFFSET, U_BASE = 0x9E3779B97F4A7C15, (1 << 33) + 5, 2 ** 32 - 2        # 64-bit seed and offset; u_base + u wraps


@pytest.mark.parametrize("n_neg", [1, 4, 16])
@pytest.mark.parametrize("N", [2, 7, 1000])
@pytest.mark.parametrize("U", [1, 3, 65])
def test_sampler_is_the_reference_bit_for_bit(fmx, U, N, n_neg):
    table = zipf_table(fmx, N)
    thresh, alias, q, logq = table
    n_try = max(64, 8 * n_neg)
    rng = np.random.default_rng(U * 131 + N * 7 + n_neg)
    own = rng.integers(-1, N, size=U)                                        # -1: no own item
    excl = [np.unique(rng.integers(0, N, size=rng.integers(0, min(N, 6)))) for _ in range(U)]
    for kw in (dict(), dict(own=own), dict(own=own, excl=excl)):
        want = alias_ref.sample(thresh, alias, logq, SEED, OFFSET, U_BASE, U, n_neg, n_try, **kw)
        got = run_sampler(fmx, (thresh, alias, logq), U, n_neg, n_try, SEED, OFFSET, U_BASE, **kw)
        same_sample(got, want, f"U={U} N={N} n_neg={n_neg} {sorted(kw)}")
        if "own" in kw:
            assert (got[0] != own[:, None]).all()
        filled = got[0] >= 0
        assert np.array_equal(got[1][filled], logq[got[0][filled]]) and np.isneginf(got[1][~filled]).all()
    got = run_sampler(fmx, (thresh, alias, logq), U, n_neg, n_try, SEED, OFFSET, U_BASE, own=own, with_logq=False)   # no logq at all
    np.testing.assert_array_equal(got[0], alias_ref.sample(thresh, alias, None, SEED, OFFSET, U_BASE, U, n_neg, n_try, own=own)[0])


def test_a_fill_crosses_the_rounds(fmx):
    """n_try = 130 (rounds of 64, 64 and 2 draws) with the 800 most popular of 1000 positions excluded (2 % of a draw's mass is
    left): under this seed rows fill their two slots in the first round, in the second, in the third, and not at all"""
    U, N, n_neg, n_try, cut = 65, 1000, 2, 130, 800
    thresh, alias, q, logq = zipf_table(fmx, N)
    excl = [np.arange(cut)] * U
    ok = alias_ref.draws(thresh, alias, SEED, 1, 0, U, n_try) >= cut
    first, second, total = ok[:, :64].sum(1), ok[:, :128].sum(1), ok.sum(1)
    assert (first >= n_neg).any() and ((first < n_neg) & (second >= n_neg)).any() and ((second < n_neg) & (total >= n_neg)).any()
    assert (total < n_neg).any()
    want = alias_ref.sample(thresh, alias, logq, SEED, 1, 0, U, n_neg, n_try, excl=excl)
    got = run_sampler(fmx, (thresh, alias, logq), U, n_neg, n_try, SEED, 1, 0, excl=excl)
    same_sample(got, want, "n_try=130")
    assert (got[0][got[0] >= 0] >= cut).all() and ((got[0] < 0).sum(1) > 0).sum() == (total < n_neg).sum()


def test_everything_excluded_and_zero_weights(fmx):
    U, N, n_neg = 5, 7, 4
    thresh, alias, q, logq = zipf_table(fmx, N)
    got = run_sampler(fmx, (thresh, alias, logq), U, n_neg, 64, 3, 0, 0, excl=[np.arange(N)] * U)
    assert (got[0] == -1).all() and np.isneginf(got[1]).all()
    # zero-weight positions are never drawn
    zeros = [0, 3, 4, 17, 49]
    table = zipf_table(fmx, 50, zeros)
    assert not table[0][zeros].any() and not table[2][zeros].any()
    got = run_sampler(fmx, (table[0], table[1], table[3]), 65, 16, 1024, 11, 2, 0)
    assert (got[0] >= 0).all() and not np.isin(got[0], zeros).any() and np.isfinite(got[1]).all()
    same_sample(got, alias_ref.sample(table[0], table[1], table[3], 11, 2, 0, 65, 16, 1024), "zero weights")
    # with replacement: a position drawn twice is returned twice
    assert any(len(set(r.tolist())) < len(r) for r in got[0])


def test_a_corrupt_alias_entry_is_dropped(fmx):
    """alias entries outside [0, N) with threshold 0: every draw of those cells is dropped, never used as an address"""
    N = 7
    thresh, alias, q, logq = zipf_table(fmx, N)
    alias = alias.copy()
    small = np.flatnonzero(thresh < (1 << 24))
    assert len(small) >= 2
    alias[small[0]], alias[small[1]] = N + 100000, -5
    want = alias_ref.sample(thresh, alias, logq, 5, 6, 7, 33, 4, 64)
    got = run_sampler(fmx, (thresh, alias, logq), 33, 4, 64, 5, 6, 7)
    same_sample(got, want, "corrupt alias")
    assert (got[0] < N).all()


def test_a_batch_cut_in_two_calls(fmx):
    U, N, n_neg, n_try, cut = 65, 1000, 4, 64, 30
    thresh, alias, q, logq = zipf_table(fmx, N)
    rng = np.random.default_rng(8)
    own = rng.integers(0, N, size=U)
    excl = [np.unique(rng.integers(0, 20, size=5)) for _ in range(U)]
    table = (thresh, alias, logq)
    whole = run_sampler(fmx, table, U, n_neg, n_try, SEED, OFFSET, 100, own=own, excl=excl)
    head = run_sampler(fmx, table, cut, n_neg, n_try, SEED, OFFSET, 100, own=own[:cut], excl=excl[:cut])
    tail = run_sampler(fmx, table, U - cut, n_neg, n_try, SEED, OFFSET, 100 + cut, own=own[cut:], excl=excl[cut:])
    same_sample((np.concatenate([head[0], tail[0]]), np.concatenate([head[1], tail[1]])), whole, "two calls")
    again = run_sampler(fmx, table, U, n_neg, n_try, SEED, OFFSET, 100, own=own, excl=excl)
    same_sample(again, whole, "run to run")
    other = run_sampler(fmx, table, U, n_neg, n_try, SEED, OFFSET + 1, 100, own=own, excl=excl)
    assert not np.array_equal(other[0], whole[0])


# =====================================================================================================================
# the corrected calls
# =====================================================================================================================
FWD = ("S", "sfirst", "sbi", "logit", "bi", "first", "loss_b", "dz")


def corr_for(N, seed):
    return np.random.default_rng(seed).uniform(-8.0, 0.0, N).astype(np.float32)


@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("k", [4, 16])
def test_zero_corr_is_the_uncorrected_call(fmx, k, G):
    hyp = fmx.Hyper(**HYP)
    for B in (1, 3, 5):
        N = B * G
        rows, x = make_lists(B, G, seed=17 * G + B, real_x=True)
        zero = torch.zeros(N, device="cuda")
        for rule in ("ftrl", "signadam", "adam"):
            what = f"k={k} G={G} B={B} {rule}"
            t1, _ = build_table(fmx, SIZES, k, RULES[rule], seed=7)
            t2 = clone_table(fmx, t1)
            e1, e2 = fmx.FMEngine(t1, max_batch=N), fmx.FMEngine(t2, max_batch=N)
            idx_d, xv_d = dev(e1, rows, x)
            for e in (e1, e2):
                for name in FWD:
                    getattr(e, name).fill_(float("nan"))
            assert e1.list_forward(hyp, idx_d, G, xv_d, want_first=True, want_bi=True) == B
            assert e2.list_forward_q(hyp, idx_d, G, zero, xv_d, want_first=True, want_bi=True) == B
            torch.cuda.synchronize()
            for name in FWD:
                same_bits(getattr(e2, name)[:N], getattr(e1, name)[:N], f"{what} {name}")
            h1, h2 = fmx.Hyper(**HYP), fmx.Hyper(**HYP)
            e1.list_step(h1, rule, idx_d, G, xv_d)
            e2.list_step_q(h2, rule, idx_d, G, zero, xv_d)
            torch.cuda.synchronize()
            e1.check_error_flag()
            e2.check_error_flag()
            same_bits(t2.rows, t1.rows, what + " rows")
            same_bits(t2.bias, t1.bias, what + " bias")
            same_bits(e2.loss_out, e1.loss_out, what + " loss_out")
            assert t1.step == t2.step


def reference(t, pr, rows, x, G, corr, rule, B):
    grows = rows.astype(np.int64) + np.asarray(t.offsets_host[:-1], np.int64)[None, :]
    xx = x if x is not None else np.ones(rows.shape, np.float32)
    if rule == "ftrl":
        h = dict(alpha=HYP["alpha"], beta=HYP["beta"], l1=HYP["l1"], l2=HYP["l2"])
        return listq_step_f64(pr["ftrl_state"], grows, xx, G, corr, "ftrl", h, inv_b=1.0 / B)
    return listq_step_f64(dict(V=pr["V"], w=pr["w"], bias=pr["bias"]), grows, xx, G, corr, "sgd", dict(lr=HYP["lr"]), inv_b=1.0 / B)


@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("k", [4, 16])
def test_forward_and_step_within_float64(fmx, k, G, B):
    N = B * G
    hyp = fmx.Hyper(**HYP)
    corr = corr_for(N, seed=G * 100 + B)
    corr_d = torch.from_numpy(corr).cuda()
    for real_x in (False, True):
        rows, x = make_lists(B, G, seed=31 * G + B, real_x=real_x)
        for rule in ("sgd", "ftrl"):
            what = f"k={k} G={G} B={B} x={real_x} {rule}"
            t, pr = build_table(fmx, SIZES, k, RULES[rule], seed=7)
            eng = fmx.FMEngine(t, max_batch=N)
            idx_d, xv_d = dev(eng, rows, x)
            eng.forward(hyp, idx_d, xv_d)                                   # FMX_LOSS_NONE: the serving score
            want = [b[:N].clone() for b in (eng.S, eng.sfirst, eng.sbi, eng.logit, eng.bi, eng.first)]
            for name in FWD:
                getattr(eng, name).fill_(float("nan"))
            eng.list_forward_q(hyp, idx_d, G, corr_d, xv_d, want_first=True, want_bi=True)
            torch.cuda.synchronize()
            eng.check_error_flag()
            for name, w in zip(FWD[:6], want):
                same_bits(getattr(eng, name)[:N], w, f"{what} {name}: the uncorrected forward's bits")
            ref = reference(t, pr, rows, x, G, corr, rule, B)
            loss, dz = eng.loss_b[:N].cpu().numpy(), eng.dz[:N].cpu().numpy()
            assert np.isfinite(loss).all() and np.isfinite(dz).all(), what
            within(loss, ref["loss_b"], ref["floor"]["loss_b"], what + " loss")
            within(dz, ref["dz"], ref["floor"]["dz"], what + " dz")
            assert (loss.reshape(B, G)[:, 1:].view(np.int32) == 0).all(), what + ": the negatives' loss slots hold +0"
            # the correction is seen: the uncorrected loss of the same rows differs
            eng.list_forward(hyp, idx_d, G, xv_d)
            torch.cuda.synchronize()
            assert not np.array_equal(eng.dz[:N].cpu().numpy(), dz), what
            # the step
            bias0 = t.bias.clone()
            eng.list_step_q(hyp, rule, idx_d, G, corr_d, xv_d)
            torch.cuda.synchronize()
            eng.check_error_flag()
            same_bits(t.bias, bias0, what + " bias")
            within(float(eng.loss_out.item()), ref["loss"], ref["floor"]["loss"], what + " loss_out")
            if rule == "ftrl":
                zV, nV, zw, nw = [a.numpy() for a in t.export_ftrl_state()]
                assert_ftrl_step_within_f64(dict(zV=zV, nV=nV, zw=zw, nw=nw, zb=t.bias[0].item(), nb=t.bias[1].item()), ref,
                                            before=pr["ftrl_state"])
                continue
            u, new, fl = ref["urows"], ref["new"], ref["floor"]
            got = dict(V=t.rows[:, :k].cpu().numpy(), w=t.rows[:, t.kp].cpu().numpy())
            for kk in ("V", "w"):
                b0 = np.asarray(pr[kk], np.float64)[u]
                within(got[kk][u], new[kk][u], fl[kk], f"{what} {kk}")
                within(got[kk][u].astype(np.float64) - b0, new[kk][u] - b0, fl[kk], f"{what} {kk} (the step)")
                mask = np.ones(len(got[kk]), bool)
                mask[u] = False
                np.testing.assert_array_equal(got[kk][mask], pr[kk][mask], err_msg=kk + " untouched rows")


@pytest.mark.parametrize("rule", list(RULES))
def test_bias_is_bit_unchanged(fmx, rule):
    G, B = 5, 3
    t, _ = build_table(fmx, SIZES, 10, RULES[rule])
    eng = fmx.FMEngine(t, max_batch=B * G)
    hyp = fmx.Hyper(**HYP)
    rows0 = t.rows.clone()
    for s in range(3):
        rows, x = make_lists(B, G, seed=40 + s, real_x=bool(s % 2))
        idx_d, xv_d = dev(eng, rows, x)
        bias0 = t.bias.clone()
        eng.list_step_q(hyp, rule, idx_d, G, torch.from_numpy(corr_for(B * G, s)).cuda(), xv_d)
        torch.cuda.synchronize()
        eng.check_error_flag()
        same_bits(t.bias, bias0, f"{rule} step {s}: bias and its state")
    assert not torch.equal(t.rows, rows0)


@pytest.mark.parametrize("rule", ["signadam", "adam"])
@pytest.mark.parametrize("B,n_pool,n_steps", [(7, 3, 5), (171, 5, 37)])   # 171 lists of 3: 513 rows, the sorts run ahead; the pool wraps
def test_stream_is_its_steps(fmx, rule, B, n_pool, n_steps):
    G, k = 3, 10
    t1, _ = build_table(fmx, SIZES, k, RULES[rule])
    t2 = clone_table(fmx, t1)
    e1, e2 = fmx.FMEngine(t1, max_batch=B * G), fmx.FMEngine(t2, max_batch=B * G)
    pool_d = torch.from_numpy(np.stack([make_lists(B, G, seed=100 + j)[0] for j in range(n_pool)])).cuda().contiguous()
    corr_d = torch.from_numpy(np.stack([corr_for(B * G, 200 + j) for j in range(n_pool)])).cuda().contiguous()
    losses1 = torch.full((n_steps,), float("nan"), device="cuda")
    e1.list_stream_q(fmx.Hyper(**HYP), rule, pool_d, G, corr_d, n_steps, loss_out=losses1)
    h2, losses2 = fmx.Hyper(**HYP), []
    for s in range(n_steps):
        e2.list_step_q(h2, rule, pool_d[s % n_pool], G, corr_d[s % n_pool])
        losses2.append(e2.loss_out.clone())
    torch.cuda.synchronize()
    e1.check_error_flag()
    e2.check_error_flag()
    same_bits(t1.rows, t2.rows, "rows")
    same_bits(t1.bias, t2.bias, "bias")
    same_bits(losses1, torch.cat(losses2), "loss_out")
    assert t1.step == t2.step
    # ... and not the uncorrected stream's
    t3 = clone_table(fmx, build_table(fmx, SIZES, k, RULES[rule])[0])
    fmx.FMEngine(t3, max_batch=B * G).list_stream(fmx.Hyper(**HYP), rule, pool_d, G, n_steps)
    torch.cuda.synchronize()
    assert not torch.equal(t3.rows, t1.rows)


@pytest.mark.parametrize("G", [2, 3, 8, 16])
def test_a_list_alone_and_inside_a_batch(fmx, G):
    t, _ = build_table(fmx, SIZES, 10, "weights")
    eng = fmx.FMEngine(t, max_batch=3 * G)
    hyp = fmx.Hyper(**HYP)
    rows, x = make_lists(3, G, seed=G, real_x=True)
    idx_d, xv_d = dev(eng, rows, x)
    corr_d = torch.from_numpy(corr_for(3 * G, G)).cuda()
    eng.list_forward_q(hyp, idx_d, G, corr_d, xv_d, inv_b=0.25)
    torch.cuda.synchronize()
    loss3, dz3, z3 = eng.loss_b[G:2 * G].clone(), eng.dz[G:2 * G].clone(), eng.logit[G:2 * G].clone()
    eng.loss_b.fill_(float("nan"))
    eng.dz.fill_(float("nan"))
    eng.list_forward_q(hyp, idx_d[G:2 * G].contiguous(), G, corr_d[G:2 * G].contiguous(), xv_d[G:2 * G].contiguous(), inv_b=0.25)
    torch.cuda.synchronize()
    same_bits(eng.logit[:G], z3, "logit")
    same_bits(eng.loss_b[:G], loss3, "loss")
    same_bits(eng.dz[:G], dz3, "dz")


@pytest.mark.parametrize("rule", ["signadam", "ftrl", "adam"])
@pytest.mark.parametrize("G,B", [(5, 3), (16, 3), (2, 3)])
def test_guard_bands(fmx, rule, G, B):
    """corr sits in a guarded buffer of exactly B G floats -- a read past it would bring the NaN pattern into loss and dz -- and
    nothing is written behind loss, dz, S, logit or the workspace"""
    L = fmx._lib
    lib = L.load()
    N = B * G
    t, _ = build_table(fmx, SIZES, 10, RULES[rule])
    rows, x = make_lists(B, G, seed=9, real_x=True)
    idx_d = torch.from_numpy(rows).cuda().contiguous()
    xv_d = torch.from_numpy(x).cuda().contiguous()
    need = int(lib.fmx_fm_list_workspace_bytes(t.c_struct(), B, G))
    bufs = dict(S=Guarded(N * t.kp * 4, name="S"), loss=Guarded(N * 4, name="loss"), dz=Guarded(N * 4, name="dz"),
                logit=Guarded(N * 4, name="logit"), ws=Guarded(need, torch.int32, name="workspace"),
                loss_out=Guarded(4, name="loss_out"), error=Guarded(4, torch.int32, name="error"), corr=Guarded(N * 4, name="corr"))
    bufs["corr"].t.copy_(torch.from_numpy(corr_for(N, 5)))
    corr0 = bufs["corr"].t.clone()
    out = L.FwdOut()
    out.S, out.loss, out.dz, out.logit, out.error = (bufs[n].ptr for n in ("S", "loss", "dz", "logit", "error"))
    hyp = fmx.Hyper(**HYP)
    hyp.c.step = t.step
    st = torch.cuda.current_stream().cuda_stream
    bias0 = t.bias.clone()
    L.check(lib.fmx_fm_list_forward_q(t.c_struct(), hyp.ref(), idx_d.data_ptr(), xv_d.data_ptr(), bufs["corr"].ptr, B, G, 1.0 / B,
                                      C.byref(out), st))
    torch.cuda.synchronize()
    assert np.isfinite(bufs["loss"].t.cpu().numpy()).all() and np.isfinite(bufs["dz"].t.cpu().numpy()).all()
    L.check(lib.fmx_fm_list_step_q(t.c_struct(), hyp.ref(), L.RULES[rule], idx_d.data_ptr(), xv_d.data_ptr(), bufs["corr"].ptr, B, G,
                                   1.0 / B, bufs["ws"].ptr, need, C.byref(out), bufs["loss_out"].ptr, st))
    torch.cuda.synchronize()
    for g in bufs.values():
        g.check()
    assert int(bufs["error"].t.item()) == 0
    assert np.isfinite(bufs["loss_out"].t.cpu().numpy()).all() and float(bufs["loss_out"].t.item()) > 0
    assert np.isfinite(bufs["loss"].t.cpu().numpy()).all() and np.isfinite(bufs["dz"].t.cpu().numpy()).all()
    same_bits(bufs["corr"].t, corr0, "corr is read, never written")
    same_bits(t.bias, bias0, "bias")
    rc = lib.fmx_fm_list_step_q(t.c_struct(), hyp.ref(), L.RULES[rule], idx_d.data_ptr(), xv_d.data_ptr(), bufs["corr"].ptr, B, G,
                                1.0 / B, bufs["ws"].ptr, need - 16, C.byref(out), bufs["loss_out"].ptr, st)
    assert rc == L.ERR_SHAPE


# =====================================================================================================================
# the classes
# =====================================================================================================================
MSIZES, MITEM, N_NEG = [7, 5, 11, 30], [3], 4


def positives(n, seed):
    rng = np.random.default_rng(seed)
    Xi = np.stack([rng.integers(0, s, n) for s in MSIZES], 1).astype(np.int32)
    Xv = rng.uniform(0.5, 1.5, (n, len(MSIZES))).astype(np.float32)
    return Xi, Xv


def popular(fmx, **kw):
    return fmx.pairwise.PopularityNegatives(1.0 / np.arange(1, MSIZES[3] + 1) ** 1.1, **kw)


def state_of(m):
    return m._table.rows.detach().clone(), m._table.bias.detach().clone()


@pytest.mark.parametrize("rule", ["signadam", "adam"])
def test_fit_lists_is_the_chain_called_by_hand(fmx, rule):
    B = 33
    Xi, Xv = positives(B, seed=4)
    a, b = new_model(rule, MSIZES), new_model(rule, MSIZES)
    pop = popular(fmx, exclude=[[0, 1]] * B)
    g = torch.Generator(device="cuda").manual_seed(77)
    la = a.fit_lists(Xi, Xv, MITEM, negatives=pop, n_neg=N_NEG, generator=g)
    # by hand: alias_sample -> assemble_lists -> list_step_q
    e = b._engine
    th, al, lq = pop.table("cuda")
    idx_d, xv_d = torch.from_numpy(Xi).cuda(), torch.from_numpy(Xv).cuda()
    own = idx_d[:, MITEM[0]].to(torch.int32).contiguous()
    off, pos = fmx.recommend.exclusions_csr(pop.exclude, B, "cuda")
    neg_pos, neg_logq = e.alias_sample(th, al, lq, N_NEG, 64, own, seed=77, offset=0, excl_offsets=off, excl_pos=pos)
    assert (neg_pos >= 2).all() and (neg_pos != own[:, None]).all()
    rows, xv = fmx.pairwise.assemble_lists(idx_d, xv_d, MITEM, neg_pos.long().unsqueeze(-1))
    corr = torch.cat([lq[own.long()][:, None], neg_logq], dim=1).reshape(-1).contiguous()
    e.list_step_q(b._hyper, rule, rows, 1 + N_NEG, corr, xv)
    torch.cuda.synchronize()
    same_bits(a._table.rows, b._table.rows, "rows")
    same_bits(a._table.bias, b._table.bias, "bias")
    same_bits(la.reshape(1), e.loss_out, "loss")
    assert a._mining_offset == 1 and float(la) > 0
    # correct=False: the uncorrected step on the same draws
    c, d = new_model(rule, MSIZES), new_model(rule, MSIZES)
    lc = c.fit_lists(Xi, Xv, MITEM, negatives=popular(fmx, exclude=[[0, 1]] * B, correct=False), n_neg=N_NEG, generator=g)
    d._engine.list_step(d._hyper, rule, rows, 1 + N_NEG, xv)
    torch.cuda.synchronize()
    same_bits(c._table.rows, d._table.rows, "correct=False rows")
    same_bits(lc.reshape(1), d._engine.loss_out, "correct=False loss")
    assert float(lc) != float(la)
    # a row that cannot be filled names n_try
    with pytest.raises(ValueError, match="n_try"):
        a.fit_lists(Xi, Xv, MITEM, negatives=popular(fmx, exclude=[np.arange(MSIZES[3])] * B), n_neg=N_NEG)
    with pytest.raises(ValueError, match="weights"):
        a.fit_lists(Xi, Xv, MITEM, negatives=fmx.pairwise.PopularityNegatives(np.ones(5)), n_neg=N_NEG)


def test_same_seed_same_losses_and_a_pickled_model_continues(fmx):
    Xi, Xv = positives(24, seed=5)
    runs = []
    for seed in (5, 5, 6):
        m = new_model("signadam", MSIZES)
        g = torch.Generator(device="cuda").manual_seed(seed)
        pop = popular(fmx)
        runs.append(([float(m.fit_lists(Xi, Xv, MITEM, negatives=pop, n_neg=3, generator=g)) for _ in range(3)], m))
    torch.cuda.synchronize()
    assert runs[0][0] == runs[1][0] and all(np.isfinite(runs[0][0])) and runs[0][0] != runs[2][0]
    same_bits(runs[0][1]._table.rows, runs[1][1]._table.rows, "the same state, seed and call numbers: the same model")
    assert runs[0][1]._mining_offset == 3
    # without a generator: mining_seed; the pickled model carries the count of calls
    m = new_model("adam", MSIZES)
    pop = popular(fmx)
    for _ in range(2):
        m.fit_lists(Xi, Xv, MITEM, negatives=pop, n_neg=3)
    m2 = pickle.loads(pickle.dumps(m))
    assert m2._mining_offset == m._mining_offset == 2
    for _ in range(2):
        la, lb = m.fit_lists(Xi, Xv, MITEM, negatives=pop, n_neg=3), m2.fit_lists(Xi, Xv, MITEM, negatives=pop, n_neg=3)
        same_bits(la.reshape(1), lb.reshape(1), "loss after pickling")
    same_bits(m._table.rows, m2._table.rows, "rows after pickling")


def test_run_list_experiment_is_one_list_fit_lists_calls(fmx):
    n = 12
    Xi, Xv = positives(n, seed=6)
    a, b = new_model("signadam", MSIZES), new_model("signadam", MSIZES)
    excl = [[i % 5] for i in range(n)]
    out = a.run_list_experiment(Xi, Xv, MITEM, negatives=popular(fmx, exclude=excl), n_neg=N_NEG)
    hits = 0
    for i in range(n):
        b.fit_lists(Xi[i:i + 1], Xv[i:i + 1], MITEM, negatives=popular(fmx, exclude=[excl[i]]), n_neg=N_NEG)
        z = b._engine.logit[:1 + N_NEG].cpu().numpy()                       # the uncorrected logits before the update
        hits += int((z[1:] >= z[0]).sum() == 0)
    same_bits(a._table.rows, b._table.rows, "rows")
    assert out[3] == {"correct": hits, "wrong": n - hits} and a._mining_offset == b._mining_offset == n


def test_fit_pairs_takes_the_sampler(fmx):
    B = 20
    Xi, Xv = positives(B, seed=7)
    a, b = new_model("signadam", MSIZES), new_model("signadam", MSIZES)
    pop = popular(fmx)
    la = a.fit_pairs(Xi, Xv, MITEM, negatives=pop, n_neg=2)
    th, al, lq = pop.table("cuda")
    own = torch.from_numpy(Xi[:, MITEM[0]].astype(np.int32)).cuda()
    neg_pos, _ = b._engine.alias_sample(th, al, lq, 2, 64, own, seed=0, offset=0)
    lb = b.fit_pairs(Xi, Xv, MITEM, negatives=neg_pos.long().unsqueeze(-1))
    same_bits(a._table.rows, b._table.rows, "rows")
    same_bits(la.reshape(1), lb.reshape(1), "loss")
    out = a.run_pair_experiment(Xi, Xv, MITEM, negatives=pop, n_neg=2)
    assert out[3]["correct"] + out[3]["wrong"] == 2 * B and a._mining_offset == 2


def test_afm_takes_the_sampler_without_the_correction(fmx):
    from models.models_online_deep.afm_adam import AFMAdam
    torch.manual_seed(5)
    m = AFMAdam(MSIZES, embedding_size=4, attention_size=4, batch_size=64, n=0.01, update_rule="adam", fused_optimizer=True)
    Xi, Xv = positives(16, seed=8)
    before = m._table.rows.clone()
    loss = m.fit_lists(Xi, Xv, MITEM, negatives=popular(fmx, correct=False), n_neg=3, attention=True)
    torch.cuda.synchronize()
    assert np.isfinite(float(loss)) and float(loss) > 0 and not torch.equal(m._table.rows, before) and m._mining_offset == 1
    with pytest.raises(NotImplementedError, match="correct=False") as ei:
        m.fit_lists(Xi, Xv, MITEM, negatives=popular(fmx), n_neg=3, attention=True)
    assert "AFMAdam" in str(ei.value) and "fit_lists" in str(ei.value)
