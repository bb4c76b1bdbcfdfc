"""Popularity-sampled negatives and the log-Q corrected list loss without a GPU: the four new symbols and their argument counts,
what the header states, every refusal decided on the host (pointers that are never dereferenced), fmx.pairwise.alias_table, the
numpy sampler of tests/alias_ref.py against the realised distribution, tests/listq_f64.py against torch's float64 autograd and
against list_f64 at corr = 0, and the classes' refusals.  No device is touched."""
import ctypes as C
import importlib
import os
import pickle
import re
import subprocess

import numpy as np
import pytest
import torch

import alias_ref
from test_adaptive_rules_cpu import _fake_table
from test_list_cpu import _problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLER = "fmx_alias_sample_negatives"
COUNTS = {"fmx_fm_list_forward_q": 10, "fmx_fm_list_step_q": 14, "fmx_fm_list_stream_q": 15, SAMPLER: 16}
CALLS = ["fmx_fm_list_forward_q", "fmx_fm_list_step_q", "fmx_fm_list_stream_q"]


def _lib():
    import fmx
    L = fmx._lib
    return fmx, L, L.load()


def _header():
    return open(os.path.join(ROOT, "include", "fmx.h")).read()


def _comment(header, name):
    decl = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
    assert decl, name
    return decl, " ".join(header[:decl.start()].rsplit("/*", 1)[1].split())


def test_symbols_and_argument_counts():
    fmx, L, lib = _lib()
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    defined = set(re.findall(r"\bT\s+(fmx_\w+)", out))
    header = _header()
    for name, n in COUNTS.items():
        assert re.fullmatch(r"fmx_[a-z_]+", name)
        assert name in defined, name
        assert name in L.EXPORTS and len(getattr(lib, name).argtypes) == n, name
        decl, _ = _comment(header, name)
        assert len(decl.group(1).split(",")) == n, name
    assert lib.fmx_version() == 104


def test_header_states_the_draw_layout_and_the_corrected_loss():
    header = _header()
    _, text = _comment(header, SAMPLER)
    for words in ("Replaces:", "torch.multinomial", "redraw loop", "the reference has no counterpart", "Philox4x32-10",
                  "(seed & 0xffffffff, seed >> 32)",
                  "(offset & 0xffffffff, offset >> 32, (u_base + u) mod 2^32, 0x80000000 + (t >> 1))",
                  "a = word 2 (t & 1)", "b = word 2 (t & 1) + 1", "p = (uint64(a) * N) >> 32", "(b >> 8) < thresh[p] ? p : alias[p]",
                  "q_i = (thresh_i + sum_{j: alias_j = i} (2^24 - thresh_j)) / (N 2^24)", "WITH replacement", "never dereferenced",
                  "-1", "-inf", "n_neg <= 16", "n_try <= 1024", "n_neg <= n_try", "FMX_ERR_ARG", "FMX_ERR_UNSUPPORTED", "no LDS",
                  "no atomics", "no retry loop", "not on U"):
        assert words in text, words
    _, text = _comment(header, "fmx_fm_list_forward_q")
    for words in ("Replaces:", "c_j = z_j - corr[G i + j]", "m = max_j c_j", "e_j = exp(c_j - m)", "loss_i = log(s) - (c_0 - m)",
                  "UNCORRECTED", "serving score", "corr must be finite", "FMX_ERR_ARG", "fmx_fm_list_workspace_bytes", "bit-identical",
                  "fmx_fm_list_online_run has no corrected form"):
        assert words in text, words
    assert "no log-Q correction" not in header


def _sample(lib, thresh=0x40000, alias=0x50000, logq=0x60000, N=100, eo=None, ep=None, own=None, U=3, n_neg=1, n_try=64, pos=0x80000,
            out_q=0x90000):
    return lib.fmx_alias_sample_negatives(thresh, alias, logq, N, eo, ep, own, U, n_neg, n_try, 1, 2, 3, pos, out_q, None)


def test_sampler_refusals():
    fmx, L, lib = _lib()
    A, UN = L.ERR_ARG, L.ERR_UNSUPPORTED
    cases = [("U 0", dict(U=0), A), ("N 0", dict(N=0), A), ("n_neg 0", dict(n_neg=0), A), ("n_try 0", dict(n_try=0, n_neg=0), A),
             ("n_neg > n_try", dict(n_neg=5, n_try=4), A), ("n_neg 17", dict(n_neg=17, n_try=64), UN),
             ("n_try 1025", dict(n_try=1025), UN), ("null thresh", dict(thresh=None), A), ("null alias", dict(alias=None), A),
             ("null neg_pos", dict(pos=None), A), ("neg_logq without logq", dict(logq=None), A),
             ("excl_offsets alone", dict(eo=0xA0000), A), ("excl_pos alone", dict(ep=0xA0000), A)]
    for what, kw, want in cases:
        rc = _sample(lib, **kw)
        msg = lib.fmx_last_error_string().decode()
        assert rc == want, (what, rc, msg)
        assert SAMPLER in msg, (what, msg)


def _out(L, S=0x40000, loss=0x41000, dz=0x42000):
    o = L.FwdOut()
    o.S, o.loss, o.dz = S, loss, dz
    return o


def _call(who, lib, L, t, h, corr=0x70000, rule=None, idx=0x60000, n=4, G=4, ws=0x50000, ws_bytes=1 << 40, out=None, n_pool=1, n_steps=0):
    tp = None if t is None else C.byref(t)
    hp = None if h is None else h.ref()
    op = None if out is None else C.byref(out)
    rule = L.RULE_SIGNADAM if rule is None else rule
    if who == "fmx_fm_list_forward_q":
        return lib.fmx_fm_list_forward_q(tp, hp, idx, None, corr, n, G, 1.0, op, None)
    if who == "fmx_fm_list_step_q":
        return lib.fmx_fm_list_step_q(tp, hp, rule, idx, None, corr, n, G, 1.0, ws, ws_bytes, op, None, None)
    return lib.fmx_fm_list_stream_q(tp, hp, rule, idx, corr, n_pool, n, G, 1.0, n_steps, ws, ws_bytes, op, None, None)


@pytest.mark.parametrize("who", CALLS)
def test_corrected_calls_refusals(who):
    """A null corr, and the list family's refusals under the corrected call's own name"""
    fmx, L, lib = _lib()
    A, SH, UN = L.ERR_ARG, L.ERR_SHAPE, L.ERR_UNSUPPORTED
    h = fmx.Hyper(lr=0.01)
    t = _fake_table(L.LAYOUT_WEIGHTS)
    mapped = _fake_table(L.LAYOUT_WEIGHTS)
    mapped.field_cols, mapped.n_cols = 0x90000, 2
    cases = [("corr", dict(corr=None), A, "corr"), ("table", dict(t=None), A, "table"), ("hyper", dict(h=None), A, "hyper"),
             ("idx", dict(idx=None), A, "idx"), ("count 0", dict(n=0), A, "B_lists"), ("G 1", dict(G=1), A, "G = 1"),
             ("G 17", dict(G=17), UN, "G = 17"), ("rows beyond int32", dict(n=2 ** 28, G=8), A, "int32"),
             ("field_cols", dict(t=mapped), UN, "field_cols")]
    if who != "fmx_fm_list_forward_q":
        need = lib.fmx_fm_list_workspace_bytes(C.byref(t), 4, 4)
        cases += [("ftrl rule on a weights table", dict(rule=L.RULE_FTRL), A, "FMX_RULE_FTRL"),
                  ("fwd", dict(out=None), A, "fwd"), ("fwd->dz", dict(out=_out(L, dz=None)), A, "fwd->dz"),
                  ("workspace null", dict(ws=None), A, "workspace"),
                  ("workspace without the scratch", dict(ws_bytes=need - 16), SH, "fmx_fm_list_workspace_bytes")]
    else:
        cases += [("out", dict(out=None), A, "out")]
    for what, kw, want, word in cases:
        kw = dict(dict(t=t, h=h, out=_out(L)), **kw)
        rc = _call(who, lib, L, kw.pop("t"), kw.pop("h"), **kw)
        msg = lib.fmx_last_error_string().decode()
        assert rc == want, (who, what, rc, msg)
        assert msg and who in msg and word in msg, (who, what, msg)
    if who == "fmx_fm_list_stream_q":
        assert _call(who, lib, L, t, h, out=_out(L), ws_bytes=need) == L.OK      # n_steps = 0: everything checked, nothing launched
        for kw in (dict(n_pool=0), dict(n_steps=-1)):
            assert _call(who, lib, L, t, h, out=_out(L), **kw) == A and who in lib.fmx_last_error_string().decode()


# ---- fmx.pairwise.alias_table ----
def _zipf(N, s=1.1):
    return 1.0 / np.arange(1, N + 1, dtype=np.float64) ** s


@pytest.mark.parametrize("weights", [_zipf(50), _zipf(1000, 0.75), np.array([0, 1, 2, 3, 0, 10.5]), np.ones(7), np.array([3.0]),
                                     np.array([0.0, 0.0, 5.0]), np.random.default_rng(3).uniform(0, 1, 257) ** 8])
def test_alias_table(weights):
    from fmx.pairwise import alias_table
    thresh, alias, q, logq = alias_table(weights)
    N = len(weights)
    assert thresh.dtype == np.uint32 and alias.dtype == np.int32 and q.dtype == np.float64 and logq.dtype == np.float32
    assert thresh.shape == alias.shape == q.shape == logq.shape == (N,)
    assert thresh.max() <= 1 << 24 and alias.min() >= 0 and alias.max() < N
    num = alias_ref.realised_numerators(thresh, alias)
    assert int(num.sum()) == N << 24                                   # exactly
    assert np.array_equal(q, num / float(N << 24))
    with np.errstate(divide="ignore"):
        assert np.array_equal(logq, np.log(q).astype(np.float32))      # of the realised q, not of the weights
    zero = weights == 0
    assert not thresh[zero].any() and not np.isin(alias[thresh < (1 << 24)], np.nonzero(zero)[0]).any()
    assert not q[zero].any()              # (a positive weight below half a 2^-24 step of its cell may round to q = 0 as well)
    assert (np.abs(q - weights / weights.sum()) <= alias_ref.q_bound(alias)).all()


def test_alias_table_refuses():
    from fmx.pairwise import PopularityNegatives, alias_table
    for bad in ([0.0, 0.0], [1.0, -1.0], [1.0, float("nan")], [1.0, float("inf")], []):
        with pytest.raises(ValueError, match="alias_table"):
            alias_table(bad)
    with pytest.raises(ValueError):
        PopularityNegatives([1.0, 2.0], n_try=0)


def test_reference_sampler_follows_the_realised_distribution():
    """200,000 draws of a 50-position Zipf table under a fixed seed: every position's count within 5 binomial standard deviations
    of n q_i (the realised q: the exact law of the draws up to the position bias N / 2^32 ~ 1e-8)"""
    from fmx.pairwise import alias_table
    thresh, alias, q, _ = alias_table(_zipf(50))
    U, n_try = 2000, 100
    drawn = alias_ref.draws(thresh, alias, seed=0x123456789ABCDEF, offset=5, u_base=11, U=U, n_try=n_try)
    n = U * n_try
    count = np.bincount(drawn.reshape(-1), minlength=50)
    assert count.sum() == n == 200000
    sd = np.sqrt(n * q * (1 - q))
    assert (np.abs(count - n * q) <= 5 * sd).all(), np.abs(count - n * q) / sd


def test_reference_sampler_layout():
    from fmx.pairwise import alias_table
    thresh, alias, _, logq = alias_table(_zipf(1000))
    full = alias_ref.draws(thresh, alias, 7, 3, 0, 20, 131)
    assert np.array_equal(alias_ref.draws(thresh, alias, 7, 3, 10, 5, 131), full[10:15])        # not on U, nor on the cut
    assert np.array_equal(alias_ref.draws(thresh, alias, 7, 3, 0, 20, 64), full[:, :64])         # nor on n_try
    assert not np.array_equal(alias_ref.draws(thresh, alias, 7, 4, 0, 20, 131), full)
    # the high bit of the fourth counter word: the cells are not fmx_fm_mine_negatives' draws under the same seed and offset
    import mine_ref
    assert not np.array_equal(alias_ref.draws(np.full(1000, 1 << 24), np.arange(1000), 7, 3, 0, 20, 128)[:, 0::2],
                              mine_ref.draws(7, 3, 0, 20, 256, 1000)[:, 0::4])
    pos, lq = alias_ref.sample(thresh, alias, logq, 7, 3, 0, 20, 4, 131, own=full[:, 0], excl=[full[u, 1:3] for u in range(20)])
    for u in range(20):
        want = [d for d in full[u] if d != full[u, 0] and d not in full[u, 1:3]][:4]
        assert pos[u].tolist() == want and np.array_equal(lq[u], logq[want])


# ---- tests/listq_f64.py ----
def test_listq_f64_is_the_autograd_step_and_list_f64_at_zero():
    from list_f64 import list_step_f64
    from listq_f64 import listq_step_f64
    G, B = 4, 6
    state, local, off, x, R, F = _problem(G, B)
    rows = local + off[:-1]
    inv_b = 1.0 / B
    corr = np.random.default_rng(2).uniform(-8, 0, B * G).astype(np.float32)
    r = listq_step_f64(state, rows, x, G, corr, "sgd", dict(lr=0.05), inv_b)

    V = torch.tensor(state["V"], dtype=torch.float64, requires_grad=True)
    w = torch.tensor(state["w"], dtype=torch.float64, requires_grad=True)
    b = torch.tensor(float(state["bias"]), dtype=torch.float64)
    rt, xt = torch.tensor(rows), torch.tensor(x, dtype=torch.float64)
    e = V[rt] * xt[:, :, None]
    z = (w[rt] * xt).sum(1) + 0.5 * (e.sum(1) ** 2 - (e * e).sum(1)).sum(1) + b
    z.retain_grad()
    ls = torch.log_softmax((z - torch.tensor(corr, dtype=torch.float64)).reshape(B, G), dim=1)
    loss = -ls[:, 0].sum() * inv_b
    loss.backward()
    assert abs(r["loss"] - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
    np.testing.assert_allclose(r["logit"], z.detach().numpy(), rtol=1e-12)            # the uncorrected logit
    np.testing.assert_allclose(r["loss_b"][0::G], -ls[:, 0].detach().numpy(), rtol=1e-12)
    np.testing.assert_allclose(r["dz"], z.grad.numpy(), rtol=1e-12, atol=1e-15)
    u = r["urows"]
    np.testing.assert_allclose(r["dV"], V.grad.numpy()[u], rtol=1e-12, atol=1e-12 * np.abs(V.grad.numpy()).max())
    np.testing.assert_allclose(r["dw"], w.grad.numpy()[u], rtol=1e-12, atol=1e-12 * np.abs(w.grad.numpy()).max())
    np.testing.assert_allclose(r["new"]["V"][u], state["V"][u].astype(np.float64) - 0.05 * V.grad.numpy()[u], rtol=1e-12, atol=1e-15)
    # corr = 0: list_f64's values exactly; the floors exceed list_f64's by the subtraction's one rounding and nothing else
    r0 = listq_step_f64(state, rows, x, G, np.zeros(B * G, np.float32), "sgd", dict(lr=0.05), inv_b)
    p0 = list_step_f64(state, rows, x, G, "sgd", dict(lr=0.05), inv_b)
    for key in ("loss", "logit", "dz", "loss_b", "dV", "dw"):
        assert np.array_equal(r0[key], p0[key]), key
    assert np.array_equal(r0["new"]["V"], p0["new"]["V"])
    eps = 2.0 ** -24
    extra = np.repeat(np.abs(p0["logit"]).reshape(B, G).sum(1) * eps, G)
    np.testing.assert_allclose(r0["floor"]["dz"], p0["floor"]["dz"] + 0.25 * extra * inv_b, rtol=1e-12)
    np.testing.assert_allclose(r0["floor"]["loss_b"][0::G], p0["floor"]["loss_b"][0::G] + extra[0::G], rtol=1e-12)
    assert (r["floor"]["dz"] > 0).all() and np.array_equal(r["floor"]["logit"], p0["floor"]["logit"])
    # ftrl: the same relation
    from oracle import fm_oracle as orc
    h = dict(alpha=0.05, beta=1.0, l1=0.001, l2=0.01)
    fs = dict(zV=orc.ftrl_z_for_weight(state["V"], **h), nV=np.full_like(state["V"], 0.1), zw=orc.ftrl_z_for_weight(state["w"], **h),
              nw=np.full_like(state["w"], 0.1), zb=np.float32(0), nb=np.float32(0))
    f0 = listq_step_f64(fs, rows, x, G, np.zeros(B * G, np.float32), "ftrl", h, inv_b)
    g0 = list_step_f64(fs, rows, x, G, "ftrl", h, inv_b)
    assert np.array_equal(f0["new"]["zV"], g0["new"]["zV"]) and np.array_equal(f0["new"]["nw"], g0["new"]["nw"])


# ---- the Python surface that needs no device ----
def test_popularity_negatives_object():
    from fmx.pairwise import PopularityNegatives, alias_table, hard_negatives, popularity_negatives
    w = _zipf(50)
    p = PopularityNegatives(w, power=0.5, n_try=None)
    assert hard_negatives(p) is None and popularity_negatives(p) is p
    assert popularity_negatives(None) is None and popularity_negatives("hard") is None and popularity_negatives([[1]]) is None
    assert (p.power, p.correct, p.exclude, p.N) == (0.5, True, None, 50)
    assert [p.tries(n) for n in (1, 4, 8, 9, 15)] == [64, 64, 64, 72, 120] and PopularityNegatives(w, n_try=200).tries(15) == 200
    t = alias_table(w ** 0.5)
    assert np.array_equal(p.thresh, t[0]) and np.array_equal(p.alias, t[1]) and np.array_equal(p.logq, t[3])
    th, al, lq = p.table("cpu")
    assert th.dtype == torch.int32 and np.array_equal(th.numpy().view(np.uint32), t[0]) and p.table("cpu")[0] is th   # kept
    assert abs(p.floor_logq() - np.log(2.0 ** -24 / 50)) < 1e-12 and p.floor_logq() < lq.min()
    c = PopularityNegatives.from_counts(torch.tensor([3, 3, 1, 0, 3]), 5)
    assert c.power == 0.75 and np.allclose(c.q, np.array([1, 1, 0, 3 ** 0.75, 0]) / (2 + 3 ** 0.75), atol=1e-6)
    with pytest.raises(ValueError, match="size"):
        PopularityNegatives.from_counts(torch.tensor([5]), 5)
    p2 = pickle.loads(pickle.dumps(p))
    assert np.array_equal(p2.thresh, p.thresh) and p2._on == {}


def test_candidate_positions():
    from fmx.pairwise import candidate_positions
    cand = torch.tensor([[3, 0], [3, 9], [40, 10], [17, 4], [3, 0]])
    items = torch.tensor([[3, 0], [17, 4], [17, 5], [40, 10], [3, 9], [0, 0]])
    assert candidate_positions(items, cand).tolist() == [0, 3, -1, 2, 1, -1]


@pytest.mark.parametrize("cls", ["DeepFMAdam", "NFMAdam", "DeepFMOnn", "NFMOnn", "AFMAdam"])
def test_class_refusals(cls):
    from fmx.pairwise import PopularityNegatives
    mod = {"DeepFMAdam": "deepfm_adam", "NFMAdam": "nfm_adam", "DeepFMOnn": "deepfm_onn", "NFMOnn": "nfm_onn", "AFMAdam": "afm_adam"}[cls]
    klass = getattr(importlib.import_module("models.models_online_deep." + mod), cls)
    obj = object.__new__(klass)             # (no GPU: the constructors raise; the refusals need no state)
    pop = PopularityNegatives(np.ones(5))
    for method in ("fit_lists", "run_list_experiment"):
        with pytest.raises(NotImplementedError, match="pure FM logit") as ei:      # the list loss's own refusal, first and unchanged
            getattr(klass, method)(obj, [[0, 0]], [[1.0, 1.0]], [1], negatives=pop)
        assert cls in str(ei.value) and method in str(ei.value)
    if cls == "AFMAdam":
        for method in ("fit_lists", "run_list_experiment"):
            with pytest.raises(NotImplementedError, match="correct=False") as ei:
                getattr(klass, method)(obj, [[0, 0]], [[1.0, 1.0]], [1], negatives=pop, attention=True)
            assert cls in str(ei.value) and method in str(ei.value) and "fmx_fm_list_step_q" in str(ei.value)
            with pytest.raises(ValueError, match="15"):                            # the limit of negatives comes before it
                getattr(klass, method)(obj, [[0, 0]], [[1.0, 1.0]], [1], negatives=pop, n_neg=16, attention=True)


def test_fm_limit_of_negatives_under_the_sampler():
    from fmx.pairwise import PopularityNegatives
    from models.models_online_deep.fm_adam import FMAdam
    obj = object.__new__(FMAdam)
    for method in ("fit_lists", "run_list_experiment"):
        for n_neg in (16, 0):
            with pytest.raises(ValueError, match="15"):
                getattr(FMAdam, method)(obj, [[0, 0]], [[1.0, 1.0]], [1], negatives=PopularityNegatives(np.ones(5)), n_neg=n_neg)
