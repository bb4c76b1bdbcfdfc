"""The cross-batch item bank of the in-batch loss on the device (fmx_fm_inbatch_bank_*, include/fmx.h).

Shapes.  test_inbatch_gpu's two tables (F = 5 with the item fields (2, 4) and unit values; F = 3 with the item field (1) and real
values).  B in {1, 3, 64, 65, 257}: one row, a ragged tile, one full tile / one batch range, the first B with two batch ranges, and
four tiles and a row.  k in {3, 16, 64}: R = 8, 2 and 1 bank rows at a time.  M in {1, 63, 64, 65, 130, 2113}: one slot, around the
64-slot range, 130 = three ranges of 44 (a tail that is no multiple of R at kp = 4 and 16), 2113 past the 32-range cap (32 ranges of
67); B <= M where the step runs.  Fill states: empty; partial with count odd (no multiple of R = 8 or 2) and inside a range; exactly
full; full with the head mid-ring.  Every slot >= count and every output is pre-filled with a NaN pattern that must reach no output.

Checks: an empty bank is the plain step bit for bit; bank scores are the serving scores; the step within tests/inbatch_bank_f64.py's
floors (1e-5 |ref| + the fp32 floor, test_inbatch_gpu's tolerance); the step is the composition of public calls; B = 1; keys; the
stream; guard bands; graph capture with a wrapping ring; the class."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

from abi_geometry import PATTERN, Guarded
from inbatch_bank_f64 import bank_geometry, inbatch_bank_step_f64
from test_inbatch_gpu import SHAPES, Call, check_outputs_within, check_table_within, make_batch, variants, zipf_logq
from test_kernels_gpu import HYP
from test_list_gpu import new_model
from test_pair_gpu import RULES, build_table, clone_table, same_bits

pytestmark = pytest.mark.gpu

BS = [1, 3, 64, 65, 257]
KS = [3, 16, 64]
MS = [1, 63, 64, 65, 130, 2113]


@pytest.fixture(scope="module")
def fmx():
    import fmx as _fmx
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _fmx


def fill_states(M, B):
    """(name, head, count): empty; partial -- count odd, inside the second range where there is one; full; full, head mid-ring"""
    out = [("empty", 0, 0)]
    if M >= 3:
        splits_q, per_q = bank_geometry(M)
        c = min(M - 1, per_q + 3) if splits_q > 1 else M // 2
        c -= c % 2 == 0
        out.append(("partial", c, c))
    out.append(("full", 0, M))
    if M > 1:
        out.append(("wrapped", (3 * B) % M or M // 2, M))
    return out


class GBank:
    """A bank in guarded buffers, every word but the state pre-filled with the NaN pattern; what FMEngine takes as a bank."""

    def __init__(self, fmx, M, kp, keyed=True, corrected=True):
        self.capacity, self.kp = M, kp
        self.bufs = dict(bank_S=Guarded(M * kp * 4, name="bank.S"), bank_a=Guarded(M * 4, name="bank.a"),
                         bank_state=Guarded(8, torch.int32, name="bank.state"))
        if corrected:
            self.bufs["bank_corr"] = Guarded(M * 4, name="bank.corr")
        if keyed:
            self.bufs["bank_key"] = Guarded(M * 4, torch.int32, name="bank.key")
        for n, g in self.bufs.items():
            if n != "bank_state":
                g.t.view(torch.int32).fill_(PATTERN)
        c = self._c = fmx._lib.ItemBank()
        c.S, c.a, c.state, c.capacity, c.kp = self.bufs["bank_S"].ptr, self.bufs["bank_a"].ptr, self.bufs["bank_state"].ptr, M, kp
        c.corr = self.bufs["bank_corr"].ptr if corrected else None
        c.key = self.bufs["bank_key"].ptr if keyed else None

    keyed = property(lambda self: "bank_key" in self.bufs)
    corrected = property(lambda self: "bank_corr" in self.bufs)

    def c_struct(self):
        return C.byref(self._c)

    def load(self, head, count, k, seed=1, keys=None, n_keys=9):
        """Slots [0, count) get finite values (the padded columns of S zero, as a push leaves them), the state (head, count)"""
        rng = np.random.default_rng(seed)
        S = np.zeros((count, self.kp), np.float32)
        S[:, :k] = rng.normal(0, 0.3, (count, k))
        self.bufs["bank_S"].t.view(self.capacity, self.kp)[:count] = torch.from_numpy(S).cuda()
        self.bufs["bank_a"].t[:count] = torch.from_numpy(rng.normal(0, 0.3, count).astype(np.float32)).cuda()
        if self.corrected:
            self.bufs["bank_corr"].t[:count] = torch.from_numpy(rng.uniform(-8.0, 0.0, count).astype(np.float32)).cuda()
        if self.keyed:
            kk = rng.integers(0, n_keys, count).astype(np.int32) if keys is None else np.broadcast_to(np.asarray(keys, np.int32), (count,))
            self.bufs["bank_key"].t[:count] = torch.from_numpy(np.ascontiguousarray(kk)).cuda()
        self.bufs["bank_state"].t.copy_(torch.tensor([head, count], dtype=torch.int32))
        return self

    def state(self):
        return tuple(int(v) for v in self.bufs["bank_state"].t.tolist())

    def valid(self):
        """The valid slots as the float64 reference takes them"""
        count = self.state()[1]
        g = lambda n: self.bufs[n].t.cpu().numpy()  # noqa: E731
        return dict(S=g("bank_S").reshape(self.capacity, self.kp)[:count].copy(), a=g("bank_a")[:count].copy(),
                    corr=g("bank_corr")[:count].copy() if self.corrected else None, key=g("bank_key")[:count].copy() if self.keyed else None,
                    M=self.capacity)

    def words(self):
        return {n: g.t.view(torch.int32).clone() for n, g in self.bufs.items()}

    def copy_from(self, words):
        for n, w in words.items():
            self.bufs[n].t.view(torch.int32).copy_(w)

    def twin(self, fmx):
        b = GBank(fmx, self.capacity, self.kp, self.keyed, self.corrected)
        b.copy_from(self.words())
        return b

    def check(self):
        for g in self.bufs.values():
            g.check()


def same_bank(a, b, what):
    for n in a:
        assert torch.equal(a[n].cpu(), b[n].cpu()), f"{what}: {n}: {int((a[n].cpu() != b[n].cpu()).sum())} words differ"


def check_pushed(before, bank, out, key, corr, B, what):
    """The push: the batch's items at the slots (head + j) mod M with the bits of the public forwards' values, every other word of
    the bank unchanged, head and count advanced"""
    M, kp = bank.capacity, bank.kp
    head, count = (int(v) for v in before["bank_state"].tolist())
    slots = torch.tensor([(head + j) % M for j in range(B)])
    after = {n: w.cpu() for n, w in bank.words().items()}
    assert tuple(after["bank_state"].tolist()) == ((head + B) % M, min(M, count + B)), f"{what}: state {after['bank_state'].tolist()}"
    want = {n: w.cpu().clone() for n, w in before.items() if n != "bank_state"}
    bits = lambda a: torch.from_numpy(np.ascontiguousarray(a)).view(torch.int32)  # noqa: E731
    want["bank_S"].view(M, kp)[slots] = bits(out["Sc"].astype(np.float32))
    want["bank_a"][slots] = bits(out["ac"].astype(np.float32))
    if corr is not None:
        want["bank_corr"][slots] = bits(np.asarray(corr, np.float32))
    if key is not None:
        want["bank_key"][slots] = torch.from_numpy(np.asarray(key, np.int32))
    for n in want:
        assert torch.equal(after[n], want[n]), f"{what}: {n} after the push: {int((after[n] != want[n]).sum())} words differ"


class BankCall(Call):
    """test_inbatch_gpu's Call with the bank calls in the place of the plain forward and backward, and the push behind the update"""

    def __init__(self, fmx, t, rows, x, item, bank, key=None, corr=None, inv_b=None):
        super().__init__(fmx, t, rows, x, item, key, corr, inv_b)
        self.bank = bank
        self.lse_bytes = int(self.lib.fmx_fm_inbatch_bank_lse_bytes(self.B, bank.capacity, self.kp))
        assert self.lse_bytes > 0
        self.bufs["lse"] = Guarded(self.lse_bytes, torch.int32, name="lse")
        self.bufs["lse"].t.fill_(PATTERN)
        self.bufs.update(bank.bufs)

    def forward(self, score_out=None, bank_score_out=None):
        kp, B = self.kp, self.B
        self.L.check(self.lib.fmx_fm_inbatch_bank_forward(self.p("Su"), kp, self.p("au"), self.p("Sc"), kp, self.ac.data_ptr(), B, kp,
                                                          self.ptr(self.corr), self.ptr(self.key), self.bank.c_struct(), self.inv_b,
                                                          self.p("lse"), self.lse_bytes, self.p("loss"), self.ptr(score_out),
                                                          self.ptr(bank_score_out), self.st))

    def backward(self):
        kp, B = self.kp, self.B
        self.L.check(self.lib.fmx_fm_inbatch_bank_backward(self.p("Su"), kp, self.p("au"), self.p("Sc"), kp, self.ac.data_ptr(), B, kp,
                                                           self.ptr(self.corr), self.ptr(self.key), self.bank.c_struct(), self.inv_b,
                                                           self.p("lse"), self.lse_bytes, self.p("gSu"), self.p("gSc"), self.p("gac"),
                                                           self.st))

    def push(self):
        self.L.check(self.lib.fmx_fm_inbatch_bank_push(self.bank.c_struct(), self.p("Sc"), self.kp, self.p("sfirst"), self.p("sbi"),
                                                       self.ptr(self.corr), self.ptr(self.key), self.B, self.st))

    def compose(self, hyp, rule):
        before = self.bank.words()
        out = super().compose(hyp, rule)
        self.push()
        torch.cuda.synchronize()
        self.check()
        check_pushed(before, self.bank, out, None if self.key is None else self.key.cpu().numpy(),
                     None if self.corr is None else self.corr.cpu().numpy(), self.B, "the composition")
        return out

    def lse_rows(self):
        """(m, s, n) [B] from the head of the lse block"""
        w = self.bufs["lse"].t.view(torch.float32).cpu().numpy()
        pad = (self.B * 4 + 255) // 256 * 64
        return tuple(w[i * pad:i * pad + self.B].copy() for i in range(3))


def bank_reference(t, pr, rows, x, item, rule, key, corr, kp, bank):
    grows = rows.astype(np.int64) + np.asarray(t.offsets_host[:-1], np.int64)[None, :]
    xx = x if x is not None else np.ones(rows.shape, np.float32)
    if rule == "ftrl":
        h = dict(alpha=HYP["alpha"], beta=HYP["beta"], l1=HYP["l1"], l2=HYP["l2"])
        return inbatch_bank_step_f64(pr["ftrl_state"], grows, xx, item, "ftrl", h, bank, corr=corr, key=key, kp=kp)
    return inbatch_bank_step_f64(dict(V=pr["V"], w=pr["w"], bias=pr["bias"]), grows, xx, item, "sgd", dict(lr=HYP["lr"]), bank, corr=corr,
                                 key=key, kp=kp)


def engine_bank_step(fmx, t, rule, rows, x, item, key, corr, bank):
    """fmx_fm_inbatch_bank_step through the engine -> the engine"""
    eng = fmx.FMEngine(t, max_batch=rows.shape[0])
    idx_d, xv_d, _ = eng.to_device(rows, x)
    eng.inbatch_bank_step(fmx.Hyper(**HYP), rule, idx_d, item, bank, xv_d, corr=None if corr is None else torch.from_numpy(corr).cuda(),
                          key=None if key is None else torch.from_numpy(key).cuda())
    torch.cuda.synchronize()
    eng.check_error_flag()
    return eng


def pick(fmx, shape, rows, item, B, keyed):
    """(key, corr): test_inbatch_gpu's "keys+zipf" variant, or neither"""
    return variants(fmx, shape, rows, item, B)[1][1:] if keyed else (None, None)


# ---- 1. an empty bank: the step is fmx_fm_inbatch_step bit for bit, and afterwards the bank holds the public forwards' values ----
@pytest.mark.parametrize("rule", list(RULES))
@pytest.mark.parametrize("B", BS)
def test_an_empty_bank_is_the_plain_step(fmx, B, rule):
    Ms = [m for m in MS if m >= B]
    for n, (M, k, shape, keyed) in enumerate([(Ms[0], 3, "F5", True), (Ms[len(Ms) // 2], 16, "F3", True), (2113, 64, "F5", False)]):
        sizes = SHAPES[shape][0]
        rows, x, item = make_batch(shape, B, seed=11 * B + k)
        key, corr = pick(fmx, shape, rows, item, B, keyed)
        what = f"{shape} k={k} B={B} M={M} {rule}"
        t, _ = build_table(fmx, sizes, k, RULES[rule], seed=7)
        plain, pub = clone_table(fmx, t), clone_table(fmx, t)
        bank = GBank(fmx, M, t.kp, keyed, keyed)
        before = bank.words()
        eng = engine_bank_step(fmx, t, rule, rows, x, item, key, corr, bank)
        ep = fmx.FMEngine(plain, max_batch=B)
        idx_d, xv_d, _ = ep.to_device(rows, x)
        ep.inbatch_step(fmx.Hyper(**HYP), rule, idx_d, item, xv_d, corr=None if corr is None else torch.from_numpy(corr).cuda(),
                        key=None if key is None else torch.from_numpy(key).cuda())
        torch.cuda.synchronize()
        same_bits(t.rows, plain.rows, what + ": rows, first-order weights and moments")
        same_bits(t.bias, plain.bias, what + ": bias and its state")
        same_bits(eng.loss_out, ep.loss_out, what + " loss_out")
        same_bits(eng.loss_b[:B], ep.loss_b[:B], what + " per-row losses")
        assert int(eng.error.item()) == int(ep.error.item()) == 0 and t.step == plain.step
        c = Call(fmx, pub, rows, x, item, key, corr)                          # the public forwards on the weights before the update
        c.sides(fmx.Hyper(**HYP))
        torch.cuda.synchronize()
        out = dict(Sc=c.bufs["Sc"].t.cpu().numpy().reshape(B, t.kp), ac=c.ac.cpu().numpy())
        check_pushed(before, bank, out, key, corr, B, what)
        assert bank.state() == (B % M, B)
        bank.check()


# ---- 2. bank scores are the serving scores: score_out of batch A (held against fmx_fm_topk in test_inbatch_gpu) at the slots ----
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("B,M", [(1, 1), (3, 63), (64, 64), (65, 130), (257, 2113)])
def test_bank_scores_are_the_serving_scores(fmx, B, M, k):
    shape = "F3"
    sizes = SHAPES[shape][0]
    t, _ = build_table(fmx, sizes, k, "weights", seed=7)
    rows, x, item = make_batch(shape, B, seed=5 * B + k)
    for name, head, count in fill_states(M, B):
        bank = GBank(fmx, M, t.kp, keyed=False, corrected=False).load(head, count, k)
        c = BankCall(fmx, t, rows, x, item, bank)
        c.sides(fmx.Hyper(**HYP))
        c.push()                                                                # A's items, the weights left alone
        score, bscore = Guarded(B * B * 4, name="score_out"), Guarded(B * M * 4, name="bank_score_out")
        for g in (score, bscore):
            g.t.view(torch.int32).fill_(PATTERN)
        c.forward(score_out=score.t, bank_score_out=bscore.t)
        torch.cuda.synchronize()
        c.check()
        score.check()
        bscore.check()
        new_count = min(M, count + B)
        assert bank.state() == ((head + B) % M, new_count)
        slots = torch.tensor([(head + j) % M for j in range(B)]).cuda()
        got = bscore.t.view(B, M)
        same_bits(got[:, slots], score.t.view(B, B), f"k={k} B={B} M={M} {name}: bank_score_out at the pushed slots against score_out")
        written = got.view(torch.int32) != PATTERN
        assert bool(written[:, :new_count].all()) and not bool(written[:, new_count:].any()), f"{name}: slots >= count are left unwritten"
        assert bool(torch.isfinite(c.bufs["loss"].t).all())


# ---- 3. the step within the float64 floors over shapes and fill states; two runs give the same bits ----
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("B", BS)
def test_step_within_float64(fmx, B, k):
    n = 0
    for M in [m for m in MS if m >= B]:
        for name, head, count in fill_states(M, B):
            shape = ("F5", "F3")[n % 2]
            rule = ("sgd", "ftrl")[(n // 2) % 2]
            keyed = (n // 4) % 2 == 0 if name != "empty" else n % 2 == 0
            n += 1
            sizes = SHAPES[shape][0]
            rows, x, item = make_batch(shape, B, seed=31 * B + k + M)
            key, corr = pick(fmx, shape, rows, item, B, keyed)
            what = f"{shape} k={k} B={B} M={M} {name} {'keys+zipf' if keyed else 'free'} {rule}"
            t, pr = build_table(fmx, sizes, k, RULES[rule], seed=7)
            twin = clone_table(fmx, t)
            bias0 = t.bias.clone()
            n_keys = int(key.max()) + 3 if keyed else 1
            bank = GBank(fmx, M, t.kp, keyed, keyed).load(head, count, k, seed=M + count, n_keys=n_keys)
            bank2 = bank.twin(fmx)
            valid = bank.valid()
            out = BankCall(fmx, t, rows, x, item, bank, key, corr).compose(fmx.Hyper(**HYP), rule)
            ref = bank_reference(t, pr, rows, x, item, rule, key, corr, t.kp, valid)
            check_outputs_within(out, ref, k, what)
            check_table_within(t, pr, ref, rule, k, what)
            same_bits(t.bias, bias0, what + " bias")
            if count and not keyed:
                assert (ref["n"] > 0).all() and (out["loss"] > 0).all(), what + ": every row has negatives"
            out2 = BankCall(fmx, twin, rows, x, item, bank2, key, corr).compose(fmx.Hyper(**HYP), rule)
            for name2 in out:
                same_bits(torch.from_numpy(out2[name2]), torch.from_numpy(out[name2]), f"{what} {name2}: run to run")
            same_bits(twin.rows, t.rows, what + " rows: run to run")
            same_bank(bank2.words(), bank.words(), what + " bank: run to run")


# ---- 4. the step is the composition of the public calls under every rule; the bias and its state never move ----
@pytest.mark.parametrize("rule", list(RULES))
@pytest.mark.parametrize("k", [3, 16])
def test_step_is_the_composition_under_every_rule(fmx, rule, k):
    for n, (B, M) in enumerate([(1, 1), (3, 63), (64, 65), (65, 130), (257, 2113)]):
        shape = ("F5", "F3")[n % 2]
        sizes = SHAPES[shape][0]
        for name, head, count in fill_states(M, B)[1:]:
            rows, x, item = make_batch(shape, B, seed=7 * B + k)
            key, corr = pick(fmx, shape, rows, item, B, True)
            what = f"{shape} k={k} B={B} M={M} {name} {rule}"
            t, _ = build_table(fmx, sizes, k, RULES[rule], seed=7)
            twin = clone_table(fmx, t)
            before, bias0 = t.rows.clone(), t.bias.clone()
            bank = GBank(fmx, M, t.kp).load(head, count, k, seed=B + count, n_keys=int(key.max()) + 3)
            bank2 = bank.twin(fmx)
            out = BankCall(fmx, t, rows, x, item, bank, key, corr).compose(fmx.Hyper(**HYP), rule)
            eng = engine_bank_step(fmx, twin, rule, rows, x, item, key, corr, bank2)
            bank2.check()
            same_bits(twin.rows, t.rows, what + " rows, first-order weights and moments")
            same_bits(eng.loss_out, torch.from_numpy(out["loss_out"]), what + " loss_out")
            same_bits(eng.loss_b[:B], torch.from_numpy(out["loss"]), what + " per-row losses")
            same_bank(bank2.words(), bank.words(), what + ": the step's bank against the composition's")
            same_bits(t.bias, bias0, what + ": the composition's bias")
            same_bits(twin.bias, bias0, what + ": the step's bias and its state")
            assert twin.step == t.step and not torch.equal(t.rows, before), what
            assert np.isfinite(out["loss"]).all() and (out["loss"] > 0).any()


# ---- 5. one row against a non-empty bank: it has negatives ----
@pytest.mark.parametrize("rule", ["sgd", "ftrl"])
@pytest.mark.parametrize("k", KS)
def test_one_row_against_a_bank(fmx, k, rule):
    shape, B, M = "F5", 1, 130
    sizes = SHAPES[shape][0]
    rows, x, item = make_batch(shape, B, seed=3 + k)
    t, pr = build_table(fmx, sizes, k, RULES[rule], seed=7)
    before = t.rows.clone()
    _, head, count = fill_states(M, B)[1]
    bank = GBank(fmx, M, t.kp, keyed=False, corrected=False).load(head, count, k, seed=k)
    valid = bank.valid()
    out = BankCall(fmx, t, rows, x, item, bank).compose(fmx.Hyper(**HYP), rule)
    ref = bank_reference(t, pr, rows, x, item, rule, None, None, t.kp, valid)
    what = f"k={k} {rule} B=1 M={M} count={count}"
    check_outputs_within(out, ref, k, what)
    check_table_within(t, pr, ref, rule, k, what)
    assert float(out["loss"][0]) > 0 and float(out["loss_out"][0]) > 0
    grow = rows[0].astype(np.int64) + np.asarray(t.offsets_host[:-1], np.int64)
    ctx = [f for f in range(len(sizes)) if f not in item]
    for f in (ctx[0], item[0]):                                                 # a context row and an item row move
        assert not torch.equal(t.rows[grow[f]], before[grow[f]]), f"{what}: the row of field {f} did not move"
    assert out["gSu"].any() and out["gac"].any()


# ---- 6. keys: a bank whose every item is row 0's item leaves row 0 at the plain step's bits; a keyed step needs a keyed bank ----
@pytest.mark.parametrize("k", [3, 16])
@pytest.mark.parametrize("B,M", [(3, 63), (65, 130)])
def test_keys_mask_the_bank(fmx, B, M, k):
    shape = "F5"
    sizes = SHAPES[shape][0]
    rows, x, item = make_batch(shape, B, seed=B + k)
    key, corr = pick(fmx, shape, rows, item, B, True)
    assert (key != key[0]).any()
    t, _ = build_table(fmx, sizes, k, "weights", seed=7)
    hyp = fmx.Hyper(**HYP)
    plain = Call(fmx, t, rows, x, item, key, corr)
    plain.sides(hyp)
    plain.forward()
    plain.backward()
    _, head, count = fill_states(M, B)[1]
    bank = GBank(fmx, M, t.kp).load(head, count, k, keys=int(key[0]))
    c = BankCall(fmx, t, rows, x, item, bank, key, corr)
    c.sides(hyp)
    c.forward()
    c.backward()
    torch.cuda.synchronize()
    plain.check()
    c.check()
    lse_plain = plain.bufs["lse"].t.view(torch.float32).cpu().numpy()
    pad = (B * 4 + 255) // 256 * 64
    for i, (name, got) in enumerate(zip("msn", c.lse_rows())):
        assert got[0].view(np.int32) == lse_plain[i * pad].view(np.int32), f"row 0's {name}"
    a, b = plain.numpy(), c.numpy()
    for name in ("loss", "gSu"):
        same_bits(torch.from_numpy(b[name][:1].copy()), torch.from_numpy(a[name][:1].copy()), f"B={B} M={M} k={k}: row 0's {name}")
    others = key != key[0]
    assert (b["loss"][others] > a["loss"][others]).all(), "the other rows take the bank's items as negatives"
    assert (b["gSu"][others] != a["gSu"][others]).any()
    # a step keyed against an unkeyed bank (and the reverse) is refused on the host
    L, lib = fmx._lib, fmx._lib.load()
    unkeyed = GBank(fmx, M, t.kp, keyed=False, corrected=True)
    eng = fmx.FMEngine(t, max_batch=B)
    idx_d, xv_d, _ = eng.to_device(rows, x)
    rows0 = t.rows.clone()
    for bk, kk in ((unkeyed, torch.from_numpy(key).cuda()), (bank, None)):
        with pytest.raises(L.FmxError, match="key and bank->key") as ei:
            eng.inbatch_bank_step(hyp, "sgd", idx_d, item, bk, xv_d, corr=torch.from_numpy(corr).cuda(), key=kk)
        assert ei.value.code == L.ERR_ARG and "fmx_fm_inbatch_bank_step" in str(ei.value)
    torch.cuda.synchronize()
    same_bits(t.rows, rows0, "a refused step launches nothing")
    assert unkeyed.state() == (0, 0)


# ---- 7. the stream is its steps: B = 65 and M = 150, the third push wraps ----
@pytest.mark.parametrize("rule", ["signadam", "ftrl", "adam"])
def test_stream_is_its_steps(fmx, rule):
    shape, k, B, M, n_pool = "F5", 16, 65, 150, 3
    sizes, item, _ = SHAPES[shape]
    pool = [make_batch(shape, B, seed=40 + j)[0] for j in range(n_pool)]
    keys = [fmx.pairwise.item_keys(torch.from_numpy(r), item, sizes).numpy() for r in pool]
    corrs = [zipf_logq(fmx, r, item, sizes) for r in pool]
    idx_pool = torch.from_numpy(np.stack(pool)).cuda().contiguous()
    key_pool = torch.from_numpy(np.stack(keys)).cuda().contiguous()
    corr_pool = torch.from_numpy(np.stack(corrs)).cuda().contiguous()
    t1, _ = build_table(fmx, sizes, k, RULES[rule], seed=7)
    t2, t3 = clone_table(fmx, t1), clone_table(fmx, t1)
    bias0 = t1.bias.clone()
    b1, b2, b3 = (GBank(fmx, M, t1.kp) for _ in range(3))
    e1, e2, e3 = (fmx.FMEngine(t, max_batch=B) for t in (t1, t2, t3))
    h1, h2, h3 = (fmx.Hyper(**HYP) for _ in range(3))
    l1, l3 = torch.zeros(5, device="cuda"), torch.zeros(5, device="cuda")
    e1.inbatch_bank_stream(h1, rule, idx_pool, item, 3, b1, corr_pool, key_pool, loss_out=l1[:3])
    torch.cuda.synchronize()
    assert b1.state() == (3 * B % M, M)                                         # the third push wrapped
    e1.inbatch_bank_stream(h1, rule, idx_pool, item, 2, b1, corr_pool, key_pool, loss_out=l1[3:])
    want = []
    for s in (0, 1, 2, 0, 1):
        e2.inbatch_bank_step(h2, rule, idx_pool[s], item, b2, None, corr=corr_pool[s], key=key_pool[s])
        want.append(e2.loss_out.reshape(()).clone())
    e3.inbatch_bank_stream(h3, rule, idx_pool, item, 3, b3, corr_pool, key_pool, loss_out=l3[:3])
    e3.inbatch_bank_stream(h3, rule, idx_pool, item, 2, b3, corr_pool, key_pool, loss_out=l3[3:])
    torch.cuda.synchronize()
    for e in (e1, e2, e3):
        e.check_error_flag()
    for b in (b1, b2, b3):
        b.check()
    same_bits(t1.rows, t2.rows, f"{rule}: the stream's rows against five steps")
    same_bits(l1, torch.stack(want), f"{rule}: the stream's losses")
    same_bank(b1.words(), b2.words(), f"{rule}: the stream's bank and state against five steps'")
    same_bits(t3.rows, t1.rows, f"{rule}: run to run")
    same_bits(l3, l1, f"{rule}: run to run, losses")
    same_bank(b3.words(), b1.words(), f"{rule}: run to run, bank")
    assert b1.state() == (5 * B % M, M)
    for t in (t1, t2):
        same_bits(t.bias, bias0, f"{rule}: bias")
    assert t1.step == t2.step and (t1.step == 8 if rule == "adam" else True)
    assert bool(torch.isfinite(l1).all()) and float(l1[0]) > 0
    # the pool's second pass meets its own items in the bank: the keys mask them, so no row's own item is its negative
    assert not (b1.words()["bank_key"].view(torch.int32) == PATTERN).any()


# ---- 8. nothing is written around the step's workspace, the bank's arrays or its outputs (GBank: every test above) ----
@pytest.mark.parametrize("rule", ["signadam", "ftrl", "adam"])
@pytest.mark.parametrize("B,M", [(3, 63), (65, 65), (257, 2113)])
def test_guard_bands_of_the_step(fmx, rule, B, M):
    L = fmx._lib
    lib = L.load()
    shape, k = "F3", 10
    sizes = SHAPES[shape][0]
    rows, x, item = make_batch(shape, B, seed=9)
    _, key, corr = variants(fmx, shape, rows, item, B)[1]
    t, _ = build_table(fmx, sizes, k, RULES[rule])
    idx_d, xv_d = torch.from_numpy(rows).cuda(), torch.from_numpy(x).cuda()
    key_d, corr_d = torch.from_numpy(key).cuda(), torch.from_numpy(corr).cuda()
    _, head, count = fill_states(M, B)[-1]
    bank = GBank(fmx, M, t.kp).load(head, count, k, n_keys=int(key.max()) + 3)
    need = int(lib.fmx_fm_inbatch_bank_workspace_bytes(t.c_struct(), B, M, len(item)))
    assert need > int(lib.fmx_fm_inbatch_workspace_bytes(t.c_struct(), B, len(item)))
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
    args = (t.c_struct(), hyp.ref(), L.RULES[rule], idx_d.data_ptr(), xv_d.data_ptr(), fields, len(item), corr_d.data_ptr(), key_d.data_ptr(),
            bank.c_struct(), B, 1.0 / B, bufs["ws"].ptr)
    L.check(lib.fmx_fm_inbatch_bank_step(*args, need, C.byref(out), bufs["loss_out"].ptr, st))
    torch.cuda.synchronize()
    for g in list(bufs.values()) + [bank]:
        g.check()
    assert int(bufs["error"].t.item()) == 0
    assert np.isfinite(bufs["loss_out"].t.cpu().numpy()).all() and float(bufs["loss_out"].t.item()) > 0
    assert (bufs["loss"].t.view(torch.int32) != PATTERN).all() and bool(torch.isfinite(bufs["loss"].t).all())
    same_bits(t.bias, bias0, "bias")
    assert bank.state() == ((head + B) % M, M)
    state = bank.words()
    assert lib.fmx_fm_inbatch_bank_step(*args, need - 1, C.byref(out), bufs["loss_out"].ptr, st) == L.ERR_SHAPE
    torch.cuda.synchronize()
    same_bank(bank.words(), state, "a refused step leaves the bank alone")
    # fwd may be null: the losses stay in the workspace
    L.check(lib.fmx_fm_inbatch_bank_step(*args, need, None, bufs["loss_out"].ptr, st))
    torch.cuda.synchronize()
    for g in list(bufs.values()) + [bank]:
        g.check()


# ---- 9. one captured step, replayed on new batches until the ring wraps, against eager steps on a twin ----
def test_a_captured_step_replays(fmx):
    import update_forms as uf
    shape, k, B, M, rule, n = "F5", 16, 257, 600, "ftrl", 4                     # 4 x 257 > 600: the third replay wraps
    sizes, item, _ = SHAPES[shape]
    batches = []
    for j in range(n + 1):
        rows = make_batch(shape, B, seed=70 + j)[0]
        batches.append((torch.from_numpy(rows).cuda(), fmx.pairwise.item_keys(torch.from_numpy(rows), item, sizes).cuda(),
                        torch.from_numpy(zipf_logq(fmx, rows, item, sizes)).cuda()))
    t0, _ = build_table(fmx, sizes, k, RULES[rule], seed=7)

    class Side:
        def __init__(self):
            self.t = clone_table(fmx, t0)
            self.eng = fmx.FMEngine(self.t, max_batch=B)
            self.hyp = fmx.Hyper(**HYP)
            self.bank = GBank(fmx, M, self.t.kp)
            self.statics = (torch.zeros((B, len(sizes)), dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda"),
                            torch.zeros(B, device="cuda"))

        def load(self, batch):
            for dst, src in zip(self.statics, batch):
                dst.copy_(src, non_blocking=True)

        def call(self):
            idx, key, corr = self.statics
            self.eng.inbatch_bank_step(self.hyp, rule, idx, item, self.bank, None, corr=corr, key=key)

        def snap(self, losses):
            return dict(rows=self.t.rows.clone(), bias=self.t.bias.clone(), loss=torch.stack(losses), error=self.eng.error.clone(),
                        **self.bank.words())

    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        a, b = Side(), Side()
        fresh = a.bank.words()
        a.load(batches[0])
        a.call()                                            # eager: the workspace allocated, the table's order learnt
        a.t.rows.copy_(t0.rows)
        a.t.bias.copy_(t0.bias)
        a.bank.copy_from(fresh)                             # ... and the bank as it was: empty, every slot the NaN pattern
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
    assert tuple(rb["bank_state"].tolist()) == (n * B % M, M) and tuple(tb["bank_state"].tolist()) == ((n + 1) * B % M, M)
    uf.same(ra, rb, "four replays against four eager steps")
    uf.same(ta, tb, "the eager step behind the replays")
    assert len({float(v) for v in rb["loss"]}) > 1
    for side in (a, b):
        side.bank.check()


# ---- 10. the class ----
def test_fit_in_batch_bank_is_the_engine_call(fmx):
    shape, B, M = "F3", 65, 150
    sizes, item, _ = SHAPES[shape]
    batches = [make_batch(shape, B, seed=4 + j)[:2] for j in range(3)]
    for kw, keyed, corrected in ((dict(log_q=True), True, True), (dict(), True, False), (dict(log_q=True, mask_duplicates=False), False, True)):
        a, b = new_model("signadam", sizes), new_model("signadam", sizes)
        same_bits(a._table.rows, b._table.rows, "the same seed gives the same model")
        bias0 = b._table.bias.clone()
        ba, bb = (fmx.pairwise.ItemBank(M, a._table.kp, "cuda", keyed=keyed, corrected=corrected) for _ in range(2))
        for rows, x in batches:                                                 # the third push wraps
            log_q = zipf_logq(fmx, rows, item, sizes)
            idx, xv = torch.from_numpy(rows).cuda(), torch.from_numpy(x).cuda()
            kk = dict(kw, log_q=log_q) if "log_q" in kw else kw
            la = a.fit_in_batch_bank(rows, x, item, bank=ba, **kk)
            b._engine.inbatch_bank_step(b._hyper, "signadam", idx, item, bb, xv, corr=torch.from_numpy(log_q).cuda() if corrected else None,
                                        key=fmx.pairwise.item_keys(idx, item, sizes) if keyed else None)
            torch.cuda.synchronize()
            same_bits(la.reshape(1), b._engine.loss_out, f"{sorted(kw)} loss")
            assert float(la) > 0
        same_bits(a._table.rows, b._table.rows, f"{sorted(kw)} rows")
        same_bits(a._table.bias, bias0, "bias untouched")
        for n in ("S", "a", "corr", "key", "state"):
            if getattr(ba, n) is not None:
                same_bits(getattr(ba, n).view(torch.int32), getattr(bb, n).view(torch.int32), f"{sorted(kw)} bank.{n}")
        assert ba.count() == M and ba.head() == 3 * B % M
        ba.clear()
        assert ba.count() == 0 and ba.head() == 0
    # bank=None is fit_in_batch, bit for bit
    rows, x = batches[0]
    log_q = zipf_logq(fmx, rows, item, sizes)
    a, b = new_model("signadam", sizes), new_model("signadam", sizes)
    la, lb = a.fit_in_batch_bank(rows, x, item, log_q=log_q, bank=None), b.fit_in_batch(rows, x, item, log_q=log_q)
    torch.cuda.synchronize()
    same_bits(a._table.rows, b._table.rows, "bank=None: rows")
    same_bits(la.reshape(1), lb.reshape(1), "bank=None: loss")
    # a bank that disagrees with the other arguments is refused by name
    m = new_model("signadam", sizes)
    kp = m._table.kp
    with pytest.raises(ValueError, match="mask_duplicates"):
        m.fit_in_batch_bank(rows, x, item, bank=fmx.pairwise.ItemBank(M, kp, "cuda", keyed=False, corrected=False))
    with pytest.raises(ValueError, match="log_q"):
        m.fit_in_batch_bank(rows, x, item, bank=fmx.pairwise.ItemBank(M, kp, "cuda", keyed=True, corrected=True))
    with pytest.raises(fmx._lib.FmxError, match="do not fit a bank"):
        m.fit_in_batch_bank(rows, x, item, bank=fmx.pairwise.ItemBank(B - 1, kp, "cuda", corrected=False))
    # adam counts its steps
    m = new_model("adam", sizes)
    bank = fmx.pairwise.ItemBank(M, m._table.kp, "cuda")
    for _ in range(3):
        m.fit_in_batch_bank(rows, x, item, log_q=log_q, bank=bank)
    assert m._table.step == 3 and bank.count() == M


@pytest.mark.parametrize("cls", ["DeepFMAdam", "NFMAdam", "AFMAdam"])
def test_the_deep_and_attentional_classes_refuse(fmx, cls):
    mod = {"DeepFMAdam": "deepfm_adam", "NFMAdam": "nfm_adam", "AFMAdam": "afm_adam"}[cls]
    klass = getattr(importlib.import_module("models.models_online_deep." + mod), cls)
    m = object.__new__(klass)                                                   # (the refusal needs no state)
    bank = fmx.pairwise.ItemBank(16, 4, "cuda", corrected=False)
    with pytest.raises(NotImplementedError, match="pure FM logit") as ei:
        m.fit_in_batch_bank(np.zeros((2, 3), np.int64), None, [2], bank=bank)
    assert cls in str(ei.value) and "fit_in_batch_bank" in str(ei.value) and bank.count() == 0


def test_small_batches_with_a_bank_learn_a_planted_model(fmx):
    """test_inbatch_gpu's planted model (context c's item is planted[c]) at B = 8 with M = 256, under its criteria: the loss falls,
    and hr@1, hr@5 and mrr of the planted item rise over the untrained model.  480 steps: the 3,840 training rows of its sixty
    steps of 64.  (The first steps meet a filling bank -- 7, 15, 23 ... negatives -- and the last ones 256 + 7: the loss has to
    fall against a list that grows.)"""
    sizes, item, B, M, held_n = [20, 6, 20], [2], 8, 256, 64
    rng = np.random.default_rng(1)
    planted = rng.permutation(sizes[2])

    def batch(n):
        c = rng.integers(0, sizes[0], size=n)
        return np.stack([c, rng.integers(0, sizes[1], size=n), planted[c]], axis=1).astype(np.int32)
    m = new_model("signadam", sizes)
    bank = fmx.pairwise.ItemBank(M, m._table.kp, "cuda", corrected=False)
    held = batch(held_n)
    before = m.evaluate_ranking(held, None, item, held[:, 2])
    losses = [float(m.fit_in_batch_bank(batch(B), None, item, bank=bank)) for _ in range(480)]
    after = m.evaluate_ranking(held, None, item, held[:, 2])
    print("before", before, "after", after, "loss", np.mean(losses[:5]), "->", np.mean(losses[-5:]))
    assert bank.count() == M
    assert np.isfinite(losses).all() and np.mean(losses[-5:]) < np.mean(losses[:5])
    assert after["n"] == before["n"] == held_n
    assert after["hr@1"] > before["hr@1"] and after["hr@5"] > before["hr@5"] and after["mrr"] > before["mrr"]
