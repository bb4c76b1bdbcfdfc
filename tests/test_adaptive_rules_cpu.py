"""The persistent adaptive rules (FMX_RULE_ADAGRAD / FMX_RULE_ADAM on FMX_LAYOUT_MOMENTS tables) without a GPU.

flat_adaptive_step is the float64 statement of one flat mini-batch FM step under either rule; the -m gpu tests
(test_adaptive_rules_gpu.py) compare the HIP kernels against it.  Here it is pinned to torch itself: torch.optim.SparseAdam
and torch.optim.Adagrad on per-field nn.Embedding(sparse=True) modules (the bias an nn.Embedding(1, 1, sparse=True) indexed
0), in float64, over 20 steps with duplicate indices and some x = 0.  Also: the closed forms of the first step, the C
layout of fmx_hyper_t, and the refusals that are decided on the host.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------
# the float64 statement
# ---------------------------------------------------------------------------------------------------------------
def adam_consts(lr, beta1, beta2, t):
    """(step size, 1 - beta1, 1 - beta2) of step t (1-based), as SparseAdam computes them."""
    return lr * np.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t), 1.0 - beta1, 1.0 - beta2


def flat_gradients(st, rows, x, y, loss_kind, inv_b=None):
    """Forward + row-reduced gradients of the flat FM step in float64.  rows [B, F] flat row numbers, x [B, F].
    -> (urows sorted unique touched rows, gV [U, k], gw [U], gb, extras) with extras['gabs_V'] / ['gabs_w'] / ['gabs_b']:
    the sums of |term| the gradients are made of, and extras['gnoise_V'] / ['gnoise_w'] / ['gnoise_b']: the gradients'
    fp32 noise scale."""
    V, w, b = st["V"].astype(np.float64), st["w"].astype(np.float64), float(st["bias"])
    B, F = rows.shape
    x = x.astype(np.float64)
    inv_b = 1.0 / B if inv_b is None else inv_b
    e = V[rows] * x[:, :, None]                                    # [B, F, k]
    S = e.sum(1)
    sbi = 0.5 * (S * S - (e * e).sum(1)).sum(1)
    z = (w[rows] * x).sum(1) + sbi + b
    sig = 1.0 / (1.0 + np.exp(-z))
    if loss_kind == "logits":
        dz = (sig - y) * inv_b
    else:
        p = sig
        dz = (1.0 / (1.0 + np.exp(-p)) - y) * p * (1.0 - p) * inv_b
    urows, inv = np.unique(rows.reshape(-1), return_inverse=True)
    U, k = len(urows), V.shape[1]
    termV = (dz[:, None, None] * x[:, :, None]) * (S[:, None, :] - e)       # [B, F, k]
    termw = dz[:, None] * x
    gV, gw = np.zeros((U, k)), np.zeros(U)
    aV, aw = np.zeros((U, k)), np.zeros(U)
    Sabs = np.abs(e).sum(1)                                                  # the fp32 noise of S - e
    np.add.at(gV, inv, termV.reshape(-1, k))
    np.add.at(gw, inv, termw.reshape(-1))
    np.add.at(aV, inv, (np.abs(termV) + np.abs(dz[:, None, None] * x[:, :, None]) * (Sabs[:, None, :] + np.abs(e))).reshape(-1, k))
    np.add.at(aw, inv, np.abs(termw).reshape(-1))
    # fp32 noise of the gradients: the products' own (2e-6 of the sums of |term|) plus that of dlogit, which is absolute --
    # sigmoid(z) - y cancels -- at about one ulp of sigmoid plus the logit's rounding (zabs: the sum of |term| of z)
    zabs = (np.abs(w[rows] * x)).sum(1) + 0.5 * (S * S + (e * e).sum(1)).sum(1) + abs(b)
    dzn = inv_b * (1.2e-7 + 0.25 * 2e-7 * zabs)
    nV, nw = 2e-6 * aV, 2e-6 * aw
    np.add.at(nV, inv, ((dzn[:, None] * np.abs(x))[:, :, None] * np.abs(S[:, None, :] - e)).reshape(-1, k))
    np.add.at(nw, inv, (dzn[:, None] * np.abs(x)).reshape(-1))
    return urows, gV, gw, float(dz.sum()), dict(gabs_V=aV, gabs_w=aw, gabs_b=float(np.abs(dz).sum()), z=z, dz=dz, gnoise_V=nV,
                                                gnoise_w=nw, gnoise_b=2e-6 * float(np.abs(dz).sum()) + float(dzn.sum()))


def rule_apply(p, m, v, g, rule, h, t):
    """One application of the rule to arrays (float64).  -> new (p, m, v)."""
    if rule == "adagrad":
        v2 = v + g * g
        return p - h["lr"] * (g / (np.sqrt(v2) + h["eps"])), m, v2
    ss, c1, c2 = adam_consts(h["lr"], h["beta1"], h["beta2"], t)
    m2 = m + c1 * (g - m)
    v2 = v + c2 * (g * g - v)
    return p - ss * (m2 / (np.sqrt(v2) + h["eps"])), m2, v2


def flat_adaptive_step(st, rows, x, y, loss_kind, rule, h, t, inv_b=None):
    """One step of the flat table under `rule`, float64.  st: V [R, k], w [R], bias, mV, vV, mw, vw, mb, vb (moments of
    adagrad: m stays 0, G in v).  t: the 1-based step number (adam).  Untouched rows keep their values.  -> (new state,
    urows, extras)."""
    urows, gV, gw, gb, ex = flat_gradients(st, rows, x, y, loss_kind, inv_b)
    new = {k_: np.array(v_, dtype=np.float64, copy=True) for k_, v_ in st.items()}
    pV, mV, vV = rule_apply(new["V"][urows], new["mV"][urows], new["vV"][urows], gV, rule, h, t)
    new["V"][urows], new["mV"][urows], new["vV"][urows] = pV, mV, vV
    pw, mw, vw = rule_apply(new["w"][urows], new["mw"][urows], new["vw"][urows], gw, rule, h, t)
    new["w"][urows], new["mw"][urows], new["vw"][urows] = pw, mw, vw
    pb, mb, vb = rule_apply(np.float64(st["bias"]), np.float64(st["mb"]), np.float64(st["vb"]), gb, rule, h, t)
    new["bias"], new["mb"], new["vb"] = pb, mb, vb
    ex.update(gV=gV, gw=gw, gb=gb)
    return new, urows, ex


def zero_state(V, w, bias):
    R, k = V.shape
    return dict(V=V.astype(np.float64), w=w.astype(np.float64), bias=np.float64(bias), mV=np.zeros((R, k)), vV=np.zeros((R, k)),
                mw=np.zeros(R), vw=np.zeros(R), mb=np.float64(0), vb=np.float64(0))


def problem(sizes, k, B, seed, zero_x=True):
    """Seeded flat problem: Zipf-skewed indices (duplicates), real x with some exact zeros."""
    rng = np.random.default_rng(seed)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    idx = np.stack([np.minimum(rng.zipf(1.3, size=B) - 1, s - 1) for s in sizes], axis=1).astype(np.int32)
    x = rng.uniform(0.2, 1.5, size=(B, len(sizes))).astype(np.float32)
    if zero_x:
        x[rng.uniform(size=x.shape) < 0.1] = 0.0
    y = (rng.uniform(size=B) < 0.4).astype(np.float32)
    return offs, idx, x, y


# ---------------------------------------------------------------------------------------------------------------
# the statement against torch
# ---------------------------------------------------------------------------------------------------------------
class TorchFM(torch.nn.Module):
    """The FM logit on per-field nn.Embedding(sparse=True) modules, float64 (the bias: an Embedding(1, 1) indexed 0)."""

    def __init__(self, sizes, k, V, w, bias, offs):
        super().__init__()
        self.first = torch.nn.ModuleList([torch.nn.Embedding(s, 1, sparse=True).double() for s in sizes])
        self.second = torch.nn.ModuleList([torch.nn.Embedding(s, k, sparse=True).double() for s in sizes])
        self.bias = torch.nn.Embedding(1, 1, sparse=True).double()
        with torch.no_grad():
            for f in range(len(sizes)):
                lo, hi = int(offs[f]), int(offs[f + 1])
                self.first[f].weight.copy_(torch.from_numpy(w[lo:hi].astype(np.float64)).reshape(-1, 1))
                self.second[f].weight.copy_(torch.from_numpy(V[lo:hi].astype(np.float64)))
            self.bias.weight.fill_(float(bias))

    def forward(self, idx, x):
        F = idx.shape[1]
        e = torch.stack([self.second[f](idx[:, f]) * x[:, f:f + 1] for f in range(F)], 1)
        fo = sum(self.first[f](idx[:, f])[:, 0] * x[:, f] for f in range(F))
        S = e.sum(1)
        return fo + 0.5 * (S * S - (e * e).sum(1)).sum(1) + self.bias(torch.zeros(idx.shape[0], dtype=torch.long))[:, 0]

    def flat(self, offs):
        V = torch.cat([m.weight.detach() for m in self.second]).numpy()
        w = torch.cat([m.weight.detach()[:, 0] for m in self.first]).numpy()
        return V, w, float(self.bias.weight.detach()[0, 0])


HYP = {"adam": dict(lr=0.02, beta1=0.9, beta2=0.999, eps=1e-8), "adagrad": dict(lr=0.05, eps=1e-10)}


@pytest.mark.parametrize("loss_kind", ["logits", "sigmoid"])
@pytest.mark.parametrize("rule", ["adam", "adagrad"])
def test_statement_equals_torch_sparse_optimizers(rule, loss_kind):
    sizes, k, B, T = [5, 40, 3, 17], 6, 48, 20
    rng = np.random.default_rng(11)
    R = sum(sizes)
    V0, w0, b0 = rng.normal(size=(R, k)) * 0.3, rng.normal(size=R) * 0.3, 0.1
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    model = TorchFM(sizes, k, V0, w0, b0, offs)
    h = HYP[rule]
    params = list(model.parameters())
    if rule == "adam":
        opt = torch.optim.SparseAdam(params, lr=h["lr"], betas=(h["beta1"], h["beta2"]), eps=h["eps"])
    else:
        opt = torch.optim.Adagrad(params, lr=h["lr"], eps=h["eps"])
    st = zero_state(V0, w0, b0)
    for t in range(1, T + 1):
        _, idx, x, y = problem(sizes, k, B, 100 + t)
        rows = idx.astype(np.int64) + offs[:-1][None, :]
        st, _, _ = flat_adaptive_step(st, rows, x, y, loss_kind, rule, h, t)
        opt.zero_grad()
        z = model(torch.from_numpy(idx.astype(np.int64)), torch.from_numpy(x.astype(np.float64)))
        yy = torch.from_numpy(y.astype(np.float64))
        loss = torch.nn.functional.binary_cross_entropy_with_logits(z if loss_kind == "logits" else torch.sigmoid(z), yy)
        loss.backward()
        opt.step()
        V, w, b = model.flat(offs)
        np.testing.assert_allclose(st["V"], V, rtol=1e-11, atol=1e-13)
        np.testing.assert_allclose(st["w"], w, rtol=1e-11, atol=1e-13)
        np.testing.assert_allclose(st["bias"], b, rtol=1e-11, atol=1e-13)
    # the moments too: the oracle's state is torch's optimizer state
    key = "exp_avg_sq" if rule == "adam" else "sum"
    vt = torch.cat([opt.state[m.weight][key].to_dense() if opt.state[m.weight][key].is_sparse else opt.state[m.weight][key]
                    for m in model.second]).numpy()
    np.testing.assert_allclose(st["vV"], vt, rtol=1e-11, atol=1e-15)


def test_lazy_rows_and_zero_x():
    """A row whose index occurs with x = 0 is touched (its moments decay); a row that does not occur keeps its state."""
    sizes, k = [4, 4], 3
    offs = np.array([0, 4, 8])
    rng = np.random.default_rng(2)
    st = zero_state(rng.normal(size=(8, k)), rng.normal(size=8), 0.0)
    st["mV"][:] = 0.5
    st["vV"][:] = 0.25
    idx = np.array([[0, 1], [0, 2]], dtype=np.int32)
    x = np.array([[0.0, 1.0], [0.0, 1.0]], dtype=np.float32)
    rows = idx.astype(np.int64) + offs[:-1][None, :]
    new, urows, _ = flat_adaptive_step(st, rows, x, np.array([1.0, 0.0]), "logits", "adam", HYP["adam"], 3)
    assert list(urows) == [0, 5, 6]
    np.testing.assert_allclose(new["mV"][0], 0.5 * 0.9)                  # g = 0: m decays, the weight moves with it
    assert np.all(new["mV"][[1, 2, 3, 4, 7]] == 0.5) and np.all(new["V"][[1, 2, 3, 4, 7]] == st["V"][[1, 2, 3, 4, 7]])


@pytest.mark.parametrize("eps", [1e-8, 1e-3])
def test_first_adam_step_is_signadam_with_scaled_eps(eps):
    """From zero state: m = (1-b1) g, v = (1-b2) g^2, step size lr sqrt(1-b2) / (1-b1)  =>  p -= lr g / (|g| + eps/sqrt(1-b2))."""
    sizes, k, B = [7, 30, 5], 4, 64
    offs, idx, x, y = problem(sizes, k, B, 3)
    rng = np.random.default_rng(4)
    R = int(offs[-1])
    st = zero_state(rng.normal(size=(R, k)) * 0.3, rng.normal(size=R) * 0.3, 0.2)
    rows = idx.astype(np.int64) + offs[:-1][None, :]
    h = dict(HYP["adam"], eps=eps)
    new, urows, ex = flat_adaptive_step(st, rows, x, y, "logits", "adam", h, 1)
    e2 = eps / np.sqrt(1.0 - h["beta2"])
    sign = lambda p, g: p - h["lr"] * g / (np.abs(g) + e2)
    np.testing.assert_allclose(new["V"][urows], sign(st["V"][urows], ex["gV"]), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(new["w"][urows], sign(st["w"][urows], ex["gw"]), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(new["bias"], sign(st["bias"], ex["gb"]), rtol=1e-12)


def test_first_adagrad_step_is_signadam():
    """From zero state: G = g^2  =>  p -= lr g / (|g| + eps), the reference's fresh-Adam rule with the same eps."""
    sizes, k, B = [7, 30, 5], 4, 64
    offs, idx, x, y = problem(sizes, k, B, 5)
    rng = np.random.default_rng(6)
    R = int(offs[-1])
    st = zero_state(rng.normal(size=(R, k)) * 0.3, rng.normal(size=R) * 0.3, 0.2)
    rows = idx.astype(np.int64) + offs[:-1][None, :]
    h = HYP["adagrad"]
    new, urows, ex = flat_adaptive_step(st, rows, x, y, "sigmoid", "adagrad", h, 1)
    sign = lambda p, g: p - h["lr"] * g / (np.abs(g) + h["eps"])
    np.testing.assert_allclose(new["V"][urows], sign(st["V"][urows], ex["gV"]), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(new["w"][urows], sign(st["w"][urows], ex["gw"]), rtol=1e-12, atol=1e-15)


# ---------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------
def test_hyper_struct_matches_the_header(tmp_path):
    import fmx
    H = fmx._lib.Hyper
    names = [f[0] for f in H._fields_]
    assert names == ["lr", "eps", "alpha", "beta", "l1", "l2", "beta1", "beta2", "step", "reserved"]
    src = tmp_path / "hyper.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fmx.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(fmx_hyper_t));\n'
                   + "".join(f'  printf(" %zu", offsetof(fmx_hyper_t, {n}));\n' for n in names) + "  return 0;\n}\n")
    exe = tmp_path / "hyper"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(H)] + [getattr(H, n).offset for n in names]
    assert C.sizeof(H) == 40
    # positional and keyword construction both keep working; the new fields default to Adam's usual values
    h = fmx.Hyper(0.5, 1e-3, 0.1, 2.0, 0.0, 0.0)
    assert (h.c.lr, h.c.beta, h.c.step) == (0.5, 2.0, 0)
    assert np.float32(h.c.beta1) == np.float32(0.9) and np.float32(h.c.beta2) == np.float32(0.999)
    h = fmx.Hyper(lr=0.1, beta1=0.5, beta2=0.75, step=7)
    assert (h.c.beta1, h.c.beta2, h.c.step) == (0.5, 0.75, 7)


def _fake_table(layout, k=16):
    """A table struct whose pointers are never dereferenced: the calls below return from their host-side checks."""
    import fmx
    L = fmx._lib
    t = L.Table()
    t.rows, t.field_offsets, t.bias = 0x10000, 0x20000, 0x30000
    t.n_rows, t.n_fields, t.k, t.kp = 100, 2, k, 16
    t.layout = layout
    t.z_offset = 32 if layout != L.LAYOUT_WEIGHTS else 0
    t.row_stride = 64 if layout != L.LAYOUT_WEIGHTS else 32
    t.max_field_rows = 50
    return t


def test_rules_and_layouts_are_paired_on_the_host():
    import fmx
    L = fmx._lib
    lib = L.load()
    h = fmx.Hyper(lr=0.01)
    out = L.FwdOut()
    out.S = out.dz = out.loss = 0x40000
    ws = 0x50000
    for layout, rule, want in [(L.LAYOUT_WEIGHTS, L.RULE_ADAM, L.ERR_ARG), (L.LAYOUT_FTRL, L.RULE_ADAGRAD, L.ERR_ARG),
                               (L.LAYOUT_MOMENTS, L.RULE_SIGNADAM, L.ERR_ARG), (L.LAYOUT_MOMENTS, L.RULE_FTRL, L.ERR_ARG),
                               (L.LAYOUT_MOMENTS, 5, L.ERR_ARG), (3, L.RULE_ADAM, L.ERR_ARG)]:
        t = _fake_table(layout)
        rc = lib.fmx_fm_step(C.byref(t), h.ref(), rule, L.LOSS_BCE_LOGITS, 0x60000, None, 0x70000, 64, 1.0 / 64, ws, 1 << 40,
                             C.byref(out), None, None)
        assert rc == want, (layout, rule, rc, lib.fmx_last_error_string())
    # the MOMENTS geometry is FTRL's: z_offset >= kp + 4, row_stride >= z_offset + 2 kp
    t = _fake_table(L.LAYOUT_MOMENTS)
    t.row_stride = 60
    assert lib.fmx_workspace_bytes(C.byref(t), 64) < 0
    t.row_stride = 64
    assert lib.fmx_workspace_bytes(C.byref(t), 64) > 0
    # adam's betas and step are checked before anything is launched
    t = _fake_table(L.LAYOUT_MOMENTS)
    for bad in (fmx.Hyper(beta1=1.0), fmx.Hyper(beta2=-0.1), fmx.Hyper(step=-1)):
        rc = lib.fmx_fm_step(C.byref(t), bad.ref(), L.RULE_ADAM, L.LOSS_BCE_LOGITS, 0x60000, None, 0x70000, 64, 1.0 / 64, ws,
                             1 << 40, C.byref(out), None, None)
        assert rc == L.ERR_ARG


@pytest.mark.parametrize("rule", ["adam", "adagrad"])
def test_entry_points_outside_the_table_steps_refuse_the_adaptive_rules(rule):
    import fmx
    L = fmx._lib
    lib = L.load()
    r = L.RULES[rule]
    h = fmx.Hyper(lr=0.01)
    t = _fake_table(L.LAYOUT_MOMENTS)
    m = L.Mlp(0x80000, 2, 16, 32, 0)
    out = L.FwdOut()
    out.S = out.bi = out.sfirst = out.logit = out.dz = out.loss = 0x40000
    name = "FMX_RULE_ADAM" if rule == "adam" else "FMX_RULE_ADAGRAD"
    calls = {
        "fmx_deepfm_stream": lambda: lib.fmx_deepfm_stream(C.byref(t), h.ref(), r, C.byref(m), L.LOSS_BCE_LOGITS, 1, 0x60000, 0x70000,
                                                           1, 64, 1.0 / 64, 1, 0x50000, 1 << 40, 0x90000, C.byref(out), 0xA0000,
                                                           0xB0000, 0xC0000, 0.01, None, None),
        "fmx_online_run_mlp": lambda: lib.fmx_online_run_mlp(C.byref(t), h.ref(), r, L.LOSS_BCE_SIGMOID, C.byref(m), 0, 1, 0.0, 0.0,
                                                             None, 0x60000, None, 0x70000, 4, 0x50000, 1 << 40, C.byref(out),
                                                             0xD0000, 0xE0000, None),
        "fmx_mlp_fit": lambda: lib.fmx_mlp_fit(C.byref(m), h.ref(), r, L.LOSS_BCE_SIGMOID, 0x40000, 16, 0x40000, 0x70000, 1, 1.0,
                                               0xA0000, 0xB0000, None, None),
        "fmx_owner_step": lambda: lib.fmx_owner_step(None, C.byref(t), h.ref(), r, L.LOSS_BCE_LOGITS, 0x60000, 0x70000, 64, 0,
                                                     0x50000, 1 << 40, None, None, None, None),
    }
    for who, call in calls.items():
        rc = call()
        msg = lib.fmx_last_error_string().decode()
        assert rc == L.ERR_UNSUPPORTED, (who, rc, msg)
        assert name in msg and who.split(" ")[0] in msg, msg


def test_multi_gpu_trainers_refuse_the_adaptive_rules():
    import fmx
    from fmx.owner import HipOwnerBackend
    for rule in ("adam", "adagrad"):
        with pytest.raises(ValueError):
            fmx.HipBackend(None, fmx.Hyper(), rule, "logits")
        with pytest.raises(ValueError):
            fmx.HipDeepBackend(None, fmx.Hyper(), rule)
        with pytest.raises(ValueError):
            HipOwnerBackend([5, 7], 4, fmx.Hyper(), rule, "logits", 0, 1)
