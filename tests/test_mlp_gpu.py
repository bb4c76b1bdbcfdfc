"""fmx_mlp_section (the relu MLP at mini-batch sizes: fp32 MFMA GEMMs for forward, loss, backward) against a float64
PyTorch autograd reference of the same network (reference deepfm_adam.py:79-89,106-119: nn.Linear + relu + autograd).
Tolerance: fp32 sums over up to 4096 samples in a different order than the reference -> 2e-5 relative to the largest
magnitude of each output, and of each layer's W and b gradient on its own (plus the fp32 noise floor of a cancelled sum)."""
import numpy as np
import pytest
import torch

from helpers import mlp_f64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fmx():
    import fmx as _fmx
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _fmx


CASES = [  # B, k, kp, hidden, layers, loss
    (4096, 16, 16, 256, 3, "logits"),       # BASELINE configs[3]
    (300, 10, 12, 40, 2, "sigmoid"),        # reference embedding size, ragged tiles, the double-sigmoid loss
    (37, 4, 4, 33, 1, "logits"),            # odd hidden: the scalar-load path; one layer
    (1000, 16, 16, 64, 5, "logits"),        # the reference's depth
    (4096, 16, 20, 256, 3, "logits"),       # bi rows strided (records), gbi padded
    # the chain kernel (hidden = 256) and the streaming weight gradients away from configs[3]: a ragged last slab of 16 rows,
    # every k the chain takes, one layer (no 256 x 256 GEMM at all), the deepest network, few rows per batch split
    (1000, 32, 32, 256, 2, "sigmoid"),
    (37, 48, 48, 256, 1, "logits"),
    (530, 64, 64, 256, 4, "logits"),
    (100, 16, 16, 256, 8, "logits"),
    (2048, 16, 16, 128, 3, "logits"),       # GEMM launches for the chain's part, streaming weight gradients (128-wide layers)
    (700, 24, 24, 72, 3, "logits"),         # narrow first layer of 24 columns (two natural tiles), 72-wide layers (two blocks, ragged)
    (1, 16, 16, 256, 3, "logits"),          # one sample
    (17, 16, 16, 256, 3, "logits"),         # one row past a 16-row slab
    (129, 52, 52, 64, 2, "logits"),         # 48 < in < 64: layer 0 off the streamed weight gradients
    (300, 64, 66, 256, 2, "logits"),        # layer 0 at in >= 64 with ld_bi % 4 != 0: the GEMM weight gradients
    (64, 4, 4, 1, 2, "logits"),             # hidden = 1
    (500, 24, 32, 72, 8, "logits"),         # eight layers away from hidden = 256
    (4096, 16, 16, 256, 3, "sigmoid"),      # configs[3] under the double-sigmoid loss
]


def reference(params, k, H, L, loss, bi, base, y, inv_b):
    r = mlp_f64(params.cpu().numpy(), k, H, L, bi.cpu().numpy(), base.cpu().numpy(), y.cpu().numpy(), loss, inv_b)
    return r["loss"], r["dz"], r["gbi"], r["flat"], r["out"], r


def live_units(params, k, H, L, bi):
    """params with the incoming weights and bias of every unit that is dead (relu off) for every sample negated, layer by
    layer on the float64 forward: such a unit contributes nothing and receives an exactly-0 gradient, so a kernel that
    skipped or mis-indexed it would still pass.  Negation is exact in fp32; units live for some sample are left alone."""
    p = np.asarray(params, dtype=np.float32).copy()
    x, off = np.asarray(bi, np.float64), 0
    for l in range(L):
        i = k if l == 0 else H
        W, b = p[off:off + H * i].reshape(H, i), p[off + H * i:off + H * i + H]
        dead = ((x @ W.astype(np.float64).T + b) <= 0).all(0)
        W[dead] *= -1
        b[dead] *= -1
        x = np.maximum(x @ W.astype(np.float64).T + b, 0.0)
        off += H * i + H
    return p


def assert_live(r, L, what):
    """Every layer's float64 gradient has non-zero W and b entries: the case exercises every layer."""
    for l in range(L):
        assert np.any(r["grads"][l][0]) and np.any(r["grads"][l][1]), f"{what}: layer {l} has no live unit (a dead network)"


def close(a, b, what, rel=2e-5, floor=0.0):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = max(np.abs(b).max(), 1e-30)
    err = np.abs(a - b)
    assert (err <= rel * scale + floor).all(), f"{what}: max err {err.max():.3e} vs scale {scale:.3e}"


def close_per_tensor(grads, r, k, H, L, B, what):
    """Each layer's W and b gradient against its own maximum (an error confined to one layer's bias, one split or one 16-row
    slab of a small layer stays visible), plus four times the fp32 rounding noise expected in the element (helpers.mlp_f64's
    gnoise: each sum's own |terms|, the inputs' noise carried through the signed products)."""
    off = 0
    for l in range(L):
        i = k if l == 0 else H
        for name, n, g_ref, g_noise in (("W", H * i, r["grads"][l][0], r["gnoise"][l][0]), ("b", H, r["grads"][l][1], r["gnoise"][l][1])):
            close(grads[off:off + n], g_ref.reshape(-1), f"{what}: {name}{l}", floor=4 * g_noise.reshape(-1))
            off += n
    assert off == grads.size


@pytest.mark.parametrize("B,k,kp,H,L,loss", CASES)
def test_mlp_section_vs_autograd(fmx, B, k, kp, H, L, loss):
    section_vs_autograd(fmx, B, k, kp, H, L, loss)


@pytest.mark.parametrize("B,k,kp,H,L,loss", [(4096, 16, 16, 256, 3, "logits"), (1000, 32, 32, 256, 2, "sigmoid")])
def test_mlp_section_without_chain_vs_autograd(fmx, B, k, kp, H, L, loss):
    """mlp_chain = 0: the separate GEMM launches instead of k_mlp_chain at hidden = 256 (configs[3], and a ragged last slab)."""
    lib = fmx._lib.load()
    prev = lib.fmx_set_option(b"mlp_chain", 0)
    try:
        section_vs_autograd(fmx, B, k, kp, H, L, loss)
    finally:
        lib.fmx_set_option(b"mlp_chain", prev)


def section_vs_autograd(fmx, B, k, kp, H, L, loss):
    torch.manual_seed(B + H + L)
    n_par = sum(H * (k if l == 0 else H) + H for l in range(L))
    # the double-sigmoid loss multiplies by p (1 - p), p = sigmoid(z): with 256 relu outputs summed into z, N(0, 1 / H) weights put
    # p within 1e-8 of 1 where fp32 cancels (the reference's fp32 does too; float64 is then a different function): smaller weights
    # there keep the comparison about the kernels
    wscale = 0.25 if (loss == "sigmoid" and H >= 256) else 1.0
    params = (torch.randn(n_par) * (wscale / np.sqrt(H))).cuda()
    bi_full = torch.zeros(B, kp)
    bi_full[:, :k] = torch.randn(B, k) * 0.5
    params = torch.from_numpy(live_units(params.cpu().numpy(), k, H, L, bi_full[:, :k].numpy())).cuda()
    bi_d = bi_full.cuda()
    base = (torch.randn(B) * 0.3).cuda()
    y = (torch.rand(B) < 0.3).float().cuda()
    inv_b = 1.0 / B
    grads = torch.zeros_like(params)
    import ctypes as C
    lib = fmx._lib.load()
    m = fmx._lib.Mlp(params.data_ptr(), L, k, H, 0)
    ws = torch.empty(int(lib.fmx_mlp_section_workspace_bytes(C.byref(m), B)) // 4, device="cuda")
    dz = torch.empty(B, device="cuda")
    gbi = torch.full((B, kp), 7.0, device="cuda")
    logit = torch.empty(B, device="cuda")
    loss_out = torch.zeros(1, device="cuda")
    p0 = params.clone()
    fmx._lib.check(lib.fmx_mlp_section(C.byref(m), fmx._lib.LOSSES[loss], bi_d.data_ptr(), kp, base.data_ptr(), y.data_ptr(), B,
                                       inv_b, ws.data_ptr(), logit.data_ptr(), dz.data_ptr(), gbi.data_ptr(), kp,
                                       grads.data_ptr(), 0.0, loss_out.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    r_loss, r_dz, r_gbi, r_flat, r_out, r = reference(params, k, H, L, loss, bi_d[:, :k], base, y, inv_b)
    assert_live(r, L, "section")
    close(logit.cpu().numpy(), r_out, "logit")
    close(loss_out.item(), r_loss, "loss")
    close(dz.cpu().numpy(), r_dz, "dz")
    close(gbi.cpu().numpy()[:, :k], r_gbi, "gbi")
    assert (gbi.cpu().numpy()[:, k:] == 0).all(), "padding columns of gbi must be zeroed"
    close(grads.cpu().numpy(), r_flat, "flat gradients")
    close_per_tensor(grads.cpu().numpy(), r, k, H, L, B, "gradients")
    assert torch.equal(params, p0), "lr_apply = 0 must leave the parameters alone"
    # determinism + the fused SGD application
    grads2 = torch.zeros_like(params)
    fmx._lib.check(lib.fmx_mlp_section(C.byref(m), fmx._lib.LOSSES[loss], bi_d.data_ptr(), kp, base.data_ptr(), y.data_ptr(), B,
                                       inv_b, ws.data_ptr(), None, dz.data_ptr(), gbi.data_ptr(), kp,
                                       grads2.data_ptr(), 0.25, loss_out.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(grads, grads2), "two runs must give identical bits"
    np.testing.assert_array_equal((p0 - 0.25 * grads).cpu().numpy(), params.cpu().numpy())


def test_mlp_section_rejects_bad_arguments(fmx):
    import ctypes as C
    lib = fmx._lib.load()
    params = torch.zeros(100, device="cuda")
    m = fmx._lib.Mlp(params.data_ptr(), 9, 4, 8, 0)           # too many layers
    assert lib.fmx_mlp_section_workspace_bytes(C.byref(m), 16) < 0
    m = fmx._lib.Mlp(params.data_ptr(), 1, 4, 8, 0)
    x = torch.zeros(64, device="cuda")
    rc = lib.fmx_mlp_section(C.byref(m), fmx._lib.LOSSES["logits"], x.data_ptr(), 2, x.data_ptr(), x.data_ptr(), 4, 0.25,
                             x.data_ptr(), None, x.data_ptr(), x.data_ptr(), 4, x.data_ptr(), 0.0, None, None)
    assert rc == fmx._lib.ERR_SHAPE                                # ld_bi < k


@pytest.mark.parametrize("B,k,kp,H,L", [(4096, 16, 16, 256, 3), (300, 10, 12, 40, 2), (50, 4, 4, 33, 4), (200, 16, 16, 64, 1),
                                        (300, 10, 12, 40, 8), (17, 16, 16, 256, 3)])
def test_mlp_hedge_section_vs_autograd(fmx, B, k, kp, H, L):
    """fmx_mlp_hedge_section against a float64 autograd statement of Hedge backprop (reference deepfm_onn.py:109-154)."""
    import ctypes as C
    torch.manual_seed(B + H)
    n_par = sum(H * (k if l == 0 else H) + H for l in range(L))
    # small enough that sigmoid(base + sum of H activations) stays away from 1.0f: where fp32 saturates, BCELoss clamps
    # log(1 - p) at -100 and a float64 reference (which does not saturate there) stops being a reference
    params = (torch.randn(n_par) * min(1.0 / np.sqrt(H), 2.0 / H)).cuda()
    bi = torch.zeros(B, kp)
    bi[:, :k] = torch.randn(B, k) * 0.5
    params = torch.from_numpy(live_units(params.cpu().numpy(), k, H, L, bi[:, :k].numpy())).cuda()
    bi_d, base = bi.cuda(), (torch.randn(B) * 0.3).cuda()
    y = (torch.rand(B) < 0.3).float().cuda()
    alpha = torch.full((L,), 1.0 / (L + 1)).cuda()
    lr, hb, hs = 0.05, 0.99, 0.2
    a0 = alpha.cpu().numpy().astype(np.float64)
    r = mlp_f64(params.cpu().numpy(), k, H, L, bi[:, :k].numpy(), base.cpu().numpy(), y.cpu().numpy(), hedge_alpha=a0)
    assert_live(r, L, "hedge section")
    p = params.cpu().numpy().astype(np.float64)
    new = p - lr * r["flat"]
    a1 = np.maximum(a0 * hb ** r["losses"], hs / L)
    a1 = a1 / a1.sum()
    lib = fmx._lib.load()
    m = fmx._lib.Mlp(params.data_ptr(), L, k, H, 0)
    ws = torch.empty(int(lib.fmx_mlp_section_workspace_bytes(C.byref(m), B)) // 4, device="cuda")
    grads, lout, p0 = torch.zeros_like(params), torch.zeros(L, device="cuda"), params.clone()
    fmx._lib.check(lib.fmx_mlp_hedge_section(C.byref(m), lr, hb, hs, alpha.data_ptr(), bi_d.data_ptr(), kp, base.data_ptr(),
                                             y.data_ptr(), B, ws.data_ptr(), grads.data_ptr(), lout.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    close(lout.cpu().numpy(), r["losses"], "per-layer losses")
    close(alpha.cpu().numpy(), a1, "alpha")
    close((params - p0).cpu().numpy(), new - p, "parameter deltas", rel=5e-5)
    close_per_tensor(grads.cpu().numpy(), r, k, H, L, B, "hedge gradients")
    np.testing.assert_array_equal((p0 - lr * grads).cpu().numpy(), params.cpu().numpy())



@pytest.mark.parametrize("B,k,ld_bi,H,L", [(4096, 16, 16, 256, 3), (300, 10, 12, 40, 2), (1, 4, 4, 1, 1), (700, 24, 36, 72, 3),
                                           (17, 16, 20, 256, 2)])
def test_mlp_forward_batch_vs_f64(fmx, B, k, ld_bi, H, L):
    """fmx_mlp_forward_batch (forward() / predict() of the MLP classes beyond 16 samples) against float64: the logit and every
    layer's sigmoid, bi rows strided (ld_bi > k) in two cases."""
    import ctypes as C
    torch.manual_seed(B + k + H)
    n_par = sum(H * (k if l == 0 else H) + H for l in range(L))
    params = (torch.randn(n_par) * min(1.0 / np.sqrt(H), 2.0 / H)).cuda()
    bi = torch.zeros(B, ld_bi)
    bi[:, :k] = torch.randn(B, k) * 0.5
    bi[:, k:] = 1e3                                   # columns past k must not be read
    params = torch.from_numpy(live_units(params.cpu().numpy(), k, H, L, bi[:, :k].numpy())).cuda()
    bi_d, base = bi.cuda(), (torch.randn(B) * 0.3).cuda()
    lib = fmx._lib.load()
    m = fmx._lib.Mlp(params.data_ptr(), L, k, H, 0)
    ws = torch.empty(int(lib.fmx_mlp_section_workspace_bytes(C.byref(m), B)) // 4, device="cuda")
    logit, layers = torch.full((B,), 7.0, device="cuda"), torch.full((L, B), 7.0, device="cuda")
    p0 = params.clone()
    fmx._lib.check(lib.fmx_mlp_forward_batch(C.byref(m), bi_d.data_ptr(), ld_bi, base.data_ptr(), B, ws.data_ptr(), logit.data_ptr(),
                                             layers.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    r = mlp_f64(params.cpu().numpy(), k, H, L, bi[:, :k].numpy(), base.cpu().numpy())
    assert np.any(r["out"] != base.cpu().numpy()), "the network must contribute to the logit"
    close(logit.cpu().numpy(), r["out"], "logit")
    for l in range(L):
        close(layers.cpu().numpy()[l], r["layers"][l], f"layers_out[{l}]")
    assert torch.equal(params, p0)
