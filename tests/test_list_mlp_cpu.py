"""tests/list_mlp_f64.py -- the float64 reference of the list (sampled-softmax) loss on the whole network's logit of DeepFM / NFM --
against a direct float64 autograd of the same objective and against tests/pair_mlp_f64.py at G = 2, where the two losses coincide.
No device is touched."""
import numpy as np
import torch


def _small(rng, k, H, L, N):
    n_par = sum(H * (k if l == 0 else H) + H for l in range(L))
    return (rng.normal(0, 0.5, n_par).astype(np.float32), rng.normal(0, 0.7, (N, k)).astype(np.float32),
            rng.normal(0, 0.5, N).astype(np.float32))


def test_list_mlp_f64_is_the_autograd():
    from list_mlp_f64 import list_mlp_f64
    k, H, L, G, B = 4, 5, 2, 3, 4
    params, bi, base = _small(np.random.default_rng(29), k, H, L, B * G)
    inv_b = 1.0 / B
    r = list_mlp_f64(params, k, H, L, bi, base, G, inv_b)

    p = torch.tensor(params, dtype=torch.float64, requires_grad=True)
    x0 = torch.tensor(bi, dtype=torch.float64, requires_grad=True)
    b0 = torch.tensor(base, dtype=torch.float64, requires_grad=True)
    x, off = x0, 0
    for l in range(L):
        i = k if l == 0 else H
        W, b = p[off:off + H * i].view(H, i), p[off + H * i:off + H * i + H]
        x = torch.relu(x @ W.t() + b)
        off += H * i + H
    z = (b0 + x.sum(1)).view(B, G)
    loss = (torch.logsumexp(z, dim=1) - z[:, 0]).sum() * inv_b             # the objective, stated another way
    loss.backward()
    assert abs(r["loss"] - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
    np.testing.assert_allclose(r["out"], z.detach().numpy().reshape(-1), rtol=1e-12, atol=0.0)
    for name, got, want in (("dz", r["dz"], b0.grad.numpy()), ("gbi", r["gbi"], x0.grad.numpy()), ("flat", r["flat"], p.grad.numpy())):
        np.testing.assert_allclose(got, want, rtol=1e-11, atol=1e-12 * np.abs(want).max(), err_msg=name)
    assert np.abs(r["dz"].reshape(B, G).sum(1)).max() <= 1e-15 and (r["dz"].reshape(B, G)[:, 0] < 0).all()
    assert np.any(p.grad.numpy()) and np.any(x0.grad.numpy())
    off = 0
    for l in range(L):                                                     # the per-layer views are the flat layout
        i = k if l == 0 else H
        np.testing.assert_array_equal(r["grads"][l][0].reshape(-1), r["flat"][off:off + H * i])
        np.testing.assert_array_equal(r["grads"][l][1], r["flat"][off + H * i:off + H * i + H])
        for nz in r["gnoise"][l]:
            assert (nz >= 0).all() and np.isfinite(nz).all()
        assert r["gnoise"][l][0].shape == (H, i)
        off += H * i + H
    for name in ("dz_noise", "logit_noise"):
        assert r[name].shape == (B * G,) and (r[name] > 0).all() and np.isfinite(r[name]).all()
    assert r["gbi_noise"].shape == (B * G, k) and np.isfinite(r["gbi_noise"]).all()


def test_list_mlp_f64_at_two_rows_is_the_pair_helper():
    """G = 2: -log softmax(z)[0] = -log sigmoid(z_0 - z_1), the pair loss under margin 0"""
    from list_mlp_f64 import list_mlp_f64
    from pair_mlp_f64 import pair_mlp_f64
    k, H, L, B = 5, 7, 3, 6
    params, bi, base = _small(np.random.default_rng(31), k, H, L, 2 * B)
    a = list_mlp_f64(params, k, H, L, bi, base, 2, 1.0 / B)
    b = pair_mlp_f64(params, k, H, L, bi, base, 0.0, 1.0 / B)
    assert abs(a["loss"] - b["loss"]) <= 1e-12 * abs(b["loss"])
    np.testing.assert_allclose(a["loss_i"], b["loss_i"], rtol=1e-12, atol=1e-15)
    for name in ("out", "dz", "gbi", "flat"):
        np.testing.assert_allclose(a[name], b[name], rtol=1e-11, atol=1e-13 * np.abs(b[name]).max(), err_msg=name)
