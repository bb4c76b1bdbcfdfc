"""RRF_Online -- drop-in for reference models/models_online/RRF_Online.py:18-187 (reparameterised random Fourier
features, online).  phi(x) = [cos, sin](x (e^gamma * eps)) (:70-75); SGD on w and gamma with the reference's gradient
formulas (:88-123), including its `lr_w * exp(w)` term in d_w (:97) and, for the logit loss, the per-batch softmax
weight that equals 1 at batch size 1 (:101-102).  fp64.  device="host" (the default, like the reference's CPU path) runs
the loop in numpy; device="gpu" runs the whole stream in one fmx_rrf_run launch (include/fmx.h: one wavefront, eps in
LDS; staging, slabs and progress lines: _device.py): same return triple and prints, NaN samples dropped from pred and real as the
host loop drops them.  The device's exp / sin / cos differ from the host's in the last place and this model's dynamics amplify that (tests/golden/
make_golden.py pins 100 steps for that reason): agreement is to a tolerance, not to the bit (measured: 6e-16 of the largest
magnitude over the fixtures; profiles/path_b_times.json).  Measured at 8 features, 6 spectral samples, 4,000 samples on an MI355X:
1.6-1.7 us per sample, copies included, against the host loop's 9.6-9.7; RRF_Online.grid -- many (lr_w, lr_gamma, spectral
samples) settings over one device-resident stream side by side -- runs 256 settings x 3,000 samples in 21 ms, 380 times the host
running them one after another.  The gpu path never falls back:
outside the kernel's limits (features <= 64, spectral samples <= 64) it raises.  After a run `y_hat` holds the raw scores [N]
on either device, NaN where a sample was skipped."""
import time

import numpy as np
import torch
from torch.nn import Module

from models.models_online import _device

Tensor_type = torch.DoubleTensor


class RRF_Online(Module):
    def __init__(self, inputs_matrix, outputs, task, loss_type=None, gamma=None, w=None, num_sampled_spectral=10,
                 random_seed=100, lr_RRF_w=0.05, lr_RRF_gamma=0.05, device="host"):
        super(RRF_Online, self).__init__()
        self.device = _device.check_device(device)
        self.X = inputs_matrix
        self.Y = outputs
        self.loss_type = loss_type
        self.num_feature = inputs_matrix.shape[1]
        self.model_name = "RRF_Online"
        self.task = task
        self.num_sampled_spectral = num_sampled_spectral
        self.lr_RRF_w = lr_RRF_w
        self.lr_RRF_gamma = lr_RRF_gamma
        self.random_seed = random_seed
        self._init_param(gamma, w, loss_type)

    def _init_param(self, gamma, w, loss_type):
        """Draw order of the reference (:47-67): numpy rand for gamma, then torch randn for w and for eps."""
        if self.task == "cls":
            self.loss_type = "logit" if loss_type is None else "hinge"
        elif self.task == "reg":
            self.loss_type = "l2" if loss_type is None else "l1"
        else:
            raise NotImplementedError("wrong task assigned")
        if gamma is None:
            self.gamma = Tensor_type(np.log(np.random.rand(self.num_feature, 1)))
        else:
            self.gamma = Tensor_type(np.log(gamma) * np.ones((self.num_feature, 1)))
        self.w = 0.1 * torch.randn(2 * self.num_sampled_spectral).type(Tensor_type) if w is None else w
        self.eps = torch.randn(self.num_feature, self.num_sampled_spectral).type(Tensor_type)

    def _compute_phi(self, x_t):
        z = x_t.matmul(self.gamma.exp().mul(self.eps))
        return torch.cat([z.cos(), z.sin()], 1)

    def _predict(self, phi):
        return phi.matmul(self.w)

    def online_learning(self):
        start = time.time()
        print("==" * 20)
        if self.loss_type not in ("logit", "l2"):
            raise NotImplementedError("wrong loss type in get_grad")
        X, Y = _device.host_stream(self.X, self.Y)
        gamma = self.gamma.numpy().reshape(-1).copy()
        w = self.w.numpy().copy()
        eps = self.eps.numpy()
        D = self.num_sampled_spectral
        cls = self.task == "cls"
        if self.device == "gpu":
            pred, real = self._online_learning_gpu(X, Y, cls)
            end = time.time()
            print("learning time : %f " % (end - start))
            return pred, real, (end - start)
        pred_list, real_list = [], []
        self.y_hat = np.empty(X.shape[0], dtype=np.float64)
        for t in range(X.shape[0]):
            x, y = X[t], Y[t]
            eg = np.exp(gamma)
            z = x @ (eg[:, None] * eps)
            cz, sz = np.cos(z), np.sin(z)
            phi = np.concatenate([cz, sz])
            scalar = float(phi @ w)
            self.y_hat[t] = scalar
            if not np.isnan(scalar):
                coef = -y if self.loss_type == "logit" else (scalar - y)     # logit: -y * softmax over a batch of 1
                d_w = self.lr_RRF_w * np.exp(w) + coef * phi
                d_phi = coef * w
                # d phi / d gamma_n: -x_n eps_nd sin(z_d) e^gamma_n for the cos half, +x_n eps_nd cos(z_d) e^gamma_n for sin
                d_gamma = (x[:, None] * eps * (-sz * d_phi[:D] + cz * d_phi[D:])[None, :]).sum(axis=1) * eg
                w = w - self.lr_RRF_w * d_w
                gamma = gamma - self.lr_RRF_gamma * d_gamma
                pred_list.append([1.0 if scalar >= 0 else -1.0] if cls else [scalar])
                real_list.append(y)
            if t % 1000 == 0:
                print(" %d th : pred %f , real %f " % (t, (1.0 if scalar >= 0 else -1.0) if cls and not np.isnan(scalar)
                                                     else scalar, y))
        self.w = torch.from_numpy(w.copy())
        self.gamma = torch.from_numpy(gamma.reshape(-1, 1).copy())
        end = time.time()
        print("learning time : %f " % (end - start))
        return np.asarray(pred_list, dtype=np.float64), np.asarray(real_list, dtype=np.float64), (end - start)

    @staticmethod
    def _kept(scalars, Y, cls):
        """raw y_hat [N] (NaN: a skipped sample) -> (pred [n_kept, 1], real [n_kept]) as the host loop collects them"""
        keep = ~np.isnan(scalars)
        kept = scalars[keep]
        pred = (np.where(kept >= 0, 1.0, -1.0) if cls else kept).reshape(-1, 1)
        return np.asarray(pred, dtype=np.float64), np.asarray(Y[keep], dtype=np.float64)

    def _online_learning_gpu(self, X, Y, cls):
        """The same stream through fmx_rrf_run; gamma and w are read and written back."""
        g = _device.Launch(X, Y)
        eps, gamma, w = g.put(self.eps), g.put(self.gamma.reshape(-1)), g.put(self.w)
        g.call("fmx_rrf_run", self.num_sampled_spectral, float(self.lr_RRF_w), float(self.lr_RRF_gamma),
               0 if self.loss_type == "logit" else 1, eps, gamma, w)
        scalars = self.y_hat = g.pred.cpu().numpy()
        self.w, self.gamma = w.cpu(), gamma.cpu().reshape(-1, 1)
        _device.print_progress(scalars, Y, cls)
        return self._kept(scalars, Y, cls)

    @classmethod
    def grid(cls, inputs_matrix, outputs, task, lr_ws, lr_gammas, num_sampled_spectrals, loss_type=None, device="gpu"):
        """An extension the reference lacks (one setting per object there): every triple of `lr_ws` x `lr_gammas` x
        `num_sampled_spectrals` over the SAME stream -> list of (model, predictions) in the order of itertools.product.
        The models are constructed in that order, so each draws (numpy rand for gamma, torch randn for w and eps) what
        that many consecutive single runs would draw.  device="gpu": fmx_rrf_grid, one wavefront per setting, split into
        launches of at most 256 settings; every model is what its own device="gpu" run leaves behind, bit for bit.
        device="host": the same settings one after another through the host loop (prints included)."""
        import itertools
        _device.check_device(device)
        settings = list(itertools.product(lr_ws, lr_gammas, num_sampled_spectrals))
        models = [cls(inputs_matrix, outputs, task, loss_type=loss_type, num_sampled_spectral=ds, lr_RRF_w=lw, lr_RRF_gamma=lg,
                      device=device) for lw, lg, ds in settings]
        if models and models[0].loss_type not in ("logit", "l2"):
            raise NotImplementedError("wrong loss type in get_grad")
        if device == "host":
            return [(mdl, mdl.online_learning()[0]) for mdl in models]
        return [r for part in _device.launches(models) for r in cls._grid_launch(part)]

    @staticmethod
    def _grid_launch(models):
        m0 = models[0]
        X, Y = _device.host_stream(m0.X, m0.Y)
        g = _device.Launch(X, Y, S=len(models))
        dss = torch.tensor([mdl.num_sampled_spectral for mdl in models], dtype=torch.int32, device=g.dev)
        lws = torch.tensor([float(mdl.lr_RRF_w) for mdl in models], dtype=torch.float64, device=g.dev)
        lgs = torch.tensor([float(mdl.lr_RRF_gamma) for mdl in models], dtype=torch.float64, device=g.dev)
        eps, gamma, w = (g.put(_device.pack_slab([getattr(mdl, name) for mdl in models])) for name in ("eps", "gamma", "w"))
        g.call("fmx_rrf_grid", len(models), dss, lws, lgs, max(mdl.num_sampled_spectral for mdl in models),
               0 if m0.loss_type == "logit" else 1, eps, gamma, w)
        _device.check_status(g.host_status(), "fmx_rrf_grid", "num_sampled_spectral")
        ph = g.pred.cpu().numpy()
        ws = _device.unpack_slab(w.cpu(), [mdl.w.shape for mdl in models])
        gammas = _device.unpack_slab(gamma.cpu(), [mdl.gamma.shape for mdl in models])
        out = []
        for s, mdl in enumerate(models):
            mdl.w, mdl.gamma, mdl.y_hat = ws[s], gammas[s], ph[s].copy()
            out.append((mdl, mdl._kept(mdl.y_hat, Y, mdl.task == "cls")[0]))
        return out
