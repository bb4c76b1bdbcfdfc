"""FM_FTRL -- drop-in for reference models/models_online/FM_FTRL.py:27-92 (hot path B, fp64).

Per sample x (a column of At):  y_hat = w1^T x + ||W2 x'||^2 with x' = x without its last feature (:61-63);
cumulative gradients g_w1 += s x, g_W2 += 2 W2 x' x'^T -- without the factor s, a reference quirk kept here (:76-77);
then w1 = -eta g_w1, W2 = -eta g_W2 (:79-80).  device="host" (the default, like the reference's CPU path): the loop runs
in numpy fp64 (one matvec and one rank-1 update per sample instead of the reference's two matmuls).  device="gpu": the
same draws, then the whole stream in one fmx_ftrl_dense_run launch (include/fmx.h: one wavefront, g_W2 in LDS; staging, slabs
and progress lines: _device.py) -- same
return value and prints, predictions and weights equal to the host's up to the order of the fp64 sums (measured: 7e-16 of the
largest magnitude; profiles/path_b_times.json).  Measured at 8 features, m = 8, 4,000 samples on an MI355X: 1.0-1.1 us per sample,
copies included, against the host loop's 5.3-6.6; FM_FTRL.grid -- many settings walking one device-resident stream side by side --
runs 256 settings x 3,000 samples in 16 ms, 290 times the host running them one after another.  The gpu path never falls back:
outside the kernel's limits (features <= 64, 2 m <= 128) it raises.  After a run `y_hat` holds the raw scores [N] on either device
(for cls the returned predictions are their signs).
"""
import time

import numpy as np
import torch

from models.models_online import _device
from models.models_online.FM_Base import FM_Base

Tensor_type = torch.DoubleTensor
numpy_type = np.float64


class FM_FTRL(FM_Base):
    def __init__(self, inputs_matrix, outputs, task, learning_rate, num_feature, device="host"):
        super(FM_FTRL, self).__init__(inputs_matrix, outputs, task, learning_rate, num_feature)
        self.device = _device.check_device(device)
        self.model_name = "FM_FTRL"

    def _init_parameter(self):
        """randn init in the reference's draw order (:42-43)"""
        self.w1 = torch.randn(self.num_feature, 1).type(Tensor_type)
        self.W2 = torch.randn(2 * self.m, self.num_feature - 1).type(Tensor_type)

    def _shape_predictions(self, scalars, cls):
        """raw y_hat [N] -> what online_learning returns: (N, 1) of +-1 for cls, (N, 1, 1) for reg"""
        if cls:
            return np.where(scalars >= 0, 1.0, -1.0).reshape(-1, 1)
        return scalars.reshape(-1, 1, 1).copy()

    def online_learning(self):
        start = time.time()
        self._init_parameter()
        print(self.model_name + "_" + str(self.eta) + "_" + str(self.m) + "_start")
        if self.task not in ("cls", "reg"):
            raise NotImplementedError
        cls = self.task == "cls"
        X, y = self._stream()
        if self.device == "gpu":
            pred_list = self._online_learning_gpu(X, y, cls)
            end = time.time()
            print("learning time : %f " % (end - start))
            return pred_list, y.copy(), (end - start)
        w1 = self.w1.numpy().reshape(-1).copy()
        W2 = self.W2.numpy().copy()
        g_w1 = np.zeros_like(w1)
        g_W2 = np.zeros_like(W2)
        eta = self.eta
        pred_list = np.empty((self.num_data, 1) if cls else (self.num_data, 1, 1), dtype=numpy_type)
        self.y_hat = np.empty(self.num_data, dtype=numpy_type)
        for idx in range(self.num_data):
            x = X[idx]
            xs = x[:-1]
            t = W2 @ xs
            scalar = w1 @ x + t @ t
            if np.isnan(scalar):
                raise ValueError("Nan contained")
            pred = (1.0 if scalar >= 0 else -1.0) if cls else scalar
            sign_idx = self._grad_loss(scalar, y[idx], cls)
            g_w1 += sign_idx * x
            g_W2 += 2.0 * np.outer(t, xs)
            w1 = -eta * g_w1
            W2 = -eta * g_W2
            pred_list[idx] = pred
            self.y_hat[idx] = scalar
            if idx % 1000 == 0:
                print(" %d th : pred %f , real %f " % (idx, pred, y[idx]))
        self.w1 = torch.from_numpy(w1.reshape(-1, 1).copy())
        self.W2 = torch.from_numpy(W2.copy())
        end = time.time()
        print("learning time : %f " % (end - start))
        return pred_list, y.copy(), (end - start)

    def _online_learning_gpu(self, X, y, cls):
        """The same stream through fmx_ftrl_dense_run, from the parameters just drawn and zero cumulative gradients."""
        g = _device.Launch(X, y)
        w1, W2 = g.put(self.w1.reshape(-1)), g.put(self.W2)
        g_w1, g_W2 = torch.zeros_like(w1), torch.zeros_like(W2)
        g.call("fmx_ftrl_dense_run", 2 * self.m, float(self.eta), 0 if cls else 1, w1, W2, g_w1, g_W2)
        st = g.host_status()
        n_ok = int(st[0, 1]) if int(st[0, 0]) == 1 else g.n          # samples in front of a NaN prediction
        self.y_hat = g.pred.cpu().numpy()
        _device.print_progress(self.y_hat, y, cls, n_ok)             # the host loop's lines, up to where it would have raised
        _device.check_status(st, "fmx_ftrl_dense_run")
        self.w1, self.W2 = w1.cpu().reshape(-1, 1), W2.cpu()
        return self._shape_predictions(self.y_hat, cls)

    @classmethod
    def grid(cls, inputs_matrix, outputs, task, learning_rates, num_features, device="gpu"):
        """An extension the reference lacks (its notebooks run one (learning_rate, m) pair per object): every pair of
        `learning_rates` x `num_features` over the SAME stream -> list of (model, predictions) in the order of
        itertools.product.  Each setting's parameters are drawn from the global torch RNG in that order: what that many
        consecutive single runs would draw.  device="gpu": fmx_ftrl_dense_grid, one wavefront per setting, at most 256
        settings per launch; every model is what `cls(..., lr, m, device="gpu").online_learning()` leaves behind, bit for
        bit.  device="host": the same settings one after another through the host loop (prints included)."""
        import itertools
        _device.check_device(device)
        if task not in ("cls", "reg"):
            raise NotImplementedError
        settings = list(itertools.product(learning_rates, num_features))
        models = [cls(inputs_matrix, outputs, task, lr, m, device=device) for lr, m in settings]
        if device == "host":
            return [(mdl, mdl.online_learning()[0]) for mdl in models]
        for mdl in models:
            mdl._init_parameter()
        return [r for part in _device.launches(models) for r in cls._grid_launch(part, task == "cls")]

    @staticmethod
    def _grid_launch(models, is_cls):
        g = _device.Launch(*models[0]._stream(), S=len(models))
        m2s = torch.tensor([2 * mdl.m for mdl in models], dtype=torch.int32, device=g.dev)
        etas = torch.tensor([float(mdl.eta) for mdl in models], dtype=torch.float64, device=g.dev)
        w1, W2 = g.put(_device.pack_slab([mdl.w1 for mdl in models])), g.put(_device.pack_slab([mdl.W2 for mdl in models]))
        g_w1, g_W2 = torch.zeros_like(w1), torch.zeros_like(W2)
        g.call("fmx_ftrl_dense_grid", len(models), m2s, etas, max(2 * mdl.m for mdl in models), 0 if is_cls else 1, w1, W2, g_w1, g_W2)
        _device.check_status(g.host_status(), "fmx_ftrl_dense_grid", "num_feature")
        ph = g.pred.cpu().numpy()
        w1s = _device.unpack_slab(w1.cpu(), [mdl.w1.shape for mdl in models])
        W2s = _device.unpack_slab(W2.cpu(), [mdl.W2.shape for mdl in models])
        out = []
        for s, mdl in enumerate(models):
            mdl.w1, mdl.W2, mdl.y_hat = w1s[s], W2s[s], ph[s].copy()
            out.append((mdl, mdl._shape_predictions(mdl.y_hat, is_cls)))
        return out
