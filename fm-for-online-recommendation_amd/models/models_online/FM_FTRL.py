"""FM_FTRL -- drop-in for reference models/models_online/FM_FTRL.py:27-92 (hot path B, fp64).

Per sample x (a column of At):  y_hat = w1^T x + ||W2 x'||^2 with x' = x without its last feature (:61-63);
cumulative gradients g_w1 += s x, g_W2 += 2 W2 x' x'^T -- without the factor s, a reference quirk kept here (:76-77);
then w1 = -eta g_w1, W2 = -eta g_W2 (:79-80).  device="host" (the default, like the reference's CPU path): the loop runs
in numpy fp64 (one matvec and one rank-1 update per sample instead of the reference's two matmuls).  device="gpu": the
same draws, then the whole stream in one fmx_ftrl_dense_run launch (include/fmx.h: one wavefront, g_W2 in LDS) -- same
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

from models.models_online.FM_Base import FM_Base

Tensor_type = torch.DoubleTensor
numpy_type = np.float64

GRID_MAX_SETTINGS = 256      # settings per launch: one workgroup each, one per CU of an MI355X


class FM_FTRL(FM_Base):
    def __init__(self, inputs_matrix, outputs, task, learning_rate, num_feature, device="host"):
        super(FM_FTRL, self).__init__(inputs_matrix, outputs, task, learning_rate, num_feature)
        if device not in ("host", "gpu"):
            raise ValueError("device must be 'host' or 'gpu'")
        self.device = device
        self.model_name = "FM_FTRL"

    def _init_parameter(self):
        """randn init in the reference's draw order (:42-43)"""
        self.w1 = torch.randn(self.num_feature, 1).type(Tensor_type)
        self.W2 = torch.randn(2 * self.m, self.num_feature - 1).type(Tensor_type)

    def _stream(self):
        X = self.At.t().contiguous().numpy().astype(numpy_type, copy=False)      # [N, d]
        y = np.asarray(self.b.reshape(-1).numpy(), dtype=numpy_type)
        return X, y

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
            if cls:
                pred = 1.0 if scalar >= 0 else -1.0
                sign_idx = (-1.0 / (1.0 + np.exp(scalar * y[idx]))) * y[idx]
            else:
                pred = scalar
                sign_idx = 2.0 * (scalar - y[idx])
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
        import ctypes as C

        from fmx import _lib
        lib = _lib.load()
        dev = torch.device("cuda", torch.cuda.current_device())
        n, D = X.shape
        Xd, yd = torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev)
        w1, W2 = self.w1.reshape(-1).to(dev).contiguous(), self.W2.to(dev).contiguous()
        g_w1, g_W2 = torch.zeros_like(w1), torch.zeros_like(W2)
        pred = torch.empty(n, dtype=torch.float64, device=dev)
        status = torch.zeros(2, dtype=torch.int32, device=dev)
        ptr = lambda t: C.c_void_p(t.data_ptr())
        _lib.check(lib.fmx_ftrl_dense_run(ptr(Xd), ptr(yd), n, D, 2 * self.m, float(self.eta), 0 if cls else 1, ptr(w1), ptr(W2),
                                          ptr(g_w1), ptr(g_W2), ptr(pred), ptr(status),
                                          C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        st = status.cpu()
        n_ok = int(st[1]) if int(st[0]) == 1 else n                # samples in front of a NaN prediction
        self.y_hat = pred.cpu().numpy()
        p = self._shape_predictions(self.y_hat, cls)
        for idx in range(0, n_ok, 1000):                             # the host loop's lines, up to where it would have raised
            print(" %d th : pred %f , real %f " % (idx, p[idx].item(), y[idx]))
        if n_ok < n:
            raise ValueError("Nan contained")
        self.w1, self.W2 = w1.cpu().reshape(-1, 1), W2.cpu()
        return p

    @classmethod
    def grid(cls, inputs_matrix, outputs, task, learning_rates, num_features, device="gpu"):
        """An extension the reference lacks (its notebooks run one (learning_rate, m) pair per object): every pair of
        `learning_rates` x `num_features` over the SAME stream -> list of (model, predictions) in the order of
        itertools.product.  Each setting's parameters are drawn from the global torch RNG in that order: what that many
        consecutive single runs would draw.  device="gpu": fmx_ftrl_dense_grid, one wavefront per setting, at most 256
        settings per launch; every model is what `cls(..., lr, m, device="gpu").online_learning()` leaves behind, bit for
        bit.  device="host": the same settings one after another through the host loop (prints included)."""
        import itertools
        if device not in ("host", "gpu"):
            raise ValueError("device must be 'host' or 'gpu'")
        if task not in ("cls", "reg"):
            raise NotImplementedError
        settings = list(itertools.product(learning_rates, num_features))
        models = [cls(inputs_matrix, outputs, task, lr, m, device=device) for lr, m in settings]
        if device == "host":
            return [(mdl, mdl.online_learning()[0]) for mdl in models]
        for mdl in models:
            mdl._init_parameter()
        out = []
        for lo in range(0, len(models), GRID_MAX_SETTINGS):
            out.extend(cls._grid_launch(models[lo:lo + GRID_MAX_SETTINGS], task == "cls"))
        return out

    @staticmethod
    def _grid_launch(models, is_cls):
        import ctypes as C

        from fmx import _lib
        lib = _lib.load()
        dev = torch.device("cuda", torch.cuda.current_device())
        X, y = models[0]._stream()
        n, D = X.shape
        S, m2_max = len(models), max(2 * mdl.m for mdl in models)
        Xd, yd = torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev)
        m2s = torch.tensor([2 * mdl.m for mdl in models], dtype=torch.int32, device=dev)
        etas = torch.tensor([float(mdl.eta) for mdl in models], dtype=torch.float64, device=dev)
        w1_h = torch.stack([mdl.w1.reshape(-1) for mdl in models])
        W2_h = torch.zeros((S, m2_max * (D - 1)), dtype=torch.float64)
        for s, mdl in enumerate(models):
            W2_h[s, :2 * mdl.m * (D - 1)] = mdl.W2.reshape(-1)
        w1, W2 = w1_h.to(dev).contiguous(), W2_h.to(dev)
        g_w1, g_W2 = torch.zeros_like(w1), torch.zeros_like(W2)
        pred = torch.empty((S, n), dtype=torch.float64, device=dev)
        status = torch.zeros((S, 2), dtype=torch.int32, device=dev)
        ptr = lambda t: C.c_void_p(t.data_ptr())
        _lib.check(lib.fmx_ftrl_dense_grid(ptr(Xd), ptr(yd), n, D, S, ptr(m2s), ptr(etas), m2_max, 0 if is_cls else 1, ptr(w1), ptr(W2),
                                           ptr(g_w1), ptr(g_W2), ptr(pred), ptr(status),
                                           C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        st_h = status.cpu()
        if bool((st_h[:, 0] == 2).any()):
            raise ValueError("a setting's num_feature lies outside [1, max]: not run (fmx_ftrl_dense_grid status 2)")
        if bool((st_h[:, 0] == 1).any()):
            raise ValueError("Nan contained")
        w1_o, W2_o, ph = w1.cpu(), W2.cpu(), pred.cpu().numpy()
        out = []
        for s, mdl in enumerate(models):
            mdl.w1 = w1_o[s].reshape(-1, 1).clone()
            mdl.W2 = W2_o[s, :2 * mdl.m * (D - 1)].reshape(2 * mdl.m, D - 1).clone()
            mdl.y_hat = ph[s].copy()
            out.append((mdl, mdl._shape_predictions(mdl.y_hat, is_cls)))
        return out
