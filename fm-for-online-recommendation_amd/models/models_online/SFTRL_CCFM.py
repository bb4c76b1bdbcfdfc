"""SFTRL_CCFM -- drop-in for reference models/models_online/SFTRL_CCFM.py:18-121 (sketched FTRL, convex-concave FM).

y_hat = ||BP^T x||^2 - ||BN^T x||^2 (:42-44); the gradient sign s picks the sketch: s <= 0 appends sqrt(-eta s) x to
BP, s > 0 appends sqrt(eta s) x to BN (:77-121).  fp64 like the reference.  device="host" (the default, like the
reference's CPU path; see _sketch.py) or device="gpu": the whole stream in one fmx_sftrl_run launch (include/fmx.h, staged by _device.py;
one wavefront, sketches in LDS, the shrink as a Jacobi eigen-decomposition of B B^T -- same B B^T, predictions and
counts, columns of B up to sign).  The gpu path never falls back: outside the kernel's limits it raises."""
import time

import numpy as np
import torch

from models.models_online import _device
from models.models_online.FM_Base import FM_Base
from models.models_online._sketch import Sketch

Tensor_type = torch.DoubleTensor


class SFTRL_CCFM(FM_Base):
    _linear_term = False

    def __init__(self, inputs_matrix, outputs, task, learning_rate, num_feature, device="host"):
        super(SFTRL_CCFM, self).__init__(inputs_matrix, outputs, task, learning_rate, num_feature)
        self.device = _device.check_device(device)
        self.model_name = "SFTRL_CCFM"
        self.row_count_p = 0
        self.row_count_n = 0
        d = self._sketch_dim()
        self.BT_P = Tensor_type(np.zeros([d, 2 * self.m]))
        self.BT_N = Tensor_type(np.zeros([d, 2 * self.m]))

    def _sketch_dim(self):
        return self.num_feature

    def online_learning(self):
        start = time.time()
        print("==" * 20)
        print(self.model_name + "_" + str(self.eta) + "_" + str(self.m) + "_start")
        if self.task not in ("cls", "reg"):
            raise NotImplementedError
        cls = self.task == "cls"
        X, y = self._stream()
        d = self._sketch_dim()
        if self.device == "gpu":
            preds = self._online_learning_gpu(X, y, d, cls)
            end = time.time()
            print("learning time : %f " % (end - start))
            return preds, y.copy(), (end - start)
        P, N = Sketch(d, self.m, self._thres), Sketch(d, self.m, self._thres)
        P.B, P.count = self.BT_P.numpy().copy(), self.row_count_p
        N.B, N.count = self.BT_N.numpy().copy(), self.row_count_n
        w = g_w = None
        if self._linear_term:
            w, g_w = self.w.numpy().reshape(-1).copy(), self.g_w.numpy().reshape(-1).copy()
        preds = np.empty((self.num_data,) + self._pred_shape(cls), dtype=np.float64)
        for idx in range(self.num_data):
            x = X[idx]
            xs = x[:d]
            scalar = P.energy(xs) - N.energy(xs)
            if self._linear_term:
                scalar += float(w @ x)
            if np.isnan(scalar):
                raise ValueError("Nan contained")
            pred = (1.0 if scalar >= 0 else -1.0) if cls else scalar
            sign = self._grad_loss(scalar, y[idx], cls)
            if self._linear_term:
                g_w += sign * x
                w = -self.eta * g_w
            if sign <= 0:
                P.append(np.sqrt(-self.eta * sign) * xs)
            else:
                N.append(np.sqrt(self.eta * sign) * xs)
            preds[idx] = pred
            if idx % 1000 == 0:
                print(" %d th : pred %f , real %f " % (idx, pred, y[idx]))
        self.BT_P, self.row_count_p = torch.from_numpy(P.B.copy()), P.count
        self.BT_N, self.row_count_n = torch.from_numpy(N.B.copy()), N.count
        if self._linear_term:
            self.w = torch.from_numpy(w.reshape(-1, 1).copy())
            self.g_w = torch.from_numpy(g_w.reshape(-1, 1).copy())
        end = time.time()
        print("learning time : %f " % (end - start))
        return preds, y.copy(), (end - start)

    def _online_learning_gpu(self, X, y, d, cls):
        """The same stream through fmx_sftrl_run; state (sketches, counts, linear term) is read and written back."""
        g = _device.Launch(X, y)
        BP, BN = g.put(self.BT_P), g.put(self.BT_N)
        counts = torch.tensor([self.row_count_p, self.row_count_n], dtype=torch.int32, device=g.dev)
        w, g_w = (g.put(self.w.reshape(-1)), g.put(self.g_w.reshape(-1))) if self._linear_term else (None, None)
        g.call("fmx_sftrl_run", d, self.m, float(self.eta), float(self._thres), 0 if cls else 1, BP, BN, counts, w, g_w)
        _device.check_status(g.host_status(), "fmx_sftrl_run")
        c = counts.cpu()
        self.BT_P, self.row_count_p = BP.cpu(), int(c[0])
        self.BT_N, self.row_count_n = BN.cpu(), int(c[1])
        if self._linear_term:
            self.w, self.g_w = w.cpu().reshape(-1, 1), g_w.cpu().reshape(-1, 1)
        p = g.pred.cpu().numpy()
        _device.print_progress(p, y, False)                          # the device's prediction as it is (+-1 already for cls)
        return p.reshape((g.n,) + self._pred_shape(cls))

    @classmethod
    def grid(cls, inputs_matrix, outputs, task, learning_rates, num_features):
        """An extension the reference lacks (its notebooks try one (learning_rate, m) pair per run): every pair of
        `learning_rates` x `num_features` over the SAME stream in ONE launch (fmx_sftrl_grid: one wavefront per setting,
        up to 256 settings side by side).  -> list of (model, predictions) in the order of itertools.product; every model
        is what `cls(..., lr, m, device="gpu").online_learning()` leaves behind, bit for bit."""
        import itertools
        if task not in ("cls", "reg"):
            raise NotImplementedError
        models = [cls(inputs_matrix, outputs, task, lr, m, device="gpu") for lr, m in itertools.product(learning_rates, num_features)]
        return cls._grid_launch(models, task == "cls") if models else []

    @staticmethod
    def _grid_launch(models, is_cls):
        m0 = models[0]
        g = _device.Launch(*m0._stream(), S=len(models))
        ms = torch.tensor([mdl.m for mdl in models], dtype=torch.int32, device=g.dev)
        etas = torch.tensor([float(mdl.eta) for mdl in models], dtype=torch.float64, device=g.dev)
        BP, BN = g.put(_device.pack_slab([mdl.BT_P for mdl in models])), g.put(_device.pack_slab([mdl.BT_N for mdl in models]))
        counts = torch.tensor([[mdl.row_count_p, mdl.row_count_n] for mdl in models], dtype=torch.int32, device=g.dev)
        w = g_w = None
        if m0._linear_term:
            w, g_w = g.put(_device.pack_slab([mdl.w for mdl in models])), g.put(_device.pack_slab([mdl.g_w for mdl in models]))
        g.call("fmx_sftrl_grid", m0._sketch_dim(), len(models), ms, etas, max(mdl.m for mdl in models), float(m0._thres), 0 if is_cls else 1,
               BP, BN, counts, w, g_w)
        _device.check_status(g.host_status(), "fmx_sftrl_grid", "num_feature")
        ch, ph = counts.cpu(), g.pred.cpu().numpy()
        BPs, BNs = (_device.unpack_slab(B.cpu(), [mdl.BT_P.shape for mdl in models]) for B in (BP, BN))
        if m0._linear_term:
            ws, g_ws = (_device.unpack_slab(t.cpu(), [mdl.w.shape for mdl in models]) for t in (w, g_w))
        out = []
        for s, mdl in enumerate(models):
            mdl.BT_P, mdl.BT_N, mdl.row_count_p, mdl.row_count_n = BPs[s], BNs[s], int(ch[s, 0]), int(ch[s, 1])
            if m0._linear_term:
                mdl.w, mdl.g_w = ws[s], g_ws[s]
            out.append((mdl, ph[s].reshape((g.n,) + mdl._pred_shape(is_cls))))
        return out

    def _pred_shape(self, cls):
        return (1,) if cls else ()
