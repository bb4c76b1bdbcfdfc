"""FM_Base -- drop-in for reference models/models_online/FM_Base.py:15-69 (hot path B, fp64, host side).

Path B is strictly sequential (each prediction depends on the previous update) on d = 8 features, so the default of
every class is the host, like the reference's own CPU path (BASELINE.json configs[0]: "plumbing only").  All four
learners of the family (FM_FTRL, SFTRL_CCFM, SFTRL_Vanila, RRF_Online) also take device="gpu": the whole stream in one
launch, one wavefront per stream (include/fmx.h: fmx_ftrl_dense_run, fmx_sftrl_run, fmx_rrf_run; the host glue around those
calls, shared by the four classes, is _device.py).  Measured on an MI355X at 8
features (profiles/path_b_times.json): one FM_FTRL / RRF_Online stream runs at 1.0-1.7 us per sample on the
device against 5-10 on the host; the sketch classes, whose shrink is a Jacobi eigen-decomposition on one wavefront, at 13-66 against
8.  The classes' grid() classmethods run many settings over one device-resident stream side by side: 256 settings take about
the time of a few, 290-380 times the host running them one after another.
"""
import numpy as np
import torch
from torch.nn import Module

from models.models_online import _device

tensor_type = torch.DoubleTensor


class FM_Base(Module):
    def __init__(self, inputs_matrix, outputs, task, learning_rate, feature_m):
        super(FM_Base, self).__init__()
        self.At = inputs_matrix.t()          # [d, N]: column idx is sample idx (reference :21)
        self.b = outputs
        self._thres = 1e-12
        self.num_data = inputs_matrix.shape[0]
        self.num_feature = inputs_matrix.shape[1]
        self.task = task
        self.eta = learning_rate
        self.m = feature_m

    def _stream(self):
        """-> the stream as contiguous fp64 numpy, X [N, d] and y [N]"""
        return _device.host_stream(self.At.t(), self.b)

    @staticmethod
    def _grad_loss(scalar, y, cls):
        """d loss / d y_hat of the numpy host loops: cls (-1 / (1 + e^(s y))) y, reg 2 (s - y)   (reference :44-51 applied as in
        FM_FTRL.py:69, SFTRL_CCFM.py:50)"""
        return (-1.0 / (1.0 + np.exp(scalar * y))) * y if cls else 2.0 * (scalar - y)

    def online_learning(self, logger=None):
        raise NotImplementedError
