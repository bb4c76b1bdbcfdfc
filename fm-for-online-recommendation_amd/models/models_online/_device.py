"""Host glue shared by the path B classes (FM_FTRL, SFTRL_CCFM, SFTRL_Vanila, RRF_Online) around their device path: the `device`
keyword, the stream as fp64 numpy, what one library call needs staged on the device (`Launch`), the [S, width_max] slabs a grid
keeps its settings' parameters in, and the progress lines.  Each class builds its own state tensors, makes one call through
`Launch.call` and writes the state back; the kernels and their C ABI are csrc/fmx_sftrl.hip and include/fmx.h.
"""
import math

import numpy as np
import torch

GRID_MAX_SETTINGS = 256      # settings per launch: one workgroup each, one per CU of an MI355X


def check_device(device):
    if device not in ("host", "gpu"):
        raise ValueError("device must be 'host' or 'gpu'")
    return device


def launches(models):
    """a grid's models in launches of at most GRID_MAX_SETTINGS"""
    return [models[lo:lo + GRID_MAX_SETTINGS] for lo in range(0, len(models), GRID_MAX_SETTINGS)]


def host_stream(inputs, outputs):
    """inputs [N, D] and outputs (N elements) as torch tensors -> contiguous fp64 numpy [N, D] and [N], what the host loops walk
    and the device paths stage"""
    X = np.ascontiguousarray(inputs.numpy().astype(np.float64, copy=False))
    return X, np.asarray(outputs.reshape(-1).numpy(), dtype=np.float64)


def pack_slab(tensors):
    """per-setting tensors of different sizes -> zero-filled [S, width_max] fp64 slab on the host, row s = tensors[s] flattened"""
    slab = torch.zeros((len(tensors), max(t.numel() for t in tensors)), dtype=torch.float64)
    for s, t in enumerate(tensors):
        slab[s, :t.numel()] = t.reshape(-1)
    return slab


def unpack_slab(slab, shapes):
    """-> row s of a host slab cut to its own width and reshaped to shapes[s], as a copy that owns its memory"""
    return [slab[s, :math.prod(shape)].reshape(shape).clone() for s, shape in enumerate(shapes)]


def print_progress(scores, real, cls, n=None):
    """The host loops' line for every 1000th of the first n samples (default: all), from raw scores: cls prints the sign, +-1, but a
    NaN score as it is."""
    for idx in range(0, len(scores) if n is None else n, 1000):
        s = scores[idx]
        print(" %d th : pred %f , real %f " % (idx, (1.0 if s >= 0 else -1.0) if cls and not np.isnan(s) else s, real[idx]))


class Launch:
    """What one path B library call needs on the current device: the stream X [N, D], y [N]; pred and status for S settings ([S, n]
    and [S, 2]) or, without S, for a single run ([n] and [2]); the library and torch's current stream.  The library declares every
    pointer parameter as c_void_p, so data_ptr() and None pass as they are."""

    def __init__(self, X, y, S=None):
        from fmx import _lib                      # lazy: the host paths and an empty grid need neither the library nor a device
        self._lib, self.lib = _lib, _lib.load()
        self.dev = torch.device("cuda", torch.cuda.current_device())
        self.n, self.D = X.shape
        self.Xd, self.yd = torch.from_numpy(X).to(self.dev), torch.from_numpy(y).to(self.dev)
        lead = () if S is None else (S,)
        self.pred = torch.empty(lead + (self.n,), dtype=torch.float64, device=self.dev)
        self.status = torch.zeros(lead + (2,), dtype=torch.int32, device=self.dev)

    def put(self, t):
        """a host tensor -> contiguous on the device"""
        return t.to(self.dev).contiguous()

    def call(self, entry, *args):
        """lib.<entry>(X, y, N, D, *args, pred, status, stream), tensors among args by their data_ptr(); raises FmxError on a refusal"""
        ptrs = [a.data_ptr() if torch.is_tensor(a) else a for a in args]
        self._lib.check(getattr(self.lib, entry)(self.Xd.data_ptr(), self.yd.data_ptr(), self.n, self.D, *ptrs, self.pred.data_ptr(),
                                                 self.status.data_ptr(), torch.cuda.current_stream(self.dev).cuda_stream))

    def host_status(self):
        """-> status on the host as [S, 2] (a single run: [1, 2])"""
        return self.status.cpu().reshape(-1, 2)


def check_status(st, entry, knob=None):
    """Status codes of the FM_FTRL and sketch kernels (include/fmx.h): 2, a grid setting whose `knob` lies outside the range the launch
    was sized for, and 1, a NaN prediction, which raises what the host loop raises.  fmx_rrf_grid counts NaN samples in
    status[0] >= 0 (they are dropped, not an error) and refuses a setting with -2."""
    refused = -2 if entry == "fmx_rrf_grid" else 2
    if bool((st[:, 0] == refused).any()):
        raise ValueError("a setting's %s lies outside [1, max]: not run (%s status %d)" % (knob, entry, refused))
    if refused == 2 and bool((st[:, 0] == 1).any()):
        raise ValueError("Nan contained")
