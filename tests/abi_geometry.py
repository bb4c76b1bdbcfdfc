"""Guard bands for the C ABI's table geometries (helper module of test_abi_geometry_cpu.py / test_abi_geometry_gpu.py).

include/fmx.h accepts a family of row geometries (kp, z_offset, row_stride, the alignment of `rows`); fmx.FlatTable builds one
of them per (layout, kp).  GuardedTable builds any of them by hand, inside ONE buffer the test owns,

    [ guard rows | lead floats | n_rows x row_stride table | guard rows ]

and fills the guards, the lead and every DEAD float of every row (a float the header does not name) with a quiet NaN that
carries a payload.  A kernel that addresses a row wrongly then either reads a NaN into a live result or writes over the
pattern: both end in a failed assertion on the test's own memory, never in a fault.  `guarded` does the same for plain
buffers (workspaces, outputs): the bytes after the size the header names must keep their bits.

Everything is compared through int32 views: a NaN never equals itself as a float, and -0.0 equals +0.0.
"""
import ctypes as C

import numpy as np
import torch

PATTERN = 0x7FC5A5A5          # a quiet NaN (exponent all ones, top mantissa bit set) with a recognisable payload
GUARD_ROWS = 64
LAYOUT_IDS = {"weights": 0, "ftrl": 1, "moments": 2}
BIAS_FLOATS = {"weights": 1, "ftrl": 2, "moments": 4}


def _round_up(x, m):
    return (x + m - 1) // m * m


def default_geometry(layout, kp):
    """(z_offset, row_stride) of fmx.FlatTable for this layout and kp."""
    if layout == "weights":
        return 0, (_round_up(kp + 4, 32) if kp >= 16 else 2 * kp)
    zo = _round_up(kp + 4, 32) if kp >= 16 else 2 * kp
    return zo, (_round_up(zo + 2 * kp, 32) if kp >= 16 else 4 * kp)


def need(layout, kp, z_offset):
    """The smallest row_stride include/fmx.h allows."""
    return kp + 4 if layout == "weights" else z_offset + 2 * kp


def live_mask(layout, k, kp, z_offset, row_stride):
    """bool [row_stride]: the floats of a row that include/fmx.h names.
      weights            [ V[0..kp) | w ]
      ftrl / moments     [ V[0..kp) | w, zw / mw, nw / vw, 0 ] and [ zV / mV [0..kp) | nV / vV [0..kp) ] from z_offset
    Components k..kp of every kp-wide block are live (the kernels sum over kp) and hold zero, as does the fourth float of the
    ftrl / moments head; everything else (the pad of a weights row from kp + 1 on, the floats between the head and z_offset,
    the floats past z_offset + 2 kp) is dead."""
    m = np.zeros(row_stride, dtype=bool)
    m[:kp + 1] = True
    if layout != "weights":
        m[kp + 1:kp + 4] = True
        m[z_offset:z_offset + 2 * kp] = True
    return m


def zero_mask(layout, k, kp, z_offset, row_stride):
    """bool [row_stride]: the live floats that hold zero and must stay exactly zero."""
    m = np.zeros(row_stride, dtype=bool)
    m[k:kp] = True
    if layout != "weights":
        m[kp + 3] = True
        m[z_offset + k:z_offset + kp] = True
        m[z_offset + kp + k:z_offset + 2 * kp] = True
    return m


def _live_pairs(layout, kp, zo_src, zo_dst):
    """[(source float, destination float, count)] that carry a row's live floats from one geometry into another."""
    if layout == "weights":
        return [(0, 0, kp + 1)]
    return [(0, 0, kp + 4), (zo_src, zo_dst, 2 * kp)]


def bits(a):
    """The int32 bits of a float32 array (numpy or torch, any device) as numpy."""
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().contiguous().numpy()
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


class Guarded:
    """`nbytes` bytes (a multiple of 4) handed to a kernel, inside a larger buffer whose head and tail carry PATTERN.
    .t is the payload as a tensor of `dtype` (zero-filled), .ptr its address (512-byte aligned plus 256: 16-byte aligned)."""
    HEAD, TAIL = 64, 1024     # int32 words

    def __init__(self, nbytes, dtype=torch.float32, device="cuda", shape=None, name=""):
        nbytes = int(nbytes)
        assert nbytes >= 0 and nbytes % 4 == 0, nbytes
        self.name, self.words = name, nbytes // 4
        self.buf = torch.full((self.HEAD + self.words + self.TAIL,), PATTERN, dtype=torch.int32, device=device)
        body = self.buf[self.HEAD:self.HEAD + self.words]
        body.zero_()
        self.t = body.view(dtype)
        if shape is not None:
            self.t = self.t.view(shape)
        self.ptr = body.data_ptr() if self.words else self.buf.data_ptr() + 4 * self.HEAD
        self.nbytes = nbytes

    def check(self):
        b = self.buf.cpu().numpy()
        head, tail = b[:self.HEAD], b[self.HEAD + self.words:]
        assert (head == PATTERN).all(), f"{self.name}: {int((head != PATTERN).sum())} words in front of the buffer were written"
        bad = np.flatnonzero(tail != PATTERN)
        assert bad.size == 0, (f"{self.name}: {bad.size} words past its {self.nbytes} bytes were written "
                               f"(first at byte {self.nbytes + 4 * int(bad[0])})")


def guarded(nbytes, dtype=torch.float32, device="cuda", shape=None, name=""):
    """-> (pointer, checker, tensor view of the payload)."""
    g = Guarded(nbytes, dtype, device, shape, name)
    return g.ptr, g.check, g.t


class GuardSet:
    """The guarded buffers of one call: new() makes one, check() checks them all, outputs() returns the bits of those made
    with out=True."""

    def __init__(self, device="cuda"):
        self.device, self.items, self.outs = device, [], []

    def new(self, name, shape, dtype=torch.float32, out=False, src=None):
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        n = int(np.prod(shape)) if shape else 1
        g = Guarded(n * torch.empty(0, dtype=dtype).element_size(), dtype, self.device, shape, name)
        if src is not None:
            g.t.copy_(torch.as_tensor(src, dtype=dtype).reshape(shape))
        self.items.append(g)
        if out:
            self.outs.append(g)
        return g

    def raw(self, name, nbytes):
        """A zero-filled buffer of exactly nbytes (a workspace)."""
        g = Guarded(nbytes, torch.int32, self.device, None, name)
        self.items.append(g)
        return g

    def check(self):
        for g in self.items:
            g.check()

    def outputs(self):
        return {g.name: bits(g.t) for g in self.outs}


class GuardedTable:
    """An fmx_table_t built by hand at any geometry the header allows (or does not: the CPU tests hand check_table bad ones).
    Duck-types what the tests use of fmx.FlatTable: c_struct(), k, kp, layout, n_fields, n_cols, n_rows, row_stride, z_offset,
    bias, mapped."""

    def __init__(self, feature_sizes, k, kp, layout, z_offset=None, row_stride=None, lead=0, device="cuda", field_cols=None,
                 field_base=None, n_cols=None):
        self.feature_sizes = [int(s) for s in feature_sizes]
        self.n_fields, self.k, self.kp, self.layout = len(self.feature_sizes), int(k), int(kp), layout
        dzo, dstride = default_geometry(layout, kp)
        self.z_offset = dzo if z_offset is None else int(z_offset)
        if layout == "weights":
            self.z_offset = 0
        self.row_stride = dstride if row_stride is None else int(row_stride)
        self.lead = int(lead)
        assert self.lead in (0, 4)
        self.device = torch.device(device)
        self.offsets_host = np.concatenate([[0], np.cumsum(self.feature_sizes, dtype=np.int64)]).astype(np.int64)
        self.n_rows = int(self.offsets_host[-1])
        s = self.row_stride
        self._g = GUARD_ROWS * s
        self.buf = torch.full((2 * self._g + self.lead + self.n_rows * s,), PATTERN, dtype=torch.int32, device=self.device)
        lo = self._g + self.lead
        self.rows_i32 = self.buf[lo:lo + self.n_rows * s].view(self.n_rows, s)
        self.rows = self.rows_i32.view(torch.float32)
        self.offsets = torch.from_numpy(self.offsets_host).to(self.device)
        # the bias and the field tables sit in guarded buffers of their own
        self._bias = Guarded(4 * BIAS_FLOATS[layout], torch.float32, self.device, None, "bias")
        self.bias = self._bias.t
        self.mapped = field_cols is not None
        if self.mapped:
            self.field_cols = torch.tensor([int(c) for c in field_cols], dtype=torch.int32, device=self.device)
            self.field_base = torch.tensor([int(b) for b in field_base], dtype=torch.int32, device=self.device)
            self.n_cols = int(n_cols)
        else:
            self.n_cols = self.n_fields
        self._live = live_mask(layout, self.k, self.kp, self.z_offset, s)
        self._zero = zero_mask(layout, self.k, self.kp, self.z_offset, s)
        live_t = torch.from_numpy(self._live).to(self.device)
        self.rows_i32[:, live_t] = 0                       # live floats start as zero; dead ones keep the pattern
        self._cstruct = None

    def c_struct(self):
        import fmx
        if self._cstruct is None:
            t = fmx._lib.Table()
            t.rows = self.rows.data_ptr()
            t.field_offsets = self.offsets.data_ptr()
            t.bias = self._bias.ptr
            t.n_rows, t.n_fields = self.n_rows, self.n_fields
            t.k, t.kp, t.row_stride = self.k, self.kp, self.row_stride
            t.layout, t.z_offset = LAYOUT_IDS[self.layout], self.z_offset
            t.max_field_rows = max(self.feature_sizes)
            if self.mapped:
                t.field_cols, t.field_base, t.n_cols = self.field_cols.data_ptr(), self.field_base.data_ptr(), self.n_cols
            self._cstruct = t
        return C.byref(self._cstruct)

    def load_from(self, flat):
        """Copy the live floats (and the bias) of a default-geometry fmx.FlatTable of the same layout, k and fields."""
        assert (flat.layout, flat.k, flat.kp, flat.n_rows) == (self.layout, self.k, self.kp, self.n_rows)
        for s0, d0, n in _live_pairs(self.layout, self.kp, flat.z_offset, self.z_offset):
            self.rows[:, d0:d0 + n] = flat.rows[:, s0:s0 + n].to(self.device)
        self.bias.copy_(flat.bias.to(self.device))
        return self

    def live(self):
        """The live floats in the default geometry (dead floats zero, as torch.zeros leaves them in a FlatTable): int32 bits
        [n_rows, default row_stride]."""
        dzo, dstride = default_geometry(self.layout, self.kp)
        r = self.rows_i32.cpu().numpy()
        out = np.zeros((self.n_rows, dstride), dtype=np.int32)
        for s0, d0, n in _live_pairs(self.layout, self.kp, self.z_offset, dzo):
            out[:, d0:d0 + n] = r[:, s0:s0 + n]
        return out

    def assert_live_equals(self, flat, what=""):
        """Live floats bit-identical to the rows (and bias) of the default-geometry table that took the same calls."""
        ref = bits(flat.rows)
        got = self.live()
        assert got.shape == ref.shape, (got.shape, ref.shape)
        bad = np.argwhere(got != ref)
        assert bad.size == 0, (f"{what}: {len(bad)} live floats differ from the default geometry's; first at row {bad[0][0]}, "
                               f"float {bad[0][1]} (default geometry)")
        np.testing.assert_array_equal(bits(self.bias), bits(flat.bias), err_msg=f"{what}: bias")

    def assert_zero_components(self, what=""):
        """Components k..kp of every block (and the head's fourth float) are still exactly +0."""
        r = self.rows_i32.cpu().numpy()[:, self._zero]
        assert not r.any(), f"{what}: {int(np.count_nonzero(r))} pad components are no longer zero"

    def assert_dead_untouched(self, what=""):
        """Both guards, the lead and every dead float of every row keep the pattern, bit for bit; so do the words around
        the bias."""
        b = self.buf.cpu().numpy()
        lo = self._g + self.lead
        front, back = b[:lo], b[lo + self.n_rows * self.row_stride:]
        bad = np.flatnonzero(front != PATTERN)
        assert bad.size == 0, f"{what}: {bad.size} floats in front of the table were written (first {lo - int(bad[0])} floats before rows)"
        bad = np.flatnonzero(back != PATTERN)
        assert bad.size == 0, f"{what}: {bad.size} floats behind the table were written (first {int(bad[0])} floats past its end)"
        dead = b[lo:lo + self.n_rows * self.row_stride].reshape(self.n_rows, self.row_stride)[:, ~self._live]
        bad = np.argwhere(dead != PATTERN)
        assert bad.size == 0, (f"{what}: {len(bad)} dead floats of the rows were written; first at row {bad[0][0]}, float "
                               f"{int(np.flatnonzero(~self._live)[bad[0][1]])} of the row")
        self._bias.check()
