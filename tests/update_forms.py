"""Inputs for the tests of k_fm_update's two forms (test_update_forms_cpu.py, test_update_forms_gpu.py, test_capture_gpu.py), a
numpy model of what the update's tile waves and k_fm_fixup read from a field's sorted list, and the helpers the GPU files share.
Helper module, not collected.

The generator.  A field's kind decides how its indices are drawn:
  one      a one-row field: ONE run over the whole batch, every real tile but the first and last THROUGH
  two      two rows, drawn uniformly: two runs of about B / 2
  hot      one row takes 70 % of the samples, the rest are uniform: a long run between short ones
  tiles    exactly 64 occurrences of each row (the last row takes the remainder of a ragged batch): every run ends on a tile's
           last entry
  uniform  a large uniform field (>= 20,000 rows): almost every run has length one
  zipf     zipf(1.1): a head of long runs, a tail of single occurrences

The model (csrc/fmx_update.hip: update_body's meta words and k_fm_fixup's walk over them).  A field's list holds the composites
(row << bbits) | sample in ascending order, padded with 0xFFFFFFFF to the sorted width; tile t is entries 64 t .. 64 t + 63.  With
key(e) = e >> bbits, prev(t) the key of the entry in front of the tile (the pad's key in front of tile 0) and next(t) the key of
the entry behind it (the pad's key behind the last tile):
  an entry is the TAIL of its run when it is no pad and the entry behind it has another key;
  the tile is OPEN when its last entry is no pad and has the key next(t);
  an open tile whose last key is prev(t) is one piece of a longer run: lead = LEAD_THROUGH, trail = 0;
  any other open tile is the HEAD of the run that leaves it: trail = 1;
  unless THROUGH, lead = LEAD_CLOSES when some tail of the tile has the key prev(t) (the run that came in ends here), else LEAD_NONE.
k_fm_fixup's wave of a head tile t reads the lead words of the tiles behind it 64 at a time (j0 = 1, 65, 129, ...) up to the end
of the field and stops at the first that is not THROUGH: m = its distance when it CLOSES the run, its distance - 1 otherwise; m is
the number of following tiles whose lead record it adds to the head's own trail record."""
import numpy as np

LEAD_NONE, LEAD_CLOSES, LEAD_THROUGH = 0, 1, 2
PAD = 0xFFFFFFFF
RED_SLICE = 4096                 # bias_and_loss's slice of the batch (csrc/fmx_update.hip)
KINDS = ("one", "two", "hot", "tiles", "uniform", "zipf", "hot", "uniform")


def sorted_width(B):
    """fmx_sorted_width: the power of two >= max(B, 64)"""
    w = 64
    while w < B:
        w <<= 1
    return w


def sorted_bbits(B):
    return sorted_width(B).bit_length() - 1


def field_sizes(B, F=6, kinds=None):
    """Row counts for fields of `kinds` (default: the first F of KINDS) at batch size B."""
    kinds = KINDS[:F] if kinds is None else kinds
    size = dict(one=1, two=2, hot=50, tiles=(B + 63) // 64, uniform=20011, zipf=3000)
    out, seen = [], {}
    for kd in kinds:
        n = seen.get(kd, 0)
        seen[kd] = n + 1
        out.append(size[kd] if n == 0 else dict(hot=7, uniform=300).get(kd, size[kd]))      # a second field of a kind: a small one
    return out


def indices(sizes, B, seed, kinds=None):
    """-> int32 [B, F]: column f drawn as its kind says (kinds default to KINDS by position), in a seeded random sample order."""
    kinds = KINDS[:len(sizes)] if kinds is None else kinds
    assert len(kinds) == len(sizes)
    rng = np.random.default_rng(seed)
    cols = []
    for s, kd in zip(sizes, kinds):
        s = int(s)
        if kd == "one":
            assert s == 1
            c = np.zeros(B, np.int64)
        elif kd == "two":
            assert s == 2
            c = rng.integers(0, 2, size=B)
        elif kd == "hot":
            hot = s // 2
            c = np.where(rng.uniform(size=B) < 0.7, hot, rng.integers(0, s, size=B))
        elif kd == "tiles":
            assert s * 64 >= B
            c = rng.permutation(np.arange(B) // 64)
        elif kd == "uniform":
            c = rng.integers(0, s, size=B)
        elif kd == "zipf":
            c = np.minimum(rng.zipf(1.1, size=B) - 1, s - 1)
        else:
            raise ValueError(kd)
        cols.append(c)
    return np.stack(cols, axis=1).astype(np.int32)


def sorted_list(col, B):
    """The list fmx_sort_occurrences leaves for one field: uint32 [sorted width]."""
    bbits = sorted_bbits(B)
    out = np.full(sorted_width(B), PAD, np.uint32)
    out[:B] = np.sort((np.asarray(col[:B]).astype(np.uint32) << np.uint32(bbits)) | np.arange(B, dtype=np.uint32))
    return out


def tile_states(lst, bbits):
    """-> (lead int [tiles], trail int [tiles]) of one field's list, as update_body writes its meta words."""
    lst = np.asarray(lst, np.uint32)
    n = lst.shape[0]
    assert n % 64 == 0
    key = (lst >> np.uint32(bbits)).astype(np.int64)
    val = lst != np.uint32(PAD)
    pad_key = PAD >> bbits
    nxt = np.concatenate([key[1:], [pad_key]])
    tail = val & (key != nxt)
    T = n // 64
    key_t, tail_t = key.reshape(T, 64), tail.reshape(T, 64)
    prev = np.concatenate([[pad_key], key[63:-1:64]])                  # the key in front of every tile
    nxt_t = nxt[63::64]                                                # ... and behind it
    is_open = val[63::64] & (key_t[:, 63] == nxt_t)
    through = is_open & (key_t[:, 63] == prev)
    closes = (tail_t & (key_t == prev[:, None])).any(axis=1)
    lead = np.where(through, LEAD_THROUGH, np.where(closes, LEAD_CLOSES, LEAD_NONE))
    trail = (is_open & ~through).astype(np.int64)
    return lead.astype(np.int64), trail


def fixup_counts(lead, trail):
    """-> {head tile: m}: k_fm_fixup's walk, restated lane by lane (64 lead words per iteration, the first that is not THROUGH
    ends it; past the field's last tile a lane sees LEAD_NONE)."""
    T = len(lead)
    out = {}
    for t in np.flatnonzero(np.asarray(trail) == 1):
        t = int(t)
        m, j0 = 0, 1
        while t + j0 < T:
            st = [int(lead[t + j0 + lane]) if t + j0 + lane < T else LEAD_NONE for lane in range(64)]
            stop = [lane for lane in range(64) if st[lane] != LEAD_THROUGH]
            if stop:
                m = j0 + stop[0] - (0 if st[stop[0]] == LEAD_CLOSES else 1)
                break
            m = j0 + 63
            j0 += 64
        if t + m >= T:
            m = T - 1 - t
        out[t] = m
    return out


def field_report(lst, bbits):
    """Everything the tests assert about one field's list: tile states, the heads' m, and the conditions by name."""
    lead, trail = tile_states(lst, bbits)
    m = fixup_counts(lead, trail)
    lst = np.asarray(lst, np.uint32)
    T = len(lead)
    real = (lst != np.uint32(PAD)).reshape(T, 64).sum(axis=1)
    key = (lst >> np.uint32(bbits)).astype(np.int64).reshape(T, 64)
    # a run that ends on its tile's last entry: that tile is not open, and the next one starts a run of its own
    ends_on_boundary = [t for t in range(T - 1) if real[t] == 64 and trail[t] == 0 and lead[t] != LEAD_THROUGH
                        and lead[t + 1] == LEAD_NONE and real[t + 1] > 0]
    closes_in_padded_tile = [t for t in range(T) if lead[t] == LEAD_CLOSES and 0 < real[t] < 64]
    return dict(lead=lead, trail=trail, m=m, real=real, key=key, max_m=max(m.values(), default=0),
                ends_on_boundary=ends_on_boundary, closes_in_padded_tile=closes_in_padded_tile,
                m_is_one=[t for t, v in m.items() if v == 1 and lead[t + 1] == LEAD_CLOSES])


def report(lists, B):
    """field_report for every row of `lists` (uint32 [fields, sorted width]: numpy's sort or the device's)."""
    return [field_report(l, sorted_bbits(B)) for l in np.asarray(lists).view(np.uint32)]


def check_run_sums(lst, bbits, rep):
    """The model against the list itself: every head's run really spans m further tiles -- the tiles t + 1 .. t + m hold the
    head's last key and tile t + m + 1 does not start with it."""
    key, T = rep["key"], len(rep["lead"])
    val = (np.asarray(lst, np.uint32) != np.uint32(PAD)).reshape(T, 64)
    for t, m in rep["m"].items():
        k = key[t, 63]
        assert m >= 1, "an open tile's run goes on in the next tile"
        for j in range(1, m + 1):
            assert val[t + j, 0] and key[t + j, 0] == k
        for j in range(1, m):
            assert val[t + j].all() and (key[t + j] == k).all()
        assert t + m + 1 >= T or not (val[t + m, 63] and key[t + m, 63] == k and val[t + m + 1, 0] and key[t + m + 1, 0] == k)


# ---- shared by the GPU files ----
class option:
    """fmx_set_option(name, value) for a block; back to the value the call returned on the way out."""

    def __init__(self, lib, name, value):
        self.lib, self.name, self.value = lib, name.encode(), int(value)

    def __enter__(self):
        self.prev = self.lib.fmx_set_option(self.name, self.value)
        return self

    def __exit__(self, *exc):
        self.lib.fmx_set_option(self.name, self.prev)


def same(got, ref, what):
    """Bit for bit: the words as integers (a NaN would differ from itself otherwise).  got / ref: dicts of tensors."""
    import torch
    assert set(got) == set(ref), f"{what}: {set(got) ^ set(ref)}"
    for name in ref:
        a, b = got[name].detach().contiguous(), ref[name].detach().contiguous()
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {name}: {tuple(a.shape)} {a.dtype} vs {tuple(b.shape)} {b.dtype}"
        if a.element_size() == 4:
            a, b = a.view(torch.int32), b.view(torch.int32)
        assert torch.equal(a, b), f"{what}: {name}: {int((a != b).sum())} of {a.numel()} words differ"


def heads_on_device(eng, B):
    """report() of the lists the engine's last sort left."""
    import torch
    torch.cuda.synchronize()
    return report(eng.sorted.cpu().numpy(), B)
