"""The inputs of test_update_forms_gpu.py / test_capture_gpu.py reach what those tests are about -- shown without a device, on
numpy's sort of the same indices (update_forms.py holds the generator and the model of the tile states and of k_fm_fixup's walk).

These are conditions on the INPUTS at every batch size the GPU tests use, not measurements: k_fm_fixup's second and later
iterations over the following tiles' meta words need a head with m >= 65; its extra last workgroup and the last slice's
workgroup of the update need B > 4096; B = 4097 leaves a last slice of one sample and last real tiles of one entry."""
import numpy as np
import pytest

import update_forms as uf

BATCHES = [4097, 4161, 5000, 8192, 12289]


def lists_of(B, F=6, kinds=None, seed=0):
    sizes = uf.field_sizes(B, F, kinds)
    idx = uf.indices(sizes, B, seed, kinds)
    assert idx.shape == (B, len(sizes)) and (idx >= 0).all() and (idx < np.asarray(sizes)[None, :]).all()
    return sizes, idx, np.stack([uf.sorted_list(idx[:, f], B) for f in range(len(sizes))])


def runs_by_hand(lst, bbits):
    """{head tile: further tiles of its run}, from the runs themselves: first and last position of every key."""
    n = int((lst != np.uint32(uf.PAD)).sum())
    key = (lst[:n] >> np.uint32(bbits)).astype(np.int64)
    starts = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))
    ends = np.concatenate([starts[1:], [n]]) - 1
    out = {}
    for s, e in zip(starts, ends):
        if e // 64 > s // 64:
            assert s // 64 not in out                 # one run leaves a tile
            out[int(s // 64)] = int(e // 64 - s // 64)
    return out


def test_width_and_bits_are_the_librarys():
    import fmx
    lib = fmx._lib.load()
    for B in (1, 64, 65, 130, 300, 512, 4096, 4097, 4161, 5000, 8192, 12289, 32768):
        assert uf.sorted_width(B) == lib.fmx_sorted_width(B) and uf.sorted_bbits(B) == lib.fmx_sorted_bbits(B)


@pytest.mark.parametrize("B", BATCHES + [130, 300, 700, 1000])
def test_the_model_is_the_runs(B):
    """The meta words' model and the walk over them give, for every head, the tiles its run really spans."""
    _, _, lists = lists_of(B, 8, seed=B)
    for lst, rep in zip(lists, uf.report(lists, B)):
        assert rep["m"] == runs_by_hand(lst, uf.sorted_bbits(B))
        uf.check_run_sums(lst, uf.sorted_bbits(B), rep)
        lead, trail, real = rep["lead"], rep["trail"], rep["real"]
        assert not ((lead == uf.LEAD_THROUGH) & (trail == 1)).any()
        assert (lead[real == 0] == uf.LEAD_NONE).all() and (trail[real < 64] == 0).all()
        # the walk never ends on LEAD_NONE behind an open tile: the run that leaves a tile is in the next one
        assert all(lead[t + 1] != uf.LEAD_NONE for t in rep["m"])


def test_generator_kinds():
    B = 8192
    sizes, idx, _ = lists_of(B, 6)
    assert sizes[:2] == [1, 2] and sizes[4] >= 20000
    assert (idx[:, 0] == 0).all() and set(np.unique(idx[:, 1])) == {0, 1}
    hot = np.bincount(idx[:, 2]).max() / B
    assert 0.65 < hot < 0.78
    assert (np.bincount(idx[:, 3], minlength=B // 64) == 64).all()
    cu = np.bincount(idx[:, 4])
    assert (cu[cu > 0] == 1).mean() > 0.7                                  # mostly runs of length one
    cz = np.bincount(idx[:, 5])
    assert cz.max() > 64 and (cz == 1).sum() > 100
    np.testing.assert_array_equal(idx, uf.indices(sizes, B, 0))            # seeded
    assert not np.array_equal(idx, uf.indices(sizes, B, 1))


@pytest.mark.parametrize("B", BATCHES)
def test_conditions_of_the_large_batches(B):
    _, _, lists = lists_of(B, 6)
    reps = uf.report(lists, B)
    assert (B + uf.RED_SLICE - 1) // uf.RED_SLICE > 1                      # several slices: k_fm_fixup's extra workgroup
    best = max(r["max_m"] for r in reps)
    if B >= 4161:
        assert best >= 65, "no head reaches the second iteration of k_fm_fixup's walk"
    else:
        assert best == 64                                                  # (4097: the walk ends in its first iteration's last lane)
    if B == 12289:
        assert best >= 129
    assert reps[3]["ends_on_boundary"], "field `tiles`: no run ends on a tile's last entry in front of LEAD_NONE"
    if B % 64 == 0:                                                        # ... every run does, and nothing is handed over
        assert not reps[3]["m"] and (reps[3]["lead"] == uf.LEAD_NONE).all()
    assert any(r["m_is_one"] for r in reps), "no LEAD_CLOSES right behind a head"
    if B % 64:
        assert any(r["closes_in_padded_tile"] for r in reps), "no run ends in a tile that also holds pads"
    # the long run is handed over in several iterations AND ends in a padded tile for the ragged sizes
    one = reps[0]
    assert list(one["m"]) == [0] and one["m"][0] == (B + 63) // 64 - 1


def test_conditions_at_4097():
    B = 4097
    for F in (6, 8):
        _, _, lists = lists_of(B, F)
        assert B - (B - 1) // uf.RED_SLICE * uf.RED_SLICE == 1            # the last slice holds one sample
        assert uf.sorted_width(B) == 8192                                  # ... and half of every list is padding
        for r in uf.report(lists, B):
            real = r["real"]
            last = int(np.flatnonzero(real > 0)[-1])
            assert last == 64 and real[last] == 1 and (real[:last] == 64).all()


def test_conditions_at_32768():
    B, kinds = 32768, ("one", "tiles", "uniform")
    sizes, _, lists = lists_of(B, kinds=kinds)
    assert max(sizes) - 1 < (uf.PAD >> uf.sorted_bbits(B))                 # no sort pieces: the composites fit 32 bits
    reps = uf.report(lists, B)
    assert reps[0]["m"] == {0: 511}
    assert len(reps[1]["ends_on_boundary"]) == 511 and not reps[1]["m"]


@pytest.mark.parametrize("B", [130, 300, 512, 700])
def test_small_batches_cross_tiles(B):
    """The smaller shapes (network gradient, occurrence gradients, rider, capture): still a run over every real tile."""
    _, _, lists = lists_of(B, 6)
    reps = uf.report(lists, B)
    assert reps[0]["m"] == {0: (B + 63) // 64 - 1}
    assert sum(len(r["m"]) for r in reps) >= 3
