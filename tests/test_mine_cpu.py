"""Hard-negative mining (fmx_fm_mine_negatives) without a GPU: the symbol and its declaration, the header's statement of the
draws and the limits, the numpy Philox of tests/mine_ref.py against the published known answers and the pinned draw layout,
every refusal decided on the host (pointers that are never dereferenced), Candidates.positions_of on CPU tensors, and the
errors of the Python surface that need no device."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import mine_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "fmx_fm_mine_negatives"
N_ARGS = 20


def _lib():
    import fmx
    L = fmx._lib
    return fmx, L, L.load()


def _header_comment():
    header = open(os.path.join(ROOT, "include", "fmx.h")).read()
    decl = re.search(r"\bint " + NAME + r"\(([^;]*)\);", header)
    assert decl
    return decl, header[:decl.start()].rsplit("/*", 1)[1]


def test_symbol_declaration_and_argument_count():
    fmx, L, lib = _lib()
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert NAME in set(re.findall(r"\bT\s+(fmx_\w+)", out))
    assert NAME in L.EXPORTS and len(getattr(lib, NAME).argtypes) == N_ARGS
    decl, comment = _header_comment()
    assert len(decl.group(1).split(",")) == N_ARGS
    assert "Replaces:" in comment
    assert lib.fmx_version() == 104


def test_header_states_the_counter_layout_and_the_limits():
    _, comment = _header_comment()
    flat = " ".join(comment.split())
    for words in ("Philox4x32-10", "0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85", "word j & 3",
                  "(seed & 0xffffffff, seed >> 32)", "(offset & 0xffffffff, offset >> 32, (u_base + u) mod 2^32, j >> 2)",
                  "(uint64(word) * N) >> 32", "N / 2^32", "n_draw <= 1024", "n_neg <= 16", "n_neg <= n_draw", "4 / 8 / 16 / 32 / 64",
                  "FMX_ERR_UNSUPPORTED", "FMX_ERR_ARG", "FMX_ERR_ALIGN", "-1 / -inf", "a position drawn twice counts once"):
        assert words in flat, words


@pytest.mark.parametrize("counter, key, want", [
    ([0, 0, 0, 0], [0, 0], "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ([0xffffffff] * 4, [0xffffffff] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    got = mine_ref.philox4x32_10(counter, key)
    assert " ".join("%08x" % v for v in got) == want


def test_pinned_draw_layout():
    assert mine_ref.draws(7, 0, 0, 1, 8, 5).tolist() == [[4, 3, 0, 0, 4, 2, 1, 0]]
    # a user's draws depend on (seed, offset, u_base + u, N) only: not on U, not on n_draw, not on how a batch is cut
    full = mine_ref.draws(7, 3, 0, 20, 13, 1000)
    assert np.array_equal(mine_ref.draws(7, 3, 10, 5, 13, 1000), full[10:15])
    assert np.array_equal(mine_ref.draws(7, 3, 0, 20, 6, 1000), full[:, :6])
    assert not np.array_equal(mine_ref.draws(7, 4, 0, 20, 13, 1000), full)
    assert not np.array_equal(mine_ref.draws(8, 3, 0, 20, 13, 1000), full)
    big = mine_ref.draws(2 ** 40 + 5, 2 ** 33 + 1, 2 ** 32 - 2, 4, 9, 70001)      # the high words and the wrap of u_base + u
    assert np.array_equal(big[2:], mine_ref.draws(2 ** 40 + 5, 2 ** 33 + 1, 0, 2, 9, 70001))
    assert big.min() >= 0 and big.max() < 70001


def _call(lib, Su=0x40000, ld_u=16, au=0x50000, U=3, Sc=0x60000, ld_c=16, ac=0x70000, N=100, kp=16, eo=None, ep=None, own=None,
          n_draw=32, n_neg=1, pos=0x80000, score=0x90000):
    return lib.fmx_fm_mine_negatives(Su, ld_u, au, U, Sc, ld_c, ac, N, kp, eo, ep, own, n_draw, n_neg, 1, 2, 3, pos, score, None)


def test_host_decided_refusals():
    fmx, L, lib = _lib()
    A, SH, AL, UN = L.ERR_ARG, L.ERR_SHAPE, L.ERR_ALIGN, L.ERR_UNSUPPORTED
    cases = [("n_draw 0", dict(n_draw=0), A), ("n_draw 1025", dict(n_draw=1025, n_neg=1), UN),
             ("n_neg 0", dict(n_neg=0), A), ("n_neg 17", dict(n_neg=17, n_draw=64), UN),
             ("n_neg > n_draw", dict(n_neg=5, n_draw=4), A),
             ("kp 12", dict(kp=12), UN), ("kp 128", dict(kp=128, ld_u=128, ld_c=128), UN),
             ("N 0", dict(N=0), A), ("U 0", dict(U=0), A),
             ("null neg_pos", dict(pos=None), A), ("null neg_score", dict(score=None), A),
             ("null Su", dict(Su=None), A), ("null au", dict(au=None), A), ("null Sc", dict(Sc=None), A), ("null ac", dict(ac=None), A),
             ("excl_offsets alone", dict(eo=0xA0000), A), ("excl_pos alone", dict(ep=0xA0000), A),
             ("ld_c 6", dict(ld_c=6, kp=4), AL), ("ld_u 6", dict(ld_u=6, kp=4), AL),
             ("ld_c < kp", dict(ld_c=8), SH),
             ("Su misaligned", dict(Su=0x40004), AL), ("Sc misaligned", dict(Sc=0x60008), AL)]
    for what, kw, want in cases:
        rc = _call(lib, **kw)
        msg = lib.fmx_last_error_string().decode()
        assert rc == want, (what, rc, msg)
        assert NAME in msg, (what, msg)


def _fake_candidates(sizes, item_fields, rows):
    """A Candidates without its device side: positions_of reads the table's sizes and device, the item fields and idx only"""
    from fmx.recommend import Candidates

    class T:
        feature_sizes, n_fields, device = sizes, len(sizes), torch.device("cpu")

    c = object.__new__(Candidates)
    c.table, c.item_fields = T(), sorted(item_fields)
    c.idx = torch.as_tensor(rows, dtype=torch.int32)
    return c


def test_positions_of_one_item_field():
    sizes = [7, 50, 5]
    rows = np.zeros((6, 3), dtype=np.int64)
    rows[:, 1] = [40, 3, 17, 3, 49, 0]                       # item 3 is listed twice: the lower position counts
    rows[:, 0] = 5                                           # the other columns are ignored
    c = _fake_candidates(sizes, [1], rows)
    got = c.positions_of(torch.tensor([3, 40, 41, 0, 49, 17, -1, 50]))
    assert got.dtype == torch.int32 and got.tolist() == [1, 0, -1, 5, 4, 2, -1, -1]
    assert c.positions_of(torch.tensor([[17], [2]])).tolist() == [2, -1]
    with pytest.raises(ValueError):
        c.positions_of(torch.tensor([[1, 2]]), [1, 2])


def test_positions_of_two_item_fields():
    sizes = [7, 50, 5, 11]
    rows = np.zeros((5, 4), dtype=np.int64)
    rows[:, 1] = [40, 3, 17, 3, 3]
    rows[:, 3] = [10, 0, 4, 9, 0]                            # (3, 0) is listed at 1 and 4
    c = _fake_candidates(sizes, [3, 1], rows)
    items = torch.tensor([[3, 0], [3, 9], [40, 10], [17, 4], [17, 5], [3, 10], [0, 0], [50, 0], [3, 11], [-1, 0]])
    assert c.positions_of(items).tolist() == [1, 3, 0, 2, -1, -1, -1, -1, -1, -1]
    # the columns in the caller's order of item fields
    assert c.positions_of(items[:, [1, 0]], [3, 1]).tolist() == c.positions_of(items).tolist()


def test_whole_field_positions_need_no_index():
    c = _fake_candidates([7, 50, 5], [1], np.zeros((50, 3), dtype=np.int64))
    c._identity = True
    assert c.positions_of(torch.tensor([0, 49, 50, -3, 12])).tolist() == [0, 49, -1, -1, 12]
    assert not hasattr(c, "_inverse")


def test_python_surface_errors_that_need_no_device():
    from fmx.pairwise import HardNegatives, hard_negatives
    from models.models_online_deep.fm_adam import FMAdam
    assert hard_negatives(None) is None and hard_negatives(torch.zeros(3, 1)) is None and hard_negatives([[1]]) is None
    h = hard_negatives("hard")
    assert (h.n_draw, h.exclude, h.refresh_every, h.remine_every) == (32, None, 1, None)
    mine = HardNegatives(n_draw=64, refresh_every=3, remine_every=8)
    assert hard_negatives(mine) is mine
    for bad in (dict(n_draw=0), dict(refresh_every=0), dict(remine_every=0)):
        with pytest.raises(ValueError):
            HardNegatives(**bad)
    with pytest.raises(ValueError, match="hard"):
        hard_negatives("hardest")
    obj = object.__new__(FMAdam)                              # (no GPU: the constructor raises; this refusal needs no state)
    with pytest.raises(ValueError, match="exactly one item field"):
        obj._mining_candidates([1, 2], None, 1)
    assert FMAdam.mining_seed == 0


@pytest.mark.parametrize("cls, kw", [("DeepFMAdam", dict()), ("DeepFMAdam", dict(full=True)), ("NFMAdam", dict(full=True)),
                                     ("DeepFMOnn", dict()), ("NFMOnn", dict()), ("AFMAdam", dict()), ("AFMAdam", dict(attention=True))])
def test_hard_negatives_are_refused_outside_the_pure_fm(cls, kw):
    import importlib
    from fmx.pairwise import HardNegatives
    mod = {"DeepFMAdam": "deepfm_adam", "NFMAdam": "nfm_adam", "DeepFMOnn": "deepfm_onn", "NFMOnn": "nfm_onn", "AFMAdam": "afm_adam"}[cls]
    klass = getattr(importlib.import_module("models.models_online_deep." + mod), cls)
    obj = object.__new__(klass)
    for name in ("fit_pairs", "run_pair_experiment"):
        for neg in ("hard", HardNegatives(n_draw=8)):
            with pytest.raises(NotImplementedError, match="negatives='hard' mines under the pure FM score"):
                getattr(klass, name)(obj, [[0, 0]], [[1.0, 1.0]], [1], negatives=neg, **kw)
