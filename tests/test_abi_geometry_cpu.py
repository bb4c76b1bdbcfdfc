"""The table geometries of include/fmx.h without a GPU: which floats of a row are live (abi_geometry.live_mask against a
hand-written table), the guard-band checkers checking (a corrupted dead, guard or live float must fail them), the accept /
reject boundary of check_table with pointers that are never dereferenced, fmx.FlatTable's row_stride taking what the C side
takes, and the spare row of a mapped table that ends in an empty field."""
import ctypes as C

import numpy as np
import pytest
import torch

import abi_geometry as ag

CRITEO_SIZES = [63, 113, 126, 51, 224, 148, 100, 79, 104, 9, 32, 57, 82, 1457, 555, 176373, 129683, 305, 19, 11887,
                632, 3, 41738, 5170, 175446, 3170, 27, 11356, 165602, 10, 4641, 2030, 4, 172761, 18, 15, 57903, 86,
                44549]


def _r(*spans):
    return sorted(i for lo, hi in spans for i in range(lo, hi))


# (layout, k, kp, z_offset, row_stride) -> the live float numbers of a row, written out by hand from the layouts of fmx.h
LIVE = [
    (("weights", 4, 4, 0, 8), _r((0, 5))),                                   # V[4] | w ; 5..7 pad
    (("weights", 16, 16, 0, 20), _r((0, 17))),                               # the smallest stride: 17..19 pad
    (("weights", 7, 8, 0, 24), _r((0, 9))),                                  # V[7], one zero component, w
    (("ftrl", 4, 4, 8, 16), _r((0, 8), (8, 16))),                            # the default: head 0..7, (z, n) 8..15, nothing dead
    (("ftrl", 16, 16, 20, 52), _r((0, 20), (20, 52))),                       # the minimum: z right behind the head
    (("ftrl", 16, 16, 32, 64), _r((0, 20), (32, 64))),                       # the default: 20..31 dead
    (("ftrl", 16, 16, 36, 80), _r((0, 20), (36, 68))),                       # padded: 20..35 and 68..79 dead
    (("moments", 24, 32, 36, 100), _r((0, 36), (36, 100))),                  # the minimum at kp = 32
    (("moments", 61, 64, 100, 240), _r((0, 68), (100, 228))),                # 68..99 and 228..239 dead
    (("moments", 7, 8, 12, 28), _r((0, 12), (12, 28))),
]


@pytest.mark.parametrize("geom,want", LIVE, ids=[f"{g[0]}-k{g[1]}-kp{g[2]}-z{g[3]}-s{g[4]}" for g, _ in LIVE])
def test_live_mask_is_the_headers_row_layout(geom, want):
    layout, k, kp, zo, stride = geom
    m = ag.live_mask(layout, k, kp, zo, stride)
    assert m.dtype == bool and m.shape == (stride,)
    assert list(np.flatnonzero(m)) == want
    z = ag.zero_mask(layout, k, kp, zo, stride)
    assert not (z & ~m).any(), "a float that must stay zero is a live float"
    blocks = [0] if layout == "weights" else [0, zo, zo + kp]
    want_zero = sorted(b + d for b in blocks for d in range(k, kp)) + ([kp + 3] if layout != "weights" else [])
    assert sorted(np.flatnonzero(z)) == sorted(want_zero)


def test_default_geometry_is_flat_tables():
    import fmx
    for layout in ("weights", "ftrl", "moments"):
        for k in (3, 4, 7, 8, 16, 24, 32, 61, 64):
            t = fmx.FlatTable([3, 5], k, layout=layout, device="cpu")
            assert ag.default_geometry(layout, t.kp) == (t.z_offset, t.row_stride)
            assert ag.need(layout, t.kp, t.z_offset) <= t.row_stride


def _table(layout="ftrl", lead=4):
    t = ag.GuardedTable([3, 5, 2], 7, 8, layout, z_offset=12 if layout != "weights" else None,
                        row_stride=40 if layout != "weights" else 24, lead=lead, device="cpu")
    return t


def test_guarded_table_layout_and_round_trip():
    import fmx
    for layout in ("weights", "ftrl", "moments"):
        flat = fmx.FlatTable([3, 5, 2], 7, layout=layout, device="cpu")
        rng = np.random.default_rng(1)
        live = torch.from_numpy(ag.live_mask(layout, 7, 8, flat.z_offset, flat.row_stride) &
                                ~ag.zero_mask(layout, 7, 8, flat.z_offset, flat.row_stride))
        flat.rows[:, live] = torch.from_numpy(rng.normal(size=(10, int(live.sum()))).astype(np.float32))
        flat.bias[:] = 0.5
        t = _table(layout).load_from(flat)
        assert t.rows.data_ptr() % 16 == 0 and t.rows.data_ptr() % 32 == 16       # lead = 4: 16- but not 32-byte aligned
        assert _table(layout, lead=0).rows.data_ptr() % 64 == 0
        assert t.buf.numel() == 2 * ag.GUARD_ROWS * t.row_stride + 4 + 10 * t.row_stride
        t.assert_live_equals(flat)
        t.assert_dead_untouched()
        t.assert_zero_components()
        # every dead float of every row and every guard float is a NaN when a kernel reads it as a float
        dead = t.rows[:, torch.from_numpy(~ag.live_mask(layout, 7, 8, t.z_offset, t.row_stride))]
        assert dead.numel() > 0 and torch.isnan(dead).all()
        assert torch.isnan(t.buf[:t._g].view(torch.float32)).all()


def test_checkers_fail_on_a_corrupted_float():
    """The harness checks itself: one dead float, one float of each guard, the lead and one live float, corrupted by hand --
    a mask that marked everything live, or a checker that returned early, would pass all of these silently."""
    import fmx
    flat = fmx.FlatTable([3, 5, 2], 7, layout="ftrl", device="cpu")
    flat.rows[:, :7] = 0.25
    t = _table("ftrl").load_from(flat)
    t.assert_dead_untouched()
    t.assert_live_equals(flat)
    dead = int(np.flatnonzero(~t._live)[0])
    assert dead == 28                                    # z_offset = 12, kp = 8: head 0..11, (z, n) 12..27, dead 28..39
    for corrupt in (lambda: t.rows_i32[4].__setitem__(39, 0),                         # the last dead float of a row
                    lambda: t.rows_i32[9].__setitem__(28, ag.PATTERN ^ 1),            # the first dead float, one bit
                    lambda: t.buf.__setitem__(t._g - 1, 0),                           # the float just before the lead
                    lambda: t.buf.__setitem__(t._g + 2, 0),                           # inside the lead
                    lambda: t.buf.__setitem__(0, 0),                                  # the first guard float
                    lambda: t.buf.__setitem__(t.buf.numel() - t._g, 0),               # the float just past the table
                    lambda: t.buf.__setitem__(t.buf.numel() - 1, 0),                  # the last guard float
                    lambda: t._bias.buf.__setitem__(ag.Guarded.HEAD + 2, 0)):         # the float past the bias pair
        keep, keep_b = t.buf.clone(), t._bias.buf.clone()
        corrupt()
        with pytest.raises(AssertionError):
            t.assert_dead_untouched()
        t.buf.copy_(keep)
        t._bias.buf.copy_(keep_b)
        t.assert_dead_untouched()
    # a live float: one bit of a weight, a moved (z, n) float, a pad component that is no longer +0
    for r, c in ((2, 3), (0, 8), (7, 12), (9, 27)):
        keep = t.buf.clone()
        t.rows_i32[r, c] ^= 1
        with pytest.raises(AssertionError):
            t.assert_live_equals(flat)
        t.buf.copy_(keep)
    t.assert_live_equals(flat)
    keep = t.buf.clone()
    t.rows[5, 7] = -0.0                                  # component k of V: -0 is not the +0 the header asks for
    with pytest.raises(AssertionError):
        t.assert_zero_components()
    t.buf.copy_(keep)
    t.assert_zero_components()
    flat.bias[1] = 1.0
    with pytest.raises(AssertionError):
        t.assert_live_equals(flat)


def test_guarded_buffer_checker_fails_on_a_write_past_its_bytes():
    ptr, check, view = ag.guarded(40, device="cpu")
    assert ptr % 16 == 0 and view.numel() == 10 and not view.any()
    check()
    view[:] = 3.0                                        # the payload is the caller's
    check()
    g = ag.Guarded(40, device="cpu", name="ws")
    for word in (ag.Guarded.HEAD + 10, ag.Guarded.HEAD - 1, g.buf.numel() - 1):
        keep = g.buf.clone()
        g.buf[word] = 0
        with pytest.raises(AssertionError):
            g.check()
        g.buf.copy_(keep)
        g.check()
    s = ag.GuardSet(device="cpu")
    a = s.new("a", (3, 4), out=True, src=np.arange(12))
    s.raw("w", 64)
    s.check()
    assert s.outputs()["a"].shape == (3, 4)
    a.buf[ag.Guarded.HEAD + 12] = 7
    with pytest.raises(AssertionError):
        s.check()


# ---------------------------------------------------------------------------------------------------------------
# check_table's boundary (pointers never dereferenced: every call returns from its host-side checks)
# ---------------------------------------------------------------------------------------------------------------
def _fake(layout, k, kp, z_offset, row_stride, rows=0x10000):
    import fmx
    L = fmx._lib
    t = L.Table()
    t.rows, t.field_offsets, t.bias = rows, 0x20000, 0x30000
    t.n_rows, t.n_fields, t.k, t.kp = 100, 2, k, kp
    t.layout, t.z_offset, t.row_stride = ag.LAYOUT_IDS[layout], z_offset, row_stride
    t.max_field_rows = 50
    return t


def _verdicts(t):
    """(fmx_workspace_bytes, the status of a launching entry point that returns before any launch)."""
    import fmx
    L = fmx._lib
    lib = L.load()
    nbytes = int(lib.fmx_workspace_bytes(C.byref(t), 64))
    # a null `out` is refused right after the table: an accepted table answers ERR_ARG ("null argument"), a refused one its own code
    rc = lib.fmx_fm_forward(C.byref(t), fmx.Hyper().ref(), 0x60000, None, None, 64, L.LOSS_NONE, 1.0, None, None)
    return nbytes, rc, lib.fmx_last_error_string().decode()


ACCEPTED = [("weights", 4, 4, 0, 8), ("weights", 16, 16, 0, 20), ("weights", 61, 64, 0, 68), ("weights", 16, 16, 0, 68),
            ("ftrl", 4, 4, 8, 16), ("ftrl", 7, 8, 12, 28), ("ftrl", 16, 16, 20, 52), ("ftrl", 24, 32, 36, 100),
            ("ftrl", 61, 64, 68, 196), ("moments", 16, 16, 20, 52), ("moments", 16, 16, 36, 80), ("moments", 61, 64, 68, 196),
            ("moments", 4, 4, 8, 16), ("ftrl", 1, 16, 20, 52)]


@pytest.mark.parametrize("geom", ACCEPTED, ids=lambda g: "-".join(str(v) for v in g))
def test_check_table_accepts_the_minimum_geometries(geom):
    import fmx
    nbytes, rc, msg = _verdicts(_fake(*geom))
    assert nbytes > 0 and nbytes % 16 == 0
    assert rc == fmx._lib.ERR_ARG and "null argument" in msg, (rc, msg)          # past check_table, stopped by the null `out`


def _refused():
    import fmx
    L = fmx._lib
    cases = []
    for layout in ("ftrl", "moments"):
        cases += [((layout, 16, 16, 16, 64), L.ERR_SHAPE, "z_offset = kp"),
                  ((layout, 16, 16, 18, 64), L.ERR_SHAPE, "z_offset = kp + 2: not a multiple of 4"),
                  ((layout, 16, 16, 22, 64), L.ERR_SHAPE, "z_offset = kp + 6: not a multiple of 4"),
                  ((layout, 16, 16, 20, 48), L.ERR_SHAPE, "row_stride = need - 4"),
                  ((layout, 16, 16, 20, 54), L.ERR_SHAPE, "row_stride = need + 2"),
                  ((layout, 61, 64, 68, 192), L.ERR_SHAPE, "row_stride = need - 4 at kp = 64")]
    cases += [(("weights", 16, 16, 0, 16), L.ERR_SHAPE, "row_stride = need - 4"),
              (("weights", 16, 16, 0, 22), L.ERR_SHAPE, "row_stride = need + 2"),
              (("weights", 4, 4, 0, 4), L.ERR_SHAPE, "row_stride = kp"),
              (("weights", 12, 12, 0, 32), L.ERR_SHAPE, "kp = 12"),
              (("ftrl", 12, 12, 16, 64), L.ERR_SHAPE, "kp = 12"),
              (("weights", 17, 16, 0, 32), L.ERR_SHAPE, "k = kp + 1"),
              (("moments", 5, 4, 8, 16), L.ERR_SHAPE, "k = kp + 1")]
    return cases


def test_check_table_refuses_with_the_documented_code():
    import fmx
    L = fmx._lib
    for geom, want, why in _refused():
        nbytes, rc, msg = _verdicts(_fake(*geom))
        assert nbytes < 0, (why, geom)
        assert rc == want, (why, geom, rc, msg)
    for layout, geom in (("weights", (16, 16, 0, 20)), ("ftrl", (16, 16, 20, 52)), ("moments", (16, 16, 20, 52))):
        for off in (4, 8, 12):
            nbytes, rc, msg = _verdicts(_fake(layout, *geom, rows=0x10000 + off))
            assert nbytes < 0 and rc == L.ERR_ALIGN, (layout, off, rc, msg)
        nbytes, rc, msg = _verdicts(_fake(layout, *geom, rows=0x10000 + 16))          # 16-byte aligned and no more: accepted
        assert nbytes > 0 and rc == L.ERR_ARG and "null argument" in msg, (layout, rc, msg)


def _afm_verdict(t):
    """fmx_afm_forward on a fake table of two fields: its table check is the shared one (behind the entry point's name), and a
    null `idx` is refused right after it -- an accepted table answers ERR_ARG ("null argument"), a refused one its own code."""
    import fmx
    L = fmx._lib
    lib = L.load()
    afm = L.Afm(0x40000, t.k, 4)
    rc = lib.fmx_afm_forward(C.byref(t), C.byref(afm), fmx.Hyper().ref(), None, None, None, 64, L.LOSS_NONE, 1.0, None, None, None, None)
    return rc, lib.fmx_last_error_string().decode()


# the FTRL and MOMENTS rows the attentional FM's own table check used to let through (it asked for row_stride >= kp + 4 and
# never looked at z_offset): (geometry, the shared check's message)
AFM_NEWLY_REFUSED = [(("ftrl", 16, 16, 16, 64), "z_offset=16 must be a multiple of 4 and >= kp + 4 = 20"),
                     (("ftrl", 16, 16, 20, 48), "row_stride=48 must be a multiple of 4 and >= 52"),
                     (("moments", 16, 16, 16, 64), "z_offset=16 must be a multiple of 4 and >= kp + 4 = 20"),
                     (("moments", 16, 16, 20, 48), "row_stride=48 must be a multiple of 4 and >= 52"),
                     (("ftrl", 61, 64, 64, 256), "z_offset=64 must be a multiple of 4 and >= kp + 4 = 68"),
                     (("moments", 61, 64, 68, 192), "row_stride=192 must be a multiple of 4 and >= 196")]


@pytest.mark.parametrize("geom,message", AFM_NEWLY_REFUSED, ids=["-".join(str(v) for v in g) for g, _ in AFM_NEWLY_REFUSED])
def test_afm_refuses_ftrl_and_moments_rows_that_do_not_hold_both_halves(geom, message):
    import fmx
    rc, msg = _afm_verdict(_fake(*geom))
    assert rc == fmx._lib.ERR_SHAPE and msg == "fmx_afm_forward: " + message, (rc, msg)


@pytest.mark.parametrize("geom", ACCEPTED, ids=lambda g: "-".join(str(v) for v in g))
def test_afm_accepts_the_minimum_geometries(geom):
    import fmx
    rc, msg = _afm_verdict(_fake(*geom))
    assert rc == fmx._lib.ERR_ARG and msg == "fmx_afm_forward: null argument", (rc, msg)     # past the table check, stopped by the null `idx`


def test_flat_table_row_stride_takes_what_the_c_side_takes():
    import fmx
    lib = fmx._lib.load()
    for layout in ("weights", "ftrl", "moments"):
        for k in (4, 7, 16, 24, 61):
            kp = fmx.table.padded_k(k)
            zo, default = ag.default_geometry(layout, kp)
            nd = ag.need(layout, kp, zo)
            for stride in (nd, nd + 4, nd + 12, 2 * default + 4):
                t = fmx.FlatTable([5, 9], k, layout=layout, device="cpu", row_stride=stride)
                assert (t.row_stride, t.z_offset) == (stride, zo) and t.rows.shape == (14, stride)
                assert lib.fmx_workspace_bytes(t.c_struct(), 64) > 0, (layout, k, stride)
            for stride in (nd - 4, nd + 2, nd + 1, kp):
                with pytest.raises(ValueError):
                    fmx.FlatTable([5, 9], k, layout=layout, device="cpu", row_stride=stride)
                assert lib.fmx_workspace_bytes(C.byref(_fake(layout, k, kp, zo, stride)), 64) < 0, (layout, k, stride)


def test_online_run_mlp_fit_mode_takes_weights_tables_only():
    """Why the GPU file runs the fit mode of fmx_online_run_mlp on weights-layout geometries only: the fit step takes SIGNADAM or
    SGD, which pair with that layout; an FTRL or MOMENTS table is refused before anything is launched (Hedge reads any layout)."""
    import fmx
    L = fmx._lib
    lib = L.load()
    m = L.Mlp(0x80000, 2, 16, 8, 0)
    out = L.FwdOut()
    out.S = out.bi = out.sfirst = out.logit = 0x40000
    for layout, rule in (("ftrl", L.RULE_FTRL), ("ftrl", L.RULE_SIGNADAM), ("ftrl", L.RULE_SGD), ("moments", L.RULE_SGD)):
        t = _fake(layout, 16, 16, 20, 52)
        rc = lib.fmx_online_run_mlp(C.byref(t), fmx.Hyper().ref(), rule, L.LOSS_BCE_LOGITS, C.byref(m), 0, 1, 0.0, 0.0, None, 0x60000, None,
                                    0x70000, 4, 0x50000, 1 << 40, C.byref(out), 0xD0000, 0xE0000, None)
        assert rc == L.ERR_ARG, (layout, rule, rc, lib.fmx_last_error_string())


# ---------------------------------------------------------------------------------------------------------------
# a mapped table that ends in an empty field keeps one readable row behind n_rows
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3, 4, 16])
def test_mapped_table_ending_in_an_empty_field_has_a_spare_row(world):
    from fmx.plan import OwnerPlan
    plan = OwnerPlan(CRITEO_SIZES, 16, world)
    seen = 0
    for g in range(world):
        fields = plan.owner_fields(g)
        for layout in ("weights", "ftrl"):
            t = plan.table_for_owner(g, layout=layout, device="cpu")
            assert t.mapped and t.n_rows == sum(r for _, _, r in fields) and t.rows.shape == (t.n_rows, t.row_stride)
            floats = t.rows.untyped_storage().nbytes() // 4 - t.rows.storage_offset()
            assert floats >= (t.n_rows + 1) * t.row_stride, "no readable row behind n_rows"
            assert t.rows.is_contiguous() and not t.rows.any()
        seen += fields[-1][2] == 0
    assert seen >= 1, "no rank table of this plan ends in an empty field: the case is not covered"


def test_unmapped_tables_are_allocated_as_before():
    import fmx
    t = fmx.FlatTable([5, 9], 16, device="cpu")
    assert t.rows.untyped_storage().nbytes() == 14 * t.row_stride * 4
