"""k_sftrl_online (fmx_sftrl_run / fmx_sftrl_grid through the C ABI) against the float64 statement of tests/sftrl_f64.py, at the
edges the stream tests of test_sftrl_gpu.py never reach: ONE shrink per launch on a preloaded sketch whose spectrum is prescribed
(ties, a flat tail at the shift, exact rank deficiency, eigenvalues under thres, a Gram matrix that is already diagonal; d = 1, 2,
odd d, m = 1, m = d, m > d), the launch that needs more than 64 KiB of LDS (d = 32, m = 48 / 64 with 64 features), streams at those
limits, and the grid at m_max = 64.  thres = 1e-12 throughout.  The tolerance on B B^T is sftrl_f64's derived one:
64 d eps lambda_max (1 + w_cut / gap_cut), absolute, entrywise.

Measured on an MI355X (printed by the tests): the device's worst |B B^T - P| / tol over the 85 x 4 one-shrink launches is 0.0130
(d3-m2-rank_deficient, P, reg); the host Sketch's over the same cases is 0.0113 (tests/test_sftrl_shrink_cpu.py)."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from sftrl_f64 import (EPS, THRES, case_state, cases, other_state, run_stream_ref, sample_for_append, shrink_ref, spectrum_for,
                       state_for_spectrum)

pytestmark = pytest.mark.gpu

CASES = cases()
WORST = {}


def device_run(X, y, d, m, eta, task, BP, BN, counts, w=None, g_w=None):
    """One fmx_sftrl_run on copies of the state -> dict(pred, BP, BN, counts, w, g_w, status), all numpy."""
    import fmx
    lib = fmx._lib.load()
    dev = torch.device("cuda")
    X, y = np.ascontiguousarray(X, np.float64), np.ascontiguousarray(y, np.float64)
    N, D = X.shape
    assert BP.shape == BN.shape == (d, 2 * m) and BP.dtype == BN.dtype == np.float64 and d <= D
    assert 0 <= min(counts) and max(counts) <= 2 * m - 2
    assert np.isfinite(BP).all() and np.isfinite(BN).all() and np.isfinite(X).all() and np.isfinite(y).all()
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    t = dict(X=put(X), y=put(y), BP=put(BP), BN=put(BN), counts=torch.tensor(list(counts), dtype=torch.int32, device=dev),
             pred=torch.zeros(N, dtype=torch.float64, device=dev), status=torch.zeros(2, dtype=torch.int32, device=dev))
    if w is not None:
        assert w.shape == g_w.shape == (D,)
        t["w"], t["g_w"] = put(w), put(g_w)
    p = lambda k: C.c_void_p(t[k].data_ptr()) if k in t else None
    rc = lib.fmx_sftrl_run(p("X"), p("y"), N, D, d, m, float(eta), THRES, 0 if task == "cls" else 1, p("BP"), p("BN"), p("counts"), p("w"),
                           p("g_w"), p("pred"), p("status"), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.fmx_last_error_string()
    torch.cuda.synchronize()
    out = {k: t[k].cpu().numpy() for k in ("pred", "BP", "BN", "status") + (("w", "g_w") if w is not None else ())}
    out["counts"] = tuple(int(c) for c in t["counts"].cpu())
    return out


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def one_shrink(cid, d, m, D, target, v, to, task, rng, scale=1.0):
    """Preload `target` (count 2m - 2) as sketch `to` and a small random state as the other one, feed the one sample that appends v,
    and hold what comes back against the float64 statement.  -> err / tol of the new sketch's Gram matrix."""
    B, count = target
    oB, ocount = other_state(d, m, rng)
    BP, BN, counts = (B, oB, (count, ocount)) if to == "P" else (oB, B, (ocount, count))
    x, y, eta, vec = sample_for_append(v, to, task, BP, BN, D, rng, scale)
    ref = run_stream_ref(x[None, :], [y], d, m, eta, THRES, task, BP, BN, counts)
    full = B.copy()
    full[:, -1] = vec
    r = shrink_ref(full, m)
    assert np.abs(vec - v).max() <= 8 * EPS * np.abs(v).max()                                   # the sample appends what was prescribed
    assert ref["counts"] == ((r.keep, ocount) if to == "P" else (ocount, r.keep))
    out = device_run(x[None, :], [y], d, m, eta, task, BP, BN, counts)
    assert tuple(out["status"]) == (0, 0), (cid, to, task)
    new, other, k_new, k_other = (out["BP"], out["BN"], *out["counts"]) if to == "P" else (out["BN"], out["BP"], *out["counts"][::-1])
    assert k_new == r.keep, (cid, to, task, k_new, r.keep)
    assert k_other == ocount and same_bits(other, oB), (cid, to, task)                          # the other sketch: bit-unchanged
    err = float(np.abs(new @ new.T - r.P).max())
    floor, y_hat, pred = ref["floor"][0], ref["y_hat"][0], out["pred"][0]
    print(f"{cid} {to} {task}: keep {k_new}, |B B^T - P| {err:.3g}, tol {r.tol:.3g}, err/tol {err / r.tol:.4f}; y_hat {y_hat:.6g}, "
          f"pred {pred:.6g}, floor {floor:.3g}")
    assert err <= r.tol, (cid, to, task, err, r.tol)
    tail = new[:, r.keep:]
    assert not tail.any() and not np.signbit(tail).any(), (cid, to, task)                       # columns >= keep: exactly +0
    if task == "reg":
        assert abs(pred - y_hat) <= floor, (cid, to, pred, y_hat, floor)
    else:
        assert pred in (1.0, -1.0)
        if abs(y_hat) > floor:
            assert pred == (1.0 if y_hat >= 0 else -1.0), (cid, to, pred, y_hat, floor)
    return err / r.tol


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_one_shrink_per_launch(case):
    """N = 1 on a preloaded state of count 2m - 2: a unit test of sftrl_shrink through the public entry point, on both sketches and
    both tasks.  Asserts: counts = the reference's keep, the other sketch and its count bit-unchanged, B B^T within tol of P,
    columns >= keep exactly +0, pred[0] within the y_hat floor (reg) / of the right sign where |y_hat| exceeds it (cls), status 0."""
    cid, d, m, D, fam, s = case
    B, count, v = case_state(case)
    rng = np.random.default_rng([d, m, len(fam), 77])
    for to, task in itertools.product("PN", ("reg", "cls")):
        WORST[(cid, to, task)] = one_shrink(cid, d, m, D, (B, count), v, to, task, rng)
    k = max(WORST, key=WORST.get)
    print(f"worst device err/tol so far: {WORST[k]:.4f} at {k} ({len(WORST)} launches)")


def test_count_is_the_exact_rank_where_the_host_path_counts_noise():
    """d = 9 < m = 64, lambda_max = 1e8 (outside the input conditions on purpose): the exact rank is 9.  The device decomposes the
    9 x 9 matrix and keeps 9; the host Sketch keeps m - 1 = 63 there, because the trailing singular values of its 128 x 128 matrix are
    rounding noise ~ 1e-8 > thres (tests/test_sftrl_shrink_cpu.py::test_host_count_leaves_the_exact_rank_under_a_large_norm).  This is
    the device's defined behaviour; B B^T is within the same tolerance."""
    d, m = 9, 64
    B, count, v = state_for_spectrum(d, m, 1e8 * spectrum_for(d, m, "geometric"), np.random.default_rng(964))
    rng = np.random.default_rng(965)
    for to, task in itertools.product("PN", ("reg", "cls")):
        full = B.copy()
        full[:, -1] = v
        assert shrink_ref(full, m).keep == d
        one_shrink("d9-m64-1e8", d, m, d, (B, count), v, to, task, rng, scale=2.0 ** 24)


# ---- streams at the limits ---------------------------------------------------------------------------------------------------------

def make_stream(n, D, seed, task):
    """test_sftrl_gpu.make_stream's data (X / sqrt(D), a linear plus a bilinear target), for any D >= 1."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, D)) / np.sqrt(D)
    wt = rng.standard_normal(D)
    s = X @ wt + 0.5 * (X[:, 0] * X[:, 1 % D] - X[:, 2 % D] * X[:, -1]) * D
    y = np.where(s >= 0, 1.0, -1.0) if task == "cls" else s
    return X, y


def assert_stream_state(out, ref, task, lin, tag):
    if task == "cls":
        assert (out["pred"] != ref["pred"]).sum() <= 1, tag
    else:
        np.testing.assert_allclose(out["pred"], ref["pred"], rtol=1e-7, atol=1e-10, err_msg=tag)
    assert out["counts"] == ref["counts"], tag
    np.testing.assert_allclose(out["BP"] @ out["BP"].T, ref["GP"], rtol=1e-7, atol=1e-10, err_msg=tag)
    np.testing.assert_allclose(out["BN"] @ out["BN"].T, ref["GN"], rtol=1e-7, atol=1e-10, err_msg=tag)
    if lin:
        np.testing.assert_allclose(out["w"], ref["w"], rtol=1e-9, atol=1e-12, err_msg=tag)
        np.testing.assert_allclose(out["g_w"], ref["g_w"], rtol=1e-9, atol=1e-12, err_msg=tag)
    assert tuple(out["status"]) == (0, 0), tag


@pytest.mark.parametrize("task", ["cls", "reg"])
@pytest.mark.parametrize("D,d,m,lin,legs", [(64, 32, 64, True, 2), (32, 32, 48, False, 2), (2, 1, 1, True, 1), (8, 8, 1, False, 1)])
def test_streams_at_the_limits(D, d, m, lin, legs, task):
    """400 samples per leg against run_stream_ref under the stream tests' tolerances (1e-7 relative / 1e-10 on the Gram matrices and
    reg predictions, at most one flipped cls prediction, counts exact, w at 1e-9): the two launches beyond 64 KiB of LDS (83 KB with
    the linear term over 64 features, d = 32 only reachable through the C ABI; 66 KB), each with a second leg continued from the first
    one's device state, and m = 1, where every append shrinks and both sketches stay exactly zero."""
    X, y = make_stream(400 * legs, D, 11 + D + d + m, task)
    z = lambda *s: np.zeros(s, np.float64)
    state = dict(BP=z(d, 2 * m), BN=z(d, 2 * m), counts=(0, 0), w=z(D) if lin else None, g_w=z(D) if lin else None)
    for leg in range(legs):
        Xl, yl = X[400 * leg:400 * (leg + 1)], y[400 * leg:400 * (leg + 1)]
        ref = run_stream_ref(Xl, yl, d, m, 0.03, THRES, task, **state)
        out = device_run(Xl, yl, d, m, 0.03, task, **state)
        assert_stream_state(out, ref, task, lin, f"leg {leg}")
        if m == 1:
            assert out["counts"] == (0, 0) and same_bits(out["BP"], z(d, 2)) and same_bits(out["BN"], z(d, 2))
            if not lin:                                                # ... after EVERY sample: each y_hat is then exactly 0
                assert same_bits(out["pred"], z(400) if task == "reg" else z(400) + 1.0)
            for n in (1, 2, 7):                                        # and at shorter prefixes of the stream
                o = device_run(Xl[:n], yl[:n], d, m, 0.03, task, **state)
                assert o["counts"] == (0, 0) and same_bits(o["BP"], z(d, 2)) and same_bits(o["BN"], z(d, 2))
                assert same_bits(o["pred"], out["pred"][:n])
        else:
            assert max(out["counts"]) <= 2 * m - 2 and min(ref["counts"]) > 0
        state = dict(BP=out["BP"], BN=out["BN"], counts=out["counts"], w=out.get("w"), g_w=out.get("g_w"))


@pytest.mark.parametrize("task", ["cls", "reg"])
def test_grid_at_the_limits_equals_single_runs(task):
    """fmx_sftrl_grid with d = 32, m_max = 64, 64 features and the linear term, ms = [1, 48, 64, 2] from preloaded states: four
    workgroups of a launch sized for 83 KB of LDS, every stride in use -- the bits of the four single runs, and nothing written past
    a setting's own [d, 2 ms[s]] block of its slab."""
    import fmx
    lib = fmx._lib.load()
    dev = torch.device("cuda")
    N, D, d, m_max, ms, etas = 400, 64, 32, 64, [1, 48, 64, 2], [0.03, 0.05, 0.02, 0.04]
    S = len(ms)
    X, y = make_stream(N, D, 5, task)
    rng = np.random.default_rng(6)
    BP, BN = np.full((S, d * 2 * m_max), 7.0), np.full((S, d * 2 * m_max), -7.0)
    counts, w, g_w, singles = np.zeros((S, 2), np.int32), np.zeros((S, D)), 0.01 * rng.standard_normal((S, D)), []
    for s, (m, eta) in enumerate(zip(ms, etas)):
        (bp, cp), (bn, cn) = other_state(d, m, rng), other_state(d, m, rng)
        BP[s, :d * 2 * m], BN[s, :d * 2 * m], counts[s] = bp.reshape(-1), bn.reshape(-1), (cp, cn)
        w[s] = -eta * g_w[s]
        singles.append(device_run(X, y, d, m, eta, task, bp, bn, (cp, cn), w[s].copy(), g_w[s].copy()))
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    t = dict(X=put(X), y=put(y), ms=torch.tensor(ms, dtype=torch.int32, device=dev), etas=put(np.array(etas)), BP=put(BP), BN=put(BN),
             counts=put(counts), w=put(w), g_w=put(g_w), pred=torch.zeros((S, N), dtype=torch.float64, device=dev),
             status=torch.zeros((S, 2), dtype=torch.int32, device=dev))
    p = lambda k: C.c_void_p(t[k].data_ptr())
    rc = lib.fmx_sftrl_grid(p("X"), p("y"), N, D, d, S, p("ms"), p("etas"), m_max, THRES, 0 if task == "cls" else 1, p("BP"), p("BN"),
                            p("counts"), p("w"), p("g_w"), p("pred"), p("status"), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.fmx_last_error_string()
    torch.cuda.synchronize()
    g = {k: t[k].cpu().numpy() for k in ("BP", "BN", "counts", "w", "g_w", "pred", "status")}
    assert not g["status"].any()
    for s, (m, one) in enumerate(zip(ms, singles)):
        n = d * 2 * m
        assert same_bits(g["BP"][s, :n], one["BP"].reshape(-1)) and same_bits(g["BN"][s, :n], one["BN"].reshape(-1)), s
        assert (g["BP"][s, n:] == 7.0).all() and (g["BN"][s, n:] == -7.0).all(), s
        assert tuple(g["counts"][s]) == one["counts"], s
        assert same_bits(g["w"][s], one["w"]) and same_bits(g["g_w"][s], one["g_w"]) and same_bits(g["pred"][s], one["pred"]), s
        if m == 1:
            assert one["counts"] == (0, 0) and not one["BP"].any() and not one["BN"].any()
        else:
            assert max(one["counts"]) > 0
