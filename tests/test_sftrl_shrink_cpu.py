"""tests/sftrl_f64.py is right, and the comparison it serves has power.  No device is touched.

shrink_ref (numpy eigh of B B^T) against 40-digit arithmetic (mpmath.eigsy) and against the host Sketch (LAPACK's SVD of B^T B) on
every (geometry, family) case of tests/test_sftrl_shrink_gpu.py, inside the derived tolerance of sftrl_f64's docstring; the stream
loop against the host classes' loop; four mutated shrinks that the same comparison must reject; and the one place where the host
path's column count is NOT the exact rank logic (d < m under a large sketch norm).

Measured (printed by test_shrink_ref_equals_the_host_sketch and the mpmath test), worst err / tol over all 85 cases: the host
Sketch against shrink_ref 0.0113 (d9-m64-wide), shrink_ref against 40 digits 0.0065."""
import numpy as np
import pytest

from sftrl_f64 import (EPS, FAMILIES, GEOMETRIES, THRES, case_state, cases, cut_tolerance, run_stream_ref, shrink_ref, spectrum_for,
                       state_for_spectrum)

CASES = cases()


def full_buffer(case):
    B, count, v = case_state(case)
    assert count == B.shape[1] - 2 and not B[:, 0].any() and not B[:, -1].any()
    B[:, count + 1] = v
    return B


def test_every_geometry_and_family_is_covered_and_meets_the_input_conditions():
    """Each geometry has its geometric and diagonal case, each family exists at some geometry, and every case meets the input
    conditions under which P is defined (sftrl_f64's docstring), checked on the spectrum the built buffer really has."""
    assert {(c[1], c[2]) for c in CASES} == set(GEOMETRIES) and {c[4] for c in CASES} == set(FAMILIES)
    assert len(CASES) == len({c[0] for c in CASES}) == 85
    for case in CASES:
        cid, d, m, D, fam, s = case
        lam = np.sort(np.linalg.eigvalsh((lambda B: B @ B.T)(full_buffer(case))))[::-1]
        assert np.abs(lam - s).max() <= 16 * EPS * s[0], cid                        # the prescribed spectrum
        assert lam[0] <= 2.0, cid
        assert ((lam >= 0.99e-10) | (lam <= 1.01e-13)).all(), cid                   # nothing between thres / 10 and 100 thres
        r = shrink_ref(full_buffer(case), m)
        if 0 < r.keep < d:
            w_cut, gap = r.lam[r.keep - 1] - r.shift, r.lam[r.keep - 1] - r.lam[r.keep]
            assert gap >= 1e-3 * r.lam[r.keep - 1] or w_cut <= 16 * EPS * lam[0], cid
    # the edges the families are there for
    keeps = {c[0]: shrink_ref(full_buffer(c), c[2]) for c in CASES}
    assert keeps["d1-m1-geometric"].keep == 0 and keeps["d2-m1-geometric"].keep == 0          # m = 1: every append empties the sketch
    assert keeps["d5-m5-geometric"].keep == 4 and keeps["d5-m5-geometric"].shift == 0.0       # m = d: no shift
    assert keeps["d9-m64-geometric"].keep == 9 and keeps["d32-m64-wide"].keep == 32           # m > d: keep the rank
    assert keeps["d16-m8-rank_deficient"].keep == 7 and keeps["d16-m8-under_thres"].keep == 7  # nnz < m < d
    assert keeps["d8-m4-flat_tail"].shift == pytest.approx(0.25, rel=1e-14)
    assert keeps["d31-m16-flat_tail"].lam[15] == pytest.approx(keeps["d31-m16-flat_tail"].lam[16], rel=1e-13)  # the tie at the shift


MP_WORST = {}


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_shrink_ref_against_40_digits(case):
    import mpmath as mp
    cid, d, m, D, fam, s = case
    B = full_buffer(case)
    r = shrink_ref(B, m)
    with mp.workdps(40):
        Bm = mp.matrix(B.tolist())
        E, Q = mp.eigsy(Bm * Bm.T)
        order = sorted(range(d), key=lambda i: -E[i])
        lam = [E[i] if E[i] > mp.mpf(THRES) else mp.mpf(0) for i in order]
        nnz = sum(1 for x in lam if x != 0)
        if nnz >= m:
            keep, shift = m - 1, (lam[m] if m < d else mp.mpf(0))
        else:
            keep, shift = nnz, mp.mpf(0)
        P = mp.zeros(d, d)
        for i in range(keep):
            v = Q[:, order[i]]
            P += (lam[i] - shift) * (v * v.T)
        P = np.array([[float(P[i, j]) for j in range(d)] for i in range(d)])
    assert keep == r.keep
    err = float(np.abs(P - r.P).max()) if d else 0.0
    MP_WORST[cid] = err / r.tol
    print(f"{cid}: keep {keep}, |P - P40| {err:.3g}, tol {r.tol:.3g}, err/tol {err / r.tol:.4f}; worst so far {max(MP_WORST.values()):.4f}")
    assert err <= r.tol


def test_shrink_ref_equals_the_host_sketch():
    """The host path (LAPACK SVD of the 2m x 2m matrix) on every case: equal counts, Gram matrix inside the tolerance, columns
    >= keep zero -- 100 % of the cases, none skipped.  Prints the worst err / tol (DESIGN section 4 quotes it)."""
    from models.models_online._sketch import Sketch
    worst, n = (0.0, ""), 0
    for case in CASES:
        cid, d, m, D, fam, s = case
        B, count, v = case_state(case)
        S = Sketch(d, m, THRES)
        S.B, S.count = B.copy(), count
        S.append(v)
        r = shrink_ref(full_buffer(case), m)
        assert S.count == r.keep, cid
        assert not S.B[:, r.keep:].any(), cid
        err = float(np.abs(S.B @ S.B.T - r.P).max())
        assert err <= r.tol, (cid, err, r.tol)
        assert float(np.abs(r.B @ r.B.T - r.P).max()) <= 8 * EPS * max(r.lam[0], 1e-300) * d, cid   # the reference's own buffer is P
        worst = max(worst, (err / r.tol, cid))
        n += 1
    print(f"host Sketch vs shrink_ref over {n} cases: worst err/tol {worst[0]:.4f} at {worst[1]}")
    assert n == len(CASES) == 85
    assert worst[0] < 0.25                 # a reference that used up its own tolerance would leave none to the device


def test_tolerance_formula():
    lam = np.array([1.0, 0.5, 0.25, 0.0])
    assert cut_tolerance(lam, 0, 0.0, 4) == 64 * 4 * EPS
    assert cut_tolerance(lam, 4, 0.0, 4) == 64 * 4 * EPS
    assert cut_tolerance(lam, 2, 0.25, 4) == 64 * 4 * EPS * (1 + 0.25 / 0.25)          # w_cut = 0.5 - 0.25, gap = 0.5 - 0.25
    assert cut_tolerance(lam, 1, 0.25, 4) == 64 * 4 * EPS * (1 + 0.75 / 0.5)
    assert cut_tolerance(2 * lam, 3, 0.0, 4) == 64 * 4 * EPS * 2 * (1 + 1.0)
    with pytest.raises(AssertionError):
        cut_tolerance(np.array([1.0, 1.0, 0.5]), 1, 0.5, 3)                           # a tie straddles the cut with weight 0.5


# ---- power: four wrong shrinks ----------------------------------------------------------------------------------------------------

def shrink_mutant(B, m, thres, kind):
    """shrink_ref's steps with one of them wrong -> (P, keep)."""
    d = B.shape[0]
    lam, V = np.linalg.eigh(B @ B.T)
    lam, V = lam[::-1].copy(), V[:, ::-1]
    if kind != "no_threshold":
        lam[lam <= thres] = 0.0
    nnz = int(np.count_nonzero(lam > 0))
    if nnz >= m:
        keep = m if kind == "keep_m" else m - 1
        keep = min(keep, d)
        if kind == "shift_from_m_minus_1":
            shift = float(lam[m - 1]) if m < d else 0.0
        elif kind == "shift_when_m_ge_d":
            shift = float(lam[min(m, d - 1)])
        else:
            shift = float(lam[m]) if m < d else 0.0
    else:
        keep, shift = nnz, 0.0
    wts = np.maximum(lam[:keep] - shift, 0.0)
    return (V[:, :keep] * wts[None, :]) @ V[:, :keep].T, keep


MUTANTS = {"shift_from_m_minus_1": "geometric", "keep_m": "geometric", "no_threshold": "under_thres", "shift_when_m_ge_d": "geometric"}


def test_the_unmutated_copy_is_shrink_ref():
    for case in CASES:
        B = full_buffer(case)
        r = shrink_ref(B, case[2])
        P, keep = shrink_mutant(B, case[2], THRES, "none")
        assert keep == r.keep and np.array_equal(P, r.P), case[0]


@pytest.mark.parametrize("kind", list(MUTANTS))
def test_a_mutated_shrink_is_rejected(kind):
    """Each wrong shrink leaves the tolerance, or gives another count, on at least one case of the family aimed at it."""
    caught = []
    for case in CASES:
        if case[4] != MUTANTS[kind]:
            continue
        B = full_buffer(case)
        r = shrink_ref(B, case[2])
        P, keep = shrink_mutant(B, case[2], THRES, kind)
        if keep != r.keep or np.abs(P - r.P).max() > r.tol:
            caught.append(case[0])
    print(f"{kind}: rejected on {len(caught)} cases of {MUTANTS[kind]}: {caught}")
    assert caught


# ---- the stream loop ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,task,D,m", [("SFTRL_CCFM", "cls", 32, 8), ("SFTRL_CCFM", "reg", 20, 32), ("SFTRL_Vanila", "cls", 33, 5),
                                            ("SFTRL_Vanila", "reg", 9, 64), ("SFTRL_CCFM", "cls", 6, 6), ("SFTRL_CCFM", "reg", 3, 1 + 1)])
def test_run_stream_ref_equals_the_host_classes(name, task, D, m, capsys):
    """tests/test_sftrl_gpu.py's streams and tolerances: 1e-7 relative on the Gram matrices and the predictions, counts exact; a second
    leg continued from the first one's state."""
    import torch
    from test_sftrl_gpu import classes, make_stream
    X, y = make_stream(700, D, 3 + D + m, task)
    cls = classes()[name]
    lin = name == "SFTRL_Vanila"
    d = D - 1 if lin else D
    state = dict(BP=np.zeros((d, 2 * m)), BN=np.zeros((d, 2 * m)), counts=(0, 0), w=np.zeros(D) if lin else None,
                 g_w=np.zeros(D) if lin else None)
    for lo, hi in ((0, 400), (400, 700)):
        host = cls(torch.DoubleTensor(X[lo:hi]), torch.DoubleTensor(y[lo:hi]), task, 0.03, m)
        host.BT_P, host.BT_N = torch.from_numpy(state["BP"].copy()), torch.from_numpy(state["BN"].copy())
        host.row_count_p, host.row_count_n = state["counts"]
        if lin:
            host.w, host.g_w = torch.from_numpy(state["w"].reshape(-1, 1).copy()), torch.from_numpy(state["g_w"].reshape(-1, 1).copy())
        ph, _, _ = host.online_learning()
        capsys.readouterr()
        ref = run_stream_ref(X[lo:hi], y[lo:hi], d, m, 0.03, THRES, task, **state)
        if task == "cls":
            assert (ph.reshape(-1) != ref["pred"]).sum() <= 1
        else:
            np.testing.assert_allclose(ref["pred"], ph.reshape(-1), rtol=1e-7, atol=1e-9)
        assert ref["counts"] == (host.row_count_p, host.row_count_n)
        for a, b in ((ref["GP"], host.BT_P), (ref["GN"], host.BT_N)):
            np.testing.assert_allclose(a, (b @ b.t()).numpy(), rtol=1e-7, atol=1e-10)
        if lin:
            np.testing.assert_allclose(ref["w"], host.w.numpy().reshape(-1), rtol=1e-9, atol=1e-12)
        assert (ref["floor"] >= 0).all() and (ref["floor"] <= 1e-10 * (1 + np.abs(ref["y_hat"]).max())).all()
        state = dict(BP=ref["BP"], BN=ref["BN"], counts=ref["counts"], w=ref["w"], g_w=ref["g_w"])


# ---- where the host path's count is not the exact rank ---------------------------------------------------------------------------

def test_host_count_leaves_the_exact_rank_under_a_large_norm():
    """d = 9 < m = 64, the geometric spectrum scaled to lambda_max = 1e8: the exact rank is 9 = d, the d x d route (shrink_ref, the
    device) keeps 9.  The host Sketch decomposes the 128 x 128 matrix B^T B, whose 119 trailing singular values are
    rounding noise of order eps lambda_max ~ 1e-8 -- above thres = 1e-12, so they count: nnz >= m and it keeps m - 1 = 63 columns
    (dividing by the square roots of noise on the way).  The same spectrum at lambda_max = 1 has noise ~ 1e-15 < thres and both keep
    9.  The Gram matrices agree either way, relative to lambda_max."""
    from models.models_online._sketch import Sketch
    d, m = 9, 64
    s = spectrum_for(d, m, "geometric")
    counts = {}
    for scale in (1.0, 1e8):
        B, count, v = state_for_spectrum(d, m, scale * s, np.random.default_rng(964), diagonal=False)
        S = Sketch(d, m, THRES)
        S.B, S.count = B.copy(), count
        S.append(v)
        B[:, -1] = v
        r = shrink_ref(B, m)
        noise = np.linalg.svd(B.T @ B, compute_uv=False)[d:]
        print(f"lambda_max {scale:g}: exact rank {d}, shrink_ref keeps {r.keep}, host Sketch {S.count}; trailing singular values of B^T B "
              f"{noise.min():.2g} .. {noise.max():.2g}; |G_host - P| / tol {np.abs(S.B @ S.B.T - r.P).max() / r.tol:.3g}")
        assert r.keep == d and r.shift == 0.0
        counts[scale] = S.count
        assert np.abs(S.B @ S.B.T - r.P).max() <= r.tol
        assert (noise.max() > THRES) == (scale == 1e8)
    assert counts[1.0] == d
    assert counts[1e8] != d and counts[1e8] == m - 1
