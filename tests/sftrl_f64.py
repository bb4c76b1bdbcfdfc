"""A float64 statement of the sketched-FTRL family (fmx_sftrl_run / fmx_sftrl_grid; csrc/fmx_sftrl.inc) with a derived tolerance,
written from the algorithm as the header comment of fmx_sftrl.inc and models/models_online/_sketch.py state it -- it does not
import the host Sketch, and it takes the OTHER route to the same new sketch: numpy.linalg.eigh of the d x d matrix B B^T (the host
path: LAPACK's SVD of the 2m x 2m matrix B^T B; the device: cyclic Jacobi on B B^T).

The shrink.  lambda_0 >= lambda_1 >= ... the eigenvalues of G = B B^T with eigenvectors v_i; every lambda <= thres is set to 0 and
nnz of them remain.  nnz >= m: keep = m - 1 and shift = lambda_m (0 when m >= d: beyond d the spectrum of B^T B is zero);
otherwise keep = nnz, shift = 0.  The new sketch has the columns sqrt(lambda_i - shift) v_i, i < keep, whose signs (and, inside a
group of equal eigenvalues, whose basis) no one defines; its Gram matrix
    P = sum_{i < keep} (lambda_i - shift) v_i v_i^T
is defined whenever no group of equal eigenvalues straddles the cut with a non-zero weight: a group wholly on one side of the cut
enters through its projector, a group tied AT the shift has weight 0.

The tolerance.  Two evaluations of G differ by about eps ||G|| (a sum of 2m products per entry, then the eigen-solver's backward
error, both small multiples of eps lambda_max); an eigenvalue moves by no more than that (Weyl), and the projector on the kept
eigenvectors turns by about eps ||G|| / gap_cut (Davis-Kahan), gap_cut = lambda_{keep-1} - lambda_keep being the gap AT the cut --
gaps inside the kept group or inside the dropped one do not matter, P only sees the two invariant subspaces.  A turn of the
projector moves P by the weight of what is turned across the cut, w_cut = lambda_{keep-1} - shift.  Entrywise, with 64 d for the
constants (d for the norm of a d x d perturbation, 64 for the lengths of the sums and the two solvers):
    tol = 64 d eps lambda_max (1 + w_cut / gap_cut),      the second term 0 when keep is 0 or d (nothing is cut).
It is an absolute bound on every entry of P.  Input conditions under which it means something: lambda_max <= 2; every eigenvalue
>= 1e-10 (the `wide` family's last one: 100 thres, 1e5 times the rounding noise), or in (0, 1e-13] (under thres by 10), or zero by
construction; the relative gap at the cut >= 1e-3 unless the straddling group is tied at the shift.

Helper module, not collected."""
from types import SimpleNamespace

import numpy as np

EPS = float(np.finfo(np.float64).eps)
THRES = 1e-12


def cut_tolerance(lam, keep, shift, d):
    """lam: the thresholded spectrum, descending -> the absolute entrywise tolerance on P (module docstring)."""
    lam_max = float(lam[0]) if len(lam) else 0.0
    ratio = 0.0
    if 0 < keep < d:
        w_cut = float(lam[keep - 1]) - shift
        gap_cut = float(lam[keep - 1]) - float(lam[keep])
        if w_cut > 0.0:
            assert gap_cut > 0.0, "a group of equal eigenvalues straddles the cut with a non-zero weight: P is not defined"
            ratio = w_cut / gap_cut
    return 64.0 * d * EPS * lam_max * (1.0 + ratio)


def shrink_ref(B, m, thres=THRES):
    """B [d, 2m] float64 (a full buffer) -> namespace(P [d, d], keep, lam [d] thresholded and descending, shift, tol, B [d, 2m]
    one new buffer with that Gram matrix, columns >= keep zero)."""
    B = np.asarray(B, np.float64)
    d, C = B.shape
    assert C == 2 * m
    lam, V = np.linalg.eigh(B @ B.T)
    lam, V = lam[::-1].copy(), V[:, ::-1]
    lam[lam <= thres] = 0.0
    nnz = int(np.count_nonzero(lam))
    if nnz >= m:
        keep, shift = m - 1, (float(lam[m]) if m < d else 0.0)
    else:
        keep, shift = nnz, 0.0
    wts = lam[:keep] - shift
    Bn = np.zeros((d, C), np.float64)
    Bn[:, :keep] = V[:, :keep] * np.sqrt(wts)[None, :]
    P = (V[:, :keep] * wts[None, :]) @ V[:, :keep].T
    return SimpleNamespace(P=P, keep=keep, lam=lam, shift=shift, tol=cut_tolerance(lam, keep, shift, d), B=Bn)


def grad_loss(y_hat, y, cls):
    """d loss / d y_hat: cls (-1 / (1 + e^(y_hat y))) y, reg 2 (y_hat - y)."""
    if cls:
        with np.errstate(over="ignore"):
            return (-1.0 / (1.0 + np.exp(y_hat * y))) * y
    return 2.0 * (y_hat - y)


def run_stream_ref(X, y, d, m, eta, thres, task, BP, BN, counts, w=None, g_w=None):
    """The per-sample loop of fmx_sftrl.inc's header on shrink_ref.  X [N, D], y [N]; BP, BN [d, 2m], counts (p, n), w, g_w [D] or
    None are the state before (not mutated).  task "cls" / "reg".  -> dict(pred [N], y_hat [N], floor [N], BP, BN, GP, GN, counts,
    w, g_w); floor is the float64 rounding floor of every y_hat: 8 eps (d + 2m) (||BP^T x||^2 + ||BN^T x||^2 + sum |w_i x_i|)."""
    X, y = np.asarray(X, np.float64), np.asarray(y, np.float64)
    N, D = X.shape
    cls = task == "cls"
    BP, BN = np.array(BP, np.float64).reshape(d, 2 * m), np.array(BN, np.float64).reshape(d, 2 * m)
    cp, cn = int(counts[0]), int(counts[1])
    lin = w is not None
    if lin:
        w, g_w = np.array(w, np.float64).reshape(D), np.array(g_w, np.float64).reshape(D)
    pred, y_hat, floor = np.empty(N), np.empty(N), np.empty(N)
    for i in range(N):
        x = X[i]
        xs = x[:d]
        tp, tn = BP.T @ xs, BN.T @ xs
        ep, en = float(tp @ tp), float(tn @ tn)
        s = ep - en
        fl = ep + en
        if lin:
            s += float(w @ x)
            fl += float(np.abs(w * x).sum())
        y_hat[i], floor[i] = s, 8.0 * EPS * (d + 2 * m) * fl
        pred[i] = (1.0 if s >= 0 else -1.0) if cls else s
        sign = grad_loss(s, y[i], cls)
        if lin:
            g_w = g_w + sign * x
            w = -eta * g_w
        if sign <= 0:
            cp += 1
            BP[:, cp] = np.sqrt(-eta * sign) * xs
            if cp == 2 * m - 1:
                r = shrink_ref(BP, m, thres)
                BP, cp = r.B, r.keep
        else:
            cn += 1
            BN[:, cn] = np.sqrt(eta * sign) * xs
            if cn == 2 * m - 1:
                r = shrink_ref(BN, m, thres)
                BN, cn = r.B, r.keep
    return dict(pred=pred, y_hat=y_hat, floor=floor, BP=BP, BN=BN, GP=BP @ BP.T, GN=BN @ BN.T, counts=(cp, cn), w=w, g_w=g_w)


# ---- states with a prescribed spectrum -------------------------------------------------------------------------------------------

def state_for_spectrum(d, m, spectrum, rng, diagonal=False):
    """-> (B [d, 2m], count = 2m - 2, v [d]): column 0 and column 2m - 1 of B are zero, and once v is appended as column 2m - 1
    the eigenvalues of B B^T are `spectrum` (length d, descending, at most 2m - 1 of them non-zero) to a few eps lambda_max.
    General case: B[:, 1:] = Q sqrt(diag) W^T with Q a random orthogonal d x d matrix and W random orthonormal columns.
    diagonal: every non-zero row of B has ONE entry, +-sqrt(lambda_i), in a column of its own -- B B^T is diagonal exactly (its
    off-diagonal entries are sums of exact zeros), equal entries of `spectrum` give equal diagonal bits; the rows are in random
    order (the zero rows among them) and v belongs to the smallest non-zero eigenvalue."""
    spectrum = np.asarray(spectrum, np.float64)
    C = 2 * m
    assert spectrum.shape == (d,) and (np.diff(spectrum) <= 0).all() and spectrum[-1] >= 0
    nz = int(np.count_nonzero(spectrum))
    assert 1 <= nz <= C - 1
    full = np.zeros((d, C), np.float64)
    if diagonal:
        cols = np.concatenate([C - nz + rng.permutation(nz - 1), [C - 1]]).astype(int)
        rows = rng.permutation(d)[:nz]                                  # lambda_i sits in row rows[i]: the diagonal is not sorted
        full[rows, cols] = np.sqrt(spectrum[:nz]) * rng.choice([-1.0, 1.0], size=nz)
    else:
        Q, _ = np.linalg.qr(rng.standard_normal((d, d)))
        W, _ = np.linalg.qr(rng.standard_normal((C - 1, nz)))
        full[:, 1:] = (Q[:, :nz] * np.sqrt(spectrum[:nz])[None, :]) @ W.T
    v = full[:, C - 1].copy()
    full[:, C - 1] = 0.0
    return full, C - 2, v


def other_state(d, m, rng):
    """A small random state for the sketch a test does NOT append to: (B [d, 2m], count), columns 0 and > count zero."""
    C = 2 * m
    count = int(rng.integers(0, C - 1)) if m > 1 else 0                # <= 2m - 2
    B = np.zeros((d, C), np.float64)
    B[:, 1:count + 1] = 0.3 * rng.standard_normal((d, count))
    return B, count


APPEND_ETA = {"reg": 1.0, "cls": 128.0}


def sample_for_append(v, to, task, BP, BN, D, rng=None, scale=1.0):
    """The one sample (x [D], y) under eta = APPEND_ETA[task] scale^2 whose step appends v [d] to sketch `to` ("P": sign <= 0,
    "N": sign > 0), and the vector exactly as this float64 evaluation appends it -> (x, y, eta, appended).
    reg: x = v / (8 scale) and y = y_hat +- 32, so sign = -+64 and sqrt(eta |sign|) = 8 scale.  cls: y = +1 (P) / -1 (N), |sign| =
    1 / (1 + e^(+-y_hat)) and x = v / t with t^2 = eta |sign(y_hat(v / t))| (a fixed point, t ~ 8 scale): only the scale differs.
    x is small, hence y_hat = O(|v|^2 lambda / (64 scale^2)) and its rounding floor moves sign, and with it the appended vector, by
    a few 1e-16 relative: far inside the shrink's tolerance (scale, a power of two, keeps that so for sketches of a large norm).
    Features d .. D - 1 (not in the sketches) are random when rng is given."""
    d = v.shape[0]
    eta = APPEND_ETA[task] * scale * scale
    q = lambda z: float((BP.T @ z) @ (BP.T @ z)) - float((BN.T @ z) @ (BN.T @ z))
    if task == "reg":
        xs = v / (8.0 * scale)
        y_hat = q(xs)
        y = y_hat + 32.0 if to == "P" else y_hat - 32.0
    else:
        y = 1.0 if to == "P" else -1.0
        t2 = eta / 2.0
        for _ in range(60):
            t2 = eta * abs(grad_loss(q(v / np.sqrt(t2)), y, True))
        xs = v / np.sqrt(t2)
        y_hat = q(xs)
    sign = grad_loss(y_hat, y, task == "cls")
    assert (sign <= 0) == (to == "P") and sign != 0
    x = np.zeros(D, np.float64)
    x[:d] = xs
    if rng is not None and D > d:
        x[d:] = rng.standard_normal(D - d)
    return x, float(y), eta, np.sqrt(eta * abs(sign)) * xs


# ---- the cases of the one-shrink tests --------------------------------------------------------------------------------------------

GEOMETRIES = [(1, 1), (1, 3), (2, 1), (3, 2), (5, 5), (7, 3), (8, 4), (9, 64), (16, 8), (20, 32), (31, 16), (32, 2), (32, 48), (32, 64)]
FAMILIES = ["geometric", "wide", "flat_tail", "kept_tie", "rank_deficient", "under_thres", "diagonal", "diagonal_tie"]


def features_for(d, m):
    return 64 if (d, m) in ((32, 48), (32, 64)) else d


def _geo(n, lo):
    return np.array([1.0]) if n == 1 else lo ** (np.arange(n) / (n - 1.0))


def spectrum_for(d, m, family):
    """-> the spectrum [d] of family `family` at geometry (d, m), or None where the family does not exist there.  r = min(d, 2m - 1)
    is the largest possible rank of a buffer (column 0 stays zero); keep0 = m - 1 if r >= m else r is what a full-rank buffer keeps.
      geometric       1 ... 1e-6 over r                                                    (every geometry)
      wide            1 ... 1e-10 over r                                                   (r >= 2)
      flat_tail       lambda_{m-1} = lambda_m = ... = 0.25 under a head 1.5 ... 0.5         (2 <= m < d: lambda_m exists and is the shift)
      kept_tie        geometric with lambda_1 = lambda_0                                   (keep0 >= 2: the tie lies inside the kept group)
      rank_deficient  1 ... 1e-3 over r // 2, exact zeros after                            (r >= 2)
      under_thres     1 ... 1e-3 over r // 2, then 1e-13 up to r                           (r >= 2)
      diagonal        the geometric spectrum on a diagonal Gram matrix                     (every geometry)
      diagonal_tie    the kept_tie spectrum on a diagonal Gram matrix: two equal norms     (keep0 >= 2)"""
    r = min(d, 2 * m - 1)
    keep0 = m - 1 if r >= m else r
    s = np.zeros(d, np.float64)
    if family in ("geometric", "diagonal"):
        s[:r] = _geo(r, 1e-6)
    elif family == "wide":
        if r < 2:
            return None
        s[:r] = _geo(r, 1e-10)
    elif family == "flat_tail":
        if not 2 <= m < d:
            return None
        s[:m - 1] = 1.5 * _geo(m - 1, 1.0 / 3.0)
        s[m - 1:r] = 0.25
    elif family in ("kept_tie", "diagonal_tie"):
        if keep0 < 2:
            return None
        s[:r] = _geo(r, 1e-6)
        s[1] = s[0]
    elif family in ("rank_deficient", "under_thres"):
        if r < 2:
            return None
        s[:r // 2] = _geo(r // 2, 1e-3)
        if family == "under_thres":
            s[r // 2:r] = 1e-13
    else:
        raise ValueError(family)
    return s


def cases():
    """-> [(id, d, m, D, family, spectrum)] for every family that exists at every geometry."""
    out = []
    for d, m in GEOMETRIES:
        for fam in FAMILIES:
            s = spectrum_for(d, m, fam)
            if s is not None:
                out.append((f"d{d}-m{m}-{fam}", d, m, features_for(d, m), fam, s))
    return out


def case_state(case, salt=0):
    """-> (B, count, v) of a case, from a seed of its own."""
    cid, d, m, D, fam, s = case
    rng = np.random.default_rng([d, m, FAMILIES.index(fam), salt])
    return state_for_spectrum(d, m, s, rng, diagonal=fam.startswith("diagonal"))
