"""fp64 numpy restatement of the basis-repair rule (include/mllp_hip.h: mllp_basis_repair), a brute force over all subsets
for tiny instances, and the dense fp64 solves that judge x and y.  Test infrastructure: no GPU, no library, and no code shared
with it (tests/test_basis_repair.py).

THE RULE, as a column-by-column Gaussian elimination (left-looking: every candidate is brought up to date with the
multiplier columns of the accepted ones, in the order they were accepted).  A candidate's residual on the rows not yet
pivoted is the Schur-complement column whichever elimination produced it; the device keeps an explicit Gauss-Jordan
transform instead, so the two share the definition and nothing else.
"""
import itertools

import numpy as np

from planted_oracle import dense, dense_solve      # noqa: F401  (re-exported for the tests)

U = 2.0 ** -24


def walk(A, order, tol):
    """The rule on a dense fp64 A [m, n] and a candidate list (local ids; ends at the first negative entry or after n
    entries).  Returns dict: accepted (column ids in order), pivot_rows (same order), col_of_row [m] (-1 where none),
    basis [n] 0/1, status [rank, examined, rejected among the first m candidates, code], quality [smallest accepted,
    largest rejected ratio], ratios (every ratio r / amax met on the walk, 0 for a zero column) and accepted_flags."""
    A = np.asarray(A, np.float64)
    m, n = A.shape
    free = np.ones(m, bool)
    mult, piv = [], []              # multiplier column (zero on the rows pivoted before and on its own pivot row), pivot row
    accepted, ratios, flags = [], [], []
    examined = rejected = 0
    code = 1
    for t, j in enumerate(list(order)[:n]):
        if len(accepted) == m or j < 0:
            break
        if j >= n:
            code = 3
            break
        examined += 1
        a = A[:, j]
        amax = np.abs(a).max(initial=0.0)
        w = a.copy()
        for l, p in zip(mult, piv):
            if w[p] != 0.0:
                w -= l * w[p]
        res = np.where(free, np.abs(w), -1.0)
        p = int(np.argmax(res))                     # the first (lowest) row among equal values
        r = res[p]
        ratio = r / amax if amax > 0 else 0.0
        ok = amax > 0 and r > tol * amax
        ratios.append(ratio)
        flags.append(ok)
        if not ok:
            rejected += t < m
            continue
        free[p] = False
        l = np.where(free, w / w[p], 0.0)
        mult.append(l)
        piv.append(p)
        accepted.append(int(j))
    rank = len(accepted)
    if rank == m:
        code = 0
    col_of_row = np.full(m, -1, np.int64)
    col_of_row[piv] = accepted
    basis = np.zeros(n)
    basis[accepted] = 1.0
    ratios, flags = np.array(ratios), np.array(flags, bool)
    quality = [ratios[flags].min(initial=np.inf), ratios[~flags].max(initial=0.0)]
    return dict(accepted=accepted, pivot_rows=piv, col_of_row=col_of_row, basis=basis, status=[rank, examined, rejected, code],
                quality=quality, ratios=ratios, accepted_flags=flags)


def gap_ok(ratios, tol):
    """every ratio met on the walk lies outside [tol / 64, 64 tol]: fp32 rounding cannot move it across tol"""
    ratios = np.asarray(ratios, np.float64)
    return bool(((ratios < tol / 64) | (ratios > 64 * tol)).all())


def brute_force(A, order, sigma_min=1e-9):
    """The lexicographically best (in list positions) m-subset of the list's entries whose columns form a matrix with
    smallest singular value above sigma_min * largest; None when there is none.  Tiny instances only."""
    A = np.asarray(A, np.float64)
    m, n = A.shape
    lst = []
    for j in list(order)[:n]:
        if j < 0 or j >= n:
            break
        lst.append(int(j))
    for pos in itertools.combinations(range(len(lst)), m):     # (generated in lexicographic order)
        cols = [lst[q] for q in pos]
        if len(set(cols)) < m:
            continue
        s = np.linalg.svd(A[:, cols], compute_uv=False) if m else np.ones(1)
        if m == 0 or s[-1] > sigma_min * s[0]:
            return cols
    return None


def basic_solution(A, b, c, col_of_row):
    """(x [n], y [m], cond_inf(B)) of the basis whose column for pivot row i is col_of_row[i], by dense fp64 solves"""
    A, b, c = (np.asarray(v, np.float64) for v in (A, b, c))
    m, n = A.shape
    cols = np.sort(np.asarray(col_of_row, np.int64))
    x, y = np.zeros(n), np.zeros(m)
    if m == 0:
        return x, y, 1.0
    B = A[:, cols]
    x[cols] = np.linalg.solve(B, b)
    y[:] = np.linalg.solve(B.T, c[cols])
    cond = np.linalg.norm(B, np.inf) * np.linalg.norm(np.linalg.inv(B), np.inf)
    return x, y, float(cond)


def error_units(got, want, m, cond):
    """max |got - want| in units of u = m 2^-24 cond_inf(B) ||want||_inf"""
    want = np.asarray(want, np.float64)
    scale = max(m, 1) * U * cond * np.abs(want).max(initial=0.0)
    err = np.abs(np.asarray(got, np.float64) - want).max(initial=0.0)
    return 0.0 if err == 0.0 else err / scale
