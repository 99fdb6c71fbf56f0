"""fp64 numpy restatement of the basis-simplex rule (include/mllp_hip.h: mllp_basis_simplex), the margin of every decision
it takes, a brute force over all bases for tiny instances, and the perturbed starts the tests share.  Test infrastructure:
no GPU, no library, and no code shared with it (tests/test_simplex_oracle.py, tests/test_simplex.py).

THE RULE with a fresh dense solve of the current basis in every iteration (the device updates an explicit inverse in
product form instead, so the two share the definition and nothing else): x_B = B^-1 b, y = B^-T g_B, d = g - A'y, and the
rows alpha = e_p' B^-1 A, w = B^-1 a_j from the same fresh inverse.  Row i of the inverse belongs to col_of_row[i], as the
start's factorization (basis_oracle.walk on the mask's columns ascending) assigned it; a pivot replaces col_of_row[p].

MARGINS.  Every decision records how far it was from going the other way:
  threshold tests   x_B,p against -ftol and d_j against -dtol: |value - threshold| (the LP's units);
                    alpha_j against -ptol and w_i against ptol, for EVERY nonbasic j / row i: |value - threshold| / ptol;
  argmins           (runner-up - best) / |best| (inf when the best is 0 and the runner-up is not; nothing with one candidate).
`margin` is the smallest of them over the run.  With every margin at least 2^-6 the device's fp32 decisions are the
oracle's (tests/test_simplex.py asserts that from the oracle alone before it looks at the device).
"""
import itertools

import numpy as np

import basis_oracle as bo

CODES = dict(optimal=0, singular=1, skipped=2, bad_mask=3, infeasible=4, unbounded=5, limit=6)
GUARD = 2.0 ** -6


def _argmin_margin(values):
    """(index of the smallest, lowest index among equals; relative gap to the runner-up or None)"""
    values = np.asarray(values, np.float64)
    k = int(np.argmin(values))
    if values.size < 2:
        return k, None
    rest = np.delete(values, k).min()
    best = values[k]
    gap = rest - best
    return k, (gap / abs(best) if best != 0.0 else (np.inf if gap > 0 else 0.0))


def run(A, b, c, start, max_pivots, tol=2.0 ** -12, ftol=2.0 ** -10, dtol=2.0 ** -10, ptol=2.0 ** -10, dshift=2.0 ** -4, max_m=None):
    """The rule on a dense A [m, n], b [m], c [n] and a start mask [n] (nonzero = basic), in fp64.  Returns dict: code,
    status [code, stage-D pivots, stage-P pivots, rank of the start], trace [(entering column, leaving row)], basis [n] 0/1,
    col_of_row [m], margins (every one, with a label) and margin (their minimum, inf when there is none)."""
    A, b, c = (np.asarray(v, np.float64) for v in (A, b, c))
    m, n = A.shape
    none = dict(trace=[], basis=np.zeros(n), col_of_row=np.full(m, -1, np.int64), margins=[], margin=np.inf)
    if max_m is not None and m > max_m:
        return dict(none, code=2, status=[2, 0, 0, 0])
    cols = np.flatnonzero(np.asarray(start) != 0)
    if len(cols) != m:
        return dict(none, code=3, status=[3, 0, 0, 0])
    wk = bo.walk(A, cols, tol)
    if wk["status"][0] < m:
        return dict(none, code=1, status=[1, 0, 0, wk["status"][0]], start_ratios=wk["ratios"])
    cor = np.array(wk["col_of_row"], np.int64)
    margins, trace = [], []
    count = [0, 0]

    def solve(g):
        if m == 0:
            return np.zeros((0, 0)), np.zeros(0), np.zeros(0), g.copy()
        T = np.linalg.inv(A[:, cor])
        y = np.linalg.solve(A[:, cor].T, g[cor])
        return T, np.linalg.solve(A[:, cor], b), y, g - A.T @ y

    def nonbasic():
        on = np.zeros(n, bool)
        on[cor] = True
        return np.flatnonzero(~on)

    # the shifts
    _, _, _, d0 = solve(c)
    shifted = c.copy()
    nb = nonbasic()
    shifted[nb] += np.maximum(0.0, dshift - d0[nb])
    stage, code = 0, None
    while code is None:
        g = shifted if stage == 0 else c
        T, xb, y, d = solve(g)
        nb = nonbasic()
        if stage == 0:
            if m == 0:
                stage = 1
                continue
            p, gap = _argmin_margin(xb)
            margins.append(("x_B,p against -ftol", abs(xb[p] + ftol)))
            if xb[p] >= -ftol:
                stage = 1
                continue
            if gap is not None:
                margins.append(("leaving row (D)", gap))
            alpha = T[p] @ A[:, nb]
            margins += [("alpha_j against -ptol", v) for v in np.abs(alpha + ptol) / ptol]
            cand = np.flatnonzero(alpha < -ptol)
            if cand.size == 0:
                code = 4
                break
            q, gap = _argmin_margin(np.maximum(d[nb][cand], 0.0) / -alpha[cand])
            if gap is not None:
                margins.append(("entering column (D)", gap))
            j = int(nb[cand][q])
        else:
            if nb.size == 0:
                code = 0
                break
            q, gap = _argmin_margin(d[nb])
            j = int(nb[q])
            margins.append(("d_j against -dtol", abs(d[j] + dtol)))
            if d[j] >= -dtol:
                code = 0
                break
            if gap is not None:
                margins.append(("entering column (P)", gap))
            w = T @ A[:, j]
            margins += [("w_i against ptol", v) for v in np.abs(w - ptol) / ptol]
            cand = np.flatnonzero(w > ptol)
            if cand.size == 0:
                code = 5
                break
            q, gap = _argmin_margin(np.maximum(xb[cand], 0.0) / w[cand])
            if gap is not None:
                margins.append(("leaving row (P)", gap))
            p = int(cand[q])
        if sum(count) >= max_pivots:
            code = 6
            break
        trace.append((j, int(p)))
        cor[p] = j
        count[stage] += 1
    basis = np.zeros(n)
    basis[cor] = 1.0
    return dict(code=code, status=[code, count[0], count[1], m], trace=trace, basis=basis, col_of_row=cor.copy(), margins=margins,
                margin=min([v for _, v in margins], default=np.inf), start_ratios=wk["ratios"])


def guarded(res, tol=2.0 ** -12):
    """every margin of the run is at least GUARD and the start's factorization met no ratio inside [tol / 64, 64 tol]"""
    return bool(res["margin"] >= GUARD and bo.gap_ok(res.get("start_ratios", []), tol))


def trace_array(res, max_pivots):
    """[max_pivots, 2] int32 as the device writes it: {entering column, leaving row}, -1 past the end"""
    out = np.full((max_pivots, 2), -1, np.int32)
    for t, (j, p) in enumerate(res["trace"]):
        out[t] = (j, p)
    return out


def brute_force(A, b, c, feas=1e-9, sigma_min=1e-9):
    """(columns of the cheapest nonsingular primal-feasible basis, its cost), or (None, inf): every m-subset.  Tiny
    instances only."""
    A, b, c = (np.asarray(v, np.float64) for v in (A, b, c))
    m, n = A.shape
    best, cost = None, np.inf
    for cols in itertools.combinations(range(n), m):
        B = A[:, cols]
        s = np.linalg.svd(B, compute_uv=False) if m else np.ones(1)
        if m and not s[-1] > sigma_min * s[0]:
            continue
        x = np.linalg.solve(B, b) if m else np.zeros(0)
        if (x < -feas).any():
            continue
        v = float(c[list(cols)] @ x)
        if v < cost:
            best, cost = list(cols), v
    return best, cost


def perturbed_start(A, labels, k, seed, tol=2.0 ** -12):
    """The labels with k basic columns swapped for k nonbasic ones (drawn from default_rng(seed + 7): first the columns that
    leave, then those that enter), ranked `kept labels ascending, the added columns, everything else ascending` and repaired
    by basis_oracle.walk.  Returns (mask [n] float32, the walk)."""
    labels = np.asarray(labels) != 0
    rng = np.random.default_rng(seed + 7)
    on, off = np.flatnonzero(labels), np.flatnonzero(~labels)
    out = rng.choice(on, size=k, replace=False)
    add = rng.choice(off, size=k, replace=False)
    kept = np.setdiff1d(on, out)
    order = np.concatenate([kept, add, np.setdiff1d(np.arange(labels.size), np.concatenate([kept, add]))])
    wk = bo.walk(A, order, tol)
    assert wk["status"][3] == 0, "the perturbed start could not be repaired to rank m"
    return wk["basis"].astype(np.float32), wk
