"""fp64 numpy restatement of the guarded basis-simplex rule (include/mllp_hip.h: mllp_basis_simplex_guarded): the rule of
tests/simplex_oracle.py with Bland's rule after `stall_pivots` consecutive degenerate pivots of a stage and a fresh
factorization of the basis after every `refactor_every` pivots.  Test infrastructure: no GPU, no library, and no code shared
with it (tests/test_simplex_guarded_oracle.py, tests/test_simplex_guarded.py).

Written in the manner of simplex_oracle.run: a fresh dense solve of the current basis in every iteration; a
refactorization is basis_oracle.walk on np.sort(col_of_row), which only reassigns the rows (or finds rank < m: code 7).

MARGINS.  Those of simplex_oracle.run under the same labels, with ONE change of units: the two threshold tests x_B,p against
-ftol and d_j against -dtol are |value - threshold| / tolerance here, like every threshold below, not the LP's units.  At a
degenerate vertex x_B,p is an exact 0, ftol = 2^-10 away from the threshold in any units of the LP: in absolute terms no
degenerate run could ever be guarded.  Relative to the tolerance the bar 2^-6 asks that fp32 moves the value by less than
2^-16; the cases this is used on (6 x 14, entries -1, 0, 1, solutions below 16) keep x_B and d within a few 2^-24 * 16 of
fp64.  And
  degeneracy tests  (stall_pivots > 0; in Bland mode and outside it) x_B,p against ftol and dtilde_j against dtol of the
                    pivot taken: |value - tolerance| / tolerance;
  Bland mode        every clipped or thresholded quantity, relative to its tolerance: x_B,i against -ftol for every row
                    (stage D, leaving), dtilde_j against dtol for every candidate (stage D, entering), d_j against -dtol for
                    every nonbasic column (stage P, entering), x_B,i against ftol for every candidate (stage P, leaving);
                    the ratio argmins keep their relative gap unless the best ratio is an exact clipped 0: those ties are
                    broken by integers.
A run is `guarded` when every margin is at least simplex_oracle.GUARD = 2^-6 and the start's walk and every
refactorization's walk pass basis_oracle.gap_ok.
"""
import numpy as np

import basis_oracle as bo
import simplex_oracle as so

CODES = dict(so.CODES, refactor_singular=7)
GUARD = so.GUARD


def family(seed):
    """The degenerate 6 x 14 family: (A, b, c, start mask) or None when the start's walk is not of rank 6.  Small integer
    data, a right-hand side with at most three nonzero coordinates behind it: most vertices are degenerate."""
    rng = np.random.default_rng(seed)
    A = (rng.integers(-1, 2, (6, 14)) * (rng.random((6, 14)) < 0.6)).astype(np.float64)
    x0 = np.zeros(14)
    x0[rng.choice(14, 3, replace=False)] = rng.integers(1, 4, 3)
    b = A @ x0
    c = rng.integers(0, 5, 14).astype(np.float64)
    wk = bo.walk(A, rng.permutation(14), 2.0 ** -12)
    if wk["status"][0] < 6:
        return None
    return A, b, c, wk["basis"].astype(np.float32)


def run(A, b, c, start, max_pivots, refactor_every=0, stall_pivots=0, tol=2.0 ** -12, ftol=2.0 ** -10, dtol=2.0 ** -10,
        ptol=2.0 ** -10, dshift=2.0 ** -4, max_m=None):
    """The guarded rule on a dense A [m, n], b [m], c [n] and a start mask [n], in fp64.  Returns what simplex_oracle.run
    returns (codes 0-7) and: guard [refactorizations done, pivots chosen by Bland's rule], bland [those pivots in stage D, in
    stage P], refactor_ratios (the ratios of every refactorization's walk, one array each)."""
    A, b, c = (np.asarray(v, np.float64) for v in (A, b, c))
    m, n = A.shape
    R, S = int(refactor_every), int(stall_pivots)
    assert R >= 0 and S >= 0
    none = dict(trace=[], basis=np.zeros(n), col_of_row=np.full(m, -1, np.int64), margins=[], margin=np.inf, guard=[0, 0], bland=[0, 0],
                refactor_ratios=[])
    if max_m is not None and m > max_m:
        return dict(none, code=2, status=[2, 0, 0, 0])
    cols = np.flatnonzero(np.asarray(start) != 0)
    if len(cols) != m:
        return dict(none, code=3, status=[3, 0, 0, 0])
    wk = bo.walk(A, cols, tol)
    if wk["status"][0] < m:
        return dict(none, code=1, status=[1, 0, 0, wk["status"][0]], start_ratios=wk["ratios"])
    cor = np.array(wk["col_of_row"], np.int64)
    margins, trace, refactor_ratios = [], [], []
    count, bland = [0, 0], [0, 0]
    refactors = stall = 0

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

    def ratio_argmin(values, owners, label):
        """Bland mode: the smallest ratio, the lowest owner among equal ones; a gap unless the best is a clipped 0"""
        best = values.min()
        tied = np.flatnonzero(values == best)
        q = int(tied[np.argmin(owners[tied])])
        if best != 0.0 and values.size > 1:
            margins.append((label, (np.delete(values, q).min() - best) / abs(best)))
        return q

    _, _, _, d0 = solve(c)
    shifted = c.copy()
    nb = nonbasic()
    shifted[nb] += np.maximum(0.0, dshift - d0[nb])
    stage, code = 0, None
    while code is None:
        g = shifted if stage == 0 else c
        T, xb, y, d = solve(g)
        nb = nonbasic()
        in_bland = S > 0 and stall >= S
        if stage == 0:
            if m == 0:
                stage = 1
                continue
            if in_bland:
                margins += [("x_B,i against -ftol (Bland)", v) for v in np.abs(xb + ftol) / ftol]
                rows = np.flatnonzero(xb < -ftol)
                if rows.size == 0:
                    stage, stall = 1, 0
                    continue
                p = int(rows[np.argmin(cor[rows])])
            else:
                p, gap = so._argmin_margin(xb)
                margins.append(("x_B,p against -ftol", abs(xb[p] + ftol) / ftol))
                if xb[p] >= -ftol:
                    stage, stall = 1, 0
                    continue
                if gap is not None:
                    margins.append(("leaving row (D)", gap))
            alpha = T[p] @ A[:, nb]
            margins += [("alpha_j against -ptol", v) for v in np.abs(alpha + ptol) / ptol]
            cand = np.flatnonzero(alpha < -ptol)
            if cand.size == 0:
                code = 4
                break
            dt = d[nb][cand]
            if in_bland:
                margins += [("dtilde_j against dtol (Bland)", v) for v in np.abs(dt - dtol) / dtol]
                q = ratio_argmin(np.where(dt > dtol, dt, 0.0) / -alpha[cand], nb[cand], "entering column (D, Bland)")
            else:
                q, gap = so._argmin_margin(np.maximum(dt, 0.0) / -alpha[cand])
                if gap is not None:
                    margins.append(("entering column (D)", gap))
            j = int(nb[cand][q])
            value, limit, label = dt[q], dtol, "dtilde_j against dtol (degenerate)"
        else:
            if nb.size == 0:
                code = 0
                break
            if in_bland:
                margins += [("d_j against -dtol (Bland)", v) for v in np.abs(d[nb] + dtol) / dtol]
                neg = nb[d[nb] < -dtol]
                if neg.size == 0:
                    code = 0
                    break
                j = int(neg[0])
            else:
                q, gap = so._argmin_margin(d[nb])
                j = int(nb[q])
                margins.append(("d_j against -dtol", abs(d[j] + dtol) / dtol))
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
            if in_bland:
                margins += [("x_B,i against ftol (Bland)", v) for v in np.abs(xb[cand] - ftol) / ftol]
                q = ratio_argmin(np.where(xb[cand] > ftol, xb[cand], 0.0) / w[cand], cor[cand], "leaving row (P, Bland)")
            else:
                q, gap = so._argmin_margin(np.maximum(xb[cand], 0.0) / w[cand])
                if gap is not None:
                    margins.append(("leaving row (P)", gap))
            p = int(cand[q])
            value, limit, label = xb[p], ftol, "x_B,p against ftol (degenerate)"
        if sum(count) >= max_pivots:
            code = 6
            break
        trace.append((j, int(p)))
        cor[p] = j
        count[stage] += 1
        bland[stage] += in_bland
        if S > 0:
            margins.append((label, abs(value - limit) / limit))
            stall = stall + 1 if value <= limit else 0
        if R > 0 and sum(count) % R == 0:
            wk2 = bo.walk(A, np.sort(cor), tol)
            refactor_ratios.append(wk2["ratios"])
            if wk2["status"][0] < m:
                code = 7
                break
            cor = np.array(wk2["col_of_row"], np.int64)
            refactors += 1
    basis = np.zeros(n)
    basis[cor] = 1.0
    return dict(code=code, status=[code, count[0], count[1], m], trace=trace, basis=basis,
                col_of_row=np.full(m, -1, np.int64) if code == 7 else cor.copy(), margins=margins,
                margin=min([v for _, v in margins], default=np.inf), start_ratios=wk["ratios"], guard=[refactors, sum(bland)],
                bland=bland, refactor_ratios=refactor_ratios)


def guarded(res, tol=2.0 ** -12):
    """every margin of the run is at least GUARD, and neither the start's factorization nor any refactorization met a ratio
    inside [tol / 64, 64 tol].  NOT simplex_oracle.guarded, even for a run with both guards off: the two threshold margins
    are relative to their tolerance here (MARGINS above), about 2^10 times looser than that oracle's absolute ones.  Use
    simplex_oracle.run and simplex_oracle.guarded for a statement about mllp_basis_simplex."""
    return bool(res["margin"] >= GUARD and bo.gap_ok(res.get("start_ratios", []), tol)
                and all(bo.gap_ok(r, tol) for r in res.get("refactor_ratios", [])))


CHVATAL = dict(A=[[.5, -5.5, -2.5, 9, 1, 0, 0], [.5, -1.5, -.5, 1, 0, 1, 0], [1, 0, 0, 0, 0, 0, 1]], b=[0, 0, 1],
               c=[-10, 57, 9, 24, 0, 0, 0], start=[0, 0, 0, 0, 1, 1, 1], objective=-1.0)
BEALE = dict(A=[[.25, -8, -1, 9, 1, 0, 0], [.5, -12, -.5, 3, 0, 1, 0], [0, 0, 1, 0, 0, 0, 1]], b=[0, 0, 1],
             c=[-.75, 20, -.5, 6, 0, 0, 0], start=[0, 0, 0, 0, 1, 1, 1], objective=-1.25)
