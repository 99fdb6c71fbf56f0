"""fp64 numpy restatement of the planted-basis rule (include/mllp_hip.h: mllp_graph_plant_basis), of the certificate
(mllp_lp_certificate), the dense fp64 solve that judges both, and the ragged case the tests of tests/test_planted.py share.
Test infrastructure: no GPU, no library.

ERROR BOUND of a device sum.  A row (column) of L stored terms is added in fp32 in SOME fixed order, one fma per term,
then at most two more roundings (the pivot's dominance product and floor, or the subtraction of b / c).  Any order of L
fp32 additions is within (L - 1) u sum|terms| of the exact sum to first order, u = 2^-24; with the fma's single rounding
per term and the trailing operations that is at most (L + 3) u sum|terms|, the second-order part (L u)^2 / 2 being below
1e-8 of it for L <= 2400.  `row_bound(L, abs_terms)` is that figure; every tolerance of the tests is one of them.
"""
import numpy as np

U = 2.0 ** -24
DOMINANCE, FLOOR = 1.25, 0.25


def row_bound(length, abs_terms):
    return (np.asarray(length, np.float64) + 3.0) * U * np.asarray(abs_terms, np.float64)


def _rows_of(ptr):
    return np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))


def plant(ptr, idx, val, pivot, xstar, ystar, slack, n_cols, dominance=DOMINANCE, floor=FLOOR):
    """The rule in fp64 on the given (fp32-valued) inputs.  Returns dict: values (new), pivot_pos, off, b, c, labels and
    the bounds' ingredients: pivot_abs = dominance off + floor, b_abs = sum |terms of b_i|, c_abs = sum |terms of c_j|,
    row_len, col_len."""
    ptr, idx, pivot = np.asarray(ptr, np.int64), np.asarray(idx, np.int64), np.asarray(pivot, np.int64)
    val, xstar, ystar, slack = (np.asarray(a, np.float64) for a in (val, xstar, ystar, slack))
    m = len(ptr) - 1
    rows = _rows_of(ptr)
    basic = np.zeros(n_cols, bool)
    basic[pivot] = True
    assert basic.sum() == m, "pivot is not injective"
    is_piv = idx == pivot[rows]
    assert np.array_equal(np.bincount(rows[is_piv], minlength=m), np.ones(m, np.int64)), "a pivot entry is absent (or twice)"
    pivot_pos = np.flatnonzero(is_piv)                  # (rows ascend, one per row: in row order)
    use = basic[idx] & ~is_piv
    off = np.bincount(rows[use], np.abs(val[use]), minlength=m)
    values = val.copy()
    values[pivot_pos] = np.copysign(dominance * off + floor, val[pivot_pos])
    return dict(values=values, pivot_pos=pivot_pos, off=off, basic=basic, labels=basic.astype(np.float64),
                pivot_abs=dominance * off + floor, row_len=np.diff(ptr), col_len=np.bincount(idx, minlength=n_cols),
                **rhs_and_costs(ptr, idx, values, pivot, xstar, ystar, slack, n_cols))


def rhs_and_costs(ptr, idx, values, pivot, xstar, ystar, slack, n_cols):
    """b and c of the rule from GIVEN new values (the device's own, exported, for the staged parity check)"""
    ptr, idx, pivot = np.asarray(ptr, np.int64), np.asarray(idx, np.int64), np.asarray(pivot, np.int64)
    values, xstar, ystar, slack = (np.asarray(a, np.float64) for a in (values, xstar, ystar, slack))
    m = len(ptr) - 1
    rows = _rows_of(ptr)
    basic = np.zeros(n_cols, bool)
    basic[pivot] = True
    use = basic[idx]                                    # (the pivot entry included: b_i = d x_p + rest)
    b = np.bincount(rows[use], values[use] * xstar[idx[use]], minlength=m)
    b_abs = np.bincount(rows[use], np.abs(values[use] * xstar[idx[use]]), minlength=m)
    c = np.bincount(idx, values * ystar[rows], minlength=n_cols) + np.where(basic, 0.0, slack)
    c_abs = np.bincount(idx, np.abs(values * ystar[rows]), minlength=n_cols) + np.where(basic, 0.0, np.abs(slack))
    return dict(b=b, b_abs=b_abs, c=c, c_abs=c_abs)


def certificate(ptr, idx, val, c, b, x, y, basis, ptr_m, ptr_n):
    """([n_inst, 6] fp64, [n_inst, 6] bounds of a device evaluation): the six figures of mllp_lp_certificate.  x over the
    basis, |x| off it and the mask's sum are exact on the device (bound 0)."""
    ptr, idx = np.asarray(ptr, np.int64), np.asarray(idx, np.int64)
    val, c, b, x, y, basis = (np.asarray(a, np.float64) for a in (val, c, b, x, y, basis))
    m, n = len(ptr) - 1, len(c)
    rows = _rows_of(ptr)
    res = np.abs(np.bincount(rows, val * x[idx], minlength=m) - b)
    res_bound = row_bound(np.diff(ptr), np.bincount(rows, np.abs(val * x[idx]), minlength=m) + np.abs(b))
    red = c - np.bincount(idx, val * y[rows], minlength=n)
    red_bound = row_bound(np.bincount(idx, minlength=n), np.bincount(idx, np.abs(val * y[rows]), minlength=n) + np.abs(c))
    on = basis != 0
    out, bound = np.zeros((len(ptr_m) - 1, 6)), np.zeros((len(ptr_m) - 1, 6))
    for k in range(len(ptr_m) - 1):
        r, s = slice(ptr_m[k], ptr_m[k + 1]), slice(ptr_n[k], ptr_n[k + 1])
        onk = on[s]
        out[k] = [res[r].max(initial=0.0), x[s][onk].min(initial=np.inf), np.abs(x[s][~onk]).max(initial=0.0),
                  red[s][~onk].min(initial=np.inf), np.abs(red[s][onk]).max(initial=0.0), basis[s].sum()]
        bound[k] = [res_bound[r].max(initial=0.0), 0.0, 0.0, red_bound[s][~onk].max(initial=0.0),
                    red_bound[s][onk].max(initial=0.0), 0.0]
    return out, bound


def dense(ptr, idx, val, m, n):
    A = np.zeros((m, n))
    rows = _rows_of(np.asarray(ptr, np.int64))
    A[rows, np.asarray(idx, np.int64)] = np.asarray(val, np.float64)
    return A


def dense_solve(A, b, c, basis):
    """The basic solution of `basis` by dense fp64 solves: (x_B, reduced costs of the nonbasic columns, cond(B))"""
    on = np.asarray(basis) != 0
    B = A[:, on]
    assert B.shape[0] == B.shape[1], "the basis is not square"
    if B.shape[0] == 0:
        return np.zeros(0), np.asarray(c, np.float64)[~on], 1.0
    x_b = np.linalg.solve(B, np.asarray(b, np.float64))
    y = np.linalg.solve(B.T, np.asarray(c, np.float64)[on])
    return x_b, np.asarray(c, np.float64)[~on] - A[:, ~on].T @ y, float(np.linalg.cond(B))


# ---- the shared case ---------------------------------------------------------------------------------------------------------
# lengths on both sides of the tiers' thresholds (group <= 64 < wave <= 1024 < block), and the issue's 70 and 1100
LONG = (64, 65, 70, 1024, 1025, 1100)
BIG_M, BIG_N = 1200, 2400


def _instance(m, n, row_nnz, seed, long_rows=(), long_cols=(), all_basic=False):
    """(ptr, idx local ascending, val fp32, pivot local) of one instance.  long_rows: rows of EXACTLY these lengths, about
    4 in 5 of their entries on basic columns; long_cols: columns of exactly these lengths, the longest of them basic.
    all_basic: m == n and every entry of the dense-ish pattern is on a basic column."""
    rng = np.random.default_rng(seed)
    pivot = rng.permutation(n)[:m]
    special_c = rng.choice(np.setdiff1d(np.arange(n), pivot), size=len(long_cols), replace=False) if long_cols else np.zeros(0, int)
    special_r = rng.choice(m, size=len(long_rows) + 1, replace=False) if long_rows else np.zeros(0, int)
    pairs = set()
    if len(long_cols):                      # the longest special column becomes basic: it takes over a short row's pivot
        owner_row = int(special_r[-1])
        pivot[owner_row] = special_c[int(np.argmax(long_cols))]
    basic_cols = np.setdiff1d(pivot, special_c)
    plain_cols = np.setdiff1d(np.arange(n), np.concatenate([pivot, special_c]))
    for r in range(m):
        pairs.add((r, int(pivot[r])))
    for r, length in zip(special_r[:len(long_rows)], long_rows):
        own = int(pivot[r])
        nb = min(int(0.8 * length), len(basic_cols) - 1)
        cols = np.concatenate([rng.choice(np.setdiff1d(basic_cols, [own]), size=nb, replace=False),
                               rng.choice(plain_cols, size=length - 1 - nb, replace=False)])
        pairs.update((int(r), int(c)) for c in cols)
    ordinary_r = np.setdiff1d(np.arange(m), special_r[:len(long_rows)])
    pool = np.setdiff1d(np.arange(n), special_c)
    for r in ordinary_r:
        k = n if all_basic else int(np.clip(rng.poisson(row_nnz), 1, len(pool)))
        pairs.update((int(r), int(c)) for c in rng.choice(pool, size=k, replace=False))
    for c, length in zip(special_c, long_cols):
        have = [r for r in range(m) if (r, int(c)) in pairs]
        rows = rng.choice(np.setdiff1d(ordinary_r, have), size=length - len(have), replace=False)
        pairs.update((int(r), int(c)) for r in rows)
    key = np.array(sorted(r * n + c for r, c in pairs), np.int64)
    rows, idx = key // n, key % n
    ptr = np.zeros(m + 1, np.int64)
    ptr[1:] = np.cumsum(np.bincount(rows, minlength=m))
    val = rng.standard_normal(len(idx)).astype(np.float32)
    if long_rows:
        assert sorted(np.diff(ptr)[special_r[:len(long_rows)]]) == sorted(long_rows)
    if len(long_cols):
        assert sorted(np.bincount(idx, minlength=n)[special_c]) == sorted(long_cols)
    return ptr, idx.astype(np.int32), val, pivot.astype(np.int32)


SHAPES = [(1, 1), (3, 3), (5, 12), (40, 100), (BIG_M, BIG_N)]


def ragged_case(seed=20, which=None):
    """The batch every GPU test uses: instances 1 x 1, 3 x 3 (dense, all basic), 5 x 12, 40 x 100 and one 1200 x 2400 with
    rows and columns of LONG entries (every tier, both sides of every threshold).  `which`: a sub-list of instance
    numbers (the big one alone: [4]).  Global ids; fp32 numbers: xstar, slack in U(0.5, 1.5), ystar in U(-1, 1).  An
    instance's numbers depend on its number and `seed` alone."""
    which = list(range(len(SHAPES))) if which is None else list(which)
    parts, numbers = [], []
    for k in which:
        m, n = SHAPES[k]
        big = (m, n) == (BIG_M, BIG_N)
        parts.append(_instance(m, n, 4.0 if not big else 8.0, seed + k, LONG if big else (), LONG if big else (),
                               all_basic=(m, n) == (3, 3)))
        rng = np.random.default_rng(1000 + seed + k)
        numbers.append(((rng.random(n) + 0.5).astype(np.float32), (rng.random(m) * 2 - 1).astype(np.float32),
                        (rng.random(n) + 0.5).astype(np.float32)))
    inst_m, inst_n = [SHAPES[k][0] for k in which], [SHAPES[k][1] for k in which]
    ptr_m, ptr_n = np.concatenate([[0], np.cumsum(inst_m)]), np.concatenate([[0], np.cumsum(inst_n)])
    nnz_off = np.concatenate([[0], np.cumsum([len(p[1]) for p in parts])])
    ptr = np.concatenate([[0]] + [p[0][1:] + nnz_off[i] for i, p in enumerate(parts)]).astype(np.int32)
    idx = np.concatenate([p[1] + ptr_n[i] for i, p in enumerate(parts)]).astype(np.int32)
    val = np.concatenate([p[2] for p in parts])
    pivot = np.concatenate([p[3] + ptr_n[i] for i, p in enumerate(parts)]).astype(np.int32)
    xstar, ystar, slack = (np.concatenate([t[j] for t in numbers]) for j in range(3))
    return dict(inst_m=inst_m, inst_n=inst_n, ptr_m=ptr_m, ptr_n=ptr_n, nnz_off=nnz_off, ptr=ptr, idx=idx, val=val, pivot=pivot,
                xstar=xstar, ystar=ystar, slack=slack, M=int(ptr_m[-1]), N=int(ptr_n[-1]))
