"""THE RULE of mllp_lp_pdhg, mllp_lp_pdhg_scaled and mllp_lp_pdhg_halpern (include/mllp_hip.h), restated once over a whole batch
and run by two arithmetics: an fp64 reference that carries an elementwise FIRST-ORDER BOUND next to every value, and an fp32
execution that adds in the device's lane order.  Test infrastructure: numpy and scipy, no GPU, no library.  Covered: the
set-up, K iterations with check_every = 0 (no check, no restart: the Halpern k is the iteration count), the final evaluation.

THE BOUND, with u = 2^-24.  Every rounded operation adds u |result|; the bounds of operands propagate linearly; a gathered
vector enters a row's sum as sum |a_e| bound_v[idx_e]; a row's (column's) sum of L terms adds (D(L) + 2) u sum |a_e v_e|, D the
depth of the header's order (ordered_sum.h): ceil(L/16) + 4 up to 64 terms, ceil(L/64) + 6 up to 1024, ceil(L/1024) + 6 + 4
beyond; a sum "in the order of c'x" over n terms ceil(n/1024) + 6 + 4.  The "+ 2" pays for a product rounded apart from its
sum (numpy has no fma).  The Ruiz factors are the fp32 oracle's bits (pdhg_scaled_oracle.scaling: maxima are exact in any order)
and enter as exact inputs; the Pock-Chambolle pass, eta (one more u for the hardware's root), w0, tau, sigma, tc, tr get bounds
like everything else.  clip, |.| and max(., 0) are 1-Lipschitz: the value is clipped, the bound is the unclipped value's.  The
bound of a maximum is the largest bound among the rows whose value is within their bound of the maximum.  ACCEPTANCE is
2 x the first-order bound (`ratio`): the factor pays for the higher-order terms; it is derived, nothing of it is measured.

`reference(case, call, K, ...)` and `lane32(case, call, K, ..., mut=...)` return the same dict; `mut` breaks the fp32 execution in one of
the ways listed at `Lane`, and tests/test_pdhg_rowwise_oracle.py says which rows each one affects.  `tiers()`, `mixed()`, `many()` build the three batches.
"""
import numpy as np
import scipy.sparse as sp

import pdhg_scaled_oracle as ps

U = 2.0 ** -24
CALLS = ("pdhg", "pdhg_scaled", "pdhg_halpern")
TIER_LENGTHS = (1, 2, 15, 16, 17, 63, 64, 65, 66, 127, 128, 129, 1023, 1024, 1025, 2047, 2048, 2049, 4097)


def row_tier(length):
    length = np.asarray(length)
    return np.where(length <= 64, 0, np.where(length <= 1024, 1, 2))


def depth(length):
    """D(L) of a row's sum by its tier"""
    length = np.asarray(length, np.int64)
    return np.where(length <= 64, -(-length // 16) + 4, np.where(length <= 1024, -(-length // 64) + 6, -(-length // 1024) + 10))


def depth_inst(n):
    return -(-np.asarray(n, np.int64) // 1024) + 10


# ---------------------------------------------------------------------------------------------------
# a value with its first-order bound
# ---------------------------------------------------------------------------------------------------
class V:
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = np.asarray(v, np.float64)
        self.e = np.zeros_like(self.v) if e is None else np.asarray(e, np.float64)

    @staticmethod
    def _of(o):
        return o if isinstance(o, V) else V(o)

    @staticmethod
    def _rounded(v, e):
        return V(v, e + U * np.abs(v))

    def __getitem__(self, i):
        return V(self.v[i], self.e[i])

    def __add__(self, o):
        o = V._of(o)
        return V._rounded(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        o = V._of(o)
        return V._rounded(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return V._of(o) - self

    __radd__ = __add__

    def __mul__(self, o):
        o = V._of(o)
        return V._rounded(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = V._of(o)
        return V._rounded(self.v / o.v, self.e / np.abs(o.v) + np.abs(self.v) * o.e / (o.v * o.v))


def _seg(ids, n, D, tv, te):
    """the sums of the terms (tv, te) by segment id: the propagated bounds and (D + 2) u sum |term|"""
    return V(np.bincount(ids, tv, n), np.bincount(ids, te, n) + (D + 2) * U * np.bincount(ids, np.abs(tv), n))


def _pick(ok, a, b):
    return V(np.where(ok, a.v, b.v), np.where(ok, a.e, b.e))


class Ref:
    """the fp64 arithmetic with bounds"""
    name = "fp64"

    def exact(self, a):
        return V(a)

    def abs(self, a):
        return V(np.abs(a.v), a.e)

    def clip(self, a):
        return V(np.where(a.v > 0, a.v, 0.0), a.e)

    def sqrt(self, a):
        ok = a.v > 0
        r = np.sqrt(np.where(ok, a.v, 1.0))
        return _pick(ok, V._rounded(r, a.e / (2 * r)), V(np.zeros_like(a.v)))

    def fma(self, a, b, c):
        v = a.v * b.v + c.v
        return V._rounded(v, np.abs(a.v) * b.e + np.abs(b.v) * a.e + c.e)

    def put(self, vec, r, src):
        out = V(vec.v.copy(), vec.e.copy())
        out.v[r], out.e[r] = src.v[r], src.e[r]
        return out

    def prev(self, vec, r):
        """vec with entry r taken from r - 1"""
        out = V(vec.v.copy(), vec.e.copy())
        out.v[r], out.e[r] = vec.v[r - 1], vec.e[r - 1]
        return out

    def sum_s(self, case, dr, dc):
        a = V(np.abs(case.val64))
        s = a if dr is None else (a * dr[case.erow]) * dc[case.ecol]
        return _seg(case.erow, case.M, case.Drow, s.v, s.e), _seg(case.ecol, case.N, case.Dcol, s.v, s.e)

    def dot(self, case, orient, vec, phase):
        a = case.val64
        if orient == "row":
            return _seg(case.erow, case.M, case.Drow, a * vec.v[case.ecol], np.abs(a) * vec.e[case.ecol])
        return _seg(case.ecol, case.N, case.Dcol, a * vec.v[case.erow], np.abs(a) * vec.e[case.erow])

    def inst_sum(self, case, side, p, q):
        ids, n, D = (case.ci, case.inst_n, case.Dn) if side == "n" else (case.ri, case.inst_m, case.Dm)
        return _seg(ids, case.K, D, p.v * q.v, np.abs(p.v) * q.e + np.abs(q.v) * p.e)

    def instmax(self, a, ids, K):
        mx = np.zeros(K)
        np.maximum.at(mx, ids, a.v)
        near = a.v + a.e >= mx[ids]
        be = np.zeros(K)
        np.maximum.at(be, ids[near], a.e[near])
        return V(mx, be)

    def eta(self, step, prod):
        ok = prod.v > 0
        r = self.sqrt(_pick(ok, prod, V(np.ones_like(prod.v))))
        r = V(r.v, r.e + U * np.abs(r.v))       # the hardware's root: within 1 ulp of the rounded one
        return _pick(ok, V(np.full_like(prod.v, step)) / r, V(np.full_like(prod.v, step)))

    def ratio_or_one(self, a, b):
        ok = (a.v > 0) & (b.v > 0)
        one = V(np.ones_like(a.v))
        return _pick(ok, _pick(ok, a, one) / _pick(ok, b, one), one)

    def update(self, d, R):
        ok = R.v > 0
        return _pick(ok, d / self.sqrt(_pick(ok, R, V(np.ones_like(R.v)))), d)


# ---------------------------------------------------------------------------------------------------
# fp32 in the device's lane order
# ---------------------------------------------------------------------------------------------------
class Plan:
    """the ordered sum of every segment of `ptr`: lane l of G adds terms l, l + G, ... from 0, then the lanes pairwise.  G is
    picked by row_tier of the segment's length, or is `lanes` for all (the order of c'x: 1024)"""

    def __init__(self, ptr, lanes=None):
        self.ptr = np.asarray(ptr, np.int64)
        self.len = np.diff(self.ptr)
        self.n = len(self.len)
        tier = row_tier(self.len) if lanes is None else np.full(self.n, 2)
        self.groups = []
        for t, G in enumerate((16, 64, 1024) if lanes is None else (lanes,) * 3):
            steps = -(-self.len // G)
            for s in np.unique(steps[(tier == t) & (self.len > 0)]):
                R = np.flatnonzero((tier == t) & (steps == s))
                off = np.arange(s * G)[None, :]
                P = np.where(off < self.len[R][:, None], self.ptr[R][:, None] + off, self.ptr[-1])
                self.groups.append((R, P, int(s), G))

    def sum(self, terms):
        ext = np.concatenate([np.asarray(terms, np.float32), np.zeros(1, np.float32)])
        out = np.zeros(self.n, np.float32)
        for R, P, steps, G in self.groups:
            T = ext[P].reshape(len(R), steps, G)
            acc = T[:, 0, :].copy()
            for s in range(1, steps):
                acc = acc + T[:, s, :]
            while acc.shape[1] > 1:
                acc = acc[:, 0::2] + acc[:, 1::2]
            out[R] = acc[:, 0]
        return out


class Lane:
    """fp32, products rounded apart from their sums, sums in the lane order.  `mut` = dict(kind=..., orient="row" | "col", r=the
    global row or column) breaks it:  drop_last, drop_tail (the terms from 1024 floor((L - 1) / 1024) on) of row r in the sweeps of
    an iteration and of the evaluation;  unwritten (row r keeps what it held);  neighbour_rhs (row r is finished with b_(r-1), a
    column with c_(r-1));  and, on every row,  swap_w, no_reflect, no_clip, tc_is_dc, eval_iterate (the evaluation reads the
    iterate instead of the step's output)"""
    name = "fp32 lanes"

    def __init__(self, mut=None):
        self.mut = mut or {}

    def exact(self, a):
        return np.asarray(a, np.float32)

    def abs(self, a):
        return np.abs(a)

    def clip(self, a):
        return np.where(a > 0, a, np.float32(0))

    def sqrt(self, a):
        return np.sqrt(np.where(a > 0, a, np.float32(0)))

    def fma(self, a, b, c):
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)

    def put(self, vec, r, src):
        out = vec.copy()
        out[r] = src[r]
        return out

    def prev(self, vec, r):
        out = vec.copy()
        out[r] = vec[r - 1]
        return out

    def sum_s(self, case, dr, dc):
        a, at = np.abs(case.val), np.abs(case.at_val)
        if dr is not None:
            a, at = (a * dr[case.erow]) * dc[case.ecol], (at * dr[case.at_idx]) * dc[case.at_col]
        return case.rows.sum(a), case.cols.sum(at)

    def dot(self, case, orient, vec, phase):
        if orient == "row":
            plan, terms = case.rows, case.val * vec[case.ecol]
        else:
            plan, terms = case.cols, case.at_val * vec[case.at_idx]
        m = self.mut
        if m.get("kind") in ("drop_last", "drop_tail") and m["orient"] == orient and phase in m.get("phases", ("iter", "eval")):
            r = m["r"]
            L = int(plan.len[r])
            keep = L - 1 if m["kind"] == "drop_last" else 1024 * ((L - 1) // 1024)
            terms[plan.ptr[r] + keep:plan.ptr[r + 1]] = 0       # (adding +0 is exact: the terms are dropped)
        return plan.sum(terms)

    def inst_sum(self, case, side, p, q):
        return (case.inst_n_plan if side == "n" else case.inst_m_plan).sum(p * q)

    def instmax(self, a, ids, K):
        mx = np.zeros(K, np.float32)
        np.maximum.at(mx, ids, a)
        return mx

    def eta(self, step, prod):
        ok = prod > 0
        return np.where(ok, np.float32(step) / np.sqrt(np.where(ok, prod, np.float32(1))), np.float32(step)).astype(np.float32)

    def ratio_or_one(self, a, b):
        ok = (a > 0) & (b > 0)
        return np.where(ok, np.where(ok, a, 1) / np.where(ok, b, 1), 1).astype(np.float32)

    def update(self, d, R):
        ok = R > 0
        return np.where(ok, d / np.sqrt(np.where(ok, R, np.float32(1))), d).astype(np.float32)


# ---------------------------------------------------------------------------------------------------
# the rule, once
# ---------------------------------------------------------------------------------------------------
def scaling(ar, case, scaled, ruiz, pock_chambolle):
    """dr, dc and the row and column sums of the final s_ij"""
    dr, dc = ar.exact(np.ones(case.M)), ar.exact(np.ones(case.N))
    if not scaled:
        return (dr, dc) + ar.sum_s(case, None, None)
    f = case.ruiz(ruiz)
    dr, dc = ar.exact(f[0]), ar.exact(f[1])
    if pock_chambolle:
        R, C = ar.sum_s(case, dr, dc)
        dr, dc = ar.update(dr, R), ar.update(dc, C)
    return (dr, dc) + ar.sum_s(case, dr, dc)


def start_vector(case):
    """mllp_lp_pdhg_spectral's hash start, by the column's index inside its instance (exact in fp32)"""
    j = (np.arange(case.N) - np.asarray(case.dict["ptr_n"])[case.ci]).astype(np.uint64)
    return 1.0 + (((j * np.uint64(2654435761)) & np.uint64(0xffffffff)) >> np.uint64(9)).astype(np.float64) * 2.0 ** -23


def power(ar, case, rounds, ruiz=10, pock_chambolle=True):
    """sigma_est [n_inst] of mllp_lp_pdhg_spectral after `rounds` >= 1 rounds (every instance here has rows and columns).  The
    two walks are the phase "power" of a mutation"""
    dr, dc, _, _ = scaling(ar, case, True, ruiz, pock_chambolle)
    w = ar.exact(start_vector(case))
    nu = ar.sqrt(ar.inst_sum(case, "n", w, w))
    for _ in range(rounds):
        v = w / nu[case.ci]
        u = dr * ar.dot(case, "row", dc * v, "power")
        w = dc * ar.dot(case, "col", dr * u, "power")
        nu = ar.sqrt(ar.inst_sum(case, "n", w, w))
    return ar.sqrt(nu)


def rule(ar, case, call, K, step=0.9, ruiz=10, pock_chambolle=True, primal_weight=True, reflect=True, mut=None):
    """x, y (the output point), dr, dc, xun (the last unclipped x), kkt = [primal, dual, gap, eta, w0, w], each [n_inst]"""
    assert call in CALLS
    kind = (mut or {}).get("kind")
    scaled, halpern = call != "pdhg", call == "pdhg_halpern"
    ri, ci, Kn = case.ri, case.ci, case.K
    c, b = ar.exact(case.c), ar.exact(case.b)
    step = np.float32(step)
    ones = lambda n: ar.exact(np.ones(n))       # noqa: E731
    dr, dc, R, C = scaling(ar, case, scaled, ruiz, pock_chambolle)
    if scaled:
        tr, tc = dr * dr, dc * dc
    eta = ar.eta(step, ar.instmax(C, ci, Kn) * ar.instmax(R, ri, Kn))
    w0 = ones(Kn)
    if scaled and primal_weight:
        vc, vb = dc * c, dr * b
        w0 = ar.ratio_or_one(ar.sqrt(ar.inst_sum(case, "n", vc, vc)), ar.sqrt(ar.inst_sum(case, "m", vb, vb)))
    if scaled:
        tau, sigma = eta / w0, eta * w0
        step_c, step_r = tau[ci] * (dc if kind == "tc_is_dc" else tc), sigma[ri] * tr
    else:
        step_c, step_r = eta[ci], eta[ri]
    x, y = ar.clip(ar.exact(case.x0)), ar.exact(case.y0)
    xa, ya, xh, yh, xun = x, y, x, y, x
    for k in range(K):
        cc = ar.prev(c, mut["r"]) if kind == "neighbour_rhs" and mut["orient"] == "col" else c
        xun = x - step_c * (cc - ar.dot(case, "col", y, "iter"))
        xn = xun if kind == "no_clip" else ar.clip(xun)
        xb = (xn + xn) - x
        bb = ar.prev(b, mut["r"]) if kind == "neighbour_rhs" and mut["orient"] == "row" else b
        yn = y + step_r * (bb - ar.dot(case, "row", xb, "iter"))
        if halpern:
            w1, w2 = ar.exact(np.full(Kn, k + 1.0)) / ar.exact(np.full(Kn, k + 2.0)), ar.exact(np.ones(Kn)) / ar.exact(np.full(Kn, k + 2.0))
            if kind == "swap_w":
                w1, w2 = w2, w1
            refl = reflect and kind != "no_reflect"
            x1 = ar.fma(w1[ci], xb if refl else xn, w2[ci] * xa)
            y1 = ar.fma(w1[ri], (yn + yn) - y if refl else yn, w2[ri] * ya)
        else:
            x1, y1 = xn, yn
        if kind == "unwritten":        # a row that no lane finished keeps what it held
            y1, yn = ar.put(y1, mut["r"], y), ar.put(yn, mut["r"], yh)
        x, y, xh, yh = x1, y1, xn, yn
    px, py = (xh, yh) if halpern else (x, y)
    ex, ey = (x, y) if kind == "eval_iterate" else (px, py)
    rp = ar.abs(ar.dot(case, "row", ex, "eval") - b)
    rd = ar.clip(ar.dot(case, "col", ey, "eval") - c)
    den_p, den_d = ones(Kn) + ar.instmax(ar.abs(b), ri, Kn), ones(Kn) + ar.instmax(ar.abs(c), ci, Kn)
    cx, by = ar.inst_sum(case, "n", c, ex), ar.inst_sum(case, "m", b, ey)
    gap = ar.abs(cx - by) / ((ones(Kn) + ar.abs(cx)) + ar.abs(by))
    w = w0          # (no check, no restart: the weight never moves)
    kkt = [ar.instmax(rp, ri, Kn) / den_p, ar.instmax(rd, ci, Kn) / den_d, gap, eta, w0, w]
    return dict(x=px, y=py, dr=dr, dc=dc, xun=xun, kkt=kkt, rp=rp, rd=rd)


def reference(case, call, K, **kw):
    return rule(Ref(), case, call, K, **kw)


def lane32(case, call, K, mut=None, **kw):
    return rule(Lane(mut), case, call, K, mut=mut, **kw)


def ratio(got, ref):
    """|got - ref| over the acceptance bound, 2 x the first-order bound, elementwise (0 / 0 = 0)"""
    d = np.abs(np.asarray(got, np.float64) - ref.v)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d == 0, 0.0, d / (2.0 * ref.e))


def ratios(got, ref, kkt_words=6):
    """{name: ratio array} of x, y, dr, dc and kkt [n_inst, kkt_words] against a reference; `got` holds arrays"""
    out = {k: ratio(got[k], ref[k]) for k in ("x", "y", "dr", "dc") if k in got}
    kk = np.asarray(got["kkt"], np.float64).reshape(-1, kkt_words) if not isinstance(got["kkt"], list) else np.stack(got["kkt"], 1)
    out["kkt"] = np.stack([ratio(kk[:, q], ref["kkt"][q]) for q in range(kkt_words)], 1)
    return out


def worst(rs):
    return max(float(v.max(initial=0.0)) for v in rs.values())


# ---------------------------------------------------------------------------------------------------
# the batches
# ---------------------------------------------------------------------------------------------------
class Case:
    """a batch (test_basis_repair.dense_case's dict `c` with c, b set) with x0, y0, in the forms the two arithmetics read"""

    def __init__(self, c, x0, y0, designated):
        self.dict, self.x0, self.y0, self.designated = c, np.asarray(x0, np.float32), np.asarray(y0, np.float32), designated
        self.M, self.N, self.K = c["M"], c["N"], len(c["inst_m"])
        self.inst_m, self.inst_n = np.asarray(c["inst_m"], np.int64), np.asarray(c["inst_n"], np.int64)
        self.c, self.b = np.asarray(c["c"], np.float32), np.asarray(c["b"], np.float32)
        self.A = sp.csr_matrix((c["val"].astype(np.float32), c["idx"].astype(np.int64), c["ptr"].astype(np.int64)), shape=(self.M, self.N))
        At = sp.csr_matrix(self.A.T)
        At.sort_indices()               # a column's entries by ascending row id: the library's transposition
        self.val, self.val64 = self.A.data, self.A.data.astype(np.float64)
        self.erow, self.ecol = np.repeat(np.arange(self.M), np.diff(self.A.indptr)), self.A.indices.astype(np.int64)
        self.at_val, self.at_idx = At.data, At.indices.astype(np.int64)
        self.at_col = np.repeat(np.arange(self.N), np.diff(At.indptr))
        self.ri, self.ci = np.repeat(np.arange(self.K), self.inst_m), np.repeat(np.arange(self.K), self.inst_n)
        self.rows, self.cols = Plan(self.A.indptr), Plan(At.indptr)
        self.inst_m_plan, self.inst_n_plan = Plan(c["ptr_m"], 1024), Plan(c["ptr_n"], 1024)
        self.Drow, self.Dcol = depth(self.rows.len), depth(self.cols.len)
        self.Dm, self.Dn = depth_inst(self.inst_m), depth_inst(self.inst_n)
        self._ruiz = {}

    def ruiz(self, passes):
        """the fp32 oracle's factors (block diagonal: every instance's own)"""
        if passes not in self._ruiz:
            self._ruiz[passes] = ps.scaling(self.A, passes, False, np.float32) if self.A.nnz else (np.ones(self.M, np.float32), np.ones(self.N, np.float32))
        return self._ruiz[passes]


def _mag(rng, n, positive=False):
    """magnitudes in [0.5, 1.5], random signs, fp32"""
    v = rng.uniform(0.5, 1.5, n)
    return (v if positive else v * rng.choice([-1.0, 1.0], n)).astype(np.float32)


def _finish(mats, seed, designate, dense_case):
    """c, b, x0, y0 of a batch; designated columns get c = (A'y0 rounded) - 2, so that their first step moves up"""
    rng = np.random.default_rng(seed)
    c = dense_case(mats, seed)
    x0, y0 = _mag(rng, c["N"], True), _mag(rng, c["M"])
    c["c"], c["b"] = _mag(rng, c["N"]), _mag(rng, c["M"])
    case = Case(c, x0, y0, None)
    Aty = np.asarray(case.A.T.astype(np.float64) @ y0.astype(np.float64))
    des = designate(case)
    c["c"][des] = (Aty[des].astype(np.float32) - np.float32(2)).astype(np.float32)
    return c, x0, y0, des


def clip_margin(case):
    """the smallest unclipped x of a designated column over its acceptance bound, over every run of RUNS with K >= 1"""
    worst_of = np.inf
    for call, kw, Ks in RUNS:
        for K in Ks:
            if K and case.designated.any():
                xun = reference(case, call, K, **kw)["xun"]
                with np.errstate(divide="ignore", invalid="ignore"):
                    worst_of = min(worst_of, float((xun.v / (2.0 * xun.e))[case.designated].min()))
    return worst_of


def _join(parts, dense_case, designated):
    """one Case from per-instance (matrix, c, b, x0, y0)"""
    c = dense_case([p[0] for p in parts], 0)
    c["c"], c["b"] = (np.concatenate([p[q] for p in parts]).astype(np.float32) for q in (1, 2))
    x0, y0 = (np.concatenate([p[q] for p in parts]).astype(np.float32) for q in (3, 4))
    return Case(c, x0, y0, designated(c))


def _tier_instance(rng, L, wide):
    """1 x L (wide): b = (A x0 rounded) - 2, so |A x - b| ~ 2 at the start, and every c_j below a_j y0, so that x moves up;
    L x 1: c = (A'y0 rounded) - 2, the dual residual ~ 2"""
    a = _mag(rng, L).reshape((1, L) if wide else (L, 1))
    x0, y0 = _mag(rng, a.shape[1], True), _mag(rng, a.shape[0])
    Ax, Aty = a.astype(np.float64) @ x0.astype(np.float64), a.T.astype(np.float64) @ y0.astype(np.float64)
    if wide:
        return a, Aty.astype(np.float32) - _mag(rng, L, True), Ax.astype(np.float32) - np.float32(2), x0, y0
    return a, Aty.astype(np.float32) - np.float32(2), _mag(rng, L), x0, y0


TIERS_TRIES = 64


def tiers(dense_case, seed=1):
    """one 1 x L and one L x 1 instance per L of TIER_LENGTHS, every column designated.  An instance is drawn again (the
    results of an instance do not depend on its batch) until no column's unclipped value comes within 8 acceptance bounds of
    the clip in any run of RUNS: a column that clips hides its own sum"""
    everything = lambda c: np.ones(c["N"], bool)       # noqa: E731
    parts = []
    for L in TIER_LENGTHS:
        for wide in (True, False):
            for attempt in range(TIERS_TRIES):
                part = _tier_instance(np.random.default_rng([seed, L, wide, attempt]), L, wide)
                if clip_margin(_join([part], dense_case, everything)) > 8.0:
                    break
            else:
                raise AssertionError(f"tiers: no draw of the {'1 x L' if wide else 'L x 1'} instance, L = {L}, stays clear of the clip")
            parts.append(part)
    return _join(parts, dense_case, everything)


MIXED_ROWS = {0: 0, 1: 1, 2: 16, 3: 17, 5: 64, 6: 0, 8: 65, 13: 128, 18: 1023, 23: 1024, 30: 1025, 41: 65, 47: 2049, 50: 1024,
              127: 128, 128: 1100, 192: 2048}
MIXED_SHAPE = (193, 2100)


def mixed(dense_case, seed=2):
    """one 193 x 2100 instance with the row lengths of MIXED_ROWS (2 to 6 terms elsewhere), and its transpose"""
    rng = np.random.default_rng(seed)
    m, n = MIXED_SHAPE
    a = np.zeros((m, n), np.float32)
    for r in range(m):
        L = MIXED_ROWS.get(r, int(rng.integers(2, 7)))
        a[r, rng.choice(n, L, replace=False)] = _mag(rng, L)
    c, x0, y0, des = _finish([a, a.T.copy()], seed, lambda case: case.cols.len > 64, dense_case)
    return Case(c, x0, y0, des)


MANY_SHAPES = ((2, 3), (0, 2), (3, 0), (1, 1), (5, 12))
MANY_COUNT, MANY_BIG, MANY_BIG_SHAPE = 1100, 1030, (70, 130)


def many_matrix(k, seed=3):
    m, n = MANY_BIG_SHAPE if k == MANY_BIG else MANY_SHAPES[k % len(MANY_SHAPES)]
    rng = np.random.default_rng([seed, k])
    dens = 0.1 if k == MANY_BIG else 0.6 if (m, n) == (5, 12) else 1.0
    return (_mag(rng, m * n) * (rng.random(m * n) < dens)).reshape(m, n)


def many(dense_case, seed=3):
    """1100 instances cycling through MANY_SHAPES with one 70 x 130 at 1030: items behind instance 1024 in both orientations"""
    rng = np.random.default_rng(seed)
    mats = []
    for k in range(MANY_COUNT):
        mats.append(many_matrix(k, seed))
    c, x0, y0, des = _finish(mats, seed, lambda case: np.zeros(case.N, bool), dense_case)
    # c > 0 and b = A x for an x > 0: every instance has a solution (no exact ray: mllp_lp_pdhg_rays stops none), b = 0 without columns
    c["c"] = np.abs(c["c"])
    c["b"] = np.asarray(Case(c, x0, y0, des).A.astype(np.float64) @ _mag(rng, c["N"], True).astype(np.float64)).astype(np.float32)
    return Case(c, x0, y0, des)


# what every test runs: (call, options of `rule`, the K's).  K = 3 for the Halpern call: w1 = w2 at k = 0, so the first output
# that tells the two weights apart is the third
RUNS = [("pdhg", {}, (0, 1, 2)),
        ("pdhg_scaled", dict(ruiz=0, pock_chambolle=False, primal_weight=False), (0, 1, 2)),
        ("pdhg_scaled", dict(ruiz=0, pock_chambolle=True), (0, 1, 2)),
        ("pdhg_scaled", {}, (0, 1, 2)),
        ("pdhg_halpern", dict(reflect=True), (0, 1, 2, 3)),
        ("pdhg_halpern", dict(reflect=False), (0, 1, 2, 3))]


def first_row(case, tier, least=2):
    """the first row of the given tier with at least `least` terms"""
    return int(np.flatnonzero((row_tier(case.rows.len) == tier) & (case.rows.len >= least))[0])


def first_col(case, tier, least=2):
    return int(np.flatnonzero((row_tier(case.cols.len) == tier) & (case.cols.len >= least))[0])
