"""numpy restatement of THE RULE of mllp_lp_pdhg (include/mllp_hip.h): restarted PDHG on  min c'x, A x = b, x >= 0,  one
instance at a time, parameterized by dtype.  Test infrastructure: no GPU, no library.

`solve(..., dtype=np.float64)` is the oracle; `dtype=np.float32` is the same rule with every elementwise operation rounded as
the device rounds it (fsub, fmul, fadd, fdiv in the header's expressions; numpy keeps float32 arrays times float32 scalars
in float32) and the sums in scipy's order (a row's terms one after the other) instead of the device's lanes-then-butterfly.
The distance between the two is what fp32 costs this iteration in SOME summation order, and tests/test_pdhg.py derives its
bar from it; neither run is the kernel.

MARGIN.  A check takes up to three comparisons between floats: err(avg) against err(cur), e against eps, e against
beta e_last.  (25 cnt >= 9 it is between integers.)  `margin` is the smallest relative distance |p - q| / max(|p|, |q|) of
any comparison that was evaluated, over all checks of the run: a run whose margin is well above the fp32 error of the
errors takes the same decisions in fp32 as in fp64, in any summation order.
"""
import numpy as np
import scipy.sparse as sp

import planted_oracle as po

CODE_OPTIMAL, CODE_LIMIT, CODE_NOT_FINITE = 0, 6, 8


def _clip(t):
    return np.where(t > 0, t, np.zeros_like(t))


def _nan_max(v):
    """max of non-negative numbers that keeps a NaN; 0 for none"""
    return v.dtype.type(0) if v.size == 0 else np.max(v)


def step_size(A, step, dtype):
    one = np.abs(A)
    n1 = _nan_max(np.asarray(one.sum(0)).reshape(-1).astype(dtype)) if A.shape[0] and A.shape[1] else dtype(0)
    ninf = _nan_max(np.asarray(one.sum(1)).reshape(-1).astype(dtype)) if A.shape[0] and A.shape[1] else dtype(0)
    prod = dtype(n1 * ninf)
    return dtype(dtype(step) / np.sqrt(prod)) if prod > 0 else dtype(step)


def errors(A, At, b, c, x, y, nb, nc):
    """(primal, dual, gap) of the point (x, y) in the dtype of the arguments"""
    t = b.dtype.type
    with np.errstate(invalid="ignore", over="ignore"):
        p = _nan_max(np.abs(A @ x - b)) / (t(1) + nb)
        v = At @ y - c
        d = _nan_max(np.where((v > 0) | np.isnan(v), np.abs(v), np.zeros_like(v))) / (t(1) + nc)
        cx, by = t(np.dot(c, x)), t(np.dot(b, y))
        g = np.abs(cx - by) / ((t(1) + np.abs(cx)) + np.abs(by))
    return t(p), t(d), t(g)


def _worst(e):
    return e[0] * np.nan if np.isnan(e).any() else max(e)


def _rel(p, q):
    if not (np.isfinite(p) and np.isfinite(q)):
        return np.inf
    big = max(abs(float(p)), abs(float(q)))
    return 0.0 if big == 0.0 else abs(float(p) - float(q)) / big


def solve(A, b, c, max_iters, check_every=64, eps=2.0 ** -10, step=0.9, beta=0.5, x0=None, y0=None, dtype=np.float64):
    """The rule on one instance.  A: anything scipy.sparse takes, m x n.  Returns dict: x, y, status = [code, iterations,
    restarts, average returned], kkt = [primal, dual, gap, eta], margin, checks (one dict per check)."""
    dtype = np.dtype(dtype).type
    A = sp.csr_matrix(A, dtype=dtype)
    At = sp.csr_matrix(A.T)
    m, n = A.shape
    b, c = np.asarray(b, dtype).reshape(m), np.asarray(c, dtype).reshape(n)
    eps, beta = dtype(eps), dtype(beta)
    eta = step_size(A, step, dtype)
    nb, nc = _nan_max(np.abs(b)), _nan_max(np.abs(c))
    x = _clip(np.zeros(n, dtype) if x0 is None else np.asarray(x0, dtype).reshape(n).copy())
    y = np.zeros(m, dtype) if y0 is None else np.asarray(y0, dtype).reshape(m).copy()
    xs, ys, cnt = np.zeros(n, dtype), np.zeros(m, dtype), 0
    it, restarts, e_last, margin, checks = 0, 0, dtype(np.inf), np.inf, []
    code, avg_out, out_err = None, 0, None
    with np.errstate(invalid="ignore", over="ignore"):
        while it < max_iters:
            g = c - At @ y
            xn = _clip(x - eta * g)
            xb = (xn + xn) - x
            y = y + eta * (b - A @ xb)
            x = xn
            it += 1
            if check_every <= 0:
                continue
            xs, ys, cnt = xs + x, ys + y, cnt + 1
            if it % check_every:
                continue
            xa, ya = xs / dtype(cnt), ys / dtype(cnt)
            err_a, err_c = errors(A, At, b, c, xa, ya, nb, nc), errors(A, At, b, c, x, y, nb, nc)
            ea, ec = _worst(err_a), _worst(err_c)
            use_avg = bool(ea < ec)
            e = ea if use_avg else ec
            rec = dict(it=it, cnt=cnt, ea=float(ea), ec=float(ec), use_avg=use_avg, e_last=float(e_last))
            checks.append(rec)
            if not np.isfinite(e):
                code, out_err = CODE_NOT_FINITE, err_c
                break
            margin = min(margin, _rel(ea, ec), _rel(e, eps))
            stop = bool(e <= eps)
            if not stop:
                if np.isfinite(e_last):
                    margin = min(margin, _rel(e, beta * e_last))
                if not (e <= beta * e_last or 25 * cnt >= 9 * it):
                    continue
            if use_avg:
                x, y = xa, ya
            xs, ys = np.zeros(n, dtype), np.zeros(m, dtype)
            if stop:
                code, avg_out, out_err = CODE_OPTIMAL, int(use_avg), err_a if use_avg else err_c
                break
            restarts, e_last, cnt = restarts + 1, e, 0
            rec["restart"] = True
        if code is None:
            code, out_err = CODE_LIMIT, errors(A, At, b, c, x, y, nb, nc)
    return dict(x=x, y=y, status=[code, it, restarts, avg_out], kkt=[*out_err, eta], margin=margin, checks=checks, eta=eta)


def errors64(A, b, c, x, y):
    """the three errors of a point, recomputed in fp64 (what tests/test_pdhg.py holds a device output to)"""
    A = sp.csr_matrix(A, dtype=np.float64)
    b, c, x, y = (np.asarray(v, np.float64) for v in (b, c, x, y))
    return errors(A, sp.csr_matrix(A.T), b, c, x, y, _nan_max(np.abs(b)), _nan_max(np.abs(c)))


# ---- planted instances ----------------------------------------------------------------------------------------------------
def split(c, values, x1, x2, labels):
    """per instance dict(A csr fp64, b, c, labels, xstar (on the planted basis, 0 elsewhere), ystar) of a planted case `c`
    (tests/planted_oracle.ragged_case's dict) from the values, costs and right-hand sides that are stored"""
    out = []
    for k, (m, n) in enumerate(zip(c["inst_m"], c["inst_n"])):
        r, s = slice(c["ptr_m"][k], c["ptr_m"][k + 1]), slice(c["ptr_n"][k], c["ptr_n"][k + 1])
        e = slice(c["nnz_off"][k], c["nnz_off"][k + 1])
        ptr = c["ptr"][r.start:r.stop + 1].astype(np.int64)
        A = sp.csr_matrix((np.asarray(values[e], np.float64), c["idx"][e].astype(np.int64) - c["ptr_n"][k], ptr - ptr[0]), shape=(m, n))
        lab = np.asarray(labels[s], np.float64)
        out.append(dict(A=A, b=np.asarray(x2[r], np.float64), c=np.asarray(x1[s], np.float64), labels=lab,
                        xstar=np.asarray(c["xstar"][s], np.float64) * lab, ystar=np.asarray(c["ystar"][r], np.float64), m=m, n=n))
    return out


def cpu_planted(c):
    """the same, planted by the fp64 restatement of the planting rule and rounded to fp32 (no GPU)"""
    p = po.plant(c["ptr"], c["idx"], c["val"], c["pivot"], c["xstar"], c["ystar"], c["slack"], c["N"])
    f32 = lambda a: np.asarray(a, np.float32)      # noqa: E731
    return split(c, f32(p["values"]), f32(p["c"]), f32(p["b"]), f32(p["labels"]))


def join_cases(cases):
    """one batch from several cases (the dicts of planted_oracle.ragged_case / test_basis_repair.planted_shapes)"""
    inst_m = [m for c in cases for m in c["inst_m"]]
    inst_n = [n for c in cases for n in c["inst_n"]]
    ptr_m, ptr_n = np.concatenate([[0], np.cumsum(inst_m)]), np.concatenate([[0], np.cumsum(inst_n)])
    nnz_off, ptr, idx, pivot, o_n, o_e = [0], [np.zeros(1, np.int64)], [], [], 0, 0
    for c in cases:
        ptr.append(c["ptr"][1:].astype(np.int64) + o_e)
        idx.append(c["idx"].astype(np.int64) + o_n)
        pivot.append(c["pivot"].astype(np.int64) + o_n)
        nnz_off += [int(v) + o_e for v in c["nnz_off"][1:]]
        o_n, o_e = o_n + c["N"], o_e + len(c["idx"])
    cat = lambda f: np.concatenate([c[f] for c in cases])      # noqa: E731
    return dict(inst_m=inst_m, inst_n=inst_n, ptr_m=ptr_m, ptr_n=ptr_n, nnz_off=np.array(nnz_off), ptr=np.concatenate(ptr).astype(np.int32),
                idx=np.concatenate(idx).astype(np.int32), val=cat("val"), pivot=np.concatenate(pivot).astype(np.int32),
                xstar=cat("xstar"), ystar=cat("ystar"), slack=cat("slack"), M=int(ptr_m[-1]), N=int(ptr_n[-1]))


def topm(x, m):
    """mask of the m largest entries of x, the lowest index first among equals (LPBatch.ranking's order)"""
    order = np.argsort(-np.asarray(x, np.float64), kind="stable")[:m]
    mask = np.zeros(len(x))
    mask[order] = 1.0
    return mask
