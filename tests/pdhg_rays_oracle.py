"""numpy restatement of THE RULE of mllp_lp_pdhg_rays (include/mllp_hip.h): tests/pdhg_halpern_oracle.py's iteration, word for
word, with ONE step inserted into a check -- after "e not finite: code 8" and "e <= eps: code 0", before the restart test, and
only when ray_eps >= 0: the direction from the anchor to the step's output, (rx, ry) = (xh - xa, yh - ya), is judged as a ray of
the ORIGINAL LP  min c'x, A x = b, x >= 0  by PDLP's two relative tests,

    qp = max_j (A'ry)_j^+ / b'ry              when b'ry is finite and > 0, else +inf      qp <= ray_eps: code 4, ry certifies
    qd = max(|A rx|_inf, max_j (-rx_j)^+) / -c'rx   when c'rx is finite and < 0, else +inf      else qd <= ray_eps: code 5, rx

and an instance at code 4 or 5 stops as one at code 0 does.  Test infrastructure: no GPU, no library, parameterized by dtype as
the three oracles it stands on.  `dtype=np.float32` rounds every elementwise operation as the device does (the difference is
rounded before it enters a product) and takes the sums in scipy's / numpy's order instead of the device's.

MARGIN.  `margin` is pdhg_halpern_oracle's, over the comparisons of its rule, joined by the two new ones of every check that
reaches the ray step: qp against ray_eps and, when that does not decide, qd against ray_eps (a quality of +inf is at distance
+inf).  `ray_margin` is the smallest of the new ones alone.  The signs of b'ry and c'rx are no float comparisons of two
magnitudes: a sum that rounding could carry across zero has a quality far above any ray_eps, which the margin of qp / qd shows.

A check that stops with code 0 or 8 does not look at its rays: optimal wins.  For tests, such a check records what the rays WOULD
have given (`unused`) without it reaching the cert or the margin.
"""
import numpy as np
import scipy.sparse as sp

import pdhg_halpern_oracle as ph
import pdhg_oracle as pg
import pdhg_scaled_oracle as ps
from pdhg_oracle import CODE_LIMIT, CODE_NOT_FINITE, CODE_OPTIMAL  # noqa: F401

CODE_INFEASIBLE, CODE_UNBOUNDED = 4, 5


def _pos_max(v):
    """max_j max(v_j, 0) that keeps a NaN; 0 for none"""
    return pg._nan_max(np.where((v > 0) | np.isnan(v), np.abs(v), np.zeros_like(v)))


def qualities(A, At, b, c, rx, ry):
    """(qp, by, qd, cx) of the ray (rx, ry) in the dtype of the arguments"""
    t = b.dtype.type
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        by, cx = t(np.dot(b, ry)), t(np.dot(c, rx))
        U = _pos_max(At @ ry)
        V = max(pg._nan_max(np.abs(A @ rx)), _pos_max(-rx), key=lambda v: np.inf if np.isnan(v) else v)
        qp = t(U / by) if np.isfinite(by) and by > 0 else t(np.inf)
        qd = t(V / -cx) if np.isfinite(cx) and cx < 0 else t(np.inf)
    return qp, by, qd, cx


def solve(A, b, c, max_iters, check_every=64, eps=2.0 ** -10, step=0.9, beta=0.5, ruiz=10, pock_chambolle=True,
          primal_weight=True, weight_span=16.0, reflect=True, ray_eps=2.0 ** -10, x0=None, y0=None, dtype=np.float64):
    """The rule on one instance.  Returns pdhg_halpern_oracle.solve's dict, and: ray_x, ray_y (the certificate of code 5 / 4,
    zeros otherwise), cert = [qp, by, qd, cx] of the last check that evaluated the rays ([inf, 0, inf, 0] if none), ray_margin;
    a check's dict also holds qp, by, qd, cx where it evaluated them, or `unused` where it stopped before."""
    dtype = np.dtype(dtype).type
    A = sp.csr_matrix(A, dtype=dtype)
    At = sp.csr_matrix(A.T)
    m, n = A.shape
    b, c = np.asarray(b, dtype).reshape(m), np.asarray(c, dtype).reshape(n)
    eps, beta, span, ray_eps = dtype(eps), dtype(beta), dtype(weight_span), dtype(ray_eps)
    dr, dc = ps.scaling(A, ruiz, pock_chambolle, dtype)
    tr, tc = dr * dr, dc * dc
    eta = pg.step_size(ps.scaled_abs(A, dr, dc)[0], step, dtype)
    w0 = dtype(1)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if primal_weight:
            nc, nb = ps._norm2(dc * c), ps._norm2(dr * b)
            if ps._good(nc) and ps._good(nb):
                w0 = dtype(nc / nb)
        w, w_lo, w_hi = w0, dtype(w0 / span), dtype(w0 * span)
        tau, sigma = dtype(eta / w), dtype(eta * w)
        nb, nc = pg._nan_max(np.abs(b)), pg._nan_max(np.abs(c))
        x = pg._clip(np.zeros(n, dtype) if x0 is None else np.asarray(x0, dtype).reshape(n).copy())
        y = np.zeros(m, dtype) if y0 is None else np.asarray(y0, dtype).reshape(m).copy()
        xa, ya, xh, yh, k = x.copy(), y.copy(), x.copy(), y.copy(), 0
        it, restarts, e_last, margin, checks, weights, anchors = 0, 0, dtype(np.inf), np.inf, [], [], []
        code, out_err = None, None
        cert, ray_margin = [dtype(np.inf), dtype(0), dtype(np.inf), dtype(0)], np.inf
        while it < max_iters:
            w1, w2 = dtype(dtype(k + 1) / dtype(k + 2)), dtype(dtype(1) / dtype(k + 2))
            g = c - At @ y
            xh = pg._clip(x - (tau * tc) * g)
            xb = (xh + xh) - x
            yh = y + (sigma * tr) * (b - A @ xb)
            x = ph._anchored(w1, xb if reflect else xh, w2, xa, dtype)
            y = ph._anchored(w1, (yh + yh) - y if reflect else yh, w2, ya, dtype)
            k, it = k + 1, it + 1
            if check_every <= 0 or it % check_every:
                continue
            err = pg.errors(A, At, b, c, xh, yh, nb, nc)
            e = pg._worst(err)
            rec = dict(it=it, k=k, e=float(e), e_last=float(e_last), w=float(w))
            checks.append(rec)
            if not np.isfinite(e) or e <= eps:
                if np.isfinite(e):
                    margin = min(margin, pg._rel(e, eps))
                if ray_eps >= 0:
                    rec["unused"] = [float(v) for v in qualities(A, At, b, c, xh - xa, yh - ya)]
                code, out_err = (CODE_OPTIMAL if np.isfinite(e) else CODE_NOT_FINITE), err
                break
            margin = min(margin, pg._rel(e, eps))
            if ray_eps >= 0:
                qp, by, qd, cx = cert = list(qualities(A, At, b, c, xh - xa, yh - ya))
                rec.update(qp=float(qp), by=float(by), qd=float(qd), cx=float(cx))
                ray_margin = min(ray_margin, pg._rel(qp, ray_eps))
                if qp <= ray_eps:
                    code = CODE_INFEASIBLE
                else:
                    ray_margin = min(ray_margin, pg._rel(qd, ray_eps))
                    if qd <= ray_eps:
                        code = CODE_UNBOUNDED
                if code is not None:
                    out_err = err
                    break
            if np.isfinite(e_last):
                margin = min(margin, pg._rel(e, beta * e_last))
            if not (e <= beta * e_last or 25 * k >= 9 * it):
                continue
            x, y = xh.copy(), yh.copy()
            if primal_weight:
                d, q = x - xa, y - ya
                dx, dy = dtype(np.sqrt(np.dot(d, d / tc))) if n else dtype(0), dtype(np.sqrt(np.dot(q, q / tr))) if m else dtype(0)
                if ps._good(dx) and ps._good(dy):
                    raw = dtype(np.sqrt(dtype(w * dtype(dy / dx))))
                    margin = min(margin, pg._rel(raw, w_lo), pg._rel(raw, w_hi))
                    w = min(max(raw, w_lo), w_hi)
                    tau, sigma = dtype(eta / w), dtype(eta * w)
                    weights.append(dict(it=it, dx=float(dx), dy=float(dy), raw=float(raw), w=float(w)))
            xa, ya = x.copy(), y.copy()
            anchors.append(it)
            k, e_last, restarts = 0, e, restarts + 1
            rec["restart"] = True
        if code is None:
            code, out_err = CODE_LIMIT, pg.errors(A, At, b, c, xh, yh, nb, nc)
    ray_x = xh - xa if code == CODE_UNBOUNDED else np.zeros(n, dtype)
    ray_y = yh - ya if code == CODE_INFEASIBLE else np.zeros(m, dtype)
    return dict(x=xh, y=yh, status=[code, it, restarts, 0], kkt=[*out_err, eta, w0, w], margin=min(margin, ray_margin), checks=checks, eta=eta,
                dr=dr, dc=dc, w0=w0, w=w, weights=weights, anchors=anchors, anchor=(xa, ya), ray_x=ray_x, ray_y=ray_y, cert=cert,
                ray_margin=ray_margin)


# ---- the test LPs: the answer is known by construction ------------------------------------------------------------------------
def infeasible(inst):
    """the instance with its row 0 appended again and the new right-hand side b_0 + 1 (rounded to fp32, as the instance's own
    numbers are): two rows contradict each other"""
    A = sp.csr_matrix(inst["A"])
    return dict(A=sp.vstack([A, A[0]]).tocsr(), b=np.append(inst["b"], np.float64(np.float32(inst["b"][0] + 1.0))), c=inst["c"].copy(),
                m=inst["m"] + 1, n=inst["n"])


def unbounded(inst):
    """the instance with the negative of its column 0 appended, at cost -c_0 - 1 (rounded to fp32): it stays feasible, and
    e_0 + e_new is a recession direction of cost -1"""
    A = sp.csc_matrix(inst["A"])
    return dict(A=sp.hstack([A, -A[:, 0]]).tocsr(), b=inst["b"].copy(), c=np.append(inst["c"], np.float64(np.float32(-inst["c"][0] - 1.0))),
                m=inst["m"], n=inst["n"] + 1)


def verify64(inst, code, ray_x, ray_y, ray_eps):
    """the certificate, from the data alone, in fp64: (holds, quality).  Code 4: b'ry > 0 and max (A'ry)^+ <= ray_eps (1 + 2^-6)
    b'ry.  Code 5: c'rx < 0 and max(|A rx|, (-rx)^+) <= ray_eps (1 + 2^-6) (-c'rx)"""
    A = sp.csr_matrix(inst["A"], dtype=np.float64)
    b, c = np.asarray(inst["b"], np.float64), np.asarray(inst["c"], np.float64)
    bar = float(ray_eps) * (1 + 2.0 ** -6)
    if code == CODE_INFEASIBLE:
        ry = np.asarray(ray_y, np.float64)
        by, U = float(b @ ry), max(float((A.T @ ry).max(initial=0.0)), 0.0)
        return bool(by > 0 and U <= bar * by), U / by if by > 0 else np.inf
    if code == CODE_UNBOUNDED:
        rx = np.asarray(ray_x, np.float64)
        cx, V = float(c @ rx), max(float(np.abs(A @ rx).max(initial=0.0)), float((-rx).max(initial=0.0)))
        return bool(cx < 0 and V <= bar * -cx), V / -cx if cx < 0 else np.inf
    raise ValueError(code)
