"""numpy restatement of THE RULE of mllp_lp_pdhg_halpern (include/mllp_hip.h): mllp_lp_pdhg_scaled's scaling, step and weight
with restarted Halpern PDHG (Lu and Yang's rHPDHG) as the iteration, on  min c'x, A x = b, x >= 0,  one instance at a time,
parameterized by dtype.  Test infrastructure: no GPU, no library.  The scaling is tests/pdhg_scaled_oracle.py's `scaling` /
`scaled_abs`, the step and the errors are tests/pdhg_oracle.py's `step_size` / `errors`: the errors are those of the ORIGINAL LP.

`dtype=np.float64` is the oracle; `dtype=np.float32` rounds every elementwise operation as the device does and takes the sums
in scipy's / numpy's order instead of the device's lanes-then-butterfly.  The rule's one fma outside a sum,
fma(w1, p, fmul(w2, anchor)), is formed in float64 and rounded once more to float32 -- the product of two float32 is exact
in float64, so this is the device's value except where the float64 sum falls within 2^-29 ulp of a float32 tie.  In float64
it is w1 * p + w2 * anchor.  k + 1 and k + 2 are converted to the dtype by numpy, which rounds to nearest as the device does.

MARGIN.  A check compares e against eps and, when it does not stop, e against beta e_last (25 k >= 9 it is between
integers); a weight update compares the unclamped weight against w0 / span and against w0 * span.  `margin` is the smallest
relative distance of any comparison that was evaluated.  There is ONE point per check: no average against current.
"""
import numpy as np
import scipy.sparse as sp

import pdhg_oracle as pg
import pdhg_scaled_oracle as ps
from pdhg_oracle import CODE_LIMIT, CODE_NOT_FINITE, CODE_OPTIMAL  # noqa: F401


def _anchored(w1, p, w2, a, dtype):
    """fma(w1, p, fmul(w2, a))"""
    if dtype is np.float32:
        return (w1.astype(np.float64) * p.astype(np.float64) + (w2 * a).astype(np.float64)).astype(np.float32)
    return w1 * p + w2 * a


def solve(A, b, c, max_iters, check_every=64, eps=2.0 ** -10, step=0.9, beta=0.5, ruiz=10, pock_chambolle=True,
          primal_weight=True, weight_span=16.0, reflect=True, x0=None, y0=None, dtype=np.float64):
    """The rule on one instance.  Returns pdhg_scaled_oracle.solve's dict: x, y (the output, (xh, yh)), status = [code,
    iterations, restarts, 0], kkt = [primal, dual, gap, eta, w0, final w], margin, checks (one dict per check: it, k, e,
    e_last, w, and restart where it restarted), eta, dr, dc, w0, w, weights (one dict per weight update), and anchors: the
    iteration of every move of the anchor."""
    dtype = np.dtype(dtype).type
    A = sp.csr_matrix(A, dtype=dtype)
    At = sp.csr_matrix(A.T)
    m, n = A.shape
    b, c = np.asarray(b, dtype).reshape(m), np.asarray(c, dtype).reshape(n)
    eps, beta, span = dtype(eps), dtype(beta), dtype(weight_span)
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
        while it < max_iters:
            w1, w2 = dtype(dtype(k + 1) / dtype(k + 2)), dtype(dtype(1) / dtype(k + 2))
            g = c - At @ y
            xh = pg._clip(x - (tau * tc) * g)
            xb = (xh + xh) - x
            yh = y + (sigma * tr) * (b - A @ xb)
            x = _anchored(w1, xb if reflect else xh, w2, xa, dtype)
            y = _anchored(w1, (yh + yh) - y if reflect else yh, w2, ya, dtype)
            k, it = k + 1, it + 1
            if check_every <= 0 or it % check_every:
                continue
            err = pg.errors(A, At, b, c, xh, yh, nb, nc)
            e = pg._worst(err)
            rec = dict(it=it, k=k, e=float(e), e_last=float(e_last), w=float(w))
            checks.append(rec)
            if not np.isfinite(e):
                code, out_err = CODE_NOT_FINITE, err
                break
            margin = min(margin, pg._rel(e, eps))
            if e <= eps:
                code, out_err = CODE_OPTIMAL, err
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
    return dict(x=xh, y=yh, status=[code, it, restarts, 0], kkt=[*out_err, eta, w0, w], margin=margin, checks=checks, eta=eta,
                dr=dr, dc=dc, w0=w0, w=w, weights=weights, anchors=anchors, anchor=(xa, ya))
