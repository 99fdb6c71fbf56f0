"""numpy restatement of THE RULE of mllp_lp_pdhg_scaled (include/mllp_hip.h): diagonally preconditioned, restarted PDHG with
a clamped primal weight on  min c'x, A x = b, x >= 0,  one instance at a time, parameterized by dtype.  Test infrastructure:
no GPU, no library.  The checks, the stop, the restarts and the limit are tests/pdhg_oracle.py's, whose `errors` this file
calls: the errors are those of the ORIGINAL LP.

`dtype=np.float64` is the oracle; `dtype=np.float32` rounds every elementwise operation as the device does (the rule uses
fadd, fsub, fmul, fdiv, fsqrt only, which numpy's float32 rounds identically) and takes the sums in scipy's / numpy's order
instead of the device's lanes-then-butterfly.  The maxima of a Ruiz pass are exact in any order, so with
`pock_chambolle=False` the fp32 run's dr and dc ARE the device's, bit for bit.

MARGIN.  pdhg_oracle's three comparisons of a check, and at every weight update the two comparisons of the clamp: the
unclamped weight against w0 / span and against w0 * span.
"""
import numpy as np
import scipy.sparse as sp

import pdhg_oracle as pg
from pdhg_oracle import CODE_LIMIT, CODE_NOT_FINITE, CODE_OPTIMAL  # noqa: F401


def scaled_abs(A, dr, dc):
    """S with s_ij = fmul(fmul(|a_ij|, dr_i), dc_j), in A's own pattern and order"""
    S = sp.csr_matrix(A, copy=True)
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    S.data = (np.abs(A.data) * dr[rows]) * dc[A.indices]
    return S, rows


def _update(d, v):
    """d / sqrt(v) where v > 0 (a NaN is not), d elsewhere"""
    ok = v > 0
    out = d.copy()
    out[ok] = d[ok] / np.sqrt(v[ok])
    return out


def scaling(A, ruiz, pock_chambolle, dtype):
    """(dr, dc) after `ruiz` passes on the maxima and the optional pass on the sums"""
    dtype = np.dtype(dtype).type
    A = sp.csr_matrix(A, dtype=dtype)
    m, n = A.shape
    dr, dc = np.ones(m, dtype), np.ones(n, dtype)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for _ in range(int(ruiz)):
            S, rows = scaled_abs(A, dr, dc)
            R, C = np.zeros(m, dtype), np.zeros(n, dtype)
            np.maximum.at(R, rows, S.data)
            np.maximum.at(C, A.indices, S.data)
            dr, dc = _update(dr, R), _update(dc, C)
        if pock_chambolle:
            S, _ = scaled_abs(A, dr, dc)
            R = np.asarray(S.sum(1)).reshape(-1).astype(dtype) if m and n else np.zeros(m, dtype)
            C = np.asarray(S.sum(0)).reshape(-1).astype(dtype) if m and n else np.zeros(n, dtype)
            dr, dc = _update(dr, R), _update(dc, C)
    return dr, dc


def _norm2(v):
    return np.sqrt(np.dot(v, v)) if v.size else v.dtype.type(0)


def _good(v):
    return bool(np.isfinite(v) and v > 0)


def solve(A, b, c, max_iters, check_every=64, eps=2.0 ** -10, step=0.9, beta=0.5, ruiz=10, pock_chambolle=True,
          primal_weight=True, weight_span=16.0, x0=None, y0=None, dtype=np.float64):
    """The rule on one instance.  Returns pdhg_oracle.solve's dict with kkt = [primal, dual, gap, eta, w0, final w], and
    dr, dc, w0, w, weights (one dict per weight update: it, dx, dy, raw, w)."""
    dtype = np.dtype(dtype).type
    A = sp.csr_matrix(A, dtype=dtype)
    At = sp.csr_matrix(A.T)
    m, n = A.shape
    b, c = np.asarray(b, dtype).reshape(m), np.asarray(c, dtype).reshape(n)
    eps, beta, span = dtype(eps), dtype(beta), dtype(weight_span)
    dr, dc = scaling(A, ruiz, pock_chambolle, dtype)
    tr, tc = dr * dr, dc * dc
    eta = pg.step_size(scaled_abs(A, dr, dc)[0], step, dtype)
    w0 = dtype(1)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if primal_weight:
            nc, nb = _norm2(dc * c), _norm2(dr * b)
            if _good(nc) and _good(nb):
                w0 = dtype(nc / nb)
        w, w_lo, w_hi = w0, dtype(w0 / span), dtype(w0 * span)
        tau, sigma = dtype(eta / w), dtype(eta * w)
        nb, nc = pg._nan_max(np.abs(b)), pg._nan_max(np.abs(c))
        x = pg._clip(np.zeros(n, dtype) if x0 is None else np.asarray(x0, dtype).reshape(n).copy())
        y = np.zeros(m, dtype) if y0 is None else np.asarray(y0, dtype).reshape(m).copy()
        xr, yr = x.copy(), y.copy()
        xs, ys, cnt = np.zeros(n, dtype), np.zeros(m, dtype), 0
        it, restarts, e_last, margin, checks, weights = 0, 0, dtype(np.inf), np.inf, [], []
        code, avg_out, out_err = None, 0, None
        while it < max_iters:
            g = c - At @ y
            xn = pg._clip(x - (tau * tc) * g)
            xb = (xn + xn) - x
            y = y + (sigma * tr) * (b - A @ xb)
            x = xn
            it += 1
            if check_every <= 0:
                continue
            xs, ys, cnt = xs + x, ys + y, cnt + 1
            if it % check_every:
                continue
            xa, ya = xs / dtype(cnt), ys / dtype(cnt)
            err_a, err_c = pg.errors(A, At, b, c, xa, ya, nb, nc), pg.errors(A, At, b, c, x, y, nb, nc)
            ea, ec = pg._worst(err_a), pg._worst(err_c)
            use_avg = bool(ea < ec)
            e = ea if use_avg else ec
            rec = dict(it=it, cnt=cnt, ea=float(ea), ec=float(ec), use_avg=use_avg, e_last=float(e_last), w=float(w))
            checks.append(rec)
            if not np.isfinite(e):
                code, out_err = CODE_NOT_FINITE, err_c
                break
            margin = min(margin, pg._rel(ea, ec), pg._rel(e, eps))
            stop = bool(e <= eps)
            if not stop:
                if np.isfinite(e_last):
                    margin = min(margin, pg._rel(e, beta * e_last))
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
            if primal_weight:
                d, q = x - xr, y - yr
                dx, dy = dtype(np.sqrt(np.dot(d, d / tc))) if n else dtype(0), dtype(np.sqrt(np.dot(q, q / tr))) if m else dtype(0)
                if _good(dx) and _good(dy):
                    raw = dtype(np.sqrt(dtype(w * dtype(dy / dx))))
                    margin = min(margin, pg._rel(raw, w_lo), pg._rel(raw, w_hi))
                    w = min(max(raw, w_lo), w_hi)
                    tau, sigma = dtype(eta / w), dtype(eta * w)
                    weights.append(dict(it=it, dx=float(dx), dy=float(dy), raw=float(raw), w=float(w)))
                xr, yr = x.copy(), y.copy()
        if code is None:
            code, out_err = CODE_LIMIT, pg.errors(A, At, b, c, x, y, nb, nc)
    return dict(x=x, y=y, status=[code, it, restarts, avg_out], kkt=[*out_err, eta, w0, w], margin=margin, checks=checks, eta=eta,
                dr=dr, dc=dc, w0=w0, w=w, weights=weights)
