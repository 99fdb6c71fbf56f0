"""numpy restatement of THE RULE of mllp_lp_pdhg_spectral (include/mllp_hip.h): tests/pdhg_rays_oracle.py's solve, word for
word, with ONE step inserted into the set-up -- after the scaling and the bound sqrt(|S|_1 |S|_inf), before eta is formed: P
rounds of power iteration on S'S, S = diag(dr) A diag(dc), from the hash start, give sigma_est = sqrt(nu_P), and eta =
step / sigma_est where that is finite, positive and not above the bound; otherwise eta is the bound's.  Test infrastructure: no
GPU, no library, parameterized by dtype as the oracles it stands on.  `dtype=np.float32` rounds every elementwise operation as
the device does and takes the sums in scipy's / numpy's order instead of the device's.

Nothing of the iteration is written a second time: `solve` computes eta by the rule and runs pdhg_rays_oracle.solve with
pdhg_oracle.step_size -- the ONE place where that solve forms eta -- standing aside for the call's duration.  With
power_iters = 0 the function is not replaced at all: the result is pdhg_rays_oracle.solve's, and with ray_eps < 0 that is
pdhg_halpern_oracle.solve's.

`sigma_est=` doctors the estimate (tests of the fallback): the value takes the place of the power iteration's.
"""
import numpy as np
import scipy.sparse as sp

import pdhg_oracle as pg
import pdhg_rays_oracle as pr
import pdhg_scaled_oracle as ps
from pdhg_oracle import CODE_LIMIT, CODE_NOT_FINITE, CODE_OPTIMAL  # noqa: F401

HASH = 2654435761


def start_vector(n, dtype):
    """h_j = 1 + ((j 2654435761 mod 2^32) >> 9) 2^-23: exact in fp32, in [1, 2)"""
    j = np.arange(n, dtype=np.uint64)
    bits = ((j * np.uint64(HASH)) & np.uint64(0xffffffff)) >> np.uint64(9)
    return (1.0 + bits.astype(np.float64) * 2.0 ** -23).astype(dtype)


def power(A, dr, dc, power_iters, dtype):
    """(sigma_est or 0 when void, [nu_0, nu_1, ..., as far as the rounds ran]) of S = diag(dr) A diag(dc) in `dtype`"""
    dtype = np.dtype(dtype).type
    A = sp.csr_matrix(A, dtype=dtype)
    At = sp.csr_matrix(A.T)
    n = A.shape[1]
    nus = []
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        w = start_vector(n, dtype)
        for r in range(int(power_iters) + 1):
            if r:
                u = dr * (A @ (dc * v))         # noqa: F821  (v: the round before)
                w = dc * (At @ (dr * u))
            nu = dtype(ps._norm2(w))
            nus.append(nu)
            if not ps._good(nu):
                return dtype(0), nus
            v = w / nu                          # noqa: F841
        return dtype(np.sqrt(nus[-1])), nus


def bound(A, dr, dc, dtype):
    """L_bound = sqrt(|S|_1 |S|_inf), as pdhg_oracle.step_size forms it"""
    dtype = np.dtype(dtype).type
    S = ps.scaled_abs(sp.csr_matrix(A, dtype=dtype), dr, dc)[0]
    one = np.abs(S)
    full = S.shape[0] and S.shape[1]
    n1 = pg._nan_max(np.asarray(one.sum(0)).reshape(-1).astype(dtype)) if full else dtype(0)
    ninf = pg._nan_max(np.asarray(one.sum(1)).reshape(-1).astype(dtype)) if full else dtype(0)
    with np.errstate(invalid="ignore", over="ignore"):
        return dtype(np.sqrt(dtype(n1 * ninf)))


def step_of(sigma_est, L_bound, step, dtype):
    """(eta, fell back) by the rule"""
    dtype = np.dtype(dtype).type
    if not L_bound > 0:
        return dtype(step), True
    ok = bool(np.isfinite(sigma_est) and sigma_est > 0 and sigma_est <= L_bound)
    return dtype(dtype(step) / (dtype(sigma_est) if ok else L_bound)), not ok


def solve(A, b, c, max_iters, power_iters=40, ray_eps=-1.0, step=0.9, ruiz=10, pock_chambolle=True, dtype=np.float64, sigma_est=None, **kw):
    """The rule on one instance.  Returns pdhg_rays_oracle.solve's dict, and: norm = [sigma_est (0: void or power_iters = 0),
    L_bound], nus, fallback (eta is the bound's)."""
    dtype = np.dtype(dtype).type
    A = sp.csr_matrix(A, dtype=dtype)
    dr, dc = ps.scaling(A, ruiz, pock_chambolle, dtype)
    L = bound(A, dr, dc, dtype)
    common = dict(step=step, ruiz=ruiz, pock_chambolle=pock_chambolle, ray_eps=ray_eps, dtype=dtype, **kw)
    if not power_iters and sigma_est is None:
        out = pr.solve(A, b, c, max_iters, **common)
        out.update(norm=[dtype(0), L], nus=[], fallback=True)
        return out
    est, nus = power(A, dr, dc, power_iters, dtype)
    if sigma_est is not None:
        est = dtype(sigma_est)
    eta, fallback = step_of(est, L, step, dtype)
    inner = pg.step_size
    pg.step_size = lambda S, s, t: eta if fallback is False else inner(S, s, t)
    try:
        out = pr.solve(A, b, c, max_iters, **common)
    finally:
        pg.step_size = inner
    assert not fallback or out["eta"] == eta, (out["eta"], eta)        # the bound's step is the one pdhg_oracle.step_size forms
    out.update(norm=[est, L], nus=nus, fallback=fallback)
    return out
