"""fp64 numpy statement of the soft top-m loss head (include/mllp_hip.h: mllp_topm_loss), the hash behind its noise in
integer arithmetic, and the ingredients of the error bound of a device evaluation.  Test infrastructure: no GPU, no library,
no code shared with it.

THE RULE, per instance with n columns, target count m, pos_weight pw, instance weight w; one evaluation with a_i given:
    nu   : root of F(nu) = sum_i sigmoid(a_i + nu) - m, by bisection on [logit(m/n) - max a, logit(m/n) - min a] until the
           bracket no longer shrinks in fp64
    u = a + nu, p = sigmoid(u), q = p (1 - p), Q = sum q
    l = (1 - y) u + (1 + (pw - 1) y) softplus(-u),  L = mean l
    g = ((1 - y) - (1 + (pw - 1) y)(1 - p)) / n,  G = sum g,  dz = (w / tau)(g - q G / Q)

ERROR BOUND of a device evaluation (`eval_bounds`), to first order, in the manner of planted_oracle.row_bound.  A device sum
of n terms follows ordered_sum.h with 1024 lanes: a term passes through at most ceil(n / 1024) additions in its lane, six in
the butterfly and four in the tree over the wavefronts, so the sum is within sum_bound(n, sum |terms|) = row_bound(depth,
sum |terms|), depth = min(n, ceil(n / 1024) + 10), of the exact sum of the terms it was given (row_bound(n, .) itself, which
holds for ANY order, passes 1e-4 relative from n = 1675 on its own); u = 2^-24 per rounding; K_ULP is
the ulp error of the device's expf / log1pf / logf (measured: tests/test_topm_loss.py::test_device_math_within_k_ulp), so
one call is within 2 K_ULP u relative.
    da_i   error of a_i: u |a_i| without noise; with noise the two logs and the three roundings of (z + sigma eps) / tau
    EPS_P  relative error of sigmoid from an exact argument: exp (2 K u), 1 + e (u), the quotient (u), both branches: (4 K + 2) u
    E_F    = sum_bound(n, sum p) + sum_i [q_i (da_i + u |u_i|) + EPS_P p_i]
    E_nu   = E_F / Q + ulp32(nu) + 2^-25      (the last Newton step of at most 2^-12 leaves step^2 / 2, since |F''| <= Q)
    E_u    = E_nu + da + u |u|
    E_p    = q E_u + EPS_P p
    E_l    = |n g| E_u + u [2 (1 - y) |u| + (4 K + 4) c softplus(-u) + |l|],  c = 1 + (pw - 1) y
    E_L    = (sum E_l + sum_bound(n, sum |l|)) / n + u |L|
    E_g'   = c q E_u + c (1 - p)(EPS_P + 3 u) + u |g'|,  g' = n g;   E_G' = sum E_g' + sum_bound(n, sum |g'|)
    E_q    = |1 - 2 p| q E_u + q (2 EPS_P + u);                      E_Q  = sum E_q + sum_bound(n, Q)
    E_r    = E_G' / Q + |G'| E_Q / Q^2 + u |r|,  r = G' / Q
    E_dz   = |wt| (E_g' + q E_r + |r| E_q) + 4 u |wt| (|g'| + |q r|),  wt = w / (tau n)
A mean over S samples adds (S + 1) u times the mean of the absolute terms to the mean of the samples' bounds.
"""
import numpy as np

from planted_oracle import U, row_bound

K_ULP = 2.0            # measured on gfx950: expf 0.82, log1pf 0.56, logf 1.87 ulp on the grids of the test -> 2
M32 = 0xFFFFFFFF
NEWTON_REST = 2.0 ** -25


# ---- the hash, in Python integers ------------------------------------------------------------------------------------------
def mix(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def hash_word(seed, inst_id, i, s):
    base = mix((seed & M32) ^ ((inst_id * 0x9E3779B9) & M32))
    return mix((mix((base + i) & M32) + ((s * 0x85EBCA6B) & M32)) & M32)


def uniforms(seed, inst_id, n, s):
    """t_i in (0, 1) for the n local columns of one instance in sample s (the same integers as hash_word, vectorised in
    uint64 with every product masked to 32 bits; tests/test_topm_oracle.py holds the two to each other)"""
    M = np.uint64(M32)
    base = np.uint64(mix((seed & M32) ^ ((inst_id * 0x9E3779B9) & M32)))
    i = np.arange(n, dtype=np.uint64)

    def mx(x):
        x = x & M
        x = x ^ (x >> np.uint64(16))
        x = (x * np.uint64(0x7FEB352D)) & M
        x = x ^ (x >> np.uint64(15))
        x = (x * np.uint64(0x846CA68B)) & M
        return x ^ (x >> np.uint64(16))
    h = mx((mx((base + i) & M) + np.uint64((s * 0x85EBCA6B) & M32)) & M)
    return ((h >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def gumbel(seed, inst_id, n, s):
    return -np.log(-np.log(uniforms(seed, inst_id, n, s)))


# ---- the rule ----------------------------------------------------------------------------------------------------------------
def sigmoid(u):
    e = np.exp(-np.abs(u))
    return np.where(u >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def softplus_neg(u):
    return np.maximum(-u, 0.0) + np.log1p(np.exp(-np.abs(u)))


def solve_nu(a, m):
    n = len(a)
    c0 = np.log(m / (n - m))
    lo, hi = c0 - a.max(), c0 - a.min()
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if not (lo < mid < hi):
            break
        if sigmoid(a + mid).sum() - m < 0:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def evaluate(a, y, m, pw=1.0, w=1.0, tau=1.0):
    """one evaluation of the head on given a (fp64).  0 < m < n."""
    a, y = np.asarray(a, np.float64), np.asarray(y, np.float64)
    n = len(a)
    assert 0 < m < n
    nu = solve_nu(a, m)
    u = a + nu
    p, pm = sigmoid(u), sigmoid(-u)
    q = p * pm
    c = 1.0 + (pw - 1.0) * y
    sp = softplus_neg(u)
    l = (1.0 - y) * u + c * sp
    g = ((1.0 - y) - c * pm) / n
    Q, G = q.sum(), g.sum()
    dz = (w / tau) * (g - q * G / Q)
    return dict(nu=nu, u=u, p=p, pm=pm, q=q, Q=Q, l=l, L=l.mean(), g=g, G=G, dz=dz, c=c, sp=sp, resid=p.sum() - m, a=a, y=y,
                n=n, m=m, w=w, tau=tau)


def loss_of(a, y, m, pw=1.0):
    """L alone (for central differences)"""
    return evaluate(a, y, m, pw)["L"]


def scaled(z, tau, sigma=0.0, eps=None):
    """a and the bound da of its device evaluation, from fp32-valued z (fp64 arithmetic)"""
    z = np.asarray(z, np.float64)
    if eps is None:
        a = z / tau
        return a, U * np.abs(a)
    a = (z + sigma * eps) / tau
    da = (sigma * 2.0 * K_ULP * U * (1.0 + np.abs(eps)) + U * sigma * np.abs(eps) + U * np.abs(z + sigma * eps)) / tau + U * np.abs(a)
    return a, da


def sum_bound(n, abs_terms):
    """a device sum of n terms in ordered_sum.h's order over 1024 lanes (module docstring)"""
    return row_bound(min(n, -(-n // 1024) + 10), abs_terms)


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def eval_bounds(ev, da):
    """the bounds of the module docstring for one evaluation `ev` whose a_i the device knows within da_i"""
    n, u, p, pm, q, Q, y, c = ev["n"], ev["u"], ev["p"], ev["pm"], ev["q"], ev["Q"], ev["y"], ev["c"]
    eps_p = (4.0 * K_ULP + 2.0) * U
    E_F = sum_bound(n, p.sum()) + (q * (da + U * np.abs(u)) + eps_p * p).sum()
    E_nu = E_F / Q + ulp32(ev["nu"]) + NEWTON_REST
    E_u = E_nu + da + U * np.abs(u)
    E_p = q * E_u + eps_p * p
    gp = n * ev["g"]
    E_l = np.abs(gp) * E_u + U * (2.0 * (1.0 - y) * np.abs(u) + (4.0 * K_ULP + 4.0) * c * ev["sp"] + np.abs(ev["l"]))
    E_L = (E_l.sum() + sum_bound(n, np.abs(ev["l"]).sum())) / n + U * abs(ev["L"])
    E_g = c * q * E_u + c * pm * (eps_p + 3.0 * U) + U * np.abs(gp)
    E_G = E_g.sum() + sum_bound(n, np.abs(gp).sum())
    E_q = np.abs(1.0 - 2.0 * p) * q * E_u + q * (2.0 * eps_p + U)
    E_Q = E_q.sum() + sum_bound(n, Q)
    Gp = gp.sum()
    r = Gp / Q
    E_r = E_G / Q + abs(Gp) * E_Q / Q ** 2 + U * abs(r)
    wt = abs(ev["w"] / (ev["tau"] * n))
    E_dz = wt * (E_g + q * E_r + abs(r) * E_q) + 4.0 * U * wt * (np.abs(gp) + np.abs(q * r))
    return dict(F=E_F, nu=E_nu, p=E_p, L=E_L, dz=E_dz, Q=E_Q, resid=E_F + Q * E_nu)


def instance(z, y, m, tau=1.0, sigma=0.0, n_samples=0, seed=0, inst_id=0, pw=1.0, w=1.0):
    """the head on one instance: dict(L, dz, p, nu, Q, resid) and `bound` with the same keys (a device evaluation's)"""
    z, y = np.asarray(z, np.float64), np.asarray(y, np.float64)
    n = len(z)
    if m <= 0 or m >= n:
        zero = np.zeros(n)
        return dict(L=0.0, dz=zero, p=np.full(n, 1.0 if m > 0 else 0.0), nu=0.0, Q=0.0, resid=float(n - m) if m > 0 else 0.0,
                    degenerate=True, bound=dict(L=0.0, dz=zero, p=zero, nu=0.0, Q=0.0, resid=0.0))
    a0, da0 = scaled(z, tau)
    free = evaluate(a0, y, m, pw, w, tau)
    fb = eval_bounds(free, da0)
    out = dict(p=free["p"], nu=free["nu"], Q=free["Q"], resid=free["resid"], degenerate=False, free=free)
    bound = dict(p=fb["p"], nu=fb["nu"], Q=fb["Q"], resid=fb["resid"])
    if n_samples == 0:
        out.update(L=free["L"], dz=free["dz"])
        bound.update(L=fb["L"], dz=fb["dz"])
    else:
        evs, bs = [], []
        for s in range(n_samples):
            a, da = scaled(z, tau, sigma, gumbel(seed, inst_id, n, s))
            evs.append(evaluate(a, y, m, pw, w, tau))
            bs.append(eval_bounds(evs[-1], da))
        S = float(n_samples)
        out.update(L=sum(e["L"] for e in evs) / S, dz=sum(e["dz"] for e in evs) / S, samples=evs)
        bound.update(L=sum(b["L"] for b in bs) / S + (S + 1.0) * U * sum(abs(e["L"]) for e in evs) / S,
                     dz=sum(b["dz"] for b in bs) / S + (S + 1.0) * U * sum(np.abs(e["dz"]) for e in evs) / S)
    out["bound"] = bound
    return out


def batch(z, y, seg_n, seg_m, tau=1.0, sigma=0.0, n_samples=0, seed=0, inst_id=None, iw=None, pw=None):
    """the head on a ragged batch: list of `instance` results, loss = sum_k w_k L_k and its bound"""
    ptr = np.concatenate([[0], np.cumsum(seg_n)]).astype(np.int64)
    K = len(seg_n)
    iw = np.ones(K) if iw is None else np.asarray(iw, np.float64)
    pw = np.ones(K) if pw is None else np.asarray(pw, np.float64)
    ids = np.arange(K) if inst_id is None else np.asarray(inst_id)
    res = [instance(z[ptr[k]:ptr[k + 1]], y[ptr[k]:ptr[k + 1]], int(seg_m[k]), tau, sigma, n_samples, seed, int(ids[k]), float(pw[k]),
                    float(iw[k])) for k in range(K)]
    terms = np.array([iw[k] * res[k]["L"] for k in range(K)])
    loss = terms.sum()
    loss_bound = sum(abs(iw[k]) * res[k]["bound"]["L"] for k in range(K)) + row_bound(K, np.abs(terms).sum())
    return res, loss, loss_bound, ptr


# ---- the literal iteration the closed form replaces -------------------------------------------------------------------------
def sinkhorn_topk(z, m, sinkhorn_tau, iters):
    """log-domain Sinkhorn on the 2 x n problem: row masses (n - m, m), column masses 1, costs |z - min z|, |max z - z|,
    unnormalised, temperature sinkhorn_tau.  Returns the second row of the plan (the probability of being selected)."""
    z = np.asarray(z, np.float64)
    n = len(z)
    la = -np.stack([z - z.min(), z.max() - z]) / sinkhorn_tau
    mass = np.log(np.array([n - m, m], np.float64))[:, None]

    def lse(x, axis):
        mx = x.max(axis=axis, keepdims=True)
        return mx + np.log(np.exp(x - mx).sum(axis=axis, keepdims=True))
    for _ in range(iters):
        la = la + mass - lse(la, 1)
        la = la - lse(la, 0)
    return np.exp(la[1])
