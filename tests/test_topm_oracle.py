"""The oracle of the soft top-m loss head against what it claims to state (CPU, no library): the literal Sinkhorn iteration
the closed form replaces, central differences of its own loss, the noise, the degenerate instances."""
import numpy as np
import pytest

import topm_oracle as to


def _case(n, m, seed, scale=1.0, labels="m"):
    rng = np.random.default_rng(seed)
    z = (scale * rng.standard_normal(n)).astype(np.float32).astype(np.float64)
    y = np.zeros(n)
    k = m if labels == "m" else max(1, m // 2)
    y[rng.permutation(n)[:k]] = 1.0
    return z, y


@pytest.mark.parametrize("n,m,tau_s", [(12, 5, 1.0), (100, 40, 1.0), (120, 50, 0.05)])
def test_sinkhorn_converges_to_the_closed_form(n, m, tau_s):
    """3000 log-domain Sinkhorn iterations on the 2 x n problem against p = sigmoid(z / tau + nu), tau = sinkhorn_tau / 2"""
    z, y = _case(n, m, 10 + n, scale=1.0 if tau_s == 1.0 else 0.1)
    p = to.evaluate(z / (tau_s / 2.0), y, m)["p"]
    s = to.sinkhorn_topk(z, m, tau_s, 3000)
    assert abs(p.sum() - m) < 1e-9 and abs(s.sum() - m) < 1e-9
    assert np.abs(s - p).max() < 1e-9, np.abs(s - p).max()


def _central(f, x, h=1e-5):
    g = np.zeros(len(x))
    for i in range(len(x)):
        e = np.zeros(len(x))
        e[i] = h
        g[i] = (f(x + e) - f(x - e)) / (2.0 * h)
    return g


@pytest.mark.parametrize("what", ["balanced", "unbalanced", "noisy"])
def test_central_differences_agree_with_dz(what):
    n, m, tau, w = 40, 15, 0.5, 1.3
    if what == "balanced":
        z, y = _case(n, m, 3)
        r = to.instance(z, y, m, tau, w=w)
        num = w * _central(lambda x: to.loss_of(x / tau, y, m), z)
        assert abs(to.evaluate(z / tau, y, m)["G"]) > 0      # (G is not zero even here; the q G / Q term is what keeps sum dz = 0)
    elif what == "unbalanced":
        z, y = _case(n, m, 4, labels="half")
        assert y.sum() != m
        r = to.instance(z, y, m, tau, pw=1.7, w=w)
        ev = to.evaluate(z / tau, y, m, 1.7)
        assert abs(ev["G"]) * ev["q"].max() / ev["Q"] > 1e-3 * np.abs(ev["g"]).max()      # the q G / Q term matters here
        num = w * _central(lambda x: to.loss_of(x / tau, y, m, 1.7), z)
    else:
        z, y = _case(n, m, 5)
        S, sigma, seed, iid = 3, 0.5, 11, 7
        r = to.instance(z, y, m, tau, sigma, S, seed, iid, w=w)
        eps = [to.gumbel(seed, iid, n, s) for s in range(S)]
        num = w * _central(lambda x: sum(to.loss_of((x + sigma * e) / tau, y, m) for e in eps) / S, z)
    assert np.abs(num - r["dz"]).max() < 1e-8 * max(1.0, np.abs(num).max()), np.abs(num - r["dz"]).max()
    assert abs(r["dz"].sum()) < 1e-12           # a shift of every logit changes nothing: the head sees differences only


def test_noise_is_in_the_open_interval_and_differs_by_instance():
    n = 5000
    for seed, iid, s in [(0, 0, 0), (1, 3, 2), (0xFFFFFFFF, 2 ** 31 - 1, 9)]:
        t = to.uniforms(seed, iid, n, s)
        assert (t > 0).all() and (t < 1).all() and np.isfinite(to.gumbel(seed, iid, n, s)).all()
        assert np.array_equal(t.astype(np.float32).astype(np.float64), t)            # exact in fp32
        want = [((to.hash_word(seed, iid, i, s) >> 9) + 0.5) * 2.0 ** -23 for i in range(0, n, 97)]
        assert np.array_equal(t[::97], want)                                         # the vectorised hash is the integer one
    assert ((0 + 0.5) * 2.0 ** -23 > 0) and ((2 ** 23 - 1 + 0.5) * 2.0 ** -23 < 1)    # the extremes of t
    a, b = to.uniforms(5, 0, n, 0), to.uniforms(5, 1, n, 0)
    assert (a != b).mean() > 0.99
    assert (to.uniforms(5, 0, n, 1) != a).mean() > 0.99 and (to.uniforms(6, 0, n, 0) != a).mean() > 0.99
    assert abs(a.mean() - 0.5) < 0.02 and abs(to.gumbel(5, 0, n, 0).mean() - 0.5772) < 0.06


def test_degenerate_instances():
    z, y = _case(7, 3, 1)
    for m, p in ((0, 0.0), (7, 1.0), (9, 1.0)):
        r = to.instance(z, y, m, n_samples=2, sigma=0.5)
        assert r["degenerate"] and r["L"] == 0.0 and not r["dz"].any() and (r["p"] == p).all() and r["nu"] == 0.0
    res, loss, bound, ptr = to.batch(np.concatenate([z, z]), np.concatenate([y, y]), [7, 7], [0, 3], iw=[2.0, 0.5])
    assert res[0]["degenerate"] and not res[1]["degenerate"] and loss == 0.5 * res[1]["L"] and list(ptr) == [0, 7, 14]


def test_the_bound_is_small_where_the_problem_is_well_posed():
    """Q of the shapes the issue names, and a bound on L below 1e-4 L (what the GPU parity cases assert before they compare)"""
    for n, m in [(12, 5), (100, 40), (2400, 1200)]:
        z, y = _case(n, m, n)
        r = to.instance(z, y, m)
        assert r["Q"] >= 1.0 and r["bound"]["L"] < 1e-4 * r["L"], (n, r["Q"], r["bound"]["L"], r["L"])
