"""The fp64 oracle of the basis-simplex rule (tests/simplex_oracle.py) on planted LPs, whose optimum is the planted basis by
construction (unique, nondegenerate: include/mllp_hip.h, mllp_graph_plant_basis), against a brute force over all bases, and
on hand-made LPs with a known verdict.  The host refusals of mllp_basis_simplex.  No GPU.
"""
import ctypes

import numpy as np
import pytest

import planted_oracle as po
import simplex_oracle as so
from mllp_amd import _lib

EINVAL = -1


def planted(m, n, seed):
    """(A, b, c, labels) of test_basis_repair.planted_shapes([(m, n)], seed), planted by the fp64 rule and rounded to fp32"""
    ptr, idx, val, pivot = po._instance(m, n, 4.0, seed)
    rng = np.random.default_rng(1000 + seed)
    xstar, ystar, slack = ((rng.random(n) + 0.5).astype(np.float32), (rng.random(m) * 2 - 1).astype(np.float32),
                           (rng.random(n) + 0.5).astype(np.float32))
    pl = po.plant(ptr, idx, val, pivot, xstar, ystar, slack, n)
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)    # noqa: E731
    return po.dense(ptr, idx, f32(pl["values"]), m, n), f32(pl["b"]), f32(pl["c"]), pl["labels"]


@pytest.mark.parametrize("seed", range(40, 48))
def test_tiny_planted_against_brute_force(seed):
    """5 x 12, two columns swapped: the oracle ends optimal at the labels, and so does the enumeration of all 792 bases"""
    A, b, c, labels = planted(5, 12, seed)
    start, _ = so.perturbed_start(A, labels, 2, seed)
    assert not np.array_equal(start, labels)
    res = so.run(A, b, c, start, 50)
    assert res["code"] == 0 and res["status"][3] == 5 and len(res["trace"]) == res["status"][1] + res["status"][2] > 0
    assert np.array_equal(res["basis"], labels)
    assert sorted(res["col_of_row"]) == sorted(np.flatnonzero(labels))
    best, cost = so.brute_force(A, b, c)
    assert best == sorted(np.flatnonzero(labels))
    x = np.linalg.solve(A[:, best], b)
    assert abs(cost - c[best] @ x) <= 1e-12 * max(1.0, abs(cost))


@pytest.mark.parametrize("k,seed", [(4, 59), (4, 56), (4, 49), (12, 40), (12, 41)])
def test_planted_40_by_100(k, seed):
    A, b, c, labels = planted(40, 100, seed)
    start, _ = so.perturbed_start(A, labels, k, seed)
    res = so.run(A, b, c, start, 200)
    assert res["code"] == 0 and np.array_equal(res["basis"], labels)
    assert res["status"][1] > 0 and res["status"][2] > 0          # both stages
    # the trace replays: every entering column was nonbasic, every leaving row held the column that left
    cor = so.run(A, b, c, start, 0)["col_of_row"]                 # (max_pivots 0: the start's rows)
    for j, p in res["trace"]:
        assert j not in cor
        cor[p] = j
    assert np.array_equal(cor, res["col_of_row"])


def test_the_limit_stops_on_the_path():
    A, b, c, labels = planted(40, 100, 59)
    start, _ = so.perturbed_start(A, labels, 4, 59)
    full = so.run(A, b, c, start, 200)
    n = len(full["trace"])
    assert n >= 4
    for cap in (0, 3, n - 1):
        res = so.run(A, b, c, start, cap)
        assert res["code"] == 6 and res["trace"] == full["trace"][:cap] and sum(res["status"][1:3]) == cap
    assert so.run(A, b, c, start, n)["code"] == 0                 # (the optimality test needs no pivot)


def test_verdicts_of_hand_made_lps():
    one = lambda *row: np.array([row], np.float64)     # noqa: E731
    # x1 + x2 = -1, x >= 0: primal infeasible
    assert so.run(one(1, 1), [-1.0], [1.0, 1.0], [1, 0], 10)["status"] == [4, 0, 0, 1]
    # min -x1, x1 - x2 = 1 from the basis {x1}: unbounded
    assert so.run(one(1, -1), [1.0], [-1.0, 0.0], [1, 0], 10)["status"] == [5, 0, 0, 1]
    # min -x1 - 2 x2, x1 + x2 + s = 1 from the slack basis: primal feasible, one primal pivot
    res = so.run(one(1, 1, 1), [1.0], [-1.0, -2.0, 0.0], [0, 0, 1], 10)
    assert res["status"] == [0, 0, 1, 1] and res["trace"] == [(1, 0)] and list(res["basis"]) == [0, 1, 0]
    # masks with m - 1 and m + 1 columns; a singular start; no rows
    A = np.array([[1.0, 2.0, 0.0], [1.0, 2.0, 1.0]])
    assert so.run(A, [1, 1], [0, 0, 0], [1, 0, 0], 10)["status"] == [3, 0, 0, 0]
    assert so.run(A, [1, 1], [0, 0, 0], [1, 1, 1], 10)["status"] == [3, 0, 0, 0]
    assert so.run(A, [1, 1], [0, 0, 0], [1, 1, 0], 10)["status"] == [1, 0, 0, 1]
    assert so.run(np.zeros((0, 3)), [], [1.0, 0.0, 2.0], [0, 0, 0], 10)["status"] == [0, 0, 0, 0]
    assert so.run(A, [1, 1], [0, 0, 0], [1, 0, 1], 10, max_m=1)["status"] == [2, 0, 0, 0]


def test_host_refusals():
    """MLLP_EINVAL before the graph is looked at: a null required pointer, a tolerance that is not finite and positive, a
    negative tol, max_pivots or max_m.  (A zeroed block stands in for the graph: it is never reached, and would describe
    an empty batch if it were.)"""
    L = _lib.lib()
    fake = ctypes.create_string_buffer(1 << 16)
    g = ctypes.cast(fake, ctypes.c_void_p)
    buf = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    nul = ctypes.c_void_p(0)
    good = dict(g=g, x1=buf, x2=buf, start=buf, tol=2.0 ** -12, ftol=2.0 ** -10, dtol=2.0 ** -10, ptol=2.0 ** -10, dshift=2.0 ** -4,
                max_pivots=10, max_m=10, basis=buf, col_of_row=nul, trace=nul, status=buf, scratch=nul)
    order = ("g", "x1", "x2", "start", "tol", "ftol", "dtol", "ptol", "dshift", "max_pivots", "max_m", "basis", "col_of_row", "trace",
             "status", "scratch")
    bad = [{k: nul} for k in ("g", "x1", "x2", "start", "basis", "status")]
    bad += [{k: v} for k in ("ftol", "dtol", "ptol", "dshift") for v in (0.0, -1.0, float("nan"), float("inf"))]
    bad += [{"tol": v} for v in (-1.0, float("nan"), float("inf"))] + [{"max_pivots": -1}, {"max_m": -1}]
    for change in bad:
        args = dict(good, **change)
        L.mllp_graph_dims(None, (ctypes.c_int64 * 12)())          # (some other message first)
        assert L.mllp_basis_simplex(*[args[k] for k in order], nul) == EINVAL, change
        assert b"mllp_basis_simplex" in L.mllp_last_error(), change
    n = ctypes.c_int64(7)
    assert L.mllp_basis_simplex_scratch_bytes(None, 1, ctypes.byref(n)) == EINVAL
    assert L.mllp_basis_simplex_scratch_bytes(g, -1, ctypes.byref(n)) == EINVAL
    assert L.mllp_basis_simplex_scratch_bytes(g, 1, None) == EINVAL and n.value == 7
