"""The fp64 oracle of the guarded basis-simplex rule (tests/simplex_guarded_oracle.py): it is simplex_oracle.run with both
guards off, it ends the two textbook cycling LPs at their optimum where the plain rule cycles, and on a degenerate family it
supplies the cases the device tests need (tests/test_simplex_guarded.py).  The host refusals of mllp_basis_simplex_guarded.
No GPU.

The recorded statuses, guards and traces of Chvatal's and Beale's LPs were found by an independent fp64 prototype of the
rule stated in include/mllp_hip.h; the row numbers are those the start's factorization assigns.
"""
import ctypes

import numpy as np
import pytest

import simplex_guarded_oracle as sg
import simplex_oracle as so
from mllp_amd import _lib
from test_simplex_oracle import planted

EINVAL = -1
TEXTBOOK = {"chvatal": sg.CHVATAL, "beale": sg.BEALE}
# guarded seeds of the family (found by scanning the oracle; any seed that meets the condition would do), per (R, S):
# with at least one Bland pivot in stage P (and a refactorization where R > 0) / with pivots and no Bland pivot
BLAND_P = {(3, 1): (6, 51, 52, 68, 69, 99, 114, 124), (0, 2): (68, 69, 114, 442, 601, 774, 815, 889)}
NO_BLAND = {(3, 1): (3, 11, 16, 24), (0, 2): (3, 6, 11, 16)}
STAGE_D = ((120, 3, 2), (25, 3, 1), (44, 3, 1), (130, 3, 1))      # (seed, R, S): the oracle's run takes a Bland pivot in stage D


def _lp(d):
    return d["A"], d["b"], d["c"], d["start"]


# ---------------------------------------------------------------------------------------------------
# both guards off: simplex_oracle.run
# ---------------------------------------------------------------------------------------------------
def _same(got, want):
    assert got["status"] == want["status"] and got["trace"] == want["trace"]
    assert np.array_equal(got["col_of_row"], want["col_of_row"]) and np.array_equal(got["basis"], want["basis"])
    assert got["guard"] == [0, 0]


@pytest.mark.parametrize("m,n,k,seed,cap", [(5, 12, 2, s, 50) for s in range(40, 48)]
                         + [(40, 100, k, s, c) for k, s in ((4, 59), (4, 56), (4, 49), (12, 40), (12, 41)) for c in (200, 3)])
def test_guards_off_is_the_plain_oracle_on_planted_lps(m, n, k, seed, cap):
    A, b, c, labels = planted(m, n, seed)
    start, _ = so.perturbed_start(A, labels, k, seed)
    _same(sg.run(A, b, c, start, cap), so.run(A, b, c, start, cap))


def test_guards_off_is_the_plain_oracle_on_hand_made_lps():
    one = lambda *row: np.array([row], np.float64)     # noqa: E731
    A = np.array([[1.0, 2.0, 0.0], [1.0, 2.0, 1.0]])
    cases = [(one(1, 1), [-1.0], [1.0, 1.0], [1, 0]), (one(1, -1), [1.0], [-1.0, 0.0], [1, 0]),
             (one(1, 1, 1), [1.0], [-1.0, -2.0, 0.0], [0, 0, 1]), (A, [1, 1], [0, 0, 0], [1, 0, 0]), (A, [1, 1], [0, 0, 0], [1, 1, 1]),
             (A, [1, 1], [0, 0, 0], [1, 1, 0]), (np.zeros((0, 3)), [], [1.0, 0.0, 2.0], [0, 0, 0])]
    for lp in cases:
        _same(sg.run(*lp, 10), so.run(*lp, 10))
    assert sg.run(A, [1, 1], [0, 0, 0], [1, 0, 1], 10, 3, 2, max_m=1)["status"] == [2, 0, 0, 0]
    for name, lp in TEXTBOOK.items():
        _same(sg.run(*_lp(lp), 60), so.run(*_lp(lp), 60))


# ---------------------------------------------------------------------------------------------------
# Chvatal's and Beale's cycling examples
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TEXTBOOK)
def test_the_plain_rule_cycles_and_the_guarded_rule_ends(name):
    lp = TEXTBOOK[name]
    plain = so.run(*_lp(lp), 60)
    assert plain["status"] == [6, 0, 60, 3]
    assert plain["trace"] == [(0, 0), (1, 1), (2, 0), (3, 1), (4, 0), (5, 1)] * 10      # the six-pivot cycle, ten times
    best, cost = so.brute_force(lp["A"], lp["b"], lp["c"])
    assert best == [0, 2, 4] and cost == lp["objective"]
    res = sg.run(*_lp(lp), 60, 0, 3)
    assert res["code"] == 0 and sorted(np.flatnonzero(res["basis"])) == best
    x = np.linalg.solve(np.asarray(lp["A"], float)[:, best], lp["b"])
    assert np.asarray(lp["c"], float)[best] @ x == lp["objective"]


RECORDED = [("chvatal", 0, 3, [0, 0, 7, 3], [0, 4], [(0, 0), (1, 1), (2, 0), (3, 1), (4, 0), (0, 1), (2, 2)]),
            ("chvatal", 0, 1, [0, 0, 7, 3], [0, 6], [(0, 0), (1, 1), (2, 0), (3, 1), (4, 0), (0, 1), (2, 2)]),
            ("chvatal", 1, 3, [0, 0, 4, 3], [4, 1], [(0, 0), (1, 1), (2, 0), (4, 1)]),
            ("beale", 0, 3, [0, 0, 6, 3], [0, 2], [(0, 0), (1, 1), (2, 0), (3, 1), (0, 2), (4, 1)]),
            ("beale", 1, 3, [0, 0, 5, 3], [5, 1], None)]


@pytest.mark.parametrize("name,R,S,status,guard,trace", RECORDED)
def test_recorded_runs_of_the_prototype(name, R, S, status, guard, trace):
    res = sg.run(*_lp(TEXTBOOK[name]), 60, R, S)
    assert res["status"] == status and res["guard"] == guard
    assert trace is None or res["trace"] == trace
    assert sorted(np.flatnonzero(res["basis"])) == [0, 2, 4]


# ---------------------------------------------------------------------------------------------------
# the degenerate family
# ---------------------------------------------------------------------------------------------------
def test_the_family_ends_optimal_with_both_guards():
    """every usable seed below 400 ends with code 0 under (R, S) = (3, 2); seed 120 takes one Bland pivot in stage D"""
    usable = 0
    for seed in range(400):
        f = sg.family(seed)
        if f is None:
            continue
        usable += 1
        res = sg.run(*f, 200, 3, 2)
        assert res["code"] == 0, (seed, res["status"])
        if seed == 120:
            assert res["status"] == [0, 5, 0, 6] and res["guard"] == [1, 1] and res["bland"] == [1, 0] and not sg.guarded(res)
    assert usable == 398


@pytest.mark.parametrize("R,S", list(BLAND_P))
def test_the_guarded_seeds_the_device_tests_use(R, S):
    """at least 8 guarded seeds with a stage-P Bland pivot (and a refactorization where R > 0), at least 4 with none"""
    assert len(set(BLAND_P[R, S])) >= 8 and len(set(NO_BLAND[R, S])) >= 4
    for seed in BLAND_P[R, S] + NO_BLAND[R, S]:
        res = sg.run(*sg.family(seed), 200, R, S)
        assert sg.guarded(res), (seed, min(res["margins"], key=lambda t: t[1]))
        assert res["code"] == 0 and len(res["trace"]) > 0
        assert res["guard"][0] == len(res["trace"]) // R if R else res["guard"][0] == 0
        if seed in BLAND_P[R, S]:
            assert res["bland"][1] > 0 and res["bland"][0] == 0 and (R == 0 or res["guard"][0] > 0)
        else:
            assert res["guard"][1] == 0
        # the optimum is the brute force's (the bases may differ at a degenerate vertex: the cost may not)
        A, b, c, _ = sg.family(seed)
        cols = np.flatnonzero(res["basis"])
        assert abs(c[cols] @ np.linalg.solve(A[:, cols], b) - so.brute_force(A, b, c)[1]) <= 1e-9


@pytest.mark.parametrize("seed,R,S", STAGE_D)
def test_seeds_with_a_bland_pivot_in_stage_d(seed, R, S):
    res = sg.run(*sg.family(seed), 200, R, S)
    assert res["code"] == 0 and res["bland"][0] > 0


def test_a_basis_that_cannot_be_refactorized():
    """tol = 0.5 rejects columns the start's order accepted: code 7, the basis kept, no row owners, the trace kept"""
    f = sg.family(6)
    res = sg.run(*f, 200, 1, 0, tol=0.5)
    assert res["status"] == [7, 2, 0, 6] and res["guard"] == [1, 0]
    assert len(res["trace"]) == 2 and res["basis"].sum() == 6 and (res["col_of_row"] == -1).all()
    assert sg.run(*f, 200, 0, 0, tol=0.5)["code"] != 7          # (without refactorizations the same run goes on)


# ---------------------------------------------------------------------------------------------------
# host refusals
# ---------------------------------------------------------------------------------------------------
def test_host_refusals():
    """what mllp_basis_simplex refuses, and a negative refactor_every or stall_pivots: MLLP_EINVAL before the graph is looked
    at (a zeroed block stands in for it, as in tests/test_simplex_oracle.py)"""
    L = _lib.lib()
    fake = ctypes.create_string_buffer(1 << 16)
    g = ctypes.cast(fake, ctypes.c_void_p)
    buf = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    nul = ctypes.c_void_p(0)
    good = dict(g=g, x1=buf, x2=buf, start=buf, tol=2.0 ** -12, ftol=2.0 ** -10, dtol=2.0 ** -10, ptol=2.0 ** -10, dshift=2.0 ** -4,
                max_pivots=10, max_m=10, refactor=3, stall=2, basis=buf, col_of_row=nul, trace=nul, status=buf, guard=nul, scratch=nul)
    order = ("g", "x1", "x2", "start", "tol", "ftol", "dtol", "ptol", "dshift", "max_pivots", "max_m", "refactor", "stall", "basis",
             "col_of_row", "trace", "status", "guard", "scratch")
    bad = [{k: nul} for k in ("g", "x1", "x2", "start", "basis", "status")]
    bad += [{k: v} for k in ("ftol", "dtol", "ptol", "dshift") for v in (0.0, -1.0, float("nan"), float("inf"))]
    bad += [{"tol": v} for v in (-1.0, float("nan"), float("inf"))] + [{"max_pivots": -1}, {"max_m": -1}, {"refactor": -1}, {"stall": -1}]
    for change in bad:
        args = dict(good, **change)
        L.mllp_graph_dims(None, (ctypes.c_int64 * 12)())          # (some other message first)
        assert L.mllp_basis_simplex_guarded(*[args[k] for k in order], nul) == EINVAL, change
        assert b"mllp_basis_simplex_guarded" in L.mllp_last_error(), change
