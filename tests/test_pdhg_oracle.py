"""CPU: the numpy oracle of mllp_lp_pdhg (tests/pdhg_oracle.py) does what THE RULE says, and the C ABI's new entry points
exist, refuse a null argument and report their limits without a GPU.  The device is held to this oracle by tests/test_pdhg.py.
"""
import ctypes

import numpy as np
import pytest

import pdhg_oracle as pg
import planted_oracle as po
import test_basis_repair as tb
from mllp_amd import _lib

EPS = 2.0 ** -10
SHAPES = [(1, 1), (3, 3), (5, 12), (40, 100), (193, 400)]


@pytest.fixture(scope="module")
def planted():
    return pg.cpu_planted(tb.planted_shapes(SHAPES, 20))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_oracle_converges_on_the_planted_shapes(planted, dtype):
    for inst in planted:
        r = pg.solve(inst["A"], inst["b"], inst["c"], 8192, eps=EPS, dtype=dtype)
        code, it, restarts, avg = r["status"]
        assert code == pg.CODE_OPTIMAL and it % 64 == 0 and 64 <= it <= 8192 and restarts >= 0 and avg in (0, 1), (inst["m"], r["status"])
        assert max(pg.errors64(inst["A"], inst["b"], inst["c"], r["x"], r["y"])) <= EPS * (1 + 2.0 ** -6)
        assert max(r["kkt"][:3]) <= EPS and r["x"].dtype == dtype and (r["x"] >= 0).all()
        # the iterate points at the planted vertex: its m largest entries are the planted basis
        assert np.array_equal(pg.topm(r["x"], inst["m"]), inst["labels"]), (inst["m"], inst["n"])
        assert np.abs(r["x"] - inst["xstar"]).max() <= 64 * EPS * (1 + np.abs(inst["xstar"]).max())


def test_fp32_takes_the_decisions_of_fp64_where_the_margin_allows(planted):
    for inst in planted:
        a = pg.solve(inst["A"], inst["b"], inst["c"], 8192, eps=EPS)
        f = pg.solve(inst["A"], inst["b"], inst["c"], 8192, eps=EPS, dtype=np.float32)
        if a["margin"] >= 2.0 ** -7:
            assert a["status"] == f["status"], (inst["m"], a["status"], f["status"])


def test_a_start_at_the_planted_optimum_stops_at_the_first_check(planted):
    for inst in planted:
        r = pg.solve(inst["A"], inst["b"], inst["c"], 8192, eps=EPS, x0=inst["xstar"], y0=inst["ystar"], dtype=np.float32)
        assert r["status"][:2] == [pg.CODE_OPTIMAL, 64], (inst["m"], r["status"])
        assert r["status"][2] == 0 and len(r["checks"]) == 1


def test_a_negative_start_is_clipped(planted):
    inst = planted[2]
    x0 = np.linspace(-1.0, 1.0, inst["n"])
    a = pg.solve(inst["A"], inst["b"], inst["c"], 256, x0=x0)
    b = pg.solve(inst["A"], inst["b"], inst["c"], 256, x0=np.maximum(x0, 0.0))
    assert np.array_equal(a["x"], b["x"]) and np.array_equal(a["y"], b["y"]) and a["status"] == b["status"]
    z = pg.solve(inst["A"], inst["b"], inst["c"], 0, x0=x0)
    assert z["status"] == [pg.CODE_LIMIT, 0, 0, 0] and np.array_equal(z["x"], np.maximum(x0, 0.0))


def test_check_every_zero_never_restarts(planted):
    inst = planted[3]
    r = pg.solve(inst["A"], inst["b"], inst["c"], 300, check_every=0)
    assert r["status"] == [pg.CODE_LIMIT, 300, 0, 0] and r["checks"] == [] and r["margin"] == np.inf
    # ... and is the plain iteration: 300 steps by hand
    A, b, c, eta = inst["A"], inst["b"], inst["c"], r["eta"]
    x, y = np.zeros(inst["n"]), np.zeros(inst["m"])
    for _ in range(300):
        xn = np.maximum(x - eta * (c - A.T @ y), 0.0)
        y = y + eta * (b - A @ (2 * xn - x))
        x = xn
    assert np.abs(r["x"] - x).max() <= 1e-12 and np.abs(r["y"] - y).max() <= 1e-12
    norm1, norminf = np.abs(A.toarray()).sum(0).max(), np.abs(A.toarray()).sum(1).max()
    assert eta == pytest.approx(0.9 / np.sqrt(norm1 * norminf), rel=1e-15)
    # a limit that is no multiple of check_every ends exactly there
    r = pg.solve(inst["A"], inst["b"], inst["c"], 100, check_every=64)
    assert r["status"][:2] == [pg.CODE_LIMIT, 100] and len(r["checks"]) == 1


def test_restart_bookkeeping_on_a_hand_made_lp():
    """min x0 + 2 x1 + 3 x2,  x0 + x1 = 1,  x1 + x2 = 1: the optimum is x = (0, 1, 0) (degenerate), value 2.  Every check's
    record is replayed against the rule: cnt counts from the last restart, the first check restarts (e_last = +inf), a
    restart happens exactly when e <= beta e_last or 25 cnt >= 9 it, and e_last is the last restart's e."""
    A = np.array([[1.0, 1.0, 0.0], [0.0, 1.0, 1.0]])
    b, c = np.array([1.0, 1.0]), np.array([1.0, 2.0, 3.0])
    r = pg.solve(A, b, c, 4000, check_every=8, eps=2.0 ** -16, beta=0.5)
    code, it, restarts, avg = r["status"]
    assert code == pg.CODE_OPTIMAL and np.abs(r["x"] - [0.0, 1.0, 0.0]).max() < 1e-3 and abs(c @ r["x"] - 2.0) < 1e-3
    checks = r["checks"]
    assert [k["it"] for k in checks] == list(range(8, it + 1, 8))
    assert checks[0]["e_last"] == np.inf and checks[0].get("restart") and checks[0]["cnt"] == 8
    last_restart_it, e_last, seen = 0, np.inf, 0
    by_error = by_count = 0
    for k in checks[:-1]:
        e = k["ea"] if k["use_avg"] else k["ec"]
        assert k["use_avg"] == (k["ea"] < k["ec"]) and k["cnt"] == k["it"] - last_restart_it and k["e_last"] == e_last
        want = e <= 0.5 * e_last or 25 * k["cnt"] >= 9 * k["it"]
        assert bool(k.get("restart")) == want, k
        if want:
            by_error += e <= 0.5 * e_last
            by_count += not e <= 0.5 * e_last
            last_restart_it, e_last, seen = k["it"], e, seen + 1
    assert seen == restarts and by_error >= 2, (restarts, by_error, by_count)
    final = checks[-1]
    assert min(final["ea"], final["ec"]) <= 2.0 ** -16 and avg == int(final["use_avg"]) and not final.get("restart")
    # a non-finite error ends the run with code 8 at the first check
    bad = pg.solve(A, np.array([1.0, np.inf]), c, 4000, check_every=8)
    assert bad["status"][:3] == [pg.CODE_NOT_FINITE, 8, 0]


def test_the_long_rows_make_progress_without_converging():
    """the 1200 x 2400 instance with rows and columns of up to 1100 entries: a baseline without preconditioning does not
    reach 2^-10 within 8192 iterations there (code 6), but every error falls by a factor of 4 or more from 2048 to 8192"""
    inst = pg.cpu_planted(po.ragged_case(which=[4]))[0]
    a = pg.solve(inst["A"], inst["b"], inst["c"], 2048, eps=EPS, dtype=np.float32)
    r = pg.solve(inst["A"], inst["b"], inst["c"], 8192, eps=EPS, dtype=np.float32)
    assert a["status"][0] == r["status"][0] == pg.CODE_LIMIT and r["status"][1] == 8192 and r["status"][2] > a["status"][2]
    assert all(4 * late <= early for late, early in zip(r["kkt"][:3], a["kkt"][:3])), (a["kkt"], r["kkt"])


# ---- the C ABI, without a GPU -------------------------------------------------------------------------------------------
NEW = ("mllp_lp_pdhg_limits", "mllp_lp_pdhg_scratch_bytes", "mllp_lp_pdhg")


def test_the_new_symbols_are_exported_and_bound():
    L = _lib.lib()
    header = open(_lib.HEADER_PATH).read()
    for name in NEW:
        assert name in _lib._PROTOTYPES and hasattr(L, name) and f"int {name}(" in header, name
    assert len(_lib._PROTOTYPES["mllp_lp_pdhg"][1]) == 17


def test_null_arguments_are_refused_before_any_hip_call():
    L = _lib.lib()
    z = ctypes.c_void_p(0)
    assert L.mllp_lp_pdhg(z, z, z, z, z, 10, 64, EPS, 0.9, 0.5, 0, z, z, z, z, z, z) == -1
    assert b"mllp_lp_pdhg" in L.mllp_last_error() and b"null" in L.mllp_last_error()
    n = ctypes.c_int64(-7)
    assert L.mllp_lp_pdhg_scratch_bytes(z, 0, ctypes.byref(n)) == -1 and n.value == -7
    assert L.mllp_lp_pdhg_limits(None) == -1


def test_the_limits_answer_without_a_gpu():
    lim = (ctypes.c_int64 * 2)()
    assert _lib.lib().mllp_lp_pdhg_limits(lim) == 0
    assert lim[0] == 36864 and lim[1] == 1024          # include/mllp_hip.h states both
    assert 4 * lim[0] + 1024 <= 160 * 1024 and lim[1] % 64 == 0
    from mllp_amd.graph import LPBatch, LPPdhg, pdhg_limits
    assert pdhg_limits() == (36864, 1024) and hasattr(LPBatch, "pdhg") and hasattr(LPBatch, "pdhg_basis") and LPPdhg
