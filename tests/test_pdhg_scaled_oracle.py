"""CPU: the numpy oracle of mllp_lp_pdhg_scaled (tests/pdhg_scaled_oracle.py) does what THE RULE of include/mllp_hip.h says --
the scaling equilibrates, the neutral settings are tests/pdhg_oracle.py bit for bit, the weight stays inside its clamp and
moves only at restarts --, the rule delivers what it was built for where that can be checked without a GPU, and the C ABI's
new entry points exist, refuse what they must and report their limits.  The device is held to this oracle by
tests/test_pdhg_scaled.py.
"""
import ctypes

import numpy as np
import pytest

import pdhg_oracle as pg
import pdhg_scaled_oracle as ps
import planted_oracle as po
import test_basis_repair as tb
from mllp_amd import _lib

EPS = 2.0 ** -10
SHAPES = [(5, 12), (40, 100), (193, 400)]
SEEDS = (26, 30, 42)
NEUTRAL = dict(ruiz=0, pock_chambolle=False, primal_weight=False)


@pytest.fixture(scope="module")
def planted():
    """{seed: the three shapes}, planted in fp64 and rounded to fp32"""
    return {seed: pg.cpu_planted(tb.planted_shapes(SHAPES, seed)) for seed in SEEDS}


@pytest.fixture(scope="module")
def long_rows():
    return pg.cpu_planted(po.ragged_case(which=[4]))[0]


# ---- 1. equilibration -----------------------------------------------------------------------------------------------------
def test_ruiz_equilibrates_and_pock_chambolle_bounds_the_sums(planted):
    """Ruiz's iteration halves the logarithm of every row and column maximum per pass (Ruiz 2001: convergence to maxima of 1
    at the asymptotic rate 1/2).  The planted entries lie within [2^-10, 2^10] (asserted), so ten passes leave
    |log2 max| <= 10 * 2^-10 and the maxima within 2^(10/1024) = 1.0068 of 1: the bar is [0.99, 1.01].  After the pass on the
    sums (alpha = 1) what holds is Pock and Chambolle's Lemma 2: the SPECTRAL norm of S is at most 1 (Cauchy-Schwarz over
    s_ij = |a_ij| / sqrt(R_i C_j)), here up to the rounding of the L-term sums and of the products, (L + 4) 2^-24.  The row
    and column sums themselves are NOT bounded by 1 (5 x 12, seed 26: a row sum of 1.76), so eta = step / sqrt(|S|_1 |S|_inf)
    may be below step; it is a safe step because sqrt(|S|_1 |S|_inf) >= |S|_2, which the test also asserts."""
    for inst in planted[SEEDS[0]]:
        A = inst["A"].astype(np.float32)
        assert 2.0 ** -10 <= np.abs(A.data).min() and np.abs(A.data).max() <= 2.0 ** 10
        dr, dc = ps.scaling(A, 10, False, np.float32)
        S = ps.scaled_abs(A.tocsr(), dr, dc)[0].astype(np.float64)
        rmax, cmax = S.max(axis=1).toarray().ravel(), S.max(axis=0).toarray().ravel()
        # (a row or column without entries has no maximum to equilibrate: the rule leaves its factor at 1)
        assert (dr[np.diff(S.indptr) == 0] == 1).all() and (dc[np.diff(S.tocsc().indptr) == 0] == 1).all()
        rmax, cmax = rmax[np.diff(S.indptr) > 0], cmax[np.diff(S.tocsc().indptr) > 0]
        print(inst["m"], inst["n"], "row maxima", rmax.min(), rmax.max(), "column maxima", cmax.min(), cmax.max())
        assert 0.99 <= rmax.min() and rmax.max() <= 1.01 and 0.99 <= cmax.min() and cmax.max() <= 1.01
        dr, dc = ps.scaling(A, 10, True, np.float32)
        S = ps.scaled_abs(A.tocsr(), dr, dc)[0].astype(np.float64)
        slack = 1.0 + (max(np.diff(S.indptr).max(), np.diff(S.tocsc().indptr).max()) + 4) * 2.0 ** -24
        norm2 = np.linalg.svd(S.toarray(), compute_uv=False)[0]
        print(inst["m"], inst["n"], "|S|_2", norm2, "largest row sum", S.sum(axis=1).max(), "largest column sum", S.sum(axis=0).max())
        assert norm2 <= slack
        r = ps.solve(inst["A"], inst["b"], inst["c"], 0, dtype=np.float32)
        assert r["eta"].dtype == np.float32 and r["eta"] * norm2 <= 0.9 * slack
        assert r["eta"] == pytest.approx(0.9 / np.sqrt(S.sum(axis=1).max() * S.sum(axis=0).max()), rel=slack - 1.0)
        assert np.array_equal(r["dr"], dr) and np.array_equal(r["dc"], dc)


# ---- 2. neutral settings ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_neutral_settings_are_the_baseline_oracle_bit_for_bit(planted, dtype):
    for seed in SEEDS[:2]:
        for inst in planted[seed]:
            for kw in (dict(check_every=64), dict(check_every=0), dict(check_every=32, x0=np.linspace(-1, 1, inst["n"]), y0=np.ones(inst["m"]))):
                a = pg.solve(inst["A"], inst["b"], inst["c"], 1024, eps=EPS, dtype=dtype, **kw)
                z = ps.solve(inst["A"], inst["b"], inst["c"], 1024, eps=EPS, dtype=dtype, **NEUTRAL, **kw)
                assert z["x"].dtype == dtype and np.array_equal(a["x"], z["x"]) and np.array_equal(a["y"], z["y"])
                assert a["status"] == z["status"] and a["kkt"] == z["kkt"][:4] and z["kkt"][4:] == [1, 1]
                assert (z["dr"] == 1).all() and (z["dc"] == 1).all() and z["weights"] == []


# ---- 3. the weight ------------------------------------------------------------------------------------------------------------
def test_the_weight_starts_at_one_where_a_norm_is_zero(planted):
    inst = planted[SEEDS[0]][1]
    for b, c in ((np.zeros(inst["m"]), inst["c"]), (inst["b"], np.zeros(inst["n"]))):
        r = ps.solve(inst["A"], b, c, 256, dtype=np.float32)
        assert r["w0"] == 1.0 and r["kkt"][4] == 1.0
    r = ps.solve(inst["A"], inst["b"], inst["c"], 0, dtype=np.float64)
    assert r["w0"] == pytest.approx(np.linalg.norm(r["dc"] * inst["c"]) / np.linalg.norm(r["dr"] * inst["b"]), rel=1e-14)
    assert ps.solve(inst["A"], inst["b"], inst["c"], 0, primal_weight=False)["w0"] == 1.0


def test_the_weight_stays_inside_its_clamp_and_moves_only_at_restarts(planted, long_rows):
    moved = clamped = 0
    for inst in planted[SEEDS[2]] + [long_rows]:
        for span in (16.0, 1.25, 1.0):
            r = ps.solve(inst["A"], inst["b"], inst["c"], 2048, eps=2.0 ** -14, weight_span=span, dtype=np.float32)
            w0, f32 = r["w0"], np.float32
            lo, hi = f32(w0 / f32(span)), f32(w0 * f32(span))
            restarts = [k["it"] for k in r["checks"] if k.get("restart")]
            assert [u["it"] for u in r["weights"]] == restarts[:len(r["weights"])] and len(restarts) == r["status"][2] >= 2
            assert all(lo <= f32(u["w"]) <= hi for u in r["weights"]) and lo <= r["w"] <= hi
            # the weight a check ran under is the one the last restart before it left
            at = {u["it"]: u["w"] for u in r["weights"]}
            w = float(w0)
            for k in r["checks"]:
                assert k["w"] == w, (k["it"], k["w"], w)
                w = at.get(k["it"], w) if k.get("restart") else w
            if span == 1.0:
                assert all(u["w"] == w0 for u in r["weights"]) and r["w"] == w0
            moved += any(u["w"] != w0 for u in r["weights"])
            clamped += any(u["w"] in (lo, hi) and u["raw"] != u["w"] for u in r["weights"])
    assert moved >= 4 and clamped >= 1, (moved, clamped)


# ---- 4. the claim -------------------------------------------------------------------------------------------------------------
def test_the_long_rows_converge_in_half_the_budget_the_baseline_exhausts(long_rows):
    """tests/test_pdhg_oracle.py::test_the_long_rows_make_progress_without_converging: code 6 at 8192 without scaling"""
    r = ps.solve(long_rows["A"], long_rows["b"], long_rows["c"], 4096, eps=EPS, dtype=np.float32)
    print("long rows:", r["status"], r["kkt"])
    assert r["status"][0] == ps.CODE_OPTIMAL and r["status"][1] <= 4096 and r["status"][1] % 64 == 0
    assert max(pg.errors64(long_rows["A"], long_rows["b"], long_rows["c"], r["x"], r["y"])) <= EPS * (1 + 2.0 ** -6)


def test_default_options_need_no_more_iterations_than_the_baseline(planted):
    for seed in SEEDS:
        for inst in planted[seed]:
            a = pg.solve(inst["A"], inst["b"], inst["c"], 8192, eps=EPS, dtype=np.float32)
            r = ps.solve(inst["A"], inst["b"], inst["c"], 8192, eps=EPS, dtype=np.float32)
            print(seed, inst["m"], inst["n"], "baseline", a["status"], "scaled", r["status"])
            assert a["status"][0] == r["status"][0] == 0 and r["status"][1] <= a["status"][1], (seed, inst["m"], a["status"], r["status"])
            assert max(pg.errors64(inst["A"], inst["b"], inst["c"], r["x"], r["y"])) <= EPS * (1 + 2.0 ** -6)
            assert np.array_equal(pg.topm(r["x"], inst["m"]), inst["labels"])


# ---- 5. the C ABI, without a GPU ------------------------------------------------------------------------------------------------
NEW = ("mllp_lp_pdhg_scaled_limits", "mllp_lp_pdhg_scaled_scratch_bytes", "mllp_lp_pdhg_scaled")
ORDER = ("g", "x1", "x2", "x0", "y0", "max_iters", "check_every", "eps", "step", "beta", "ruiz", "pc", "pw", "span", "lds", "x", "y", "dr", "dc",
         "status", "kkt", "scratch", "stream")


def test_the_new_symbols_are_exported_and_bound():
    L = _lib.lib()
    header = open(_lib.HEADER_PATH).read()
    for name in NEW:
        assert name in _lib._PROTOTYPES and hasattr(L, name) and f"int {name}(" in header, name
    assert len(_lib._PROTOTYPES["mllp_lp_pdhg_scaled"][1]) == len(ORDER) == len(_lib._PROTOTYPES["mllp_lp_pdhg"][1]) + 6


def test_null_arguments_are_refused_before_any_hip_call():
    L = _lib.lib()
    z = ctypes.c_void_p(0)
    assert L.mllp_lp_pdhg_scaled(z, z, z, z, z, 10, 64, EPS, 0.9, 0.5, 10, 1, 1, 16.0, 0, z, z, z, z, z, z, z, z) == -1
    assert b"mllp_lp_pdhg_scaled:" in L.mllp_last_error() and b"null" in L.mllp_last_error()
    n = ctypes.c_int64(-7)
    assert L.mllp_lp_pdhg_scaled_scratch_bytes(z, 0, ctypes.byref(n)) == -1 and n.value == -7
    assert b"mllp_lp_pdhg_scaled_scratch_bytes" in L.mllp_last_error()
    assert L.mllp_lp_pdhg_scaled_limits(None) == -1 and b"mllp_lp_pdhg_scaled_limits" in L.mllp_last_error()


def test_every_new_refusal_names_the_call_before_any_hip_call():
    """the checks of the scalar arguments come before the graph is read and before any HIP call, and a refused call
    dereferences no pointer: non-null dummies stand for the graph and the device buffers"""
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = dict(g=p, x1=p, x2=p, x0=None, y0=None, max_iters=10, check_every=64, eps=EPS, step=0.9, beta=0.5, ruiz=10, pc=1, pw=1, span=16.0, lds=0,
              x=p, y=p, dr=None, dc=None, status=p, kkt=None, scratch=None, stream=None)
    nan, inf = float("nan"), float("inf")
    bad = [dict(ruiz=-1), dict(ruiz=65), dict(span=nan), dict(span=inf), dict(span=0.5), dict(span=-2.0), dict(max_iters=-1), dict(check_every=-1),
           dict(lds=-1), dict(eps=nan), dict(step=0.0), dict(step=1.5), dict(beta=1.0), dict(beta=nan)]
    for kw in bad:
        args = dict(ok, **kw)
        assert L.mllp_lp_pdhg_scaled(*[args[k] for k in ORDER]) == -1, kw
        assert b"mllp_lp_pdhg_scaled:" in L.mllp_last_error(), (kw, L.mllp_last_error())
    assert b"weight_span" in L.mllp_last_error() or b"beta" in L.mllp_last_error()
    args = dict(ok, span=0.5)
    assert L.mllp_lp_pdhg_scaled(*[args[k] for k in ORDER]) == -1 and b"weight_span" in L.mllp_last_error()
    args = dict(ok, ruiz=65)
    assert L.mllp_lp_pdhg_scaled(*[args[k] for k in ORDER]) == -1 and b"ruiz_passes" in L.mllp_last_error()


def test_the_limits_answer_without_a_gpu():
    lim = (ctypes.c_int64 * 3)()
    assert _lib.lib().mllp_lp_pdhg_scaled_limits(lim) == 0
    assert list(lim) == [36864, 1024, 64]          # include/mllp_hip.h states all three
    assert 4 * lim[0] + 1024 <= 160 * 1024 and lim[1] % 64 == 0
    from mllp_amd.graph import LPBatch, LPPdhg, LPPdhgScaled, pdhg_limits, pdhg_scaled_limits
    assert pdhg_scaled_limits() == (36864, 1024, 64) and pdhg_scaled_limits()[:2] == pdhg_limits()
    assert hasattr(LPBatch, "pdhg_scaled") and issubclass(LPPdhgScaled, LPPdhg)
