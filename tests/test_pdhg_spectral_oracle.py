"""CPU: the numpy oracle of mllp_lp_pdhg_spectral (tests/pdhg_spectral_oracle.py) does what THE RULE of include/mllp_hip.h
says -- with power_iters = 0 it is pdhg_halpern_oracle.solve, the estimate lies just below the 2-norm of the scaled matrix that a
dense fp64 SVD gives, the hash start survives a matrix that annihilates the constant vector, a void estimate and one above the
bound fall back to the bound's step -- and the rule delivers what it was built for where that can be checked without a GPU:
fewer iterations on the long-row instance and on six small Netlib instances than the counts tests/test_pdhg_halpern_oracle.py
pins.  The device is held to this oracle by tests/test_pdhg_spectral.py.

COUNTS (iterations to code 0 at eps 2^-10, power_iters 0 -> 40; the same in fp32 and fp64):
  long rows 2176 -> 448;  afiro 704 -> 448, sc50a 832 -> 640, sc50b 832 -> 704, blend 1792 -> 1600, adlittle 2816 -> 1408,
  stocfor1 1472 -> 1216;
  planted, seed 27: 5 x 12 192 -> 192, 40 x 100 448 -> 448, 193 x 400 512 -> 256;  seed 22: 192 -> 128, 384 -> 320, 384 -> 256;
  seed 43: 192 -> 320, 192 -> 256, 384 -> 320 -- seed 43's two small shapes are SLOWER under the longer step.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import pdhg_halpern_oracle as ph
import pdhg_oracle as pg
import pdhg_scaled_oracle as ps
import pdhg_spectral_oracle as so
import planted_oracle as po
import test_basis_repair as tb

EPS = 2.0 ** -10
SHAPES = [(5, 12), (40, 100), (193, 400)]
SEEDS = (27, 22, 43)
NETLIB = {"afiro": (704, 448), "sc50a": (832, 640), "sc50b": (832, 704), "blend": (1792, 1600), "adlittle": (2816, 1408), "stocfor1": (1472, 1216)}
PLANTED = {27: ((192, 192), (448, 448), (512, 256)), 22: ((192, 128), (384, 320), (384, 256)), 43: ((192, 320), (192, 256), (384, 320))}
DTYPES = [np.float64, np.float32]


@pytest.fixture(scope="module")
def planted():
    return {seed: pg.cpu_planted(tb.planted_shapes(SHAPES, seed)) for seed in SEEDS}


@pytest.fixture(scope="module")
def long_rows():
    return pg.cpu_planted(po.ragged_case(which=[4]))[0]


def _netlib(names):
    from mllp_amd.data import load_packed
    return [dict(name=i.name, A=sp.csr_matrix((i.values, i.indices, i.indptr), shape=(i.m, i.n)), b=i.rhs, c=i.coefs) for i in load_packed(list(names))]


def _same(a, z):
    assert a["status"] == z["status"] and a["kkt"] == z["kkt"] and a["margin"] == z["margin"] and a["checks"] == z["checks"]
    for k in ("x", "y", "dr", "dc"):
        assert a[k].dtype == z[k].dtype and np.array_equal(a[k], z[k]), k


# ---- 1. power_iters = 0 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_without_rounds_it_is_the_halpern_oracle(planted, dtype):
    for inst in planted[SEEDS[0]] + planted[SEEDS[2]][:1]:
        for kw in (dict(), dict(x0=np.linspace(-1, 1, inst["n"]), y0=np.ones(inst["m"])), dict(primal_weight=False, ruiz=2, pock_chambolle=False)):
            a = ph.solve(inst["A"], inst["b"], inst["c"], 512, eps=EPS, dtype=dtype, **kw)
            z = so.solve(inst["A"], inst["b"], inst["c"], 512, power_iters=0, eps=EPS, dtype=dtype, **kw)
            _same(a, z)
            assert z["norm"][0] == 0 and z["fallback"] and z["norm"][1].dtype == dtype
            assert dtype(0.9) / z["norm"][1] == a["eta"]         # the bound is the value from which that eta follows


# ---- 2. the estimate against the dense SVD ----------------------------------------------------------------------------------------
def _ratio(inst, dtype, P=40):
    A = sp.csr_matrix(inst["A"], dtype=dtype)
    dr, dc = ps.scaling(A, 10, True, dtype)
    S = sp.diags(dr.astype(np.float64)) @ sp.csr_matrix(inst["A"], dtype=np.float64) @ sp.diags(dc.astype(np.float64))
    top = float(np.linalg.svd(S.toarray(), compute_uv=False)[0])
    est, nus = so.power(inst["A"], dr, dc, P, dtype)
    assert est.dtype == dtype and len(nus) == P + 1 and float(so.bound(inst["A"], dr, dc, dtype)) >= top * (1 - 2.0 ** -20)
    return float(est) / top


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_estimate_lies_just_below_the_two_norm(planted, long_rows, dtype):
    """upper: sigma_est <= |S|_2 (1 + 2^-20), the slack for the fp32 sums; lower: sigma_est >= 0.98 |S|_2"""
    for name, inst in [(f"seed {s}, {i['m']} x {i['n']}", i) for s in SEEDS for i in planted[s]] + [("long rows", long_rows)]:
        r = _ratio(inst, dtype)
        print(f"{name}, {np.dtype(dtype).name}: sigma_est / |S|_2 = {r:.6f}")
        assert 0.98 <= r <= 1 + 2.0 ** -20, (name, r)


# ---- 3. the start ---------------------------------------------------------------------------------------------------------------
def test_the_start_vector_is_exact_and_in_one_two():
    h32, h64 = so.start_vector(5000, np.float32), so.start_vector(5000, np.float64)
    assert np.array_equal(h32.astype(np.float64), h64) and (h64 >= 1).all() and (h64 < 2).all() and len(np.unique(h64)) > 4900
    assert h64[0] == 1.0 and h64[1] == 1.0 + ((2654435761 % 2 ** 32) >> 9) * 2.0 ** -23 and h64[3] == 1.0 + (((3 * 2654435761) % 2 ** 32) >> 9) * 2.0 ** -23


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_hash_start_is_not_annihilated_by_scsd1(dtype):
    """A 1 = 0 for scsd1 (printed): a constant start leaves the first round nothing to work on.  The hash start gives nu_1 > 0 and
    a finite estimate that stays a lower bound"""
    inst = _netlib(["scsd1"])[0]
    A = sp.csr_matrix(inst["A"], dtype=dtype)
    dr, dc = ps.scaling(A, 10, True, dtype)
    ones = np.ones(A.shape[1], np.float64)
    S = sp.diags(dr.astype(np.float64)) @ sp.csr_matrix(inst["A"], dtype=np.float64) @ sp.diags(dc.astype(np.float64))
    top = float(np.linalg.svd(S.toarray(), compute_uv=False)[0])
    print("scsd1: |A 1| / |A|_F |1| =", np.linalg.norm(sp.csr_matrix(inst["A"], dtype=np.float64) @ ones) / (sp.linalg.norm(A) * np.linalg.norm(ones)))
    est, nus = so.power(inst["A"], dr, dc, 40, dtype)
    print("scsd1:", np.dtype(dtype).name, "nu_1", nus[1], "sigma_est / |S|_2", float(est) / top)
    assert len(nus) == 41 and np.isfinite(nus).all() and nus[1] > 0
    assert 0 < float(est) <= top * (1 + 2.0 ** -20)         # (a lower bound in exact arithmetic; how tight is printed, not asserted)


# ---- 4. the fallback --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_void_estimate_and_one_above_the_bound_fall_back(planted, dtype):
    inst = planted[SEEDS[0]][1]
    base = ph.solve(inst["A"], inst["b"], inst["c"], 256, eps=EPS, dtype=dtype)
    # a matrix with no nonzeros: the product of the bound is 0, eta = step
    Z = sp.csr_matrix((4, 7))
    z = so.solve(Z, np.zeros(4), np.ones(7), 64, power_iters=40, eps=EPS, dtype=dtype)
    assert z["fallback"] and z["norm"][0] == 0 and z["norm"][1] == 0 and z["eta"] == dtype(0.9) and len(z["nus"]) == 2 and z["nus"][1] == 0
    for shape in ((0, 3), (2, 0)):
        z = so.solve(sp.csr_matrix(shape), np.ones(shape[0]), np.ones(shape[1]), 64, power_iters=3, eps=EPS, dtype=dtype)
        assert z["fallback"] and z["norm"][0] == 0 and z["eta"] == dtype(0.9)
    # an estimate doctored above the bound, not finite, or not positive: the bound's step, bit for bit
    L = base["eta"]
    for bad in (np.inf, np.nan, -1.0, 0.0, float(dtype(0.9) / L) * 1.5):
        z = so.solve(inst["A"], inst["b"], inst["c"], 256, power_iters=40, sigma_est=bad, eps=EPS, dtype=dtype)
        assert z["fallback"] and z["eta"] == base["eta"], bad
        _same(base, z)
    # ... and one just below it is taken
    ok = so.solve(inst["A"], inst["b"], inst["c"], 256, power_iters=40, sigma_est=float(dtype(0.9) / L) * 0.75, eps=EPS, dtype=dtype)
    assert not ok["fallback"] and ok["eta"] > base["eta"]


# ---- 5. the claim ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_fewer_iterations_on_the_long_rows(long_rows, dtype):
    a = so.solve(long_rows["A"], long_rows["b"], long_rows["c"], 4096, power_iters=0, eps=EPS, dtype=dtype)
    z = so.solve(long_rows["A"], long_rows["b"], long_rows["c"], 4096, power_iters=40, eps=EPS, dtype=dtype)
    print(np.dtype(dtype).name, "long rows:", a["status"], "->", z["status"], "norm", z["norm"])
    assert a["status"][:2] == [0, 2176] and z["status"][0] == 0 and z["status"][1] < a["status"][1] and not z["fallback"]
    assert z["status"][1] == 448


@pytest.mark.parametrize("dtype", DTYPES)
def test_fewer_iterations_than_the_pinned_counts_on_six_netlib_instances(dtype):
    for inst in _netlib(NETLIB):
        pinned, proto = NETLIB[inst["name"].split(".")[0]]
        z = so.solve(inst["A"], inst["b"], inst["c"], 8192, power_iters=40, eps=EPS, dtype=dtype)
        print(np.dtype(dtype).name, inst["name"], pinned, "->", z["status"], "norm", z["norm"])
        assert z["status"][0] == 0 and z["status"][1] < pinned and not z["fallback"], (inst["name"], z["status"])
        assert z["status"][1] == proto, (inst["name"], z["status"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_planted_shapes_end_optimal_and_their_counts_are_recorded(planted, dtype):
    for seed in SEEDS:
        for inst, (before, after) in zip(planted[seed], PLANTED[seed]):
            a = so.solve(inst["A"], inst["b"], inst["c"], 8192, power_iters=0, eps=EPS, dtype=dtype)
            z = so.solve(inst["A"], inst["b"], inst["c"], 8192, power_iters=40, eps=EPS, dtype=dtype)
            assert (a["status"][0], a["status"][1], z["status"][0], z["status"][1]) == (0, before, 0, after), (seed, inst["m"], a["status"], z["status"])
    assert PLANTED[43][0][1] > PLANTED[43][0][0] and PLANTED[43][1][1] > PLANTED[43][1][0]          # slower, and said so
