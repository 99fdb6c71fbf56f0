"""CPU: the numpy oracle of mllp_lp_pdhg_halpern (tests/pdhg_halpern_oracle.py) does what THE RULE of include/mllp_hip.h
says -- its first step is the scaled rule's, the scaling, the step and the weight's start are the scaled oracle's, the weight
stays inside its clamp and moves only at restarts, the anchor moves at every restart with or without the weight --, the rule
delivers what it was built for where that can be checked without a GPU (no more iterations than the scaled rule on the
planted shapes, fewer on six small Netlib instances), and the C ABI's new entry points exist, refuse what they must and
report their limits.  The device is held to this oracle by tests/test_pdhg_halpern.py.
"""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

import pdhg_halpern_oracle as ph
import pdhg_oracle as pg
import pdhg_scaled_oracle as ps
import planted_oracle as po
import test_basis_repair as tb
from mllp_amd import _lib

EPS = 2.0 ** -10
SHAPES = [(5, 12), (40, 100), (193, 400)]
SEEDS = (27, 22, 43)
NETLIB = ("afiro", "sc50a", "sc50b", "blend", "adlittle", "stocfor1")


@pytest.fixture(scope="module")
def planted():
    """{seed: the three shapes}, planted in fp64 and rounded to fp32"""
    return {seed: pg.cpu_planted(tb.planted_shapes(SHAPES, seed)) for seed in SEEDS}


@pytest.fixture(scope="module")
def long_rows():
    return pg.cpu_planted(po.ragged_case(which=[4]))[0]


@pytest.fixture(scope="module")
def netlib():
    from mllp_amd.data import load_packed
    return [dict(name=i.name, A=sp.csr_matrix((i.values, i.indices, i.indptr), shape=(i.m, i.n)), b=i.rhs, c=i.coefs) for i in load_packed(NETLIB)]


# ---- 1. what the rule shares with the scaled rule ---------------------------------------------------------------------------
@pytest.mark.parametrize("reflect", [True, False])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_first_step_is_the_scaled_rules(planted, dtype, reflect):
    """the output is (xh, yh), and the first step's output does not depend on w1, w2 or on the reflection of the ITERATE"""
    for inst in planted[SEEDS[0]]:
        for kw in (dict(), dict(x0=np.linspace(-1, 1, inst["n"]), y0=np.ones(inst["m"])), dict(primal_weight=False, ruiz=2, pock_chambolle=False)):
            a = ps.solve(inst["A"], inst["b"], inst["c"], 1, check_every=0, dtype=dtype, **kw)
            z = ph.solve(inst["A"], inst["b"], inst["c"], 1, check_every=0, reflect=reflect, dtype=dtype, **kw)
            assert z["x"].dtype == dtype and np.array_equal(a["x"], z["x"]) and np.array_equal(a["y"], z["y"])
            assert z["status"] == [6, 1, 0, 0] and z["kkt"] == a["kkt"]
            zero = ph.solve(inst["A"], inst["b"], inst["c"], 0, reflect=reflect, dtype=dtype, **kw)
            start = ps.solve(inst["A"], inst["b"], inst["c"], 0, dtype=dtype, **kw)
            assert zero["status"] == [6, 0, 0, 0] and np.array_equal(zero["x"], start["x"]) and np.array_equal(zero["y"], start["y"])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_scaling_step_and_weight_start_are_the_scaled_oracles(planted, long_rows, dtype):
    for inst in planted[SEEDS[1]] + [long_rows]:
        for kw in (dict(), dict(ruiz=3, pock_chambolle=False), dict(primal_weight=False)):
            a = ps.solve(inst["A"], inst["b"], inst["c"], 0, dtype=dtype, **kw)
            z = ph.solve(inst["A"], inst["b"], inst["c"], 128, dtype=dtype, **kw)
            assert np.array_equal(a["dr"], z["dr"]) and np.array_equal(a["dc"], z["dc"]) and a["eta"] == z["eta"] and a["w0"] == z["w0"]
            assert z["kkt"][3:5] == a["kkt"][3:5] and z["status"][3] == 0


def test_the_reflection_changes_the_iterates():
    """reflect is not decoration: from the second iteration on the two variants differ"""
    inst = pg.cpu_planted(tb.planted_shapes(SHAPES, SEEDS[0]))[1]
    a = ph.solve(inst["A"], inst["b"], inst["c"], 2, check_every=0, reflect=True, dtype=np.float32)
    z = ph.solve(inst["A"], inst["b"], inst["c"], 2, check_every=0, reflect=False, dtype=np.float32)
    assert not np.array_equal(a["x"], z["x"]) and not np.array_equal(a["y"], z["y"])


# ---- 2. the weight and the anchor -------------------------------------------------------------------------------------------
def test_the_weight_stays_inside_its_clamp_and_moves_only_at_restarts(planted, long_rows):
    moved = 0
    for inst in planted[SEEDS[2]] + [long_rows]:
        for span in (16.0, 1.25, 1.0):
            r = ph.solve(inst["A"], inst["b"], inst["c"], 2048, eps=2.0 ** -14, weight_span=span, dtype=np.float32)
            w0, f32 = r["w0"], np.float32
            lo, hi = f32(w0 / f32(span)), f32(w0 * f32(span))
            restarts = [k["it"] for k in r["checks"] if k.get("restart")]
            assert [u["it"] for u in r["weights"]] == restarts[:len(r["weights"])] and len(restarts) == r["status"][2] >= 2
            assert r["anchors"] == restarts
            assert all(lo <= f32(u["w"]) <= hi for u in r["weights"]) and lo <= r["w"] <= hi
            at = {u["it"]: u["w"] for u in r["weights"]}
            w = float(w0)
            for k in r["checks"]:       # the weight a check ran under is the one the last restart before it left
                assert k["w"] == w, (k["it"], k["w"], w)
                w = at.get(k["it"], w) if k.get("restart") else w
            if span == 1.0:
                assert all(u["w"] == w0 for u in r["weights"]) and r["w"] == w0
            moved += any(u["w"] != w0 for u in r["weights"])
    assert moved >= 4, moved


def test_the_anchor_moves_at_every_restart_without_the_weight_too(planted):
    for inst in planted[SEEDS[0]]:
        r = ph.solve(inst["A"], inst["b"], inst["c"], 2048, eps=2.0 ** -14, primal_weight=False, dtype=np.float32)
        restarts = [k["it"] for k in r["checks"] if k.get("restart")]
        assert r["weights"] == [] and r["w"] == r["w0"] == 1.0 and len(restarts) == r["status"][2] >= 2 and r["anchors"] == restarts
        # k counts from the last restart: a check right after a restart sees k = check_every
        for prev, k in zip(r["checks"], r["checks"][1:]):
            assert k["k"] == (64 if prev.get("restart") else prev["k"] + 64)
        # the anchor is the point of the last restart: run up to it and compare with the output there
        upto = ph.solve(inst["A"], inst["b"], inst["c"], restarts[-1], eps=2.0 ** -14, primal_weight=False, dtype=np.float32)
        assert np.array_equal(r["anchor"][0], upto["x"]) and np.array_equal(r["anchor"][1], upto["y"])


# ---- 3. the claim -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_no_more_iterations_than_the_scaled_rule_on_the_planted_shapes(planted, dtype):
    for seed in SEEDS:
        for inst in planted[seed]:
            a = ps.solve(inst["A"], inst["b"], inst["c"], 8192, eps=EPS, dtype=dtype)
            r = ph.solve(inst["A"], inst["b"], inst["c"], 8192, eps=EPS, dtype=dtype)
            print(seed, inst["m"], inst["n"], "scaled", a["status"], "halpern", r["status"])
            assert a["status"][0] == r["status"][0] == 0 and r["status"][1] <= a["status"][1], (seed, inst["m"], a["status"], r["status"])
            assert max(pg.errors64(inst["A"], inst["b"], inst["c"], r["x"], r["y"])) <= EPS * (1 + 2.0 ** -6)
            assert np.array_equal(pg.topm(r["x"], inst["m"]), inst["labels"])


def test_the_long_rows_converge(long_rows):
    r = ph.solve(long_rows["A"], long_rows["b"], long_rows["c"], 4096, eps=EPS, dtype=np.float32)
    print("long rows:", r["status"], r["kkt"])
    assert r["status"][0] == ph.CODE_OPTIMAL and r["status"][1] <= 4096 and r["status"][1] % 64 == 0
    assert max(pg.errors64(long_rows["A"], long_rows["b"], long_rows["c"], r["x"], r["y"])) <= EPS * (1 + 2.0 ** -6)


def test_fewer_iterations_than_the_scaled_rule_on_six_netlib_instances(netlib):
    for inst in netlib:
        a = ps.solve(inst["A"], inst["b"], inst["c"], 8192, eps=EPS, dtype=np.float32)
        r = ph.solve(inst["A"], inst["b"], inst["c"], 8192, eps=EPS, dtype=np.float32)
        u = ph.solve(inst["A"], inst["b"], inst["c"], 8192, eps=EPS, reflect=False, dtype=np.float32)
        print(inst["name"], "scaled", a["status"], "halpern", r["status"], "not reflected", u["status"])
        assert a["status"][0] == r["status"][0] == 0 and r["status"][1] < a["status"][1], (inst["name"], a["status"], r["status"])
        assert u["status"][0] == 0, (inst["name"], u["status"])         # the unreflected variant is not required to win


# ---- 4. the C ABI, without a GPU --------------------------------------------------------------------------------------------
NEW = ("mllp_lp_pdhg_halpern_limits", "mllp_lp_pdhg_halpern_scratch_bytes", "mllp_lp_pdhg_halpern")
ORDER = ("g", "x1", "x2", "x0", "y0", "max_iters", "check_every", "eps", "step", "beta", "ruiz", "pc", "pw", "span", "reflect", "lds", "x", "y",
         "dr", "dc", "status", "kkt", "scratch", "stream")


def test_the_new_symbols_are_exported_and_bound():
    L = _lib.lib()
    header = open(_lib.HEADER_PATH).read()
    for name in NEW:
        assert name in _lib._PROTOTYPES and hasattr(L, name) and f"int {name}(" in header, name
    assert len(_lib._PROTOTYPES["mllp_lp_pdhg_halpern"][1]) == len(ORDER) == len(_lib._PROTOTYPES["mllp_lp_pdhg_scaled"][1]) + 1
    scaled, halpern = _lib._PROTOTYPES["mllp_lp_pdhg_scaled"][1], _lib._PROTOTYPES["mllp_lp_pdhg_halpern"][1]
    at = ORDER.index("reflect")
    assert halpern[:at] == scaled[:at] and halpern[at] is ctypes.c_int32 and halpern[at + 1:] == scaled[at:]


def test_null_arguments_are_refused_before_any_hip_call():
    L = _lib.lib()
    z = ctypes.c_void_p(0)
    assert L.mllp_lp_pdhg_halpern(z, z, z, z, z, 10, 64, EPS, 0.9, 0.5, 10, 1, 1, 16.0, 1, 0, z, z, z, z, z, z, z, z) == -1
    assert b"mllp_lp_pdhg_halpern:" in L.mllp_last_error() and b"null" in L.mllp_last_error()
    n = ctypes.c_int64(-7)
    assert L.mllp_lp_pdhg_halpern_scratch_bytes(z, 0, ctypes.byref(n)) == -1 and n.value == -7
    assert b"mllp_lp_pdhg_halpern_scratch_bytes" in L.mllp_last_error()
    assert L.mllp_lp_pdhg_halpern_limits(None) == -1 and b"mllp_lp_pdhg_halpern_limits" in L.mllp_last_error()


def test_every_refusal_names_the_call_in_the_scaled_calls_words():
    """the checks of the scalar arguments come before the graph is read and before any HIP call, and a refused call
    dereferences no pointer: non-null dummies stand for the graph and the device buffers.  The message behind the name is
    the one mllp_lp_pdhg_scaled gives to the same arguments"""
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = dict(g=p, x1=p, x2=p, x0=None, y0=None, max_iters=10, check_every=64, eps=EPS, step=0.9, beta=0.5, ruiz=10, pc=1, pw=1, span=16.0, reflect=1,
              lds=0, x=p, y=p, dr=None, dc=None, status=p, kkt=None, scratch=None, stream=None)
    nan, inf = float("nan"), float("inf")
    bad = [dict(ruiz=-1), dict(ruiz=65), dict(span=nan), dict(span=inf), dict(span=0.5), dict(span=-2.0), dict(max_iters=-1), dict(check_every=-1),
           dict(lds=-1), dict(eps=nan), dict(step=0.0), dict(step=1.5), dict(beta=1.0), dict(beta=nan), dict(ruiz=65, span=0.5),
           dict(beta=nan, ruiz=-1), dict(x=None)]
    for kw in bad:
        args = dict(ok, **kw)
        assert L.mllp_lp_pdhg_halpern(*[args[k] for k in ORDER]) == -1, kw
        mine = L.mllp_last_error()
        assert L.mllp_lp_pdhg_scaled(*[args[k] for k in ORDER if k != "reflect"]) == -1, kw
        theirs = L.mllp_last_error()
        assert mine.startswith(b"mllp_lp_pdhg_halpern: ") and mine.split(b": ", 1)[1] == theirs.split(b": ", 1)[1], (kw, mine, theirs)
    args = dict(ok, span=0.5)
    assert L.mllp_lp_pdhg_halpern(*[args[k] for k in ORDER]) == -1 and b"weight_span" in L.mllp_last_error()
    args = dict(ok, ruiz=65)
    assert L.mllp_lp_pdhg_halpern(*[args[k] for k in ORDER]) == -1 and b"ruiz_passes" in L.mllp_last_error()


def test_the_limits_answer_without_a_gpu():
    lim, scaled = (ctypes.c_int64 * 3)(), (ctypes.c_int64 * 3)()
    assert _lib.lib().mllp_lp_pdhg_halpern_limits(lim) == 0 and _lib.lib().mllp_lp_pdhg_scaled_limits(scaled) == 0
    assert list(lim) == [36864, 1024, 64] == list(scaled)          # include/mllp_hip.h states all three
    from mllp_amd.graph import LPBatch, LPPdhg, LPPdhgHalpern, LPPdhgScaled, pdhg_halpern_limits, pdhg_scaled_limits
    assert pdhg_halpern_limits() == (36864, 1024, 64) == pdhg_scaled_limits()
    assert hasattr(LPBatch, "pdhg_halpern") and issubclass(LPPdhgHalpern, LPPdhgScaled) and issubclass(LPPdhgHalpern, LPPdhg)


@pytest.mark.gpu
def test_scratch_bytes_are_the_scaled_calls_on_a_host_created_batch():
    """(a batch is created on a device: this one needs the GPU, and runs no kernel of the call)"""
    from mllp_amd.data import load_packed
    from mllp_amd.graph import LPBatch
    b = LPBatch.from_instances(load_packed(NETLIB))
    words = [3 * n + 2 * m for m, n in zip(b.inst_m, b.inst_n)]
    for lds in (0, min(words), sorted(words)[3], max(words), 36864):
        got, want = ctypes.c_int64(-1), ctypes.c_int64(-2)
        assert _lib.lib().mllp_lp_pdhg_halpern_scratch_bytes(b._h, lds, ctypes.byref(got)) == 0
        assert _lib.lib().mllp_lp_pdhg_scaled_scratch_bytes(b._h, lds, ctypes.byref(want)) == 0
        assert got.value == want.value == 4 * (sum(2 * n + 2 * m for m, n in zip(b.inst_m, b.inst_n)) + sum(w for w in words if w > lds))
