"""Pivot a repaired basis to optimality on the device (mllp_basis_simplex; LPBatch.simplex / simplex_solved)
against the fp64 oracle of tests/simplex_oracle.py.  GPU tests.

CASES.  Planted instances as tests/test_basis_repair.py::planted_shapes builds them, planted on the device; the start is the
labels with k basic columns swapped for k nonbasic ones and repaired by the fp64 walk (simplex_oracle.perturbed_start).  The
planted optimum is unique and nondegenerate by construction, hence two kinds of assertion:

RULE-INDEPENDENT (any path): code 0, the final basis is the planted labels, `simplex_solved` certifies it optimal under
feas_tol = opt_tol = 1e-3 after a fresh factorization, and the pivots stay within max_pivots.

TRACE PARITY (guarded cases): every margin of the ORACLE's run is at least 2^-6 (simplex_oracle.guarded, asserted from the
oracle alone before the device is looked at: a condition, not a measurement); then the device's fp32 decisions are the
oracle's, and status, trace, col_of_row (as a set) and basis are equal exactly.  The seeds were found by scanning the oracle
on the CPU; any seed that meets the condition would do.
"""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import simplex_oracle as so
import test_basis_repair as tb
from guarded import PATTERNS, Guarded, same_bits
from mllp_amd import _lib

pytestmark = pytest.mark.gpu
EINVAL = -1
TOL = 2.0 ** -12
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
_INTERNAL = open(os.path.join(ROOT, "mllp_amd", "csrc", "internal.h")).read()
LDS_MAX = int(re.search(r"SIMPLEX_LDS_MAX_M\s*=\s*(\d+)", _INTERNAL).group(1))
ROW_LIMIT = int(re.search(r"SIMPLEX_MAX_M\s*=\s*(\d+)", _INTERNAL).group(1))
N_T = 400 if LDS_MAX == 192 else 2 * LDS_MAX + 16          # columns of the two instances around the threshold
NAMES = ("basis", "col_of_row", "trace", "status")


@pytest.fixture(scope="module")
def LPBatch():
    _lib.lib()
    assert torch.cuda.is_available()
    from mllp_amd.graph import LPBatch as cls
    assert hasattr(cls, "simplex") and hasattr(cls, "simplex_solved")
    return cls


# ---------------------------------------------------------------------------------------------------
# cases and helpers
# ---------------------------------------------------------------------------------------------------
def planted_case(LPBatch, shapes, seed, ks, max_pivots):
    c = tb.planted_shapes(shapes, seed)
    b, mats, st = tb._planted(LPBatch, c)
    start = np.zeros(c["N"], np.float32)
    for i in range(len(shapes)):
        s = slice(c["ptr_n"][i], c["ptr_n"][i + 1])
        start[s], _ = so.perturbed_start(mats[i], st["labels"][s], ks[i], seed + i)
    return dict(c=c, b=b, mats=mats, x1=st["x1"], x2=st["x2"], labels=st["labels"], values=st["values"], start=start,
                max_pivots=max_pivots)


def oracle(g, k, max_pivots=None, **kw):
    c = g["c"]
    s, r = slice(c["ptr_n"][k], c["ptr_n"][k + 1]), slice(c["ptr_m"][k], c["ptr_m"][k + 1])
    return so.run(g["mats"][k], g["x2"][r], g["x1"][s], g["start"][s], g["max_pivots"] if max_pivots is None else max_pivots, **kw)


def _host(res):
    torch.cuda.synchronize()
    return {k: None if getattr(res, k) is None else getattr(res, k).cpu().numpy() for k in NAMES}


def _bits(h):
    return {k: np.ascontiguousarray(v).view(np.int32).reshape(-1).copy() for k, v in h.items() if v is not None}


def _inst(c, h, k):
    """instance k's part of every output"""
    s, r = slice(c["ptr_n"][k], c["ptr_n"][k + 1]), slice(c["ptr_m"][k], c["ptr_m"][k + 1])
    part = dict(basis=s, col_of_row=r, trace=slice(k, k + 1), status=slice(k, k + 1))
    return {name: h[name][sl] for name, sl in part.items() if h[name] is not None}


def run(g, max_pivots=None, **kw):
    return g["b"].simplex(tb._dev(g["start"]), g["max_pivots"] if max_pivots is None else max_pivots, tol=TOL, **kw)


def check_trace_shape(part, what):
    code, nd, np_, _ = part["status"][0]
    t = part["trace"][0]
    assert (t[:nd + np_] >= 0).all() and (t[nd + np_:] == -1).all(), f"{what}: the trace does not hold {nd + np_} pivots, then -1"


def check_rule_independent(g, res, what):
    c = g["c"]
    h = _host(res)
    for k, m in enumerate(c["inst_m"]):
        part = _inst(c, h, k)
        code, nd, np_, rank = part["status"][0]
        print(f"{what}: instance {k} ({m} x {c['inst_n'][k]}): code {code}, {nd} + {np_} pivots")
        assert code == 0 and rank == m, f"{what}: instance {k}: status {part['status'][0]}"
        assert nd + np_ <= g["max_pivots"]
        s = slice(c["ptr_n"][k], c["ptr_n"][k + 1])
        assert np.array_equal(part["basis"], g["labels"][s]), f"{what}: instance {k}: the final basis is not the planted one"
        assert sorted(part["col_of_row"]) == sorted(np.flatnonzero(g["labels"][s]))
        check_trace_shape(part, f"{what}: instance {k}")
    got = g["b"].simplex_solved(res, 1e-3, 1e-3)
    for key in ("usable", "primal_feasible", "optimal"):
        assert got[key].dtype == torch.bool and bool(got[key].all()), key
    assert got["pivots"].cpu().tolist() == [int(r[1] + r[2]) for r in h["status"]]
    return h


def check_against_oracle(c, h, k, res, what):
    part = _inst(c, h, k)
    assert list(part["status"][0]) == res["status"], f"{what}: status {part['status'][0]}, the oracle's {res['status']}"
    assert np.array_equal(part["trace"][0], so.trace_array(res, part["trace"].shape[1])), f"{what}: another path"
    assert sorted(part["col_of_row"]) == sorted(res["col_of_row"]) and np.array_equal(part["basis"], res["basis"]), what


# ---------------------------------------------------------------------------------------------------
# rule-independent: the planted optimum is reached
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,k,max_pivots", [((5, 12), 2, 50), ((40, 100), 12, 200), ((50, 120), 25, 250)], ids=str)
def test_reaches_the_planted_optimum(LPBatch, shape, k, max_pivots):
    g = planted_case(LPBatch, [shape], 40, [k], max_pivots)
    assert not np.array_equal(g["start"], g["labels"])
    check_rule_independent(g, run(g), str(shape))


@pytest.fixture(scope="module")
def threshold(LPBatch):
    """m = threshold (T in LDS) and threshold + 1 (T in scratch) in one ragged batch, eight columns swapped in each"""
    return planted_case(LPBatch, [(LDS_MAX, N_T), (LDS_MAX + 1, N_T)], 40, [8, 8], 400)


def test_both_sides_of_the_lds_threshold(LPBatch, threshold):
    g = threshold
    c = g["c"]
    n = ctypes.c_int64(-1)
    _lib.check(_lib.lib().mllp_basis_simplex_scratch_bytes(g["b"]._h, 1 << 40, ctypes.byref(n)))
    assert n.value == 4 * (2 * N_T + (LDS_MAX + 1) ** 2)      # the shifts of both, m^2 words only above the threshold
    h = check_rule_independent(g, run(g), "threshold")
    one = planted_case(LPBatch, [(LDS_MAX, N_T)], 40, [8], 400)
    s = slice(c["ptr_n"][0], c["ptr_n"][1])
    assert np.array_equal(one["values"], g["values"][c["nnz_off"][0]:c["nnz_off"][1]]) and np.array_equal(one["x1"], g["x1"][s])
    assert np.array_equal(one["start"], g["start"][s])
    h1 = _host(run(one))
    same_bits(_bits(h1), _bits(_inst(c, h, 0)), "the threshold-sized instance alone against inside the batch")


# ---------------------------------------------------------------------------------------------------
# trace parity with the fp64 oracle on guarded cases
# ---------------------------------------------------------------------------------------------------
GUARDED = ([(5, 12, 2, s) for s in (47, 57, 59, 41, 40)] + [(40, 100, 4, s) for s in (59, 56, 49, 51, 52, 57)]
           + [(192, 400, 3, 68), (192, 400, 3, 95), (193, 400, 3, 60), (193, 400, 3, 77)])
BOTH_STAGES = {(40, 59), (40, 56), (40, 49)}


@pytest.mark.parametrize("m,n,k,seed", GUARDED)
def test_trace_parity(LPBatch, m, n, k, seed):
    g = planted_case(LPBatch, [(m, n)], seed, [k], 100)
    res = oracle(g, 0)
    print(f"{m} x {n}, k = {k}, seed {seed}: the oracle's status {res['status']}, smallest margin {res['margin']:.4f}")
    assert so.guarded(res, TOL), f"seed {seed}: a margin of the oracle's run is below 2^-6: {min(res['margins'], key=lambda t: t[1])}"
    assert res["code"] == 0 and np.array_equal(res["basis"], g["labels"])
    if (m, seed) in BOTH_STAGES:
        assert res["status"][1] > 0 and res["status"][2] > 0
    check_against_oracle(g["c"], _host(run(g)), 0, res, f"{m} x {n} seed {seed}")


def test_the_pivot_limit(LPBatch):
    """max_pivots below the oracle's count: code 6, and trace and basis are the oracle's first max_pivots steps"""
    g = planted_case(LPBatch, [(40, 100)], 59, [4], 100)
    full = oracle(g, 0)
    assert so.guarded(full, TOL) and full["code"] == 0 and len(full["trace"]) > 3
    for cap in (3, 0):
        res = oracle(g, 0, max_pivots=cap)
        assert res["code"] == 6 and res["trace"] == full["trace"][:cap]
        h = _host(run(g, max_pivots=cap))
        assert h["trace"].shape == (1, cap, 2)
        check_against_oracle(g["c"], h, 0, res, f"max_pivots {cap}")
    h = _host(run(g, max_pivots=len(full["trace"])))         # exactly enough: the optimality test needs no pivot
    assert h["status"][0, 0] == 0


def test_start_at_the_labels(threshold):
    g = dict(threshold, start=threshold["labels"].astype(np.float32))
    h = _host(run(g))
    for k, m in enumerate(g["c"]["inst_m"]):
        assert list(h["status"][k]) == [0, 0, 0, m]
    assert (h["trace"] == -1).all() and np.array_equal(h["basis"], g["labels"])


# ---------------------------------------------------------------------------------------------------
# verdicts, bad masks, singular starts, empty and skipped instances
# ---------------------------------------------------------------------------------------------------
def _feasible_start_lp(seed=3):
    """6 x 10: positive structural columns with negative costs beside a slack identity, b > 0: the slack basis is primal
    feasible and not optimal, and the LP is bounded"""
    rng = np.random.default_rng(seed)
    a = np.zeros((6, 10), np.float32)
    a[:, :4] = (rng.random((6, 4)) + 0.25) * (rng.random((6, 4)) < 0.7)
    a[0, :4] = rng.random(4) + 0.25                         # (no empty structural column)
    a[:, 4:] = np.eye(6)
    return a.astype(np.float64), (rng.random(6) + 0.5).astype(np.float32), np.concatenate([-(rng.random(4) + 0.5), np.zeros(6)]).astype(np.float32)


@pytest.fixture(scope="module")
def edge(LPBatch):
    mats = [np.array([[1.0, 1.0]]), np.array([[1.0, -1.0]]), np.array([[1.0, 1.0, 1.0]]), tb.deficient_mats()[1], np.zeros((3, 5)),
            np.zeros((0, 4)), tb.int_matrix(3, 6, 0.7, 12), tb.int_matrix(3, 6, 0.7, 14)]
    a8, b8, c8 = _feasible_start_lp()
    mats.append(a8)
    c = tb.dense_case(mats, 2)
    masks = [[1, 0], [1, 0], [0, 0, 1], [0, 0, 0, 0, 1, 1, 1, 1], [1, 1, 1, 0, 0], [0, 0, 0, 0], [0, 0, 0, 1, 1, 0], [0, 0, 1, 1, 1, 1],
             [0] * 4 + [1] * 6]
    given = {0: ([-1.0], [1.0, 1.0]), 1: ([1.0], [-1.0, 0.0]), 2: ([1.0], [-1.0, -2.0, 0.0]), 5: ([], [1.0, 0.0, 2.0, 3.0]), 8: (b8, c8)}
    for k, (rhs, cost) in given.items():
        c["b"][c["ptr_m"][k]:c["ptr_m"][k + 1]] = rhs
        c["c"][c["ptr_n"][k]:c["ptr_n"][k + 1]] = cost
    g = dict(c=c, b=tb._build(LPBatch, c, tb._dev(c["c"]), tb._dev(c["b"])), mats=c["mats"], x1=c["c"], x2=c["b"],
             start=np.concatenate(masks).astype(np.float32), max_pivots=20)
    g["oracle"] = [oracle(g, k) for k in range(len(mats))]
    return g


def test_verdicts_and_edge_instances(edge):
    g = edge
    c, want = g["c"], [r["status"] for r in g["oracle"]]
    assert want[0] == [4, 0, 0, 1]                      # x1 + x2 = -1: primal infeasible
    assert want[1] == [5, 0, 0, 1]                      # min -x1, x1 - x2 = 1 from {x1}: unbounded
    assert want[2] == [0, 0, 1, 1]                      # a primal-feasible start that is not optimal: no stage-D pivot
    assert want[3] == [1, 0, 0, 3] and want[4] == [1, 0, 0, 0]          # twin rows: a singular start; no nonzeros
    assert want[5] == [0, 0, 0, 0]                      # no rows
    assert want[6] == [3, 0, 0, 0] and want[7] == [3, 0, 0, 0]          # masks with m - 1 and m + 1 columns
    assert want[8][0] == 0 and want[8][1] == 0 and want[8][2] > 0 and so.guarded(g["oracle"][8], TOL), want[8]
    h = _host(run(g))
    for k, res in enumerate(g["oracle"]):
        check_against_oracle(c, h, k, res, f"edge instance {k}")
        check_trace_shape(_inst(c, h, k), f"edge instance {k}")
        if res["code"] in (1, 2, 3):
            part = _inst(c, h, k)
            assert not part["basis"].any() and (part["col_of_row"] == -1).all() and (part["trace"] == -1).all()
    got = g["b"].simplex_solved(run(g), 1e-3, 1e-3)
    assert got["optimal"].cpu().tolist() == [r["code"] == 0 for r in g["oracle"]]
    # m > max_m: instance 8 (6 rows) is skipped, outputs defaulted; every other instance keeps its bits
    h5 = _host(run(g, max_m=5))
    part = _inst(c, h5, 8)
    assert list(part["status"][0]) == [2, 0, 0, 0] and not part["basis"].any() and (part["col_of_row"] == -1).all()
    assert (part["trace"] == -1).all()
    for k in range(8):
        same_bits(_bits(_inst(c, h5, k)), _bits(_inst(c, h, k)), f"instance {k} beside a skipped one")
    n = ctypes.c_int64(-1)
    _lib.check(_lib.lib().mllp_basis_simplex_scratch_bytes(g["b"]._h, 5, ctypes.byref(n)))
    assert n.value == 4 * sum(c["inst_n"][:8])          # the shifts of the instances that may run; no transform in scratch
    _lib.check(_lib.lib().mllp_basis_simplex_scratch_bytes(g["b"]._h, ROW_LIMIT + 1, ctypes.byref(n)))
    assert n.value == 4 * sum(c["inst_n"])


# ---------------------------------------------------------------------------------------------------
# optional outputs, reproducibility, graph capture
# ---------------------------------------------------------------------------------------------------
def _abi_call(b, g, bufs, **kw):
    """mllp_basis_simplex through the C ABI; bufs and the overrides: name -> c_void_p / tensor / None"""
    p = lambda v: v if isinstance(v, ctypes.c_void_p) else _lib.ptr(v)      # noqa: E731
    a = dict(h=b._h, x1=b.x1, x2=b.x2, start=None, tol=TOL, ftol=2.0 ** -10, dtol=2.0 ** -10, ptol=2.0 ** -10, dshift=2.0 ** -4,
             max_pivots=g["max_pivots"], max_m=max(g["c"]["inst_m"]), scratch=None)
    a.update(kw)
    return _lib.lib().mllp_basis_simplex(a["h"], p(a["x1"]), p(a["x2"]), p(a["start"]), a["tol"], a["ftol"], a["dtol"], a["ptol"],
                                         a["dshift"], a["max_pivots"], a["max_m"], *[p(bufs.get(k)) for k in NAMES], p(a["scratch"]),
                                         _lib.current_stream())


def test_optional_outputs_and_reproducibility(threshold):
    """Each optional output alone gives the bits of the full call; two runs are bitwise equal; a graph captured once and
    replayed on a side stream equals the eager call."""
    g = threshold
    c, b = g["c"], g["b"]
    full = _bits(_host(run(g)))
    same_bits(_bits(_host(run(g))), full, "a second run")
    for want in (("col_of_row",), ("trace",), ("basis",), ()):
        got = _bits(_host(run(g, want=want)))
        assert set(got) == set(want) | {"basis", "status"}
        same_bits(got, {k: full[k] for k in got}, f"want={want}")
    with pytest.raises(ValueError):
        run(g, want=("x",))
    K, mp = len(c["inst_m"]), g["max_pivots"]
    poison = lambda n: tb._poison(n).view(torch.int32)      # noqa: E731
    bufs = dict(basis=tb._poison(c["N"]), col_of_row=poison(c["M"]), trace=poison(2 * K * mp), status=poison(4 * K))
    start, scratch = tb._dev(g["start"]), b._simplex_scratch[1]
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        rc = _abi_call(b, g, bufs, start=start, scratch=scratch)
    assert rc == 0
    for _ in range(2):
        with torch.cuda.stream(side):
            for t in bufs.values():
                t.view(torch.int32).fill_(-1)
            graph.replay()
        side.synchronize()
        same_bits({k: v.cpu().numpy().view(np.int32).reshape(-1) for k, v in bufs.items()}, full, "a replay of the captured call")


# ---------------------------------------------------------------------------------------------------
# memory contract
# ---------------------------------------------------------------------------------------------------
def test_memory_contract(threshold):
    """Guard bands around every caller buffer stay intact, inputs are not written, outputs and scratch poisoned with zeros,
    NaN or the largest float give the same bits (T in LDS and in scratch); refused calls leave the poison untouched."""
    g = threshold
    c, b = g["c"], g["b"]
    K, mp, max_m = len(c["inst_m"]), g["max_pivots"], max(c["inst_m"])
    n = ctypes.c_int64()
    _lib.check(_lib.lib().mllp_basis_simplex_scratch_bytes(b._h, max_m, ctypes.byref(n)))
    assert n.value > 0
    runs = {}
    nul = ctypes.c_void_p(0)
    for name, fill in PATTERNS.items():
        ins = dict(x1=Guarded(c["N"], device="cuda", data=g["x1"], name="x1", shift=4),
                   x2=Guarded(c["M"], device="cuda", data=g["x2"], name="x2", shift=8),
                   start=Guarded(c["N"], device="cuda", data=g["start"], name="start", shift=12))
        outs = dict(basis=Guarded(c["N"], device="cuda", fill=fill, name="basis", shift=4),
                    col_of_row=Guarded(c["M"], torch.int32, "cuda", fill=fill, name="col_of_row", shift=4),
                    trace=Guarded(2 * K * mp, torch.int32, "cuda", fill=fill, name="trace", shift=8),
                    status=Guarded(4 * K, torch.int32, "cuda", fill=fill, name="status", shift=4))
        scratch = Guarded(n.value // 4, device="cuda", fill=fill, name="scratch", shift=4)
        ptrs = {k: v.ptr for k, v in outs.items()}
        ok = dict(x1=ins["x1"].ptr, x2=ins["x2"].ptr, start=ins["start"].ptr, scratch=scratch.ptr, max_m=max_m)
        # refusals first: the poison stays
        before = {k: v.bits() for k, v in outs.items()}
        before["scratch"] = scratch.bits()
        bad = [dict(h=None), dict(x1=nul), dict(x2=nul), dict(start=nul), dict(bufs={**ptrs, "basis": nul}),
               dict(bufs={**ptrs, "status": nul}), dict(scratch=nul), dict(tol=float("nan")), dict(tol=-1.0), dict(ftol=0.0),
               dict(dtol=float("inf")), dict(ptol=-1.0), dict(dshift=float("nan")), dict(max_pivots=-1), dict(max_m=-1)]
        for kw in bad:
            args = dict(ok, **kw)
            assert _abi_call(b, g, args.pop("bufs", ptrs), **args) == EINVAL, kw
            assert b"mllp_basis_simplex" in _lib.lib().mllp_last_error()
        torch.cuda.synchronize()
        after = {k: v.bits() for k, v in outs.items()}
        after["scratch"] = scratch.bits()
        same_bits(after, before, f"buffers after the refused calls ({name} poison)")
        assert _abi_call(b, g, ptrs, **ok) == 0
        torch.cuda.synchronize()
        for v in list(ins.values()) + list(outs.values()) + [scratch]:
            v.check()
        runs[name] = {k: v.bits() for k, v in outs.items()}
    for name in runs:
        same_bits(runs[name], runs["zero"], f"outputs under {name} poison against zero poison")
    same_bits(runs["nan"], _bits(_host(run(g))), "the C ABI against LPBatch.simplex")


# ---------------------------------------------------------------------------------------------------
# driver
# ---------------------------------------------------------------------------------------------------
def test_driver_reports_pivots(tmp_path, monkeypatch):
    """8 planted instances, a quarter held out, `report_solved` with `pivots: 50`: the log gains `optimal_after_pivots` and
    `pivots` per epoch; without the key it has the keys it had."""
    from mllp_amd import experiment
    cfg = ("train_data_type: 'planted'\ntrain_lr: 1.e-3\ntrain_iter: 2\nmethods:\n  - 'gs-topk'\nbatch_size: 3\nholdout: 0.25\n"
           "planted: {instances: 8, m: 20, n: 50, row_nnz: 4, seed: 5}\n")
    base = {"obj", "val_obj", "usable", "feasible", "optimal", "skipped"} | {f"planted{5 + i}" for i in range(8)}
    for block, extra in (("report_solved: {feas_tol: 1.e-3, opt_tol: 1.e-3, max_m: 20, pivots: 50}\n", {"optimal_after_pivots", "pivots"}),
                         ("report_solved: {feas_tol: 1.e-3, opt_tol: 1.e-3, max_m: 20}\n", set())):
        (tmp_path / "cfg.yaml").write_text(cfg + block)
        monkeypatch.chdir(tmp_path)
        assert experiment.main(["--cfg", str(tmp_path / "cfg.yaml")]) == 0
        log = json.load(open(tmp_path / "train_log.json"))
        assert set(log) == base | extra
        for e in range(2):
            assert log["usable"][e] == 2 and 0 <= log["optimal"][e] <= log["feasible"][e] <= 2
            if extra:
                done, pivots = log["optimal_after_pivots"][e], log["pivots"][e]
                print(f"epoch {e}: optimal {log['optimal'][e]} of 2, after at most 50 pivots {done} of 2, {pivots} pivots in all")
                assert 0 <= done <= 2 and 0 <= pivots <= 50 * done
        assert all(len(log[k]) == 2 for k in extra)
