"""The guarded pivots on the device (mllp_basis_simplex_guarded; LPBatch.simplex(refactor_every=, stall_pivots=); DESIGN.md
4.16) against the fp64 oracle of tests/simplex_guarded_oracle.py and against mllp_basis_simplex.  GPU tests.

EQUIVALENCE: with both guards off the new entry point gives mllp_basis_simplex's bits.  TEXTBOOK: Chvatal's and Beale's
cycling LPs end optimal.  TRACE PARITY on guarded seeds of the degenerate family (a condition asserted from the oracle alone,
tests/test_simplex_guarded_oracle.py): status, guard, trace, basis and col_of_row equal the oracle's exactly.  STAGE-D BLAND:
rule-independent (those runs follow an exact ratio tie, which no guard admits).  REFACTORIZATION device against device:
right after one, the row owners are those of a fresh solve_basis.  Then instance independence, code 7, the old codes, the
driver and the memory contract.
"""
import ctypes
import json

import numpy as np
import pytest
import torch

import simplex_guarded_oracle as sg
import simplex_oracle as so
import test_basis_repair as tb
import test_simplex as ts
from guarded import PATTERNS, Guarded, same_bits
from mllp_amd import _lib
from test_simplex import LPBatch, edge, threshold  # noqa: F401  (fixtures)
from test_simplex_guarded_oracle import BLAND_P, NO_BLAND, STAGE_D

pytestmark = pytest.mark.gpu
EINVAL = -1
TOL = ts.TOL
NAMES = ts.NAMES + ("guard",)


# ---------------------------------------------------------------------------------------------------
# cases and helpers
# ---------------------------------------------------------------------------------------------------
def dense_batch(LPBatch, lps, max_pivots=200):  # noqa: F811
    """a batch of dense LPs (A, b, c, start): the dict of test_simplex's cases"""
    c = tb.dense_case([np.asarray(lp[0], np.float64) for lp in lps])
    c["b"] = np.concatenate([np.asarray(lp[1], np.float32) for lp in lps])
    c["c"] = np.concatenate([np.asarray(lp[2], np.float32) for lp in lps])
    return dict(c=c, b=tb._build(LPBatch, c, tb._dev(c["c"]), tb._dev(c["b"])), mats=c["mats"], x1=c["c"], x2=c["b"],
                start=np.concatenate([np.asarray(lp[3], np.float32) for lp in lps]), max_pivots=max_pivots, lps=lps)


def run(g, R, S, max_pivots=None, **kw):
    return g["b"].simplex(tb._dev(g["start"]), g["max_pivots"] if max_pivots is None else max_pivots, tol=kw.pop("tol", TOL),
                          refactor_every=R, stall_pivots=S, **kw)


def _host(res):
    torch.cuda.synchronize()
    return {k: None if getattr(res, k) is None else getattr(res, k).cpu().numpy() for k in NAMES}


def _inst(c, h, k):
    part = ts._inst(c, {n: h[n] for n in ts.NAMES}, k)
    if h.get("guard") is not None:
        part["guard"] = h["guard"][k:k + 1]
    return part


def _abi_call(b, g, bufs, R, S, **kw):
    """mllp_basis_simplex_guarded through the C ABI; bufs and the overrides: name -> c_void_p / tensor / None"""
    p = lambda v: v if isinstance(v, ctypes.c_void_p) else _lib.ptr(v)      # noqa: E731
    a = dict(h=b._h, x1=b.x1, x2=b.x2, start=None, tol=TOL, ftol=2.0 ** -10, dtol=2.0 ** -10, ptol=2.0 ** -10, dshift=2.0 ** -4,
             max_pivots=g["max_pivots"], max_m=max(g["c"]["inst_m"]), scratch=None, refactor=R, stall=S)
    a.update(kw)
    return _lib.lib().mllp_basis_simplex_guarded(a["h"], p(a["x1"]), p(a["x2"]), p(a["start"]), a["tol"], a["ftol"], a["dtol"], a["ptol"],
                                                 a["dshift"], a["max_pivots"], a["max_m"], a["refactor"], a["stall"],
                                                 *[p(bufs.get(k)) for k in NAMES], p(a["scratch"]), _lib.current_stream())


def abi_run(g, R, S, guard=True, **kw):
    """the C ABI into poisoned outputs: host arrays by name, shaped as LPBatch.simplex's"""
    c, b = g["c"], g["b"]
    K, mp = len(c["inst_m"]), kw.get("max_pivots", g["max_pivots"])
    poison = lambda n: tb._poison(max(n, 1)).view(torch.int32)      # noqa: E731
    bufs = dict(basis=tb._poison(max(c["N"], 1)), col_of_row=poison(c["M"]), trace=poison(2 * K * mp), status=poison(4 * K),
                guard=poison(2 * K) if guard else None)
    max_m = kw.get("max_m", max(c["inst_m"]))
    n = ctypes.c_int64()
    _lib.check(_lib.lib().mllp_basis_simplex_scratch_bytes(b._h, max_m, ctypes.byref(n)))
    scratch = tb._poison(max(n.value // 4, 1))
    assert _abi_call(b, g, bufs, R, S, start=tb._dev(g["start"]), scratch=scratch, **kw) == 0
    torch.cuda.synchronize()
    size = dict(basis=c["N"], col_of_row=c["M"], trace=2 * K * mp, status=4 * K, guard=2 * K)
    shape = dict(basis=(-1,), col_of_row=(-1,), trace=(K, mp, 2), status=(K, 4), guard=(K, 2))
    return {k: v[:size[k]].cpu().numpy().reshape(shape[k]) for k, v in bufs.items() if v is not None}


def check_against_oracle(c, h, k, res, what):
    """status, guard, trace, basis and col_of_row (row by row) are the oracle's"""
    part = _inst(c, h, k)
    assert list(part["status"][0]) == res["status"], f"{what}: status {part['status'][0]}, the oracle's {res['status']}"
    assert list(part["guard"][0]) == res["guard"], f"{what}: guard {part['guard'][0]}, the oracle's {res['guard']}"
    assert np.array_equal(part["trace"][0], so.trace_array(res, part["trace"].shape[1])), f"{what}: another path"
    assert np.array_equal(part["basis"], res["basis"]), what
    assert np.array_equal(part["col_of_row"], res["col_of_row"]), f"{what}: rows {part['col_of_row']}, the oracle's {res['col_of_row']}"


def oracle(g, k, R, S, max_pivots=None, **kw):
    return sg.run(*g["lps"][k], g["max_pivots"] if max_pivots is None else max_pivots, R, S, **kw)


# ---------------------------------------------------------------------------------------------------
# both guards off: the bits of mllp_basis_simplex
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["edge", "threshold"])
def test_guards_off_gives_the_plain_bits(case, request):
    g = request.getfixturevalue(case)
    want = ts._bits(ts._host(ts.run(g)))
    got = abi_run(g, 0, 0)
    assert not got.pop("guard").any()
    same_bits(ts._bits(got), want, f"{case}: mllp_basis_simplex_guarded(0, 0) against mllp_basis_simplex")
    res = run(g, 0, 0)
    assert res.guard is None                    # LPBatch.simplex with both 0: the plain call
    same_bits(ts._bits(ts._host(res)), want, f"{case}: LPBatch.simplex(refactor_every=0, stall_pivots=0)")


# ---------------------------------------------------------------------------------------------------
# Chvatal and Beale
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def textbook(LPBatch):  # noqa: F811
    lps = [(d["A"], d["b"], d["c"], d["start"]) for d in (sg.CHVATAL, sg.BEALE)]
    return dict(dense_batch(LPBatch, lps, 60), objective=[sg.CHVATAL["objective"], sg.BEALE["objective"]])


def test_the_cycling_examples_end_optimal(textbook):
    g = textbook
    plain = ts._host(ts.run(g))
    for k, name in enumerate(("Chvatal", "Beale")):
        print(f"{name}: mllp_basis_simplex with 60 pivots answers {list(plain['status'][k])}, basis {np.flatnonzero(ts._inst(g['c'], plain, k)['basis'])}")
    res = run(g, 0, 3)
    h = _host(res)
    for k, name in enumerate(("Chvatal", "Beale")):
        part = _inst(g["c"], h, k)
        print(f"{name}: stall_pivots 3 answers {list(part['status'][0])}, guard {list(part['guard'][0])}, trace {part['trace'][0][:8].tolist()}")
        assert part["status"][0, 0] == 0 and list(np.flatnonzero(part["basis"])) == [0, 2, 4], (name, part["status"][0])
        assert part["guard"][0, 0] == 0 and part["guard"][0, 1] > 0
        ts.check_trace_shape(part, name)
    got = g["b"].simplex_solved(res, 1e-3, 1e-3)
    assert bool(got["optimal"].all()) and bool(got["usable"].all())
    x = g["b"].solve_basis(res.basis, want=("basis", "x", "y")).x.cpu().numpy().astype(np.float64)
    for k in range(2):
        s = slice(g["c"]["ptr_n"][k], g["c"]["ptr_n"][k + 1])
        assert abs(g["x1"][s].astype(np.float64) @ x[s] - g["objective"][k]) <= 1e-4 * max(1.0, abs(g["objective"][k]))


# ---------------------------------------------------------------------------------------------------
# trace parity with the fp64 oracle on guarded seeds of the degenerate family
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,S", list(BLAND_P))
def test_trace_parity(LPBatch, R, S):  # noqa: F811
    seeds = BLAND_P[R, S] + NO_BLAND[R, S]
    g = dense_batch(LPBatch, [sg.family(s) for s in seeds])
    want = [oracle(g, k, R, S) for k in range(len(seeds))]
    for seed, res in zip(seeds, want):      # the condition, from the oracle alone
        assert sg.guarded(res, TOL) and res["code"] == 0, f"seed {seed}: {min(res['margins'], key=lambda t: t[1])}"
        assert (res["bland"][1] > 0 and res["bland"][0] == 0) if seed in BLAND_P[R, S] else res["guard"][1] == 0
    assert sum(r["bland"][1] > 0 for r in want) >= 8 and sum(r["guard"][1] == 0 for r in want) >= 4
    h = _host(run(g, R, S))
    for k, (seed, res) in enumerate(zip(seeds, want)):
        print(f"(R, S) = ({R}, {S}), seed {seed}: the oracle's status {res['status']}, guard {res['guard']}; the device's "
              f"{list(h['status'][k])}, {list(h['guard'][k])}")
    for k, (seed, res) in enumerate(zip(seeds, want)):
        check_against_oracle(g["c"], h, k, res, f"(R, S) = ({R}, {S}), seed {seed}")


def test_the_pivot_limit_on_the_guarded_path(LPBatch):  # noqa: F811
    """max_pivots below the run's length: code 6 and the oracle's first max_pivots steps, the guard counted up to there"""
    R, S = 3, 1
    g = dense_batch(LPBatch, [sg.family(s) for s in BLAND_P[R, S][:4]])
    for cap in (3, 2):
        want = [oracle(g, k, R, S, max_pivots=cap) for k in range(4)]
        assert all(sg.guarded(r, TOL) for r in want) and sum(r["code"] == 6 for r in want) >= 2    # (3: right after a refactorization)
        h = _host(run(g, R, S, max_pivots=cap))
        for k, res in enumerate(want):
            check_against_oracle(g["c"], h, k, res, f"max_pivots {cap}, instance {k}")


# ---------------------------------------------------------------------------------------------------
# Bland pivots in stage D: rule-independent
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,S", sorted({(R, S) for _, R, S in STAGE_D}))
def test_stage_d_bland_reaches_the_optimum(LPBatch, R, S):  # noqa: F811
    seeds = [s for s, r, t in STAGE_D if (r, t) == (R, S)]
    g = dense_batch(LPBatch, [sg.family(s) for s in seeds])
    want = [oracle(g, k, R, S) for k in range(len(seeds))]
    assert all(r["code"] == 0 and r["bland"][0] > 0 for r in want)
    res = run(g, R, S)
    h = _host(res)
    got = g["b"].simplex_solved(res, 1e-3, 1e-3)
    x = g["b"].solve_basis(res.basis, want=("basis", "x", "y")).x.cpu().numpy().astype(np.float64)
    for k, seed in enumerate(seeds):
        A, b, c, _ = g["lps"][k]
        cols = np.flatnonzero(want[k]["basis"])
        obj = float(c[cols] @ np.linalg.solve(A[:, cols], b))
        s = slice(g["c"]["ptr_n"][k], g["c"]["ptr_n"][k + 1])
        mine = float(c @ x[s])
        print(f"seed {seed}: status {list(h['status'][k])}, guard {list(h['guard'][k])}; objective {mine}, the oracle's {obj}")
        assert h["status"][k, 0] == 0 and bool(got["optimal"][k]), (seed, h["status"][k])
        assert abs(mine - obj) <= 1e-4 * max(1.0, abs(obj))


# ---------------------------------------------------------------------------------------------------
# refactorization: device against device
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted_40(LPBatch):  # noqa: F811
    return ts.planted_case(LPBatch, [(40, 100)], 40, [12], 200)


@pytest.mark.parametrize("case", ["threshold", "planted_40"])
def test_rows_after_a_refactorization_are_solve_basis_rows(case, request):
    """R = 8.  The full allowance: code 0 at the planted labels, certified.  A max_pivots that is a multiple of 8 below every
    instance's run: code 6 right after a refactorization, where col_of_row is what a fresh solve_basis of that basis assigns
    (the same list, the same rule -- two kernels), and guard counts max_pivots / 8 refactorizations."""
    g = request.getfixturevalue(case)
    full = run(g, 8, 0)
    h = ts.check_rule_independent(g, full, f"{case}, R = 8")
    guard = full.guard.cpu().numpy()
    length = h["status"][:, 1] + h["status"][:, 2]
    assert np.array_equal(guard[:, 0], length // 8) and not guard[:, 1].any()
    cap = 8 * int((length.min() - 1) // 8)
    assert cap >= 8, f"{case}: the shortest run has {length.min()} pivots: no refactorization to stop behind"
    res = run(g, 8, 0, max_pivots=cap)
    hc = _host(res)
    assert (hc["status"][:, 0] == 6).all() and (hc["status"][:, 1] + hc["status"][:, 2] == cap).all()
    assert (hc["guard"][:, 0] == cap // 8).all()
    fresh = g["b"].solve_basis(res.basis, tol=TOL, want=("basis", "col_of_row"))
    assert (fresh.status[:, 3] == 0).all()
    assert np.array_equal(hc["col_of_row"], fresh.col_of_row.cpu().numpy()), f"{case}: rows after the refactorization"
    assert np.array_equal(hc["basis"], fresh.basis.cpu().numpy())
    print(f"{case}: stopped after {cap} pivots and {cap // 8} refactorizations; runs of {length.tolist()} pivots")


# ---------------------------------------------------------------------------------------------------
# an instance alone gives the bits it gives inside the batch
# ---------------------------------------------------------------------------------------------------
def test_instance_independence(LPBatch, textbook):  # noqa: F811
    R, S = 3, 1
    seeds = BLAND_P[R, S][:3] + (120,)
    lps = [sg.family(s) for s in seeds] + textbook["lps"]
    g = dense_batch(LPBatch, lps)
    h = _host(run(g, R, S))
    for k in (0, 3, 4):
        one = dense_batch(LPBatch, [lps[k]])
        h1 = _host(run(one, R, S))
        same_bits(ts._bits(h1), ts._bits(_inst(g["c"], h, k)), f"instance {k} alone against inside the batch")
    g2 = ts.planted_case(LPBatch, [(5, 12), (ts.LDS_MAX + 1, ts.N_T)], 40, [2, 4], 200)      # T in scratch beside T in LDS
    h2 = _host(run(g2, 8, 2))
    one = ts.planted_case(LPBatch, [(5, 12)], 40, [2], 200)
    same_bits(ts._bits(_host(run(one, 8, 2))), ts._bits(_inst(g2["c"], h2, 0)), "5 x 12 alone against beside a scratch instance")


# ---------------------------------------------------------------------------------------------------
# code 7, and the codes of the plain entry point
# ---------------------------------------------------------------------------------------------------
def test_a_basis_that_cannot_be_refactorized(LPBatch):  # noqa: F811
    """tol = 0.5, R = 1 on seeds found by a CPU search: the refactorization rejects a column, code 7.  The oracle's walks
    keep every ratio 2^-6 (relative) away from tol, and its margins are guarded: then the device's decisions are the oracle's."""
    tol, seeds = 0.5, (6, 38, 58)
    g = dense_batch(LPBatch, [sg.family(s) for s in seeds])
    want = [oracle(g, k, 1, 0, tol=tol) for k in range(len(seeds))]
    for seed, res in zip(seeds, want):
        rat = np.concatenate([np.asarray(res["start_ratios"], float)] + [np.asarray(r, float) for r in res["refactor_ratios"]])
        assert res["code"] == 7 and res["margin"] >= sg.GUARD and (np.abs(rat - tol) >= sg.GUARD * tol).all(), seed
    h = _host(run(g, 1, 0, tol=tol))
    for k, (seed, res) in enumerate(zip(seeds, want)):
        check_against_oracle(g["c"], h, k, res, f"seed {seed}")
        part = _inst(g["c"], h, k)
        assert (part["col_of_row"] == -1).all() and part["basis"].sum() == 6 and part["status"][0, 3] == 6
        ts.check_trace_shape(part, f"seed {seed}")


def test_the_plain_codes_with_the_guard_written(edge):  # noqa: F811
    """codes 1, 2, 3, 4, 5 (and 0) of the edge instances answer as on mllp_basis_simplex, and d_guard is written over its
    poison: zeros for codes 1, 2 and 3"""
    g = dict(edge, lps=[(edge["mats"][k], edge["x2"][edge["c"]["ptr_m"][k]:edge["c"]["ptr_m"][k + 1]],
                         edge["x1"][edge["c"]["ptr_n"][k]:edge["c"]["ptr_n"][k + 1]],
                         edge["start"][edge["c"]["ptr_n"][k]:edge["c"]["ptr_n"][k + 1]]) for k in range(9)])
    c = g["c"]
    R, S = 3, 2
    want = [oracle(g, k, R, S) for k in range(9)]
    assert [r["status"] for r in want[:8]] == [r["status"] for r in edge["oracle"][:8]]
    assert [r["code"] for r in want] == [4, 5, 0, 1, 1, 0, 3, 3, 0]
    h = abi_run(g, R, S)
    for k in range(8):
        check_against_oracle(c, h, k, want[k], f"edge instance {k}")
        if want[k]["code"] in (1, 2, 3):
            part = _inst(c, h, k)
            assert not part["basis"].any() and (part["col_of_row"] == -1).all() and (part["trace"] == -1).all()
            assert not part["guard"].any()
    assert h["status"][8, 0] == 0
    h5 = abi_run(g, R, S, max_m=5)
    part = _inst(c, h5, 8)
    assert list(part["status"][0]) == [2, 0, 0, 0] and not part["basis"].any() and (part["col_of_row"] == -1).all()
    assert (part["trace"] == -1).all() and not part["guard"].any()
    for k in range(8):
        same_bits(ts._bits(_inst(c, h5, k)), ts._bits(_inst(c, h, k)), f"instance {k} beside a skipped one")
    # beyond the row limit nothing runs, as on the plain entry point
    h0 = abi_run(g, R, S, max_m=0)
    assert [int(v) for v in h0["status"][:, 0]] == [2, 2, 2, 2, 2, 0, 2, 2, 2] and not h0["guard"].any()


# ---------------------------------------------------------------------------------------------------
# driver
# ---------------------------------------------------------------------------------------------------
def test_driver_passes_refactor_and_stall(tmp_path, monkeypatch):
    """`report_solved: {..., pivots: 50, refactor: 8, stall: 2}`: the two reach LPBatch.simplex and the log has the keys of
    `pivots`; without them the call has neither keyword"""
    from mllp_amd import experiment
    from mllp_amd.graph import LPBatch as cls
    seen = []
    plain = cls.simplex

    def spy(self, *a, **kw):
        seen.append({k: kw[k] for k in ("refactor_every", "stall_pivots") if k in kw})
        res = plain(self, *a, **kw)
        seen[-1]["guard"] = res.guard is not None
        return res
    monkeypatch.setattr(cls, "simplex", spy)
    cfg = ("train_data_type: 'planted'\ntrain_lr: 1.e-3\ntrain_iter: 2\nmethods:\n  - 'gs-topk'\nbatch_size: 3\nholdout: 0.25\n"
           "planted: {instances: 8, m: 20, n: 50, row_nnz: 4, seed: 5}\n")
    base = {"obj", "val_obj", "usable", "feasible", "optimal", "skipped", "optimal_after_pivots", "pivots"} | {f"planted{5 + i}" for i in range(8)}
    for block, want in (("report_solved: {feas_tol: 1.e-3, opt_tol: 1.e-3, max_m: 20, pivots: 50, refactor: 8, stall: 2}\n",
                         dict(refactor_every=8, stall_pivots=2, guard=True)),
                        ("report_solved: {feas_tol: 1.e-3, opt_tol: 1.e-3, max_m: 20, pivots: 50}\n", dict(guard=False))):
        del seen[:]
        (tmp_path / "cfg.yaml").write_text(cfg + block)
        monkeypatch.chdir(tmp_path)
        assert experiment.main(["--cfg", str(tmp_path / "cfg.yaml")]) == 0
        log = json.load(open(tmp_path / "train_log.json"))
        assert set(log) == base
        assert seen and all(s == want for s in seen), seen
        for e in range(2):
            done, pivots = log["optimal_after_pivots"][e], log["pivots"][e]
            print(f"{want}: epoch {e}: after at most 50 pivots {done} of 2 optimal, {pivots} pivots in all")
            assert 0 <= done <= 2 and 0 <= pivots <= 50 * done


# ---------------------------------------------------------------------------------------------------
# optional output, reproducibility, memory contract
# ---------------------------------------------------------------------------------------------------
def test_memory_contract(threshold):  # noqa: F811
    """R = 8, S = 2 on both sides of the LDS threshold.  d_guard NULL gives the other outputs' bits; two runs are equal;
    guard bands around every caller buffer stay intact and inputs are not written; outputs and scratch poisoned with zeros,
    NaN or the largest float give the same bits; refused calls leave the poison untouched."""
    g = threshold
    c, b = g["c"], g["b"]
    R, S = 8, 2
    K, mp, max_m = len(c["inst_m"]), g["max_pivots"], max(c["inst_m"])
    full = abi_run(g, R, S)
    same_bits(ts._bits(abi_run(g, R, S)), ts._bits(full), "a second run")
    same_bits(ts._bits(abi_run(g, R, S, guard=False)), {k: v for k, v in ts._bits(full).items() if k != "guard"}, "d_guard NULL")
    same_bits(ts._bits(_host(run(g, R, S))), ts._bits(full), "LPBatch.simplex against the C ABI")
    assert (full["status"][:, 0] == 0).all() and (full["guard"][:, 0] > 0).all()
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
                    status=Guarded(4 * K, torch.int32, "cuda", fill=fill, name="status", shift=4),
                    guard=Guarded(2 * K, torch.int32, "cuda", fill=fill, name="guard", shift=12))
        scratch = Guarded(n.value // 4, device="cuda", fill=fill, name="scratch", shift=4)
        ptrs = {k: v.ptr for k, v in outs.items()}
        ok = dict(x1=ins["x1"].ptr, x2=ins["x2"].ptr, start=ins["start"].ptr, scratch=scratch.ptr, max_m=max_m)
        before = {k: v.bits() for k, v in outs.items()}
        before["scratch"] = scratch.bits()
        bad = [dict(h=None), dict(x1=nul), dict(x2=nul), dict(start=nul), dict(bufs={**ptrs, "basis": nul}),
               dict(bufs={**ptrs, "status": nul}), dict(scratch=nul), dict(tol=float("nan")), dict(tol=-1.0), dict(ftol=0.0),
               dict(dtol=float("inf")), dict(ptol=-1.0), dict(dshift=float("nan")), dict(max_pivots=-1), dict(max_m=-1),
               dict(refactor=-1), dict(stall=-1)]
        for kw in bad:
            args = dict(ok, **kw)
            assert _abi_call(b, g, args.pop("bufs", ptrs), R, S, **args) == EINVAL, kw
            assert b"mllp_basis_simplex_guarded" in _lib.lib().mllp_last_error()
        torch.cuda.synchronize()
        after = {k: v.bits() for k, v in outs.items()}
        after["scratch"] = scratch.bits()
        same_bits(after, before, f"buffers after the refused calls ({name} poison)")
        assert _abi_call(b, g, ptrs, R, S, **ok) == 0
        torch.cuda.synchronize()
        for v in list(ins.values()) + list(outs.values()) + [scratch]:
            v.check()
        runs[name] = {k: v.bits() for k, v in outs.items()}
    for name in runs:
        same_bits(runs[name], runs["zero"], f"outputs under {name} poison against zero poison")
    same_bits(runs["nan"], ts._bits(full), "the guarded buffers against plain ones")
