"""GPU: mllp_lp_pdhg (restarted PDHG on the resident batch; csrc/pdhg.hip) against the numpy oracle of THE RULE
(tests/pdhg_oracle.py), on planted LPs (tests/test_basis_repair.planted_shapes / _planted: the device plants them, the
oracle gets what the batch stores).

THE BAR (tests 1 and 2) is not tuned to the kernel.  It is 8 x the larger deviation, over the instances of test 1 at that
iteration count K, between the fp64 oracle and THE SAME oracle run in numpy fp32 -- both CPU code --, in units of
2^-24 max|x| (max|y|) of the instance.  That deviation is what fp32 costs this iteration in one summation order (scipy's:
a row's terms one after the other); the 8 covers the device's lane-strided order, inside the same error class.
Measured, oracle against oracle (the test computes and prints the figures on the data the device planted):
    K = 64:  13.01 units on the device-planted data (13.65 on the fp64-planted data of tools/bench_pdhg.py)  -> bar 104 units
    K = 512: 22.93 units (22.17)                                                                              -> bar 183 units
Test 2 scales the K = 512 bar by iterations / 512.  The device, for the record (one MI355X): at most 5.6 units at K = 64 and
18.2 at K = 512 (y of 5 x 12); 18.6 units on the guarded traces (x of 193 x 400 after 1536 iterations, bar 550).

THE GUARD (test 2).  Status equality with the oracle is asked only of instances whose ORACLE margin (the smallest relative
distance of any comparison a check takes from a tie) is at least 2^-7, asserted before the device is looked at.  Seeds of
planted_oracle._instance(m, n, 4.0, seed) that qualify: 5 x 12: 20, 22, 26, 27, 29-34, ...; 40 x 100: 24, 25, 28, 30, 32-34;
193 x 400: 20, 21, 27, 42, 44.  Used: 26 (margin 0.108), 30 (0.128), 42 (0.092).
"""
import ctypes

import numpy as np
import pytest
import torch

import pdhg_oracle as pg
import planted_oracle as po
import test_basis_repair as tb
from guarded import same_bits
from mllp_amd import _lib
from test_basis_repair import LPBatch  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EPS = 2.0 ** -10
EINVAL = -1
TRACE = [((5, 12), 26), ((40, 100), 30), ((193, 400), 42)]
SPLIT_WORDS = 400           # 3 n + 2 m: 46, 380 (LDS) and 1586 (scratch)


def _batch(LPBatch, c):
    b, _, st = tb._planted(LPBatch, c)
    return dict(c=c, b=b, st=st, insts=pg.split(c, st["values"], st["x1"], st["x2"], st["labels"]))


def _host(res):
    torch.cuda.synchronize()
    return {k: getattr(res, k).cpu().numpy() for k in ("x", "y", "status", "kkt")}


def _bits(h):
    return {k: np.ascontiguousarray(v).view(np.int32).reshape(-1).copy() for k, v in h.items()}


def _part(c, h, k):
    s, r = slice(c["ptr_n"][k], c["ptr_n"][k + 1]), slice(c["ptr_m"][k], c["ptr_m"][k + 1])
    return dict(x=h["x"][s], y=h["y"][r], status=h["status"][k], kkt=h["kkt"][k])


def _units(got, want):
    scale = np.abs(want).max(initial=0.0)
    return 0.0 if scale == 0.0 else float(np.abs(np.asarray(got, np.float64) - want).max() / (U * scale))


def _kkt_close(inst, x, y, got, what):
    """the device's three errors of its own output against the fp64 recomputation, within the bound of a device sum
    (planted_oracle.row_bound: (L + 3) u sum |terms|) carried through each quotient"""
    A, b, c = inst["A"], inst["b"], inst["c"]
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    want = pg.errors64(A, b, c, x, y)
    absA = abs(A)
    rows = po.row_bound(np.diff(A.indptr), absA @ np.abs(x) + np.abs(b)).max(initial=0.0) / (1 + np.abs(b).max(initial=0.0))
    cols = po.row_bound(np.diff(A.tocsc().indptr), absA.T @ np.abs(y) + np.abs(c)).max(initial=0.0) / (1 + np.abs(c).max(initial=0.0))
    cx, by = float(c @ x), float(b @ y)
    dots = po.row_bound(len(x), np.abs(c * x).sum()) + po.row_bound(len(y), np.abs(b * y).sum())
    gap = 2 * dots / (1 + abs(cx) + abs(by)) + 4 * U * want[2]
    for name, g, w, bound in zip(("primal", "dual", "gap"), got[:3], want, (rows, cols, gap)):
        assert abs(float(g) - w) <= bound + 4 * U * w, (what, name, float(g), w, bound)


@pytest.fixture(scope="module")
def plain(LPBatch):
    """the five shapes of test 1 in one batch, and per K the two oracle runs of every instance"""
    g = _batch(LPBatch, pg.join_cases([tb.planted_shapes([(1, 1), (3, 3), (5, 12), (40, 100)], 20), po.ragged_case(which=[4])]))
    g["runs"], g["dev"] = {}, {}
    for K in (64, 512):
        g["runs"][K] = [(pg.solve(i["A"], i["b"], i["c"], K, check_every=0), pg.solve(i["A"], i["b"], i["c"], K, check_every=0, dtype=np.float32))
                        for i in g["insts"]]
        g["dev"][K] = max(max(_units(f["x"], a["x"]), _units(f["y"], a["y"])) for a, f in g["runs"][K])
        print(f"K = {K}: fp32 oracle against fp64 oracle, largest deviation {g['dev'][K]:.2f} units -> bar {8 * g['dev'][K]:.1f}")
    return g


@pytest.fixture(scope="module")
def trace(LPBatch):
    """the three guarded instances in one batch, the oracle's run of each, the device's run"""
    g = _batch(LPBatch, pg.join_cases([tb.planted_shapes([shape], seed) for shape, seed in TRACE]))
    g["oracle"] = [pg.solve(i["A"], i["b"], i["c"], 8192, eps=EPS) for i in g["insts"]]
    for o in g["oracle"]:                          # the condition, from the oracle alone
        assert o["margin"] >= 2.0 ** -7 and o["status"][0] == 0, (o["status"], o["margin"])
    g["res"] = g["b"].pdhg(8192, eps=EPS, check_every=64)
    g["host"] = _host(g["res"])
    return g


# ---------------------------------------------------------------------------------------------------
# 1. plain parity
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [64, 512])
def test_plain_iterations_against_the_oracle(plain, K):
    c, b = plain["c"], plain["b"]
    bar = 8.0 * plain["dev"][K]
    assert 8.0 <= bar <= 8.0 * 64.0, f"the fp32 oracle is {plain['dev'][K]} units from the fp64 one: not the measured class"
    h = _host(b.pdhg(K, check_every=0))
    for k, (a, _) in enumerate(plain["runs"][K]):
        got = _part(c, h, k)
        assert list(got["status"]) == [6, K, 0, 0], (k, got["status"])
        ux, uy = _units(got["x"], a["x"]), _units(got["y"], a["y"])
        print(f"K = {K}, instance {k} ({c['inst_m'][k]} x {c['inst_n'][k]}): x {ux:.2f} units, y {uy:.2f} units, bar {bar:.1f}")
        assert ux <= bar and uy <= bar, (K, k, ux, uy, bar)
        assert got["kkt"][3] == pytest.approx(a["eta"], rel=4 * U)
        _kkt_close(plain["insts"][k], got["x"], got["y"], got["kkt"], f"K = {K}, instance {k}")


# ---------------------------------------------------------------------------------------------------
# 2. trace parity, guarded;  3. what holds of any run that converges
# ---------------------------------------------------------------------------------------------------
def test_the_trace_of_guarded_instances(plain, trace):
    c, h = trace["c"], trace["host"]
    for k, o in enumerate(trace["oracle"]):
        got = _part(c, h, k)
        print(f"instance {k}: oracle {o['status']} margin {o['margin']:.4f}, device {list(got['status'])}")
        assert list(got["status"]) == o["status"], (k, got["status"], o["status"])
        bar = 8.0 * plain["dev"][512] * max(o["status"][1] / 512.0, 1.0)
        ux, uy = _units(got["x"], o["x"]), _units(got["y"], o["y"])
        print(f"instance {k}: x {ux:.2f} units, y {uy:.2f} units, bar {bar:.1f}")
        assert ux <= bar and uy <= bar, (k, ux, uy, bar)


def _converged(g, h, what):
    """the rule-independent assertions on a run `h` of the batch `g` that is expected to converge everywhere"""
    c, b = g["c"], g["b"]
    for k, inst in enumerate(g["insts"]):
        got = _part(c, h, k)
        code, it, restarts, avg = got["status"]
        assert code == 0 and it % 64 == 0 and 0 < it <= 8192 and avg in (0, 1) and restarts >= 0, (what, k, got["status"])
        errs = pg.errors64(inst["A"], inst["b"], inst["c"], got["x"], got["y"])
        assert max(errs) <= EPS * (1 + 2.0 ** -6), (what, k, errs)
        assert (got["x"] >= 0).all()


def test_a_converged_run_is_optimal_and_points_at_the_planted_vertex(trace):
    c, b, h = trace["c"], trace["b"], trace["host"]
    _converged(trace, h, "trace batch")
    rep = b.pdhg_basis(trace["res"])
    solved = b.solved(rep, 1e-3, 1e-3)
    torch.cuda.synchronize()
    assert list(rep.status[:, 0].cpu().numpy()) == list(c["inst_m"]) and (rep.status[:, 3] == 0).all()
    assert np.array_equal(rep.basis.cpu().numpy(), trace["st"]["labels"])
    assert solved["optimal"].all() and solved["primal_feasible"].all()


# ---------------------------------------------------------------------------------------------------
# 4. the same bits
# ---------------------------------------------------------------------------------------------------
def _scratch_bytes(b, words):
    n = ctypes.c_int64(-1)
    _lib.check(_lib.lib().mllp_lp_pdhg_scratch_bytes(b._h, words, ctypes.byref(n)))
    return n.value


def test_same_bits_in_lds_in_scratch_alone_and_twice(LPBatch, trace):
    from mllp_amd.graph import pdhg_limits
    c, b, st = trace["c"], trace["b"], trace["st"]
    words = [3 * n + 2 * m for m, n in zip(c["inst_m"], c["inst_n"])]
    assert _scratch_bytes(b, pdhg_limits()[0]) == 0 and _scratch_bytes(b, 0) == 4 * sum(words)
    assert _scratch_bytes(b, SPLIT_WORDS) == 4 * sum(w for w in words if w > SPLIT_WORDS) > 0
    assert _scratch_bytes(b, SPLIT_WORDS) < 4 * sum(words)
    want = _bits(trace["host"])
    for lds in (None, 0, SPLIT_WORDS):
        same_bits(_bits(_host(b.pdhg(8192, eps=EPS, check_every=64, max_lds_words=lds))), want, f"max_lds_words = {lds}")
    # every instance alone (a batch of its own from the values, costs and right-hand sides the batch stores)
    for k, (shape, seed) in enumerate(TRACE):
        s, r = slice(c["ptr_n"][k], c["ptr_n"][k + 1]), slice(c["ptr_m"][k], c["ptr_m"][k + 1])
        ck = dict(tb.planted_shapes([shape], seed), val=st["values"][c["nnz_off"][k]:c["nnz_off"][k + 1]])
        alone = tb._build(LPBatch, ck, tb._dev(st["x1"][s]), tb._dev(st["x2"][r]), tb._dev(st["labels"][s]))
        for lds in (None, 0):
            got = _bits(_host(alone.pdhg(8192, eps=EPS, check_every=64, max_lds_words=lds)))
            same_bits(got, _bits(_part(c, trace["host"], k)), f"instance {k} alone, max_lds_words = {lds}")


# ---------------------------------------------------------------------------------------------------
# 5. starts and limits
# ---------------------------------------------------------------------------------------------------
def test_starts_and_limits(trace):
    c, b, st = trace["c"], trace["b"], trace["st"]
    K = len(c["inst_m"])
    xstar, ystar = tb._dev(c["xstar"] * st["labels"]), tb._dev(c["ystar"])
    warm = _host(b.pdhg(8192, eps=EPS, x0=xstar, y0=ystar))
    assert [list(s) for s in warm["status"][:, :3]] == [[0, 64, 0]] * K, warm["status"]
    rep = b.solve_basis(b.labels)
    from_rep = _host(b.pdhg(8192, eps=EPS, start=rep))
    assert [list(s) for s in from_rep["status"][:, :3]] == [[0, 64, 0]] * K, from_rep["status"]
    with pytest.raises(ValueError):
        b.pdhg(64, start=rep, x0=xstar)
    # a start with negative entries is the clipped start
    rng = np.random.default_rng(7)
    x0, y0 = rng.uniform(-1.0, 1.0, c["N"]).astype(np.float32), rng.uniform(-1.0, 1.0, c["M"]).astype(np.float32)
    neg = _bits(_host(b.pdhg(256, eps=EPS, x0=tb._dev(x0), y0=tb._dev(y0))))
    same_bits(neg, _bits(_host(b.pdhg(256, eps=EPS, x0=tb._dev(np.maximum(x0, 0)), y0=tb._dev(y0)))), "x0 against max(x0, 0)")
    zero = _host(b.pdhg(0, eps=EPS, x0=tb._dev(x0), y0=tb._dev(y0)))
    assert [list(s) for s in zero["status"]] == [[6, 0, 0, 0]] * K
    assert np.array_equal(zero["x"], np.maximum(x0, 0)) and np.array_equal(zero["y"], y0)
    for k, inst in enumerate(trace["insts"]):      # ... and its three errors are evaluated
        got = _part(c, zero, k)
        _kkt_close(inst, got["x"], got["y"], got["kkt"], f"max_iters = 0, instance {k}")
    odd = _host(b.pdhg(100, eps=0.0, check_every=64))
    assert [list(s[:2]) for s in odd["status"]] == [[6, 100]] * K and (odd["status"][:, 2] == 1).all()
    # +inf in b of instance 1: code 8 there, the other instances' bits as ever
    clean = _host(b.pdhg(1024, eps=EPS))
    keep = b.x2.clone()
    try:
        b.x2[c["ptr_m"][1]] = float("inf")
        b.invalidate_inputs()
        bad = _host(b.pdhg(1024, eps=EPS))
    finally:
        b.x2.copy_(keep)
        b.invalidate_inputs()
    assert list(bad["status"][1][:3]) == [8, 64, 0], bad["status"]
    for k in (0, 2):
        same_bits(_bits(_part(c, bad, k)), _bits(_part(c, clean, k)), f"instance {k} beside a non-finite one")


def test_every_refusal_writes_nothing(trace):
    c, b = trace["c"], trace["b"]
    K, L, z = len(c["inst_m"]), _lib.lib(), ctypes.c_void_p(0)
    poison = lambda n: torch.full((n,), float("nan"), device="cuda")      # noqa: E731
    bufs = dict(x=poison(c["N"] + 8), y=poison(c["M"]), status=poison(4 * K).view(torch.int32), kkt=poison(4 * K), scratch=poison(c["N"] * 3 + c["M"] * 2))
    x0, y0 = tb._dev(np.ones(c["N"], np.float32)), tb._dev(np.ones(c["M"], np.float32))
    ok = dict(g=b._h, x1=_lib.ptr(b.x1), x2=_lib.ptr(b.x2), x0=_lib.ptr(x0), y0=_lib.ptr(y0), max_iters=128, check_every=64, eps=EPS, step=0.9,
              beta=0.5, lds=0, x=_lib.ptr(bufs["x"]), y=_lib.ptr(bufs["y"]), status=_lib.ptr(bufs["status"]), kkt=_lib.ptr(bufs["kkt"]),
              scratch=_lib.ptr(bufs["scratch"]))
    order = ("g", "x1", "x2", "x0", "y0", "max_iters", "check_every", "eps", "step", "beta", "lds", "x", "y", "status", "kkt", "scratch")
    nan, inf = float("nan"), float("inf")
    bad = [dict(g=None), dict(x1=z), dict(x2=z), dict(x=z), dict(y=z), dict(status=z), dict(max_iters=-1), dict(check_every=-1), dict(lds=-1),
           dict(eps=nan), dict(eps=inf), dict(eps=-1.0), dict(step=nan), dict(step=inf), dict(step=0.0), dict(step=-0.5), dict(step=1.5),
           dict(beta=nan), dict(beta=inf), dict(beta=0.0), dict(beta=1.0), dict(beta=-0.5), dict(scratch=z),
           dict(x0=_lib.ptr(bufs["x"])), dict(y0=_lib.ptr(bufs["y"])), dict(x0=ctypes.c_void_p(bufs["x"].data_ptr() + 32)),
           dict(y0=_lib.ptr(bufs["kkt"])), dict(x0=_lib.ptr(bufs["status"]))]
    before = {k: v.view(torch.int32).cpu().numpy().copy() for k, v in bufs.items()}
    for kw in bad:
        args = dict(ok, **kw)
        assert L.mllp_lp_pdhg(*[args[k] for k in order], _lib.current_stream()) == EINVAL, kw
        assert b"mllp_lp_pdhg" in L.mllp_last_error(), kw
    torch.cuda.synchronize()
    same_bits({k: v.view(torch.int32).cpu().numpy() for k, v in bufs.items()}, before, "buffers after the refused calls")
    # the same arguments without a fault are accepted (kkt may be NULL, and so may the scratch when nothing needs it)
    assert L.mllp_lp_pdhg(*[dict(ok, kkt=z, eps=0.0)[k] for k in order], _lib.current_stream()) == 0
    from mllp_amd.graph import pdhg_limits
    assert L.mllp_lp_pdhg(*[dict(ok, scratch=z, eps=0.0, lds=pdhg_limits()[0])[k] for k in order], _lib.current_stream()) == 0
    torch.cuda.synchronize()
    assert (bufs["status"].view(K, 4)[:, 0] == 6).all() and torch.isnan(bufs["kkt"]).sum() == 0


def test_an_empty_instance_and_an_empty_side(LPBatch):
    """n = 0 or m = 0 is legal: no rows leaves x to the costs alone (eta = step), no columns leaves y to b alone"""
    c = tb.dense_case([np.zeros((0, 3)), tb.int_matrix(3, 6, 0.7, 12), np.zeros((2, 0))], 1)
    c["c"][:3] = [1.0, 2.0, 0.0]
    b = tb._build(LPBatch, c, tb._dev(c["c"]), tb._dev(c["b"]))
    h = _host(b.pdhg(128, eps=EPS, x0=tb._dev(np.ones(c["N"], np.float32))))
    assert list(h["status"][0][:2]) == [0, 64] and np.array_equal(h["x"][:3], [0.0, 0.0, 1.0]) and h["kkt"][0][3] == np.float32(0.9)
    assert h["status"][2][1] in (64, 128) and h["status"][2][0] in (0, 6) and np.isfinite(h["kkt"]).all()
    mid = pg.solve(c["mats"][1], c["b"][:3], c["c"][3:9], 128, eps=EPS, x0=np.ones(6))
    assert list(h["status"][1][:2]) == mid["status"][:2] or mid["margin"] < 2.0 ** -7


# ---------------------------------------------------------------------------------------------------
# driver
# ---------------------------------------------------------------------------------------------------
def test_driver_reports_pdhg(tmp_path, monkeypatch):
    """8 planted instances, a quarter held out, `report_solved` with a `pdhg` block: the log gains the three counts per
    epoch, over the two held-out instances.  PDHG has no row limit, so max_m bounds only the vertex check behind
    `optimal_after_pdhg`: with max_m below m nothing can be certified."""
    import json
    from mllp_amd import experiment
    cfg = ("train_data_type: 'planted'\ntrain_lr: 1.e-3\ntrain_iter: 2\nmethods:\n  - 'gs-topk'\nbatch_size: 3\nholdout: 0.25\n"
           "planted: {instances: 8, m: 20, n: 50, row_nnz: 4, seed: 5}\n")
    base = {"obj", "val_obj", "usable", "feasible", "optimal", "skipped"} | {f"planted{5 + i}" for i in range(8)}
    for block, max_m in (("pdhg: {iters: 4096, eps: 1.e-3}", 20), ("pdhg: {iters: 4096, eps: 1.e-3, check: 32, warm: false}", 20),
                         ("pdhg: {iters: 128, eps: 1.e-3}", 19)):
        (tmp_path / "cfg.yaml").write_text(cfg + f"report_solved: {{feas_tol: 1.e-3, opt_tol: 1.e-3, max_m: {max_m}, {block}}}\n")
        monkeypatch.chdir(tmp_path)
        assert experiment.main(["--cfg", str(tmp_path / "cfg.yaml")]) == 0
        log = json.load(open(tmp_path / "train_log.json"))
        assert set(log) == base | set(experiment.PDHG_KEYS)
        for e in range(2):
            conv, its, opt = (log[k][e] for k in experiment.PDHG_KEYS)
            print(block, max_m, "epoch", e, "converged", conv, "iterations", its, "optimal after", opt)
            assert 0 <= conv <= 2 and 0 <= opt <= 2 and 0 < its <= 2 * int(block.split("iters: ")[1].split(",")[0])
            if max_m == 19:
                assert opt == 0 and log["skipped"][e] == 2
        assert all(len(log[k]) == 2 for k in experiment.PDHG_KEYS)
    with pytest.raises(ValueError):
        experiment.pdhg_counts(None, None, {"pdhg": {"iters": 5}})
