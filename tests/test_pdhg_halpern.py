"""GPU: mllp_lp_pdhg_halpern (preconditioned, restarted Halpern PDHG with reflection; csrc/pdhg.hip) against the numpy oracle of
THE RULE (tests/pdhg_halpern_oracle.py), on planted LPs (the device plants them, the oracle gets what the batch stores), in
the pattern of tests/test_pdhg_scaled.py and on its shapes: 5 x 12, 40 x 100, 193 x 400 and the block-tier instance.

THE BAR (tests 1 and 3) is the project's: 8 x the largest deviation, over the test's own instances, between
the fp64 oracle and THE SAME oracle run in numpy fp32 -- both CPU code --, in units of 2^-24 max|.| of the vector compared, per
K and per `reflect`.  Nothing in it comes from the kernel.  The test computes and prints every figure before it asserts.
Oracle against oracle on CPU-planted data of the same shapes and seed (the device-planted figures are printed by the run):
reflected, K = 64: 132 units -> bar 1053;  K = 512: 1042 units -> bar 8339 (y of 193 x 400);  not reflected: 41.7 -> 334 and
369 -> 2950.  The reflected iterate moves twice as far per step as the step's output, and two fp32 orders drift apart
accordingly.

THE GUARD (test 3).  Decisions are compared only where the ORACLE's margin is at least 2^-7 and the fp32 and fp64 oracles
take the same decisions, asserted before the device is looked at; the margin covers the two comparisons of a check and the two
of the weight's clamp.  Seeds of tb.planted_shapes([shape], seed) that qualify under the default options, searched on the CPU
over 20 .. 45 (the range did not have to be widened): 5 x 12: all; 40 x 100: all but 39; 193 x 400: all but 32.
Used: 27 (margin 0.521), 22 (0.678), 43 (0.368) -- the seeds of tests/test_pdhg_scaled.py.
"""
import ctypes

import numpy as np
import pytest
import torch

import pdhg_halpern_oracle as ph
import pdhg_oracle as pg
import planted_oracle as po
import test_basis_repair as tb
from guarded import same_bits
from mllp_amd import _lib
from test_basis_repair import LPBatch  # noqa: F401  (the fixture)
from test_pdhg import _kkt_close
from test_pdhg_scaled import SMALL, SPLIT_WORDS, TRACE, _batch, _bits, _host, _part, _units

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -10
EINVAL = -1
ORDER = ("g", "x1", "x2", "x0", "y0", "max_iters", "check_every", "eps", "step", "beta", "ruiz", "pc", "pw", "span", "reflect", "lds", "x", "y",
         "dr", "dc", "status", "kkt", "scratch")


@pytest.fixture(scope="module")
def plain(LPBatch):
    """the three small shapes and the long-row instance in one batch; per (K, reflect) the two oracle runs of every instance"""
    g = _batch(LPBatch, pg.join_cases([tb.planted_shapes(SMALL, 20), po.ragged_case(which=[4])]))
    g["runs"], g["dev"] = {}, {}
    for K in (64, 512):
        for reflect in (True, False):
            runs = [(ph.solve(i["A"], i["b"], i["c"], K, check_every=0, reflect=reflect),
                     ph.solve(i["A"], i["b"], i["c"], K, check_every=0, reflect=reflect, dtype=np.float32)) for i in g["insts"]]
            g["runs"][K, reflect] = runs
            g["dev"][K, reflect] = max(max(_units(f["x"], a["x"]), _units(f["y"], a["y"])) for a, f in runs)
            print(f"K = {K}, reflect = {reflect}: fp32 oracle against fp64 oracle, largest deviation {g['dev'][K, reflect]:.2f} units "
                  f"-> bar {8 * g['dev'][K, reflect]:.1f}")
    return g


@pytest.fixture(scope="module")
def trace(LPBatch):
    """the three guarded instances in one batch, both oracle runs of each, the device's run"""
    g = _batch(LPBatch, pg.join_cases([tb.planted_shapes([shape], seed) for shape, seed in TRACE]))
    g["oracle"] = [ph.solve(i["A"], i["b"], i["c"], 8192, eps=EPS) for i in g["insts"]]
    g["oracle32"] = [ph.solve(i["A"], i["b"], i["c"], 8192, eps=EPS, dtype=np.float32) for i in g["insts"]]
    for o, f in zip(g["oracle"], g["oracle32"]):       # the condition, from the oracles alone
        print("oracle", o["status"], "fp32 oracle", f["status"], "margin", o["margin"], "w0", o["w0"], "w", o["w"], "weight updates", len(o["weights"]))
        assert o["margin"] >= 2.0 ** -7 and o["status"][0] == 0 and o["status"] == f["status"] and len(o["weights"]) >= 1, (o["status"], o["margin"])
    g["res"] = g["b"].pdhg_halpern(8192, eps=EPS, check_every=64)
    g["host"] = _host(g["res"])
    return g


# ---------------------------------------------------------------------------------------------------
# 1. iteration parity;  2. what the call shares with mllp_lp_pdhg_scaled, bit for bit
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reflect", [True, False])
@pytest.mark.parametrize("K", [64, 512])
def test_plain_iterations_against_the_oracle(plain, K, reflect):
    c, b = plain["c"], plain["b"]
    bar = 8.0 * plain["dev"][K, reflect]
    h = _host(b.pdhg_halpern(K, check_every=0, reflect=reflect))
    for k, (a, _) in enumerate(plain["runs"][K, reflect]):
        got = _part(c, h, k)
        assert list(got["status"]) == [6, K, 0, 0], (k, got["status"])
        ux, uy = _units(got["x"], a["x"]), _units(got["y"], a["y"])
        print(f"K = {K}, reflect = {reflect}, instance {k} ({c['inst_m'][k]} x {c['inst_n'][k]}): x {ux:.2f} units, y {uy:.2f} units, bar {bar:.1f}")
        assert ux <= bar and uy <= bar, (K, reflect, k, ux, uy, bar)
        assert (got["x"] >= 0).all() and got["kkt"][5] == got["kkt"][4] != 1.0
        _kkt_close(plain["insts"][k], got["x"], got["y"], got["kkt"], f"K = {K}, instance {k}")      # the errors are the original LP's


def test_the_first_step_and_the_set_up_are_the_scaled_calls_bits(plain, trace):
    for g in (plain, trace):
        b = g["b"]
        want = _bits(_host(b.pdhg_scaled(1, check_every=0)))
        shared = lambda h: dict(dr=h["dr"], dc=h["dc"], kkt=np.ascontiguousarray(h["kkt"][:, 3:5]))      # noqa: E731
        for reflect in (True, False):
            for lds in (None, SPLIT_WORDS):
                got = _host(b.pdhg_halpern(1, check_every=64, reflect=reflect, max_lds_words=lds))
                assert [list(s) for s in got["status"]] == [[6, 1, 0, 0]] * b.n_inst
                same_bits(_bits(got), want, f"K = 1, reflect = {reflect}, max_lds_words = {lds}")      # (status and kkt too: the same point)
        ref = _bits(shared(_host(b.pdhg_scaled(0))))
        for K, kw in ((0, {}), (64, dict(check_every=0)), (1024, dict(eps=EPS)), (192, dict(reflect=False))):
            same_bits(_bits(shared(_host(b.pdhg_halpern(K, **kw)))), ref, f"dr, dc, eta, w0 at K = {K}, {kw}")


def test_the_reflection_is_on_by_default_and_changes_the_bits(plain):
    b = plain["b"]
    on, default, off = (_bits(_host(b.pdhg_halpern(2, check_every=0, **kw), ("x", "y"))) for kw in (dict(reflect=True), {}, dict(reflect=False)))
    same_bits(on, default, "reflect = True against the default")
    assert (on["x"] != off["x"]).any() and (on["y"] != off["y"]).any()


# ---------------------------------------------------------------------------------------------------
# 3. decisions, guarded;  4. what holds of any run that converges
# ---------------------------------------------------------------------------------------------------
def test_the_decisions_of_guarded_instances(plain, trace):
    c, h = trace["c"], trace["host"]
    wdev = max(_units(f["w"], a["w"]) for a, f in zip(trace["oracle"], trace["oracle32"]))
    print(f"final weight: fp32 oracle against fp64 oracle {wdev:.2f} units -> bar {8 * wdev:.1f}")
    for k, (o, f) in enumerate(zip(trace["oracle"], trace["oracle32"])):
        got = _part(c, h, k)
        print(f"instance {k}: oracle {o['status']} margin {o['margin']:.4f} w {o['w']:.6f}, device {list(got['status'])} w {got['kkt'][5]:.6f}")
        assert list(got["status"]) == f["status"] == o["status"] and got["status"][3] == 0, (k, got["status"], o["status"])
        uw = _units(got["kkt"][5], o["w"])
        bar = 8.0 * plain["dev"][512, True] * max(o["status"][1] / 512.0, 1.0)
        ux, uy = _units(got["x"], o["x"]), _units(got["y"], o["y"])
        print(f"instance {k}: w {uw:.2f} units (bar {8 * wdev:.1f}), x {ux:.2f} units, y {uy:.2f} units, bar {bar:.1f}")
        assert uw <= 8.0 * wdev and ux <= bar and uy <= bar, (k, uw, wdev, ux, uy, bar)
        lo, hi = np.float32(got["kkt"][4]) / np.float32(16.0), np.float32(got["kkt"][4]) * np.float32(16.0)
        assert lo <= got["kkt"][5] <= hi and got["kkt"][5] != got["kkt"][4]


def test_a_converged_run_is_optimal_and_points_at_the_planted_vertex(trace):
    c, b, h = trace["c"], trace["b"], trace["host"]
    for k, inst in enumerate(trace["insts"]):
        got = _part(c, h, k)
        code, it, restarts, flag = got["status"]
        assert code == 0 and it % 64 == 0 and 0 < it <= 8192 and flag == 0 and restarts >= 0, (k, got["status"])
        errs = pg.errors64(inst["A"], inst["b"], inst["c"], got["x"], got["y"])
        assert max(errs) <= EPS * (1 + 2.0 ** -6) and max(got["kkt"][:3]) <= EPS, (k, errs)
        assert (got["x"] >= 0).all() and np.array_equal(pg.topm(got["x"], inst["m"]), inst["labels"]), k
    from mllp_amd.graph import LPPdhg, LPPdhgHalpern, LPPdhgScaled
    assert isinstance(trace["res"], LPPdhgHalpern) and isinstance(trace["res"], LPPdhgScaled) and isinstance(trace["res"], LPPdhg)
    rep = b.pdhg_basis(trace["res"])
    solved = b.solved(rep, 1e-3, 1e-3)
    torch.cuda.synchronize()
    assert list(rep.status[:, 0].cpu().numpy()) == list(c["inst_m"]) and (rep.status[:, 3] == 0).all()
    assert np.array_equal(rep.basis.cpu().numpy(), trace["st"]["labels"])
    assert solved["optimal"].all() and solved["primal_feasible"].all()


def test_the_long_rows_converge(plain):
    c, b = plain["c"], plain["b"]
    h = _host(b.pdhg_halpern(4096, eps=EPS))
    k, inst = 3, plain["insts"][3]
    got = _part(c, h, k)
    print("long rows:", list(got["status"]), got["kkt"])
    assert got["status"][0] == 0 and 0 < got["status"][1] <= 4096 and got["status"][1] % 64 == 0
    assert max(pg.errors64(inst["A"], inst["b"], inst["c"], got["x"], got["y"])) <= EPS * (1 + 2.0 ** -6)
    assert max(np.diff(inst["A"].indptr).max(), np.diff(inst["A"].tocsc().indptr).max()) > 1024       # the workgroup tier is under the sweeps


# ---------------------------------------------------------------------------------------------------
# 5. the same bits
# ---------------------------------------------------------------------------------------------------
def _scratch_bytes(b, words, fn="mllp_lp_pdhg_halpern_scratch_bytes"):
    n = ctypes.c_int64(-1)
    _lib.check(getattr(_lib.lib(), fn)(b._h, words, ctypes.byref(n)))
    return n.value


def test_same_bits_in_lds_in_scratch_alone_and_twice(LPBatch, trace):
    from mllp_amd.graph import pdhg_halpern_limits
    c, b, st = trace["c"], trace["b"], trace["st"]
    words = [3 * n + 2 * m for m, n in zip(c["inst_m"], c["inst_n"])]
    side = sum(2 * n + 2 * m for m, n in zip(c["inst_m"], c["inst_n"]))
    assert _scratch_bytes(b, pdhg_halpern_limits()[0]) == 4 * side and _scratch_bytes(b, 0) == 4 * (side + sum(words))
    assert _scratch_bytes(b, SPLIT_WORDS) == 4 * (side + sum(w for w in words if w > SPLIT_WORDS))
    assert all(_scratch_bytes(b, w) == _scratch_bytes(b, w, "mllp_lp_pdhg_scaled_scratch_bytes") for w in (0, SPLIT_WORDS, 400, 36864))
    assert sorted(w > SPLIT_WORDS for w in words) == [False, True, True]       # both launches run
    want = _bits(trace["host"])
    for lds in (None, 0, SPLIT_WORDS, 400):
        same_bits(_bits(_host(b.pdhg_halpern(8192, eps=EPS, check_every=64, max_lds_words=lds))), want, f"max_lds_words = {lds}")
    assert b._pdhg_halpern_scratch[0] == 400      # kept under its own attribute, per max_lds_words
    # without the weight the anchor still moves, in both address spaces alike
    plain_w = _bits(_host(b.pdhg_halpern(8192, eps=EPS, primal_weight=False)))
    same_bits(_bits(_host(b.pdhg_halpern(8192, eps=EPS, primal_weight=False, max_lds_words=0))), plain_w, "no weight, max_lds_words = 0")
    # every instance alone (a batch of its own from the values, costs and right-hand sides the batch stores)
    for k, (shape, seed) in enumerate(TRACE):
        s, r = slice(c["ptr_n"][k], c["ptr_n"][k + 1]), slice(c["ptr_m"][k], c["ptr_m"][k + 1])
        ck = dict(tb.planted_shapes([shape], seed), val=st["values"][c["nnz_off"][k]:c["nnz_off"][k + 1]])
        alone = tb._build(LPBatch, ck, tb._dev(st["x1"][s]), tb._dev(st["x2"][r]), tb._dev(st["labels"][s]))
        for lds in (None, 0):
            got = _bits(_host(alone.pdhg_halpern(8192, eps=EPS, check_every=64, max_lds_words=lds)))
            same_bits(got, _bits(_part(c, trace["host"], k)), f"instance {k} alone, max_lds_words = {lds}")


def test_the_anchor_moves_without_the_weight(trace):
    """primal_weight = 0: the decisions are the oracle's where its margin allows (a stale anchor would change them from the
    second restart on), and the weight stays 1"""
    c, b = trace["c"], trace["b"]
    h = _host(b.pdhg_halpern(8192, eps=EPS, primal_weight=False))
    compared = 0
    for k, inst in enumerate(trace["insts"]):
        o = ph.solve(inst["A"], inst["b"], inst["c"], 8192, eps=EPS, primal_weight=False)
        f = ph.solve(inst["A"], inst["b"], inst["c"], 8192, eps=EPS, primal_weight=False, dtype=np.float32)
        got = _part(c, h, k)
        print(f"instance {k}: oracle {o['status']} fp32 {f['status']} margin {o['margin']:.4f}, device {list(got['status'])}")
        assert list(got["kkt"][4:]) == [1.0, 1.0]
        if o["margin"] >= 2.0 ** -7 and o["status"] == f["status"]:
            compared += o["status"][2] >= 2
            assert list(got["status"]) == o["status"], (k, got["status"], o["status"])
    assert compared >= 1, "no guarded instance with two restarts: the test compares nothing"


# ---------------------------------------------------------------------------------------------------
# 6. starts and refusals
# ---------------------------------------------------------------------------------------------------
def test_starts_and_limits(trace):
    c, b, st = trace["c"], trace["b"], trace["st"]
    K = len(c["inst_m"])
    rep = b.solve_basis(b.labels)
    from_rep = _host(b.pdhg_halpern(8192, eps=EPS, start=rep))
    assert [list(s) for s in from_rep["status"]] == [[0, 64, 0, 0]] * K, from_rep["status"]
    assert (from_rep["kkt"][:, 5] == from_rep["kkt"][:, 4]).all()         # a stop does not move the weight
    same_bits(_bits(_host(b.pdhg_halpern(8192, eps=EPS, x0=rep.x, y0=rep.y))), _bits(from_rep), "x0, y0 against start=")
    xstar = tb._dev(c["xstar"] * st["labels"])
    with pytest.raises(ValueError):
        b.pdhg_halpern(64, start=rep, x0=xstar)
    rng = np.random.default_rng(7)
    x0, y0 = rng.uniform(-1.0, 1.0, c["N"]).astype(np.float32), rng.uniform(-1.0, 1.0, c["M"]).astype(np.float32)
    neg = _bits(_host(b.pdhg_halpern(256, eps=EPS, x0=tb._dev(x0), y0=tb._dev(y0))))
    same_bits(neg, _bits(_host(b.pdhg_halpern(256, eps=EPS, x0=tb._dev(np.maximum(x0, 0)), y0=tb._dev(y0)))), "x0 against max(x0, 0)")
    cold = _host(b.pdhg_halpern(256, eps=EPS))
    assert (neg["x"] != _bits(cold)["x"]).any()                           # the start is read
    for lds in (None, 0):
        zero = _host(b.pdhg_halpern(0, eps=EPS, x0=tb._dev(x0), y0=tb._dev(y0), max_lds_words=lds))
        assert [list(s) for s in zero["status"]] == [[6, 0, 0, 0]] * K
        assert np.array_equal(zero["x"], np.maximum(x0, 0)) and np.array_equal(zero["y"], y0)
        for k, inst in enumerate(trace["insts"]):
            got = _part(c, zero, k)
            _kkt_close(inst, got["x"], got["y"], got["kkt"], f"max_iters = 0, instance {k}")
    # weight_span = 1 keeps the weight where it started, through every restart
    fixed = _host(b.pdhg_halpern(8192, eps=EPS, weight_span=1.0))
    assert (fixed["status"][:, 0] == 0).all() and (fixed["status"][:, 2] >= 1).all() and (fixed["kkt"][:, 5] == fixed["kkt"][:, 4]).all()
    # a NaN in b of instance 1: code 8 there, the other instances' bits as ever
    clean = _host(b.pdhg_halpern(1024, eps=EPS))
    keep = b.x2.clone()
    try:
        b.x2[c["ptr_m"][1]] = float("nan")
        b.invalidate_inputs()
        bad = _host(b.pdhg_halpern(1024, eps=EPS))
    finally:
        b.x2.copy_(keep)
        b.invalidate_inputs()
    assert list(bad["status"][1]) == [8, 64, 0, 0] and bad["kkt"][1][4] == 1.0, (bad["status"], bad["kkt"])
    for k in (0, 2):
        same_bits(_bits(_part(c, bad, k)), _bits(_part(c, clean, k)), f"instance {k} beside a non-finite one")


def test_every_refusal_writes_nothing(trace):
    c, b = trace["c"], trace["b"]
    K, L, z = len(c["inst_m"]), _lib.lib(), ctypes.c_void_p(0)
    poison = lambda n: torch.full((n,), float("nan"), device="cuda")      # noqa: E731
    bufs = dict(x=poison(c["N"] + 8), y=poison(c["M"]), dr=poison(c["M"]), dc=poison(c["N"]), status=poison(4 * K).view(torch.int32), kkt=poison(6 * K),
                scratch=poison(c["N"] * 5 + c["M"] * 4))
    x0, y0 = tb._dev(np.ones(c["N"], np.float32)), tb._dev(np.ones(c["M"], np.float32))
    ok = dict(g=b._h, x1=_lib.ptr(b.x1), x2=_lib.ptr(b.x2), x0=_lib.ptr(x0), y0=_lib.ptr(y0), max_iters=128, check_every=64, eps=EPS, step=0.9,
              beta=0.5, ruiz=10, pc=1, pw=1, span=16.0, reflect=1, lds=0, x=_lib.ptr(bufs["x"]), y=_lib.ptr(bufs["y"]), dr=_lib.ptr(bufs["dr"]),
              dc=_lib.ptr(bufs["dc"]), status=_lib.ptr(bufs["status"]), kkt=_lib.ptr(bufs["kkt"]), scratch=_lib.ptr(bufs["scratch"]))
    nan, inf = float("nan"), float("inf")
    bad = [dict(g=None), dict(x1=z), dict(x2=z), dict(x=z), dict(y=z), dict(status=z), dict(max_iters=-1), dict(check_every=-1), dict(lds=-1),
           dict(eps=nan), dict(eps=inf), dict(eps=-1.0), dict(step=nan), dict(step=inf), dict(step=0.0), dict(step=-0.5), dict(step=1.5),
           dict(beta=nan), dict(beta=inf), dict(beta=0.0), dict(beta=1.0), dict(beta=-0.5), dict(scratch=z),
           dict(ruiz=-1), dict(ruiz=65), dict(span=nan), dict(span=inf), dict(span=0.999), dict(span=0.0), dict(span=-16.0),
           dict(x0=_lib.ptr(bufs["x"])), dict(y0=_lib.ptr(bufs["y"])), dict(x0=ctypes.c_void_p(bufs["x"].data_ptr() + 32)),
           dict(y0=_lib.ptr(bufs["kkt"])), dict(x0=_lib.ptr(bufs["status"])), dict(x0=_lib.ptr(bufs["dc"])), dict(y0=_lib.ptr(bufs["dr"])),
           dict(y0=_lib.ptr(bufs["dc"])), dict(x0=ctypes.c_void_p(bufs["dr"].data_ptr() + 4))]
    before = {k: v.view(torch.int32).cpu().numpy().copy() for k, v in bufs.items()}
    for kw in bad:
        args = dict(ok, **kw)
        assert L.mllp_lp_pdhg_halpern(*[args[k] for k in ORDER], _lib.current_stream()) == EINVAL, kw
        assert b"mllp_lp_pdhg_halpern:" in L.mllp_last_error(), kw
    torch.cuda.synchronize()
    same_bits({k: v.view(torch.int32).cpu().numpy() for k, v in bufs.items()}, before, "buffers after the refused calls")
    # the same arguments without a fault are accepted (kkt, dr and dc may be NULL; reflect is 0 or not 0)
    assert L.mllp_lp_pdhg_halpern(*[dict(ok, kkt=z, dr=z, dc=z, eps=0.0, reflect=0)[k] for k in ORDER], _lib.current_stream()) == 0
    assert L.mllp_lp_pdhg_halpern(*[dict(ok, eps=0.0, ruiz=64, span=1.0, reflect=-3)[k] for k in ORDER], _lib.current_stream()) == 0
    torch.cuda.synchronize()
    assert (bufs["status"].view(K, 4)[:, 0] == 6).all() and torch.isnan(bufs["kkt"]).sum() == 0
    assert torch.isnan(bufs["dr"]).sum() == 0 and torch.isnan(bufs["dc"]).sum() == 0 and torch.isnan(bufs["x"][:c["N"]]).sum() == 0


def test_an_empty_instance_and_an_empty_side(LPBatch):
    """n = 0 or m = 0 is legal: no rows leaves x to the costs alone (eta = step, w0 = 1: |dr b| = 0), no columns leaves y to b"""
    c = tb.dense_case([np.zeros((0, 3)), tb.int_matrix(3, 6, 0.7, 12), np.zeros((2, 0))], 1)
    c["c"][:3] = [1.0, 2.0, 0.0]
    b = tb._build(LPBatch, c, tb._dev(c["c"]), tb._dev(c["b"]))
    h = _host(b.pdhg_halpern(128, eps=EPS, x0=tb._dev(np.ones(c["N"], np.float32))))
    assert list(h["status"][0]) == [0, 64, 0, 0] and np.array_equal(h["x"][:3], [0.0, 0.0, 1.0])
    assert list(h["kkt"][0][3:]) == [np.float32(0.9), 1.0, 1.0] and list(h["kkt"][2][3:]) == [np.float32(0.9), 1.0, 1.0]
    assert h["status"][2][1] in (64, 128) and h["status"][2][0] in (0, 6) and np.isfinite(h["kkt"]).all()
    assert (h["dc"][:3] == 1).all() and (h["dr"][3:] == 1).all() and len(h["dr"]) == 5 and len(h["dc"]) == 9
    mid = ph.solve(c["mats"][1], c["b"][:3], c["c"][3:9], 128, eps=EPS, x0=np.ones(6))
    assert list(h["status"][1][:2]) == mid["status"][:2] or mid["margin"] < 2.0 ** -7


# ---------------------------------------------------------------------------------------------------
# driver
# ---------------------------------------------------------------------------------------------------
def test_driver_reports_pdhg_halpern(tmp_path, monkeypatch):
    """`halpern: true` and `halpern: {reflect: ...}` inside `report_solved: pdhg` select the call for the same three log keys,
    alone or with the `scaled:` options; an unknown option and `scaled: false` beside it are refused"""
    import json
    from mllp_amd import experiment
    cfg = ("train_data_type: 'planted'\ntrain_lr: 1.e-3\ntrain_iter: 1\nmethods:\n  - 'gs-topk'\nbatch_size: 3\nholdout: 0.25\n"
           "planted: {instances: 8, m: 20, n: 50, row_nnz: 4, seed: 5}\n")
    base = {"obj", "val_obj", "usable", "feasible", "optimal", "skipped"} | {f"planted{5 + i}" for i in range(8)}
    from mllp_amd.graph import LPBatch as Batch
    calls, inner = [], Batch.pdhg_halpern

    def recorded(self, max_iters, **kw):
        calls.append({k: kw.get(k) for k in ("ruiz", "pock_chambolle", "primal_weight", "weight_span", "reflect")})
        return inner(self, max_iters, **kw)
    monkeypatch.setattr(Batch, "pdhg_halpern", recorded)
    blocks = {"pdhg: {iters: 4096, eps: 1.e-3, scaled: true}": None,
              "pdhg: {iters: 4096, eps: 1.e-3, halpern: false}": None,
              "pdhg: {iters: 4096, eps: 1.e-3, halpern: true}": dict(ruiz=10, pock_chambolle=True, primal_weight=True, weight_span=16.0, reflect=True),
              "pdhg: {iters: 4096, eps: 1.e-3, warm: false, halpern: {reflect: false}, scaled: {ruiz: 4, pock_chambolle: false, span: 4}}":
                  dict(ruiz=4, pock_chambolle=False, primal_weight=True, weight_span=4.0, reflect=False)}
    for block, want in blocks.items():
        del calls[:]
        (tmp_path / "cfg.yaml").write_text(cfg + f"report_solved: {{feas_tol: 1.e-3, opt_tol: 1.e-3, max_m: 20, {block}}}\n")
        monkeypatch.chdir(tmp_path)
        assert experiment.main(["--cfg", str(tmp_path / "cfg.yaml")]) == 0
        log = json.load(open(tmp_path / "train_log.json"))
        assert set(log) == base | set(experiment.PDHG_KEYS)
        conv, its, opt = (log[k][0] for k in experiment.PDHG_KEYS)
        print(block, "converged", conv, "iterations", its, "optimal after", opt)
        assert 0 <= conv <= 2 and 0 <= opt <= 2 and 0 < its <= 2 * 4096 and len(log[experiment.PDHG_KEYS[0]]) == 1
        assert (calls == [] if want is None else calls and all(k == want for k in calls)), (block, calls)
    for wrong in ({"halpern": {"reflection": True}}, {"halpern": True, "scaled": False}, {"halpern": True, "scaled": {"passes": 3}}):
        with pytest.raises(ValueError):
            experiment.pdhg_counts(None, None, {"pdhg": {"iters": 5, "eps": 1e-3, "warm": False, **wrong}})
