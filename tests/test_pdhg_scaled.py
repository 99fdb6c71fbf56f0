"""GPU: mllp_lp_pdhg_scaled (preconditioned restarted PDHG; csrc/pdhg.hip) against the numpy oracle of THE RULE
(tests/pdhg_scaled_oracle.py), on planted LPs (the device plants them, the oracle gets what the batch stores), in the
pattern of tests/test_pdhg.py.

THE BAR (tests 1, 2 and 3) is the project's: 8 x the largest deviation, over the test's own instances,
between the fp64 oracle and THE SAME oracle run in numpy fp32 -- both CPU code --, in units of 2^-24 max|.| of the vector
compared.  Nothing in it comes from the kernel.  The test computes and prints every figure before it asserts.  Oracle against
oracle on the device-planted data: K = 64: 23.3 units -> bar 187;  K = 512: 667 units -> bar 5338 (y of 40 x 100 and of
193 x 400: the preconditioned iteration takes larger dual steps than the baseline's, and two fp32 orders drift apart
faster);  factors after the Pock-Chambolle pass: 1.41 units -> bar 11.3;  eta and w0: 4.14 -> 33.1;  the final weight of the
guarded runs: 57.3 -> 458.  The device, for the record (one MI355X): at most 28.1 units at K = 64 and 526 at K = 512 (y of
40 x 100), factors 1.41, eta 2.49, w0 2.09, final weight 7.97, guarded traces 12.5.

THE GUARD (test 3).  Decisions are compared only where the ORACLE's margin is at least 2^-7, asserted before the device is
looked at; the margin covers the three comparisons of a check and the two of the weight's clamp.  Seeds of
tb.planted_shapes([shape], seed) that qualify under the default options, searched on the CPU over 20 .. 45:
5 x 12: all but 39; 40 x 100: 21-24, 27, 31-39, 42-45; 193 x 400: 20, 21, 23, 25, 27, 28, 31, 32, 35, 37, 39, 41, 43, 44.
Used: 27 (margin 0.512), 22 (0.620), 43 (0.231).
"""
import ctypes

import numpy as np
import pytest
import torch

import pdhg_oracle as pg
import pdhg_scaled_oracle as ps
import planted_oracle as po
import test_basis_repair as tb
from guarded import same_bits
from mllp_amd import _lib
from test_basis_repair import LPBatch  # noqa: F401  (the fixture)
from test_pdhg import _kkt_close

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EPS = 2.0 ** -10
EINVAL = -1
SMALL = [(5, 12), (40, 100), (193, 400)]
TRACE = [((5, 12), 27), ((40, 100), 22), ((193, 400), 43)]
SPLIT_WORDS = 100           # 3 n + 2 m: 46 (LDS), 380 and 1586 (scratch)
NEUTRAL = dict(ruiz=0, pock_chambolle=False, primal_weight=False)
FIELDS = ("x", "y", "status", "kkt", "dr", "dc")


def _batch(LPBatch, c):
    b, _, st = tb._planted(LPBatch, c)
    return dict(c=c, b=b, st=st, insts=pg.split(c, st["values"], st["x1"], st["x2"], st["labels"]))


def _host(res, fields=FIELDS):
    torch.cuda.synchronize()
    return {k: getattr(res, k).cpu().numpy() for k in fields}


def _bits(h):
    return {k: np.ascontiguousarray(v).view(np.int32).reshape(-1).copy() for k, v in h.items()}


def _part(c, h, k):
    s, r = slice(c["ptr_n"][k], c["ptr_n"][k + 1]), slice(c["ptr_m"][k], c["ptr_m"][k + 1])
    out = dict(x=h["x"][s], y=h["y"][r], status=h["status"][k], kkt=h["kkt"][k])
    if "dr" in h:
        out.update(dr=h["dr"][r], dc=h["dc"][s])
    return out


def _units(got, want):
    want = np.atleast_1d(np.asarray(want, np.float64))
    scale = np.abs(want).max(initial=0.0)
    return 0.0 if scale == 0.0 else float(np.abs(np.atleast_1d(np.asarray(got, np.float64)) - want).max() / (U * scale))


@pytest.fixture(scope="module")
def plain(LPBatch):
    """the three small shapes and the long-row instance in one batch; per K the two oracle runs of every instance, and the
    two oracle runs of the scaling with the Pock-Chambolle pass"""
    g = _batch(LPBatch, pg.join_cases([tb.planted_shapes(SMALL, 20), po.ragged_case(which=[4])]))
    g["runs"], g["dev"] = {}, {}
    for K in (64, 512):
        g["runs"][K] = [(ps.solve(i["A"], i["b"], i["c"], K, check_every=0), ps.solve(i["A"], i["b"], i["c"], K, check_every=0, dtype=np.float32))
                        for i in g["insts"]]
        g["dev"][K] = max(max(_units(f["x"], a["x"]), _units(f["y"], a["y"])) for a, f in g["runs"][K])
        print(f"K = {K}: fp32 oracle against fp64 oracle, largest deviation {g['dev'][K]:.2f} units -> bar {8 * g['dev'][K]:.1f}")
    g["dev"]["factors"] = max(max(_units(f["dr"], a["dr"]), _units(f["dc"], a["dc"])) for a, f in g["runs"][64])
    g["dev"]["scalars"] = max(max(_units(f["eta"], a["eta"]), _units(f["w0"], a["w0"])) for a, f in g["runs"][64])
    print(f"factors: {g['dev']['factors']:.2f} units, eta and w0: {g['dev']['scalars']:.2f} units (fp32 oracle against fp64 oracle)")
    return g


@pytest.fixture(scope="module")
def trace(LPBatch):
    """the three guarded instances in one batch, both oracle runs of each, the device's run"""
    g = _batch(LPBatch, pg.join_cases([tb.planted_shapes([shape], seed) for shape, seed in TRACE]))
    g["oracle"] = [ps.solve(i["A"], i["b"], i["c"], 8192, eps=EPS) for i in g["insts"]]
    g["oracle32"] = [ps.solve(i["A"], i["b"], i["c"], 8192, eps=EPS, dtype=np.float32) for i in g["insts"]]
    for o in g["oracle"]:                          # the condition, from the oracle alone
        print("oracle", o["status"], "margin", o["margin"], "w0", o["w0"], "w", o["w"], "weight updates", len(o["weights"]))
        assert o["margin"] >= 2.0 ** -7 and o["status"][0] == 0 and len(o["weights"]) >= 1, (o["status"], o["margin"])
    g["res"] = g["b"].pdhg_scaled(8192, eps=EPS, check_every=64)
    g["host"] = _host(g["res"])
    return g


# ---------------------------------------------------------------------------------------------------
# 1. the scaling factors
# ---------------------------------------------------------------------------------------------------
def test_ruiz_factors_are_the_fp32_oracles_bits(plain):
    """maxima are exact in any order and every elementwise operation is correctly rounded: no tolerance.  The long-row
    instance puts the workgroup tier (rows above 1024 terms) under the walk."""
    c, b = plain["c"], plain["b"]
    for passes in (10, 1, 0):
        h = _host(b.pdhg_scaled(0, ruiz=passes, pock_chambolle=False))
        for k, inst in enumerate(plain["insts"]):
            got = _part(c, h, k)
            dr, dc = ps.scaling(inst["A"], passes, False, np.float32)
            same_bits(_bits(dict(dr=got["dr"], dc=got["dc"])), _bits(dict(dr=dr, dc=dc)), f"{passes} Ruiz passes, instance {k}")
            assert list(got["status"]) == [6, 0, 0, 0]
    assert max(np.diff(plain["insts"][3]["A"].indptr).max(), np.diff(plain["insts"][3]["A"].tocsc().indptr).max()) > 1024


def test_pock_chambolle_factors_within_the_bar(plain):
    c, b = plain["c"], plain["b"]
    bar = 8.0 * plain["dev"]["factors"]
    h = _host(b.pdhg_scaled(0))
    for k, (a, _) in enumerate(plain["runs"][64]):
        got = _part(c, h, k)
        ur, uc = _units(got["dr"], a["dr"]), _units(got["dc"], a["dc"])
        print(f"instance {k} ({c['inst_m'][k]} x {c['inst_n'][k]}): dr {ur:.2f} units, dc {uc:.2f} units, bar {bar:.1f}")
        assert ur <= bar and uc <= bar, (k, ur, uc, bar)


# ---------------------------------------------------------------------------------------------------
# 2. iteration parity
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [64, 512])
def test_plain_iterations_against_the_oracle(plain, K):
    c, b = plain["c"], plain["b"]
    bar, sbar = 8.0 * plain["dev"][K], 8.0 * plain["dev"]["scalars"]
    h = _host(b.pdhg_scaled(K, check_every=0))
    for k, (a, _) in enumerate(plain["runs"][K]):
        got = _part(c, h, k)
        assert list(got["status"]) == [6, K, 0, 0], (k, got["status"])
        ux, uy = _units(got["x"], a["x"]), _units(got["y"], a["y"])
        ue, uw = _units(got["kkt"][3], a["eta"]), _units(got["kkt"][4], a["w0"])
        print(f"K = {K}, instance {k} ({c['inst_m'][k]} x {c['inst_n'][k]}): x {ux:.2f} units, y {uy:.2f} units, bar {bar:.1f}; "
              f"eta {ue:.2f}, w0 {uw:.2f}, bar {sbar:.1f}")
        assert ux <= bar and uy <= bar, (K, k, ux, uy, bar)
        assert ue <= sbar and uw <= sbar and got["kkt"][5] == got["kkt"][4] != 1.0, (k, ue, uw, sbar, got["kkt"])
        _kkt_close(plain["insts"][k], got["x"], got["y"], got["kkt"], f"K = {K}, instance {k}")      # the errors are the original LP's


# ---------------------------------------------------------------------------------------------------
# 3. decisions, guarded;  6. what holds of any run that converges
# ---------------------------------------------------------------------------------------------------
def test_the_decisions_of_guarded_instances(plain, trace):
    c, h = trace["c"], trace["host"]
    wdev = max(_units(f["w"], a["w"]) for a, f in zip(trace["oracle"], trace["oracle32"]))
    print(f"final weight: fp32 oracle against fp64 oracle {wdev:.2f} units -> bar {8 * wdev:.1f}")
    for k, o in enumerate(trace["oracle"]):
        got = _part(c, h, k)
        print(f"instance {k}: oracle {o['status']} margin {o['margin']:.4f} w {o['w']:.6f}, device {list(got['status'])} w {got['kkt'][5]:.6f}")
        assert list(got["status"]) == o["status"], (k, got["status"], o["status"])
        uw = _units(got["kkt"][5], o["w"])
        bar = 8.0 * plain["dev"][512] * max(o["status"][1] / 512.0, 1.0)
        ux, uy = _units(got["x"], o["x"]), _units(got["y"], o["y"])
        print(f"instance {k}: w {uw:.2f} units (bar {8 * wdev:.1f}), x {ux:.2f} units, y {uy:.2f} units, bar {bar:.1f}")
        assert uw <= 8.0 * wdev and ux <= bar and uy <= bar, (k, uw, wdev, ux, uy, bar)
        lo, hi = np.float32(got["kkt"][4]) / np.float32(16.0), np.float32(got["kkt"][4]) * np.float32(16.0)
        assert lo <= got["kkt"][5] <= hi and got["kkt"][5] != got["kkt"][4]


def test_a_converged_run_is_optimal_and_points_at_the_planted_vertex(trace):
    c, b, h = trace["c"], trace["b"], trace["host"]
    for k, inst in enumerate(trace["insts"]):
        got = _part(c, h, k)
        code, it, restarts, avg = got["status"]
        assert code == 0 and it % 64 == 0 and 0 < it <= 8192 and avg in (0, 1) and restarts >= 0, (k, got["status"])
        errs = pg.errors64(inst["A"], inst["b"], inst["c"], got["x"], got["y"])
        assert max(errs) <= EPS * (1 + 2.0 ** -6) and max(got["kkt"][:3]) <= EPS, (k, errs)
        assert (got["x"] >= 0).all() and np.array_equal(pg.topm(got["x"], inst["m"]), inst["labels"]), k
    from mllp_amd.graph import LPPdhg, LPPdhgScaled
    assert isinstance(trace["res"], LPPdhgScaled) and isinstance(trace["res"], LPPdhg)
    rep = b.pdhg_basis(trace["res"])
    solved = b.solved(rep, 1e-3, 1e-3)
    torch.cuda.synchronize()
    assert list(rep.status[:, 0].cpu().numpy()) == list(c["inst_m"]) and (rep.status[:, 3] == 0).all()
    assert np.array_equal(rep.basis.cpu().numpy(), trace["st"]["labels"])
    assert solved["optimal"].all() and solved["primal_feasible"].all()


def test_the_long_rows_converge_where_the_baseline_does_not(plain):
    c, b = plain["c"], plain["b"]
    h, base = _host(b.pdhg_scaled(4096, eps=EPS)), _host(b.pdhg(4096, eps=EPS), ("x", "y", "status", "kkt"))
    k, inst = 3, plain["insts"][3]
    got = _part(c, h, k)
    print("long rows: scaled", list(got["status"]), got["kkt"], "baseline", list(base["status"][k]), base["kkt"][k])
    assert got["status"][0] == 0 and 0 < got["status"][1] <= 4096 and got["status"][1] % 64 == 0
    assert max(pg.errors64(inst["A"], inst["b"], inst["c"], got["x"], got["y"])) <= EPS * (1 + 2.0 ** -6)
    assert list(base["status"][k][:2]) == [6, 4096]


# ---------------------------------------------------------------------------------------------------
# 4. neutral settings;  5. the same bits
# ---------------------------------------------------------------------------------------------------
def test_neutral_settings_are_mllp_lp_pdhg_bit_for_bit(plain, trace):
    for g, iters in ((trace, 8192), (plain, 1024)):
        b = g["b"]
        for kw in (dict(check_every=64), dict(check_every=0), dict(check_every=64, max_lds_words=SPLIT_WORDS)):
            n = min(iters, 256) if kw["check_every"] == 0 else iters
            want = _host(b.pdhg(n, eps=EPS, **kw), ("x", "y", "status", "kkt"))
            got = _host(b.pdhg_scaled(n, eps=EPS, **NEUTRAL, **kw))
            assert (got["dr"] == 1).all() and (got["dc"] == 1).all() and (got["kkt"][:, 4:] == 1).all()
            same_bits(_bits(dict(x=got["x"], y=got["y"], status=got["status"], kkt=got["kkt"][:, :4])), _bits(want), f"neutral settings, {kw}")


def _scratch_bytes(b, words):
    n = ctypes.c_int64(-1)
    _lib.check(_lib.lib().mllp_lp_pdhg_scaled_scratch_bytes(b._h, words, ctypes.byref(n)))
    return n.value


def test_same_bits_in_lds_in_scratch_alone_and_twice(LPBatch, trace):
    from mllp_amd.graph import pdhg_scaled_limits
    c, b, st = trace["c"], trace["b"], trace["st"]
    words = [3 * n + 2 * m for m, n in zip(c["inst_m"], c["inst_n"])]
    side = sum(2 * n + 2 * m for m, n in zip(c["inst_m"], c["inst_n"]))
    assert _scratch_bytes(b, pdhg_scaled_limits()[0]) == 4 * side and _scratch_bytes(b, 0) == 4 * (side + sum(words))
    assert _scratch_bytes(b, SPLIT_WORDS) == 4 * (side + sum(w for w in words if w > SPLIT_WORDS))
    assert sorted(w > SPLIT_WORDS for w in words) == [False, True, True]       # both launches run
    want = _bits(trace["host"])
    for lds in (None, 0, SPLIT_WORDS, 400):
        same_bits(_bits(_host(b.pdhg_scaled(8192, eps=EPS, check_every=64, max_lds_words=lds))), want, f"max_lds_words = {lds}")
    # every instance alone (a batch of its own from the values, costs and right-hand sides the batch stores)
    for k, (shape, seed) in enumerate(TRACE):
        s, r = slice(c["ptr_n"][k], c["ptr_n"][k + 1]), slice(c["ptr_m"][k], c["ptr_m"][k + 1])
        ck = dict(tb.planted_shapes([shape], seed), val=st["values"][c["nnz_off"][k]:c["nnz_off"][k + 1]])
        alone = tb._build(LPBatch, ck, tb._dev(st["x1"][s]), tb._dev(st["x2"][r]), tb._dev(st["labels"][s]))
        for lds in (None, 0):
            got = _bits(_host(alone.pdhg_scaled(8192, eps=EPS, check_every=64, max_lds_words=lds)))
            same_bits(got, _bits(_part(c, trace["host"], k)), f"instance {k} alone, max_lds_words = {lds}")


# ---------------------------------------------------------------------------------------------------
# 7. starts and refusals
# ---------------------------------------------------------------------------------------------------
def test_starts_and_limits(trace):
    c, b, st = trace["c"], trace["b"], trace["st"]
    K = len(c["inst_m"])
    rep = b.solve_basis(b.labels)
    from_rep = _host(b.pdhg_scaled(8192, eps=EPS, start=rep))
    assert [list(s) for s in from_rep["status"][:, :3]] == [[0, 64, 0]] * K, from_rep["status"]
    assert (from_rep["kkt"][:, 5] == from_rep["kkt"][:, 4]).all()         # a stop does not move the weight
    xstar = tb._dev(c["xstar"] * st["labels"])
    with pytest.raises(ValueError):
        b.pdhg_scaled(64, start=rep, x0=xstar)
    rng = np.random.default_rng(7)
    x0, y0 = rng.uniform(-1.0, 1.0, c["N"]).astype(np.float32), rng.uniform(-1.0, 1.0, c["M"]).astype(np.float32)
    neg = _bits(_host(b.pdhg_scaled(256, eps=EPS, x0=tb._dev(x0), y0=tb._dev(y0))))
    same_bits(neg, _bits(_host(b.pdhg_scaled(256, eps=EPS, x0=tb._dev(np.maximum(x0, 0)), y0=tb._dev(y0)))), "x0 against max(x0, 0)")
    zero = _host(b.pdhg_scaled(0, eps=EPS, x0=tb._dev(x0), y0=tb._dev(y0)))
    assert [list(s) for s in zero["status"]] == [[6, 0, 0, 0]] * K
    assert np.array_equal(zero["x"], np.maximum(x0, 0)) and np.array_equal(zero["y"], y0)
    # weight_span = 1 keeps the weight where it started, through every restart
    fixed = _host(b.pdhg_scaled(8192, eps=EPS, weight_span=1.0))
    assert (fixed["status"][:, 0] == 0).all() and (fixed["status"][:, 2] >= 1).all() and (fixed["kkt"][:, 5] == fixed["kkt"][:, 4]).all()
    # a NaN in b of instance 1: code 8 there, the other instances' bits as ever
    clean = _host(b.pdhg_scaled(1024, eps=EPS))
    keep = b.x2.clone()
    try:
        b.x2[c["ptr_m"][1]] = float("nan")
        b.invalidate_inputs()
        bad = _host(b.pdhg_scaled(1024, eps=EPS))
    finally:
        b.x2.copy_(keep)
        b.invalidate_inputs()
    assert list(bad["status"][1][:3]) == [8, 64, 0] and bad["kkt"][1][4] == 1.0, (bad["status"], bad["kkt"])
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
              beta=0.5, ruiz=10, pc=1, pw=1, span=16.0, lds=0, x=_lib.ptr(bufs["x"]), y=_lib.ptr(bufs["y"]), dr=_lib.ptr(bufs["dr"]),
              dc=_lib.ptr(bufs["dc"]), status=_lib.ptr(bufs["status"]), kkt=_lib.ptr(bufs["kkt"]), scratch=_lib.ptr(bufs["scratch"]))
    order = ("g", "x1", "x2", "x0", "y0", "max_iters", "check_every", "eps", "step", "beta", "ruiz", "pc", "pw", "span", "lds", "x", "y", "dr", "dc",
             "status", "kkt", "scratch")
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
        assert L.mllp_lp_pdhg_scaled(*[args[k] for k in order], _lib.current_stream()) == EINVAL, kw
        assert b"mllp_lp_pdhg_scaled:" in L.mllp_last_error(), kw
    torch.cuda.synchronize()
    same_bits({k: v.view(torch.int32).cpu().numpy() for k, v in bufs.items()}, before, "buffers after the refused calls")
    # the same arguments without a fault are accepted (kkt, dr and dc may be NULL)
    assert L.mllp_lp_pdhg_scaled(*[dict(ok, kkt=z, dr=z, dc=z, eps=0.0)[k] for k in order], _lib.current_stream()) == 0
    assert L.mllp_lp_pdhg_scaled(*[dict(ok, eps=0.0, ruiz=64, span=1.0)[k] for k in order], _lib.current_stream()) == 0
    torch.cuda.synchronize()
    assert (bufs["status"].view(K, 4)[:, 0] == 6).all() and torch.isnan(bufs["kkt"]).sum() == 0
    assert torch.isnan(bufs["dr"]).sum() == 0 and torch.isnan(bufs["dc"]).sum() == 0 and torch.isnan(bufs["x"][:c["N"]]).sum() == 0


def test_an_empty_instance_and_an_empty_side(LPBatch):
    """n = 0 or m = 0 is legal: no rows leaves x to the costs alone (eta = step, w0 = 1: |dr b| = 0), no columns leaves y to b"""
    c = tb.dense_case([np.zeros((0, 3)), tb.int_matrix(3, 6, 0.7, 12), np.zeros((2, 0))], 1)
    c["c"][:3] = [1.0, 2.0, 0.0]
    b = tb._build(LPBatch, c, tb._dev(c["c"]), tb._dev(c["b"]))
    h = _host(b.pdhg_scaled(128, eps=EPS, x0=tb._dev(np.ones(c["N"], np.float32))))
    assert list(h["status"][0][:2]) == [0, 64] and np.array_equal(h["x"][:3], [0.0, 0.0, 1.0])
    assert list(h["kkt"][0][3:]) == [np.float32(0.9), 1.0, 1.0] and list(h["kkt"][2][3:]) == [np.float32(0.9), 1.0, 1.0]
    assert h["status"][2][1] in (64, 128) and h["status"][2][0] in (0, 6) and np.isfinite(h["kkt"]).all()
    assert (h["dc"][:3] == 1).all() and (h["dr"][3:] == 1).all() and len(h["dr"]) == 5 and len(h["dc"]) == 9
    mid = ps.solve(c["mats"][1], c["b"][:3], c["c"][3:9], 128, eps=EPS, x0=np.ones(6))
    assert list(h["status"][1][:2]) == mid["status"][:2] or mid["margin"] < 2.0 ** -7
    dr, dc = ps.scaling(np.asarray(c["mats"][1], np.float32), 10, False, np.float32)
    alone = _host(b.pdhg_scaled(0, pock_chambolle=False))
    assert np.array_equal(alone["dr"][:3], dr) and np.array_equal(alone["dc"][3:9], dc)


# ---------------------------------------------------------------------------------------------------
# driver
# ---------------------------------------------------------------------------------------------------
def test_driver_reports_pdhg_scaled(tmp_path, monkeypatch):
    """`scaled: true` and `scaled: {...}` inside `report_solved: pdhg` select the preconditioned call for the same three
    log keys; an unknown option is refused"""
    import json
    from mllp_amd import experiment
    cfg = ("train_data_type: 'planted'\ntrain_lr: 1.e-3\ntrain_iter: 1\nmethods:\n  - 'gs-topk'\nbatch_size: 3\nholdout: 0.25\n"
           "planted: {instances: 8, m: 20, n: 50, row_nnz: 4, seed: 5}\n")
    base = {"obj", "val_obj", "usable", "feasible", "optimal", "skipped"} | {f"planted{5 + i}" for i in range(8)}
    from mllp_amd.graph import LPBatch as Batch
    calls, inner = [], Batch.pdhg_scaled

    def recorded(self, max_iters, **kw):
        calls.append({k: kw.get(k) for k in ("ruiz", "pock_chambolle", "primal_weight", "weight_span")})
        return inner(self, max_iters, **kw)
    monkeypatch.setattr(Batch, "pdhg_scaled", recorded)
    blocks = {"pdhg: {iters: 4096, eps: 1.e-3, warm: false}": None,
              "pdhg: {iters: 4096, eps: 1.e-3, scaled: true}": dict(ruiz=10, pock_chambolle=True, primal_weight=True, weight_span=16.0),
              "pdhg: {iters: 4096, eps: 1.e-3, warm: false, scaled: {ruiz: 4, pock_chambolle: false, span: 4}}":
                  dict(ruiz=4, pock_chambolle=False, primal_weight=True, weight_span=4.0)}
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
    with pytest.raises(ValueError):
        experiment.pdhg_counts(None, None, {"pdhg": {"iters": 5, "eps": 1e-3, "warm": False, "scaled": {"passes": 3}}})
