"""GPU: mllp_lp_pdhg_spectral (mllp_lp_pdhg_rays with a step from power iteration on the device; csrc/pdhg_wide.hip).

THREE BARS.  (1) With power_iters = 0 every output of mllp_lp_pdhg_rays, and that call's whole scratch layout with its state
words, is that call's BIT FOR BIT; d_norm is {0, the bound}.  (2) The estimate is held to the fp64 oracle
(tests/pdhg_spectral_oracle.py) by the project's bar: 8 x the largest deviation of the fp32 oracle from the fp64 oracle over the
test's own instances, in units of 2^-24 sigma, per P; the figure is asserted finite before the device is looked at.  What follows
from the estimate is exact: kkt[3] = fdiv(step, norm[0]) and fdiv(step, norm[1]) = mllp_lp_pdhg_wide's eta, bit for bit.
(3) x and y after K plain iterations, and the decisions of the guarded instances, against the oracle by tests/test_pdhg_halpern.py's
protocol under the new step.

THE GUARD.  Decisions are compared only where the fp64 oracle's margin is at least 2^-7 and the fp32 oracle takes the same
decisions, asserted before the device is looked at.  Re-derived on the CPU under power_iters = 40 over the seeds 27, 22, 43 of the
three shapes: 5 x 12: 27 (margin 0.154), 22 (0.625), not 43 (0.005);  40 x 100: 22 (0.045), 43 (0.026), not 27 (0.003);  193 x 400:
all three (0.66, 0.38, 0.137).  Used: 27, 22, 43 -- the seeds of tests/test_pdhg_scaled.py still qualify.

Batches: `plain` and `trace` are tests/test_pdhg_wide.py's (5 x 12, 40 x 100, 193 x 400 and the long-row instance; the three
guarded instances), and an empty-sided batch with an all-zero instance.
"""
import ctypes

import numpy as np
import pytest
import torch

import pdhg_spectral_oracle as so
import test_basis_repair as tb
from guarded import PATTERNS, Guarded, same_bits
from mllp_amd import _lib
from test_basis_repair import LPBatch  # noqa: F401  (the fixture)
from test_pdhg_rays import _join
from test_pdhg_scaled import _bits, _host, _part, _units
from test_pdhg_wide import plain, trace  # noqa: F401  (the fixtures of that file: its batches)

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -10
MARGIN = 2.0 ** -7
STEP = np.float32(0.9)
RAYS = ("x", "y", "status", "kkt", "dr", "dc", "ray_x", "ray_y", "cert")
ALL = RAYS + ("norm",)
OUTS = ("x", "y", "dr", "dc", "ray_x", "ray_y", "status", "kkt", "cert", "norm")          # the C call's order


def _scratch_bytes(b, rows=0, fn="mllp_lp_pdhg_spectral_scratch_bytes"):
    n = ctypes.c_int64(-1)
    _lib.check(getattr(_lib.lib(), fn)(b._h, rows, ctypes.byref(n)))
    return n.value


class Raw:
    """the outputs and the scratch of a sequence of C calls on one batch (Guarded, at the natural alignment of a float);
    `fn`: mllp_lp_pdhg_spectral, or mllp_lp_pdhg_rays on the same buffers without d_norm"""

    def __init__(self, g, fn="mllp_lp_pdhg_spectral", fill=PATTERNS["nan"], rows=0):
        c, b = g["c"], g["b"]
        K = len(c["inst_m"])
        self.b, self.rows, self.fn = b, rows, fn
        f = lambda n, name, shift, dtype=torch.float32: Guarded(n, dtype, "cuda", fill=fill, name=name, shift=shift)       # noqa: E731
        self.o = dict(x=f(c["N"], "x", 4), y=f(c["M"], "y", 8), dr=f(c["M"], "dr", 12), dc=f(c["N"], "dc", 8), ray_x=f(c["N"], "ray_x", 12),
                      ray_y=f(c["M"], "ray_y", 4), status=f(4 * K, "status", 4, torch.int32), kkt=f(6 * K, "kkt", 4), cert=f(4 * K, "cert", 8))
        if fn.endswith("spectral"):
            self.o["norm"] = f(2 * K, "norm", 12)
        self.scratch = f(_scratch_bytes(b, rows, fn + "_scratch_bytes") // 4, "scratch", 4)

    def call(self, begin, end, check_every=64, eps=EPS, ray_eps=-1.0, power=40):
        b, spec = self.b, self.fn.endswith("spectral")
        outs = [self.o[k].ptr for k in OUTS if k in self.o]
        rc = getattr(_lib.lib(), self.fn)(b._h, _lib.ptr(b.x1), _lib.ptr(b.x2), None, None, begin, end, check_every, eps, 0.9, 0.5, 10, 1, 1, 16.0, 1,
                                          ray_eps, *([power] if spec else []), self.rows, *outs, self.scratch.ptr, _lib.current_stream())
        assert rc == 0, _lib.lib().mllp_last_error()
        torch.cuda.synchronize()
        for v in list(self.o.values()) + [self.scratch]:
            v.check()
        return {k: v.bits().view(np.int32) for k, v in self.o.items()}


# ---------------------------------------------------------------------------------------------------
# 1. power_iters = 0: the rays call's bits
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [64, 0])
@pytest.mark.parametrize("K", [0, 1, 64])
@pytest.mark.parametrize("ray_eps", [EPS, -1.0])
def test_zero_rounds_are_the_rays_call_in_every_output_and_in_the_state(plain, ray_eps, K, rows):  # noqa: F811
    n_inst = plain["b"].n_inst
    mine, theirs = Raw(plain, rows=rows), Raw(plain, "mllp_lp_pdhg_rays", rows=rows)
    got, want = mine.call(0, K, ray_eps=ray_eps, power=0), theirs.call(0, K, ray_eps=ray_eps)
    same_bits({k: got[k] for k in want}, want, f"ray_eps = {ray_eps}, K = {K}, rows_per_item = {rows}")
    # the scratch: the rays' layout word for word (the 16 state words of every instance and its cert words among them), two words behind
    s_mine, s_theirs = mine.scratch.bits().view(np.int32), theirs.scratch.bits().view(np.int32)
    assert len(s_mine) == len(s_theirs) + 2 * n_inst
    same_bits(dict(scratch=s_mine[:len(s_theirs)]), dict(scratch=s_theirs), "the rays' words of the scratch")
    norm = got["norm"].view(np.float32).reshape(-1, 2)
    assert (norm[:, 0] == 0).all() and np.array_equal(s_mine[len(s_theirs):].view(np.float32).reshape(-1, 2), norm)
    eta = got["kkt"].view(np.float32).reshape(-1, 6)[:, 3]
    assert np.array_equal(STEP / norm[:, 1], eta)            # the bound is the value from which that eta follows


@pytest.mark.parametrize("rows", [64, None])
def test_zero_rounds_are_the_halpern_call_at_the_decisions(trace, rows):  # noqa: F811
    from mllp_amd.graph import LPPdhgRays, LPPdhgSpectral
    res = trace["b"].pdhg_spectral(8192, eps=EPS, power_iters=0, rows_per_item=rows)
    assert isinstance(res, LPPdhgSpectral) and isinstance(res, LPPdhgRays) and res.calls == 1
    got = _host(res, ALL)
    same_bits(_bits({k: got[k] for k in trace["want"]}), trace["want"], f"8192 iterations, power_iters = 0, rows_per_item = {rows}")
    assert not got["ray_x"].any() and not got["ray_y"].any() and (got["norm"][:, 0] == 0).all()


# ---------------------------------------------------------------------------------------------------
# 2. the estimate
# ---------------------------------------------------------------------------------------------------
def _estimates(insts, P):
    """per instance (fp32 oracle, fp64 oracle) of sigma_est"""
    import pdhg_scaled_oracle as ps
    import scipy.sparse as sp
    out = []
    for i in insts:
        pair = []
        for dt in (np.float32, np.float64):
            dr, dc = ps.scaling(sp.csr_matrix(i["A"], dtype=dt), 10, True, dt)
            pair.append(so.power(i["A"], dr, dc, P, dt)[0])
        out.append(tuple(pair))
    return out


@pytest.mark.parametrize("P", [1, 2, 40])
def test_the_estimate_is_the_oracles(plain, P):  # noqa: F811
    c, b = plain["c"], plain["b"]
    est = _estimates(plain["insts"], P)
    devs = [_units(e32, e64) for e32, e64 in est]
    assert np.isfinite(devs).all() and all(np.isfinite(e64) and e64 > 0 for _, e64 in est), (devs, est)     # before the device is looked at
    bar = 8.0 * max(devs)
    print(f"P = {P}: fp32 oracle against fp64 oracle {['%.2f' % d for d in devs]} units -> bar {bar:.2f}")
    wide = _host(b.pdhg_wide(0), ("kkt",))["kkt"]
    for rows in (64, None):
        got = _host(b.pdhg_spectral(0, power_iters=P, rows_per_item=rows), ALL)
        failed = []
        for k, (_, e64) in enumerate(est):
            u = _units(got["norm"][k, 0], e64)
            print(f"P = {P}, rows_per_item = {rows}, instance {k} ({c['inst_m'][k]} x {c['inst_n'][k]}): device {got['norm'][k, 0]!r}, {u:.2f} units, bar {bar:.2f}")
            if not u <= bar:
                failed.append((k, u, bar))
        # what follows from the estimate is exact: the bound is the wide call's, the step is fdiv(step, sigma_est)
        assert np.array_equal(STEP / got["norm"][:, 1], wide[:, 3]), (got["norm"], wide[:, 3])
        assert (got["norm"][:, 0] > 0).all() and (got["norm"][:, 0] <= got["norm"][:, 1]).all()
        assert np.array_equal(got["kkt"][:, 3], STEP / got["norm"][:, 0]), (got["kkt"][:, 3], got["norm"])
        assert [list(s) for s in got["status"]] == [[6, 0, 0, 0]] * b.n_inst
        assert not failed, (P, rows, failed)


# ---------------------------------------------------------------------------------------------------
# 3. iterations and decisions under the new step
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runs(plain):  # noqa: F811
    """per K the two oracle runs of every instance of `plain` at power_iters = 40, and the largest deviation between them"""
    out = {}
    for K in (64, 512):
        pairs = [(so.solve(i["A"], i["b"], i["c"], K, check_every=0), so.solve(i["A"], i["b"], i["c"], K, check_every=0, dtype=np.float32))
                 for i in plain["insts"]]
        dev = max(max(_units(f["x"], a["x"]), _units(f["y"], a["y"])) for a, f in pairs)
        assert np.isfinite(dev)
        print(f"K = {K}: fp32 oracle against fp64 oracle, largest deviation {dev:.2f} units -> bar {8 * dev:.1f}")
        out[K] = (pairs, dev)
    return out


@pytest.mark.parametrize("K", [64, 512])
def test_plain_iterations_against_the_oracle(plain, runs, K):  # noqa: F811
    c, b = plain["c"], plain["b"]
    pairs, dev = runs[K]
    bar = 8.0 * dev
    h = _host(b.pdhg_spectral(K, check_every=0), ALL)
    for k, (a, _) in enumerate(pairs):
        got = _part(c, h, k)
        assert list(got["status"]) == [6, K, 0, 0] and not a["fallback"], (k, got["status"])
        ux, uy = _units(got["x"], a["x"]), _units(got["y"], a["y"])
        print(f"K = {K}, instance {k} ({c['inst_m'][k]} x {c['inst_n'][k]}): x {ux:.2f} units, y {uy:.2f} units, bar {bar:.1f}")
        assert ux <= bar and uy <= bar, (K, k, ux, uy, bar)


@pytest.fixture(scope="module")
def guarded(trace):  # noqa: F811
    o64 = [so.solve(i["A"], i["b"], i["c"], 8192, eps=EPS) for i in trace["insts"]]
    o32 = [so.solve(i["A"], i["b"], i["c"], 8192, eps=EPS, dtype=np.float32) for i in trace["insts"]]
    for o, f in zip(o64, o32):         # the condition, from the oracles alone
        print("oracle", o["status"], "fp32 oracle", f["status"], "margin", o["margin"], "norm", o["norm"])
        assert o["margin"] >= MARGIN and o["status"][0] == 0 and o["status"] == f["status"] and not o["fallback"], (o["status"], f["status"], o["margin"])
    return dict(o64=o64, o32=o32, host=_host(trace["b"].pdhg_spectral(8192, eps=EPS), ALL))


def test_the_decisions_of_guarded_instances(trace, runs, guarded):  # noqa: F811
    c, h = trace["c"], guarded["host"]
    for k, (o, f) in enumerate(zip(guarded["o64"], guarded["o32"])):
        got = _part(c, h, k)
        print(f"instance {k}: oracle {o['status']} margin {o['margin']:.4f}, device {list(got['status'])}")
        assert list(got["status"]) == f["status"] == o["status"], (k, got["status"], o["status"])
        bar = 8.0 * runs[512][1] * max(o["status"][1] / 512.0, 1.0)
        ux, uy = _units(got["x"], o["x"]), _units(got["y"], o["y"])
        print(f"instance {k}: x {ux:.2f} units, y {uy:.2f} units, bar {bar:.1f}")
        assert ux <= bar and uy <= bar, (k, ux, uy, bar)
    # pdhg_basis takes the result unchanged
    res = trace["b"].pdhg_spectral(8192, eps=EPS)
    out = trace["b"].pdhg_basis(res)
    torch.cuda.synchronize()
    assert np.array_equal(out.basis.cpu().numpy(), trace["st"]["labels"])


def test_the_long_rows_end_at_the_oracles_count(plain):  # noqa: F811
    inst = plain["insts"][3]
    o32, o64 = (so.solve(inst["A"], inst["b"], inst["c"], 4096, eps=EPS, dtype=dt) for dt in (np.float32, np.float64))
    base = so.solve(inst["A"], inst["b"], inst["c"], 4096, eps=EPS, power_iters=0, dtype=np.float32)
    assert o32["status"] == o64["status"] and o32["status"][0] == 0 and o32["status"][1] < base["status"][1], (o32["status"], base["status"])
    got = _part(plain["c"], _host(plain["b"].pdhg_spectral(4096, eps=EPS), ALL), 3)
    print("long rows: oracle", o32["status"], "at power_iters = 0", base["status"], "device", list(got["status"]))
    assert list(got["status"]) == o32["status"]


# ---------------------------------------------------------------------------------------------------
# 4. execution moves no bit
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 2, 3])
def test_an_instance_alone_has_its_bits_inside_the_batch(LPBatch, plain, k):  # noqa: F811
    inside = _host(plain["b"].pdhg_spectral(128, eps=EPS), ALL)
    alone = _join(LPBatch, [plain["insts"][k]])
    for rows in (None, 128):
        got = _host(alone["b"].pdhg_spectral(128, eps=EPS, rows_per_item=rows), ALL)
        want = dict(_part(plain["c"], inside, k), norm=inside["norm"][k])
        same_bits(_bits({n: got[n] for n in want}), _bits(want), f"instance {k} alone (rows_per_item = {rows}) against inside the batch")


@pytest.mark.parametrize("split", [(64, 128), (63, 65)])
def test_two_calls_give_the_single_calls_bits(trace, split):  # noqa: F811
    K1, K2 = split
    single = Raw(trace).call(0, K2)
    two = Raw(trace, rows=128)
    first = two.call(0, K1)
    assert (first["status"].reshape(-1, 4)[:, 0] == 6).all()
    second = two.call(K1, K2, power=7)          # (ignored: the set-up does not run, eta and d_norm are the state's)
    same_bits(second, single, f"(0, {K1}) then ({K1}, {K2}) against (0, {K2})")
    assert (single["norm"].view(np.float32).reshape(-1, 2)[:, 0] > 0).all()


def test_polling_gives_the_single_calls_bits(trace, guarded):  # noqa: F811
    want = _bits(guarded["host"])
    last = int(guarded["host"]["status"][:, 1].max())
    res = trace["b"].pdhg_spectral(8192, eps=EPS, poll_every=128)
    same_bits(_bits(_host(res, ALL)), want, "poll_every = 128 against the single call")
    assert res.calls == -(-last // 128) < 8192 // 128


# ---------------------------------------------------------------------------------------------------
# 5. the fallback
# ---------------------------------------------------------------------------------------------------
def test_empty_sides_and_an_all_zero_instance_take_the_bounds_step(LPBatch):  # noqa: F811
    c = tb.dense_case([np.zeros((0, 3)), tb.int_matrix(3, 6, 0.7, 12), np.zeros((2, 0)), np.zeros((2, 3))], 1)
    b = tb._build(LPBatch, c, tb._dev(c["c"]), tb._dev(c["b"]))
    x0 = tb._dev(np.ones(c["N"], np.float32))
    for K in (0, 128):
        base = _host(b.pdhg_spectral(K, eps=EPS, power_iters=0, x0=x0), ALL)
        got = _host(b.pdhg_spectral(K, eps=EPS, power_iters=40, x0=x0), ALL)
        print(K, got["status"].tolist(), got["norm"].tolist(), got["kkt"][:, 3].tolist())
        assert got["norm"].shape == (4, 2) and list(got["norm"][[0, 2, 3], 0]) == [0, 0, 0] and list(got["norm"][[0, 2, 3], 1]) == [0, 0, 0]
        assert list(got["kkt"][[0, 2, 3], 3]) == [STEP] * 3 and got["norm"][1, 0] > 0 and got["kkt"][1, 3] == STEP / got["norm"][1, 0]
        for k in (0, 2, 3):         # an instance that fell back has the bits of the call without rounds
            same_bits(_bits(dict(_part(c, got, k), norm=got["norm"][k])), _bits(dict(_part(c, base, k), norm=base["norm"][k])), f"instance {k}, K = {K}")


@pytest.mark.parametrize("m", [3, 193])
def test_scratch_bytes_is_the_headers_closed_form(LPBatch, m):  # noqa: F811
    shapes = [(m, 2 * m + 6), (5, 12)]
    b = tb._build(LPBatch, tb.planted_shapes(shapes, 40))
    M, N = sum(s[0] for s in shapes), sum(s[1] for s in shapes)
    for rows in (0, 64, 128, 4096):
        assert _scratch_bytes(b, rows) == 4 * (29 * len(shapes) + 6 * N + 5 * M), (m, rows)
    from mllp_amd.graph import pdhg_spectral_limits
    assert pdhg_spectral_limits() == (1024, 64, 64, 4096, 1024)
    for bad in (-1, 1025):
        with pytest.raises(ValueError):
            b.pdhg_spectral(8, power_iters=bad)


# ---------------------------------------------------------------------------------------------------
# 6. the driver
# ---------------------------------------------------------------------------------------------------
def test_driver_selects_the_spectral_call(tmp_path, monkeypatch):
    """`spectral: true` and `spectral: {iters: P}` inside `report_solved: pdhg` select LPBatch.pdhg_spectral (and imply `wide`), alone
    and beside `rays`; without the key no call reaches it and every log key is the one it was"""
    import json
    from mllp_amd import experiment
    from mllp_amd.graph import LPBatch as Batch
    cfg = ("train_data_type: 'planted'\ntrain_lr: 1.e-3\ntrain_iter: 1\nmethods:\n  - 'gs-topk'\nbatch_size: 3\nholdout: 0.25\n"
           "planted: {instances: 8, m: 20, n: 50, row_nnz: 4, seed: 5}\n")
    base = {"obj", "val_obj", "usable", "feasible", "optimal", "skipped"} | {f"planted{5 + i}" for i in range(8)}
    calls, inner = [], Batch.pdhg_spectral

    def recorded(self, max_iters, **kw):
        calls.append({k: kw.get(k) for k in ("power_iters", "ray_eps", "rows_per_item", "poll_every", "reflect")})
        res = inner(self, max_iters, **kw)
        calls[-1]["estimates"] = res.norm[:, 0].cpu().tolist()
        return res
    monkeypatch.setattr(Batch, "pdhg_spectral", recorded)
    blocks = {"pdhg: {iters: 2048, eps: 1.e-3, wide: true}": None,
              "pdhg: {iters: 2048, eps: 1.e-3, spectral: false}": None,
              "pdhg: {iters: 2048, eps: 1.e-3, spectral: true}": dict(power_iters=40, ray_eps=None, rows_per_item=None, poll_every=None, reflect=True),
              "pdhg: {iters: 2048, eps: 1.e-3, warm: false, spectral: {iters: 8}, rays: {eps: 1.e-2}, wide: {rows: 128, poll: 512}}":
                  dict(power_iters=8, ray_eps=1e-2, rows_per_item=128, poll_every=512, reflect=True)}
    logs = {}
    for block, want in blocks.items():
        del calls[:]
        (tmp_path / "cfg.yaml").write_text(cfg + f"report_solved: {{feas_tol: 1.e-3, opt_tol: 1.e-3, max_m: 20, {block}}}\n")
        monkeypatch.chdir(tmp_path)
        assert experiment.main(["--cfg", str(tmp_path / "cfg.yaml")]) == 0
        log = json.load(open(tmp_path / "train_log.json"))
        keys = set(experiment.PDHG_KEYS) | (set(experiment.PDHG_RAY_KEYS) if "rays" in block else set())
        assert set(log) == base | keys, block
        logs[block] = {k: log[k][0] for k in keys}
        if want is None:
            assert calls == []
            continue
        assert calls and all({k: v for k, v in call.items() if k != "estimates"} == want for call in calls), (block, calls)
        assert all(e > 0 for call in calls for e in call["estimates"])
    keys = list(blocks)
    print({k: logs[k] for k in keys})
    assert logs[keys[2]]["pdhg_converged"] >= 1
    for wrong in ({"spectral": {"rounds": 3}}, {"spectral": True, "wide": False}, {"spectral": {"iters": -1}}, {"spectral": True, "scaled": False},
                  {"spectral": True, "rays": True, "wide": False}):
        with pytest.raises(ValueError):
            experiment.pdhg_counts(None, None, {"pdhg": {"iters": 5, "eps": 1e-3, "warm": False, **wrong}})
