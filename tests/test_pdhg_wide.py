"""GPU: mllp_lp_pdhg_wide (mllp_lp_pdhg_halpern's rule as ordinary launches across the whole device; csrc/pdhg_wide.hip).

THE BAR is bit equality with `LPBatch.pdhg_halpern` on the same batch, in x, y, dr, dc, status and kkt: that call is held to
the numpy oracle of the rule by tests/test_pdhg_halpern.py, and the wide call claims to be a second execution of the SAME
rule.  No new oracle, no tolerance.  Batches, helpers and seeds are that file's.

Shapes.  `plain`: 5 x 12 (one item per orientation), 40 x 100 (two column items at rows_per_item = 64), 193 x 400 (four row
items with a ragged last block of one row, seven column items) and the long-row instance of planted_oracle.ragged_case (the
block tier under the sweeps).  rows_per_item 64, 128 and the default.
"""
import ctypes

import numpy as np
import pytest
import torch

import pdhg_oracle as pg
import planted_oracle as po
import test_basis_repair as tb
from guarded import PATTERNS, Guarded, same_bits
from mllp_amd import _lib
from test_basis_repair import LPBatch  # noqa: F401  (the fixture)
from test_pdhg_scaled import SMALL, TRACE, _batch, _bits, _host, _part

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -10
EINVAL = -1
STALE = 9
ORDER = ("g", "x1", "x2", "x0", "y0", "iter_begin", "iter_end", "check_every", "eps", "step", "beta", "ruiz", "pc", "pw", "span", "reflect",
         "rows", "x", "y", "dr", "dc", "status", "kkt", "scratch")


def _scratch_bytes(b, rows=0):
    n = ctypes.c_int64(-1)
    _lib.check(_lib.lib().mllp_lp_pdhg_wide_scratch_bytes(b._h, rows, ctypes.byref(n)))
    return n.value


@pytest.fixture(scope="module")
def plain(LPBatch):
    g = _batch(LPBatch, pg.join_cases([tb.planted_shapes(SMALL, 20), po.ragged_case(which=[4])]))
    g["want"] = {}
    return g


@pytest.fixture(scope="module")
def trace(LPBatch):
    g = _batch(LPBatch, pg.join_cases([tb.planted_shapes([shape], seed) for shape, seed in TRACE]))
    g["want"] = _bits(_host(g["b"].pdhg_halpern(8192, eps=EPS, check_every=64)))
    return g


# ---------------------------------------------------------------------------------------------------
# plain iterations
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [64, 128, None])
@pytest.mark.parametrize("reflect", [True, False])
@pytest.mark.parametrize("K", [0, 1, 64, 512])
def test_plain_iterations_have_the_persistent_calls_bits(plain, K, reflect, rows):
    b = plain["b"]
    if (K, reflect) not in plain["want"]:       # the reference, once per (K, reflect)
        plain["want"][K, reflect] = _bits(_host(b.pdhg_halpern(K, check_every=0, reflect=reflect)))
    res = b.pdhg_wide(K, check_every=0, reflect=reflect, rows_per_item=rows)
    got = _host(res)
    assert [list(s) for s in got["status"]] == [[6, K, 0, 0]] * b.n_inst and res.calls == 1
    same_bits(_bits(got), plain["want"][K, reflect], f"K = {K}, reflect = {reflect}, rows_per_item = {rows}")


def test_the_long_rows_and_the_ragged_block_are_under_the_sweeps(plain):
    c = plain["c"]
    assert list(c["inst_m"][:3]) == [5, 40, 193] and 193 % 64 == 1 and c["inst_n"][1] > 64
    inst = plain["insts"][3]
    assert max(np.diff(inst["A"].indptr).max(), np.diff(inst["A"].tocsc().indptr).max()) > 1024


# ---------------------------------------------------------------------------------------------------
# decisions
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [64, None, 128])
def test_decisions_restarts_and_weights(trace, rows):
    b = trace["b"]
    status = trace["want"]["status"].reshape(-1, 4)
    # every instance stops, after restarts, and not all at one check: an instance goes idle while another runs
    assert (status[:, 0] == 0).all() and len(set(status[:, 1])) >= 2 and (status[:, 2] >= 1).all(), status
    from mllp_amd.graph import LPPdhgHalpern, LPPdhgWide
    res = b.pdhg_wide(8192, eps=EPS, check_every=64, rows_per_item=rows)
    assert isinstance(res, LPPdhgWide) and isinstance(res, LPPdhgHalpern)
    same_bits(_bits(_host(res)), trace["want"], f"8192 iterations, rows_per_item = {rows}")


def test_decisions_under_other_options(trace):
    c, b, st = trace["c"], trace["b"], trace["st"]
    rep = b.solve_basis(b.labels)
    rng = np.random.default_rng(7)
    x0, y0 = tb._dev(rng.uniform(-1.0, 1.0, c["N"]).astype(np.float32)), tb._dev(rng.uniform(-1.0, 1.0, c["M"]).astype(np.float32))
    for kw in (dict(max_iters=8192, eps=EPS, primal_weight=False), dict(max_iters=1000, eps=EPS, check_every=48),
               dict(max_iters=100, eps=EPS, check_every=48), dict(max_iters=256, eps=EPS, x0=x0, y0=y0), dict(max_iters=8192, eps=EPS, start=rep),
               dict(max_iters=8192, eps=EPS, reflect=False, weight_span=1.0)):
        want = _host(b.pdhg_halpern(**kw))
        print(kw.keys(), [list(s) for s in want["status"]])
        same_bits(_bits(_host(b.pdhg_wide(**kw))), _bits(want), f"{sorted(kw)}")
    limit = _host(b.pdhg_halpern(100, eps=EPS, check_every=48))["status"]
    assert [list(s[:2]) for s in limit] == [[6, 100]] * 3 and 100 % 48 and 1000 % 48, limit         # a limit between two checks, on instances that run
    with pytest.raises(ValueError):
        b.pdhg_wide(64, start=rep, x0=x0)
    for bad in (dict(rows_per_item=0), dict(rows_per_item=96), dict(rows_per_item=1 << 20), dict(poll_every=0)):
        with pytest.raises(ValueError):
            b.pdhg_wide(64, **bad)
    # pdhg_basis takes the result unchanged
    res = b.pdhg_wide(8192, eps=EPS)
    out = b.pdhg_basis(res)
    torch.cuda.synchronize()
    assert np.array_equal(out.basis.cpu().numpy(), st["labels"])


# ---------------------------------------------------------------------------------------------------
# continuation and stale state, through the C ABI on the test's own buffers
# ---------------------------------------------------------------------------------------------------
class Raw:
    """the outputs and the scratch of a sequence of C calls on one batch (Guarded, at the natural alignment of a float)"""

    def __init__(self, g, fill=PATTERNS["nan"], rows=0):
        c, b = g["c"], g["b"]
        K = len(c["inst_m"])
        self.b, self.rows = b, rows
        self.o = dict(x=Guarded(c["N"], device="cuda", fill=fill, name="x", shift=4), y=Guarded(c["M"], device="cuda", fill=fill, name="y", shift=8),
                      dr=Guarded(c["M"], device="cuda", fill=fill, name="dr", shift=12), dc=Guarded(c["N"], device="cuda", fill=fill, name="dc", shift=8),
                      status=Guarded(4 * K, torch.int32, "cuda", fill=fill, name="status", shift=4),
                      kkt=Guarded(6 * K, device="cuda", fill=fill, name="kkt", shift=4))
        self.scratch = Guarded(_scratch_bytes(b, rows) // 4, device="cuda", fill=fill, name="scratch", shift=4)

    def call(self, begin, end, check_every=64, eps=EPS):
        b = self.b
        rc = _lib.lib().mllp_lp_pdhg_wide(b._h, _lib.ptr(b.x1), _lib.ptr(b.x2), None, None, begin, end, check_every, eps, 0.9, 0.5, 10, 1, 1, 16.0,
                                          1, self.rows, *[self.o[k].ptr for k in ("x", "y", "dr", "dc", "status", "kkt")], self.scratch.ptr,
                                          _lib.current_stream())
        assert rc == 0, _lib.lib().mllp_last_error()
        torch.cuda.synchronize()
        for v in list(self.o.values()) + [self.scratch]:
            v.check()
        return {k: v.bits().view(np.int32) for k, v in self.o.items()}


def _rows(flat):
    """the flat bit arrays of a result with status and kkt as [n_inst, .]"""
    return {n: v.reshape(-1, 4) if n == "status" else v.reshape(-1, 6) if n == "kkt" else v for n, v in flat.items()}


@pytest.mark.parametrize("split", [(100, 8192), (64, 128), (63, 65)])
def test_two_calls_give_the_single_calls_bits(trace, split):
    K1, K2 = split
    single = Raw(trace).call(0, K2)
    if K2 == 8192:
        same_bits(single, trace["want"], "the C call on guarded buffers against pdhg_halpern")
    two = Raw(trace, rows=128)
    first = two.call(0, K1)
    assert (first["status"].reshape(-1, 4)[:, 1] <= K1).all() and (first["status"].reshape(-1, 4)[:, 0] == 6).any()
    same_bits(two.call(K1, K2), single, f"(0, {K1}) then ({K1}, {K2}) against (0, {K2})")


def test_polling_stops_early_with_the_single_calls_bits(trace):
    b = trace["b"]
    last = int(trace["want"]["status"].reshape(-1, 4)[:, 1].max())
    res = b.pdhg_wide(8192, eps=EPS, check_every=64, poll_every=256)
    same_bits(_bits(_host(res)), trace["want"], "poll_every = 256 against the single call")
    print("last stop at", last, "calls", res.calls)
    assert res.calls == -(-last // 256) < 8192 // 256
    # a limit that is no multiple of the chunk, and none that stops
    want = _bits(_host(b.pdhg_halpern(300, eps=0.0, check_every=64)))
    res = b.pdhg_wide(300, eps=0.0, check_every=64, poll_every=128)
    same_bits(_bits(_host(res)), want, "poll_every = 128, 300 iterations")
    assert res.calls == 3


def test_a_stopped_instance_keeps_its_bits_through_later_calls(trace):
    want = trace["want"]
    its = want["status"].reshape(-1, 4)[:, 1]
    first_stop = int(its.min())
    r = Raw(trace)
    at = r.call(0, first_stop)
    k = int(np.argmin(its))
    assert at["status"].reshape(-1, 4)[k, 0] == 0 and (at["status"].reshape(-1, 4)[:, 0] == 6).sum() == (its > first_stop).sum() >= 1
    c = trace["c"]
    for begin, end in ((first_stop, first_stop + 64), (first_stop + 64, 8192), (8192, 8192), (8192, 8300)):
        got = r.call(begin, end)
        same_bits(_bits(_part(c, _rows(got), k)), _bits(_part(c, _rows(want), k)), f"instance {k} after ({begin}, {end})")
        if end == 8192:
            same_bits(got, want, f"every instance after ({begin}, {end})")


@pytest.mark.parametrize("fill", list(PATTERNS))
def test_stale_state_is_refused_per_instance(trace, fill):
    r = Raw(trace, fill=PATTERNS[fill])
    before = r.scratch.bits()
    got = r.call(64, 128)
    assert [list(s) for s in got["status"].reshape(-1, 4)] == [[STALE, 0, 0, 0]] * 3
    assert all((got[k] == 0).all() for k in ("x", "y", "dr", "dc", "kkt"))
    K = 3
    state = lambda s: np.concatenate([s[21 * k:21 * k + 16] for k in range(K)])         # noqa: E731  (the sixteen state words of every instance)
    assert np.array_equal(state(r.scratch.bits()), state(before))                       # left as found
    # a real state that ended elsewhere
    single = r.call(0, 128)
    kept = r.scratch.bits()
    got = r.call(64, 128)
    assert [list(s) for s in got["status"].reshape(-1, 4)] == [[STALE, 0, 0, 0]] * 3 and all((got[k] == 0).all() for k in ("x", "y", "dr", "dc", "kkt"))
    assert np.array_equal(state(r.scratch.bits()), state(kept))
    same_bits(r.call(128, 256), Raw(trace).call(0, 256), "the state still continues where it ended")
    assert (single["status"].reshape(-1, 4)[:, 0] == 6).all()


# ---------------------------------------------------------------------------------------------------
# refusals, empty cases, scratch
# ---------------------------------------------------------------------------------------------------
def test_every_refusal_writes_nothing(trace):
    c, b = trace["c"], trace["b"]
    K, L, z = len(c["inst_m"]), _lib.lib(), ctypes.c_void_p(0)
    poison = lambda n: torch.full((n,), float("nan"), device="cuda")      # noqa: E731
    bufs = dict(x=poison(c["N"] + 8), y=poison(c["M"]), dr=poison(c["M"]), dc=poison(c["N"]), status=poison(4 * K).view(torch.int32), kkt=poison(6 * K),
                scratch=poison(_scratch_bytes(b) // 4))
    x0, y0 = tb._dev(np.ones(c["N"], np.float32)), tb._dev(np.ones(c["M"], np.float32))
    ok = dict(g=b._h, x1=_lib.ptr(b.x1), x2=_lib.ptr(b.x2), x0=_lib.ptr(x0), y0=_lib.ptr(y0), iter_begin=0, iter_end=128, check_every=64, eps=EPS,
              step=0.9, beta=0.5, ruiz=10, pc=1, pw=1, span=16.0, reflect=1, rows=0, x=_lib.ptr(bufs["x"]), y=_lib.ptr(bufs["y"]), dr=_lib.ptr(bufs["dr"]),
              dc=_lib.ptr(bufs["dc"]), status=_lib.ptr(bufs["status"]), kkt=_lib.ptr(bufs["kkt"]), scratch=_lib.ptr(bufs["scratch"]))
    nan, inf = float("nan"), float("inf")
    bad = [dict(g=None), dict(x1=z), dict(x2=z), dict(x=z), dict(y=z), dict(status=z), dict(iter_begin=-1), dict(iter_end=-1), dict(iter_begin=129),
           dict(iter_begin=64, iter_end=63), dict(check_every=-1),
           dict(eps=nan), dict(eps=inf), dict(eps=-1.0), dict(step=nan), dict(step=inf), dict(step=0.0), dict(step=-0.5), dict(step=1.5),
           dict(beta=nan), dict(beta=inf), dict(beta=0.0), dict(beta=1.0), dict(beta=-0.5), dict(scratch=z),
           dict(ruiz=-1), dict(ruiz=65), dict(span=nan), dict(span=inf), dict(span=0.999), dict(span=0.0), dict(span=-16.0),
           dict(rows=-64), dict(rows=1), dict(rows=96), dict(rows=4160), dict(rows=1 << 40),
           dict(x0=_lib.ptr(bufs["x"])), dict(y0=_lib.ptr(bufs["y"])), dict(x0=ctypes.c_void_p(bufs["x"].data_ptr() + 32)),
           dict(y0=_lib.ptr(bufs["kkt"])), dict(x0=_lib.ptr(bufs["status"])), dict(x0=_lib.ptr(bufs["dc"])), dict(y0=_lib.ptr(bufs["dr"])),
           dict(y0=_lib.ptr(bufs["dc"])), dict(x0=ctypes.c_void_p(bufs["dr"].data_ptr() + 4))]
    before = {k: v.view(torch.int32).cpu().numpy().copy() for k, v in bufs.items()}
    for kw in bad:
        args = dict(ok, **kw)
        assert L.mllp_lp_pdhg_wide(*[args[k] for k in ORDER], _lib.current_stream()) == EINVAL, kw
        assert b"mllp_lp_pdhg_wide:" in L.mllp_last_error(), kw
    n = ctypes.c_int64(-7)
    for rows in (-64, 1, 96, 4160):
        assert L.mllp_lp_pdhg_wide_scratch_bytes(b._h, rows, ctypes.byref(n)) == EINVAL and n.value == -7
    torch.cuda.synchronize()
    same_bits({k: v.view(torch.int32).cpu().numpy() for k, v in bufs.items()}, before, "buffers after the refused calls")
    # the same arguments without a fault are accepted (kkt, dr and dc may be NULL; reflect is 0 or not 0; the largest rows_per_item)
    assert L.mllp_lp_pdhg_wide(*[dict(ok, kkt=z, dr=z, dc=z, eps=0.0, reflect=0)[k] for k in ORDER], _lib.current_stream()) == 0
    assert L.mllp_lp_pdhg_wide(*[dict(ok, eps=0.0, ruiz=64, span=1.0, reflect=-3, rows=4096)[k] for k in ORDER], _lib.current_stream()) == 0
    torch.cuda.synchronize()
    assert (bufs["status"].view(K, 4)[:, 0] == 6).all() and torch.isnan(bufs["kkt"]).sum() == 0
    assert torch.isnan(bufs["dr"]).sum() == 0 and torch.isnan(bufs["dc"]).sum() == 0 and torch.isnan(bufs["x"][:c["N"]]).sum() == 0


def test_an_empty_instance_and_an_empty_side(LPBatch):
    c = tb.dense_case([np.zeros((0, 3)), tb.int_matrix(3, 6, 0.7, 12), np.zeros((2, 0))], 1)
    c["c"][:3] = [1.0, 2.0, 0.0]
    b = tb._build(LPBatch, c, tb._dev(c["c"]), tb._dev(c["b"]))
    x0 = tb._dev(np.ones(c["N"], np.float32))
    for K in (0, 128):
        want = _host(b.pdhg_halpern(K, eps=EPS, x0=x0))
        same_bits(_bits(_host(b.pdhg_wide(K, eps=EPS, x0=x0))), _bits(want), f"empty sides, {K} iterations")
    assert list(want["status"][0]) == [0, 64, 0, 0] and len(want["dr"]) == 5 and len(want["dc"]) == 9


@pytest.mark.parametrize("m", [3, 192, 193, 200])
def test_scratch_bytes_is_the_headers_closed_form(LPBatch, m):
    shapes = [(m, 2 * m + 6), (5, 12)]
    b = tb._build(LPBatch, tb.planted_shapes(shapes, 40))
    M, N = sum(s[0] for s in shapes), sum(s[1] for s in shapes)
    for rows in (0, 64, 128, 4096):
        assert _scratch_bytes(b, rows) == 4 * (21 * len(shapes) + 6 * N + 5 * M), (m, rows)
    assert "which is 4 (21 n_inst + 6 N + 5 M)" in " ".join(open(_lib.HEADER_PATH).read().replace("\n *", " ").split())
    from mllp_amd.graph import pdhg_wide_limits
    assert pdhg_wide_limits() == (1024, 64, 64, 4096)


# ---------------------------------------------------------------------------------------------------
# driver
# ---------------------------------------------------------------------------------------------------
def test_driver_reports_pdhg_wide(tmp_path, monkeypatch):
    """`wide: true` and `wide: {rows: R, poll: P}` inside `report_solved: pdhg` select the call for the same three log keys, with
    the `halpern:` and `scaled:` options; an unknown option and `scaled: false` beside it are refused"""
    import json
    from mllp_amd import experiment
    cfg = ("train_data_type: 'planted'\ntrain_lr: 1.e-3\ntrain_iter: 1\nmethods:\n  - 'gs-topk'\nbatch_size: 3\nholdout: 0.25\n"
           "planted: {instances: 8, m: 20, n: 50, row_nnz: 4, seed: 5}\n")
    base = {"obj", "val_obj", "usable", "feasible", "optimal", "skipped"} | {f"planted{5 + i}" for i in range(8)}
    from mllp_amd.graph import LPBatch as Batch
    calls, inner = [], Batch.pdhg_wide

    def recorded(self, max_iters, **kw):
        calls.append({k: kw.get(k) for k in ("ruiz", "pock_chambolle", "primal_weight", "weight_span", "reflect", "rows_per_item", "poll_every")})
        return inner(self, max_iters, **kw)
    monkeypatch.setattr(Batch, "pdhg_wide", recorded)
    blocks = {"pdhg: {iters: 2048, eps: 1.e-3, halpern: true}": None,
              "pdhg: {iters: 2048, eps: 1.e-3, wide: false}": None,
              "pdhg: {iters: 2048, eps: 1.e-3, wide: true}":
                  dict(ruiz=10, pock_chambolle=True, primal_weight=True, weight_span=16.0, reflect=True, rows_per_item=None, poll_every=None),
              "pdhg: {iters: 2048, eps: 1.e-3, warm: false, wide: {rows: 128, poll: 512}, halpern: {reflect: false}, scaled: {ruiz: 4, span: 4}}":
                  dict(ruiz=4, pock_chambolle=True, primal_weight=True, weight_span=4.0, reflect=False, rows_per_item=128, poll_every=512)}
    logs = {}
    for block, want in blocks.items():
        del calls[:]
        (tmp_path / "cfg.yaml").write_text(cfg + f"report_solved: {{feas_tol: 1.e-3, opt_tol: 1.e-3, max_m: 20, {block}}}\n")
        monkeypatch.chdir(tmp_path)
        assert experiment.main(["--cfg", str(tmp_path / "cfg.yaml")]) == 0
        log = json.load(open(tmp_path / "train_log.json"))
        assert set(log) == base | set(experiment.PDHG_KEYS)
        logs[block] = [log[k][0] for k in experiment.PDHG_KEYS]
        conv, its, opt = logs[block]
        print(block, "converged", conv, "iterations", its, "optimal after", opt)
        assert 0 <= conv <= 2 and 0 <= opt <= 2 and 0 < its <= 2 * 2048 and len(log[experiment.PDHG_KEYS[0]]) == 1
        assert (calls == [] if want is None else calls and all(k == want for k in calls)), (block, calls)
    keys = list(blocks)
    assert logs[keys[2]] == logs[keys[0]]           # the same rule: the same three figures as `halpern: true`
    for wrong in ({"wide": {"row": 64}}, {"wide": True, "scaled": False}, {"wide": True, "halpern": {"reflection": True}}, {"wide": {"rows": 96}}):
        with pytest.raises(ValueError):
            experiment.pdhg_counts(None, None, {"pdhg": {"iters": 5, "eps": 1e-3, "warm": False, **wrong}})
