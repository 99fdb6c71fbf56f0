"""GPU: mllp_lp_pdhg_rays (mllp_lp_pdhg_wide with certificates of infeasibility and unboundedness; csrc/pdhg_wide.hip).

Two bars.  Where detection stops nothing -- off, or on instances it only looks at -- the six outputs of mllp_lp_pdhg_wide are that
call's, BIT FOR BIT.  Where it decides, {code, iterations, restarts, 0} are the fp32 oracle's (tests/pdhg_rays_oracle.py), on
instances whose oracle margin is at least 2^-7 and on which the fp32 and the fp64 oracle agree -- both asserted before the device
is looked at -- and every ray the device returns is verified in fp64 from the data alone.  The qualities themselves are held to
the fp64 oracle instance by instance: 8 x the deviation of the fp32 oracle from the fp64 oracle on the same instance, in units of
2^-24 of the largest value of the instance's four, with a floor that the test states.

The test LPs are built on the host from pg.cpu_planted(tb.planted_shapes(...)), so that the answer is known by construction
(pdhg_rays_oracle.infeasible / unbounded).  MIXED: feasible, infeasible and unbounded of 5 x 12, 40 x 100 and 193 x 400 at the seeds
27, 22 and 43 -- every case of the table of tests/test_pdhg_rays_oracle.py -- 27 instances in one batch, instance 9 s + 3 shape +
kind (the last stops at 832 iterations; the smallest ray margin, 0.108, is instance 14's: 40 x 100, seed 22, unbounded).  LONG: the infeasible long-row instance (1201 x 2400, rows
and columns of more than 1024 terms: the block tier under both accumulators of both sweeps), which stops at 3200.
"""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import pdhg_oracle as pg
import pdhg_rays_oracle as pr
import planted_oracle as po
import test_basis_repair as tb
from guarded import PATTERNS, Guarded, same_bits
from mllp_amd import _lib
from test_basis_repair import LPBatch  # noqa: F401  (the fixture)
from test_pdhg_scaled import _bits, _host
from test_pdhg_wide import plain, trace  # noqa: F401  (the fixtures of that file: its batches)

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -10
MARGIN = 2.0 ** -7
SHAPES = [(5, 12), (40, 100), (193, 400)]
SEEDS = (27, 22, 43)
KINDS = (("feasible", lambda inst: inst, 0), ("infeasible", pr.infeasible, 4), ("unbounded", pr.unbounded, 5))
WIDE = ("x", "y", "status", "kkt", "dr", "dc")
ALL = WIDE + ("ray_x", "ray_y", "cert")
K_MIXED = 1024          # beyond the last stop of MIXED (832)
INF = np.float32(np.inf).view(np.int32)
ORDER = ("g", "x1", "x2", "x0", "y0", "iter_begin", "iter_end", "check_every", "eps", "step", "beta", "ruiz", "pc", "pw", "span", "reflect",
         "ray_eps", "rows", "x", "y", "dr", "dc", "ray_x", "ray_y", "status", "kkt", "cert", "scratch")


def _join(LPBatch, lps):
    """one batch from host LPs (dicts of A, b, c): CSR in the batch's column numbers"""
    inst_m, inst_n = [lp["A"].shape[0] for lp in lps], [lp["A"].shape[1] for lp in lps]
    ptr_m, ptr_n = np.concatenate([[0], np.cumsum(inst_m)]), np.concatenate([[0], np.cumsum(inst_n)])
    mats = [sp.csr_matrix(lp["A"]) for lp in lps]
    for a in mats:
        a.sort_indices()
    nnz = np.concatenate([[0], np.cumsum([a.nnz for a in mats])])
    ptr = np.concatenate([[0]] + [a.indptr[1:] + nnz[k] for k, a in enumerate(mats)]).astype(np.int32)
    idx = np.concatenate([a.indices + ptr_n[k] for k, a in enumerate(mats)]).astype(np.int32)
    val = np.concatenate([a.data for a in mats]).astype(np.float32)
    c = dict(inst_m=inst_m, inst_n=inst_n, ptr_m=ptr_m, ptr_n=ptr_n, ptr=ptr, idx=idx, val=val, M=int(ptr_m[-1]), N=int(ptr_n[-1]))
    b = tb._build(LPBatch, c, tb._dev(np.concatenate([lp["c"] for lp in lps])), tb._dev(np.concatenate([lp["b"] for lp in lps])))
    return dict(c=c, b=b, lps=lps)


def _oracles(lps, K, **kw):
    """the fp32 and the fp64 oracle of every instance, which must agree on the status with a margin of at least 2^-7"""
    out = []
    for k, lp in enumerate(lps):
        o32 = pr.solve(lp["A"], lp["b"], lp["c"], K, dtype=np.float32, **kw)
        o64 = pr.solve(lp["A"], lp["b"], lp["c"], K, dtype=np.float64, **kw)
        assert o32["status"] == o64["status"] and min(o32["margin"], o64["margin"]) >= MARGIN, (k, o32["status"], o64["status"], o32["margin"])
        out.append((o32, o64))
    return out


def _cut(g, h, k):
    """instance k's part of a result"""
    c = g["c"]
    s, r = slice(c["ptr_n"][k], c["ptr_n"][k + 1]), slice(c["ptr_m"][k], c["ptr_m"][k + 1])
    return dict(x=h["x"][s], y=h["y"][r], dr=h["dr"][r], dc=h["dc"][s], ray_x=h["ray_x"][s], ray_y=h["ray_y"][r],
                status=h["status"].reshape(-1, 4)[k], kkt=h["kkt"].reshape(-1, 6)[k], cert=h["cert"].reshape(-1, 4)[k])


@pytest.fixture(scope="module")
def mixed(LPBatch):
    insts = [inst for seed in SEEDS for inst in pg.cpu_planted(tb.planted_shapes(SHAPES, seed))]
    lps = [make(inst) for inst in insts for _, make, _ in KINDS]
    g = _join(LPBatch, lps)
    g["codes"] = [code for _ in insts for _, _, code in KINDS]
    g["quality"] = {}
    g["oracle"] = _oracles(lps, K_MIXED, eps=EPS, ray_eps=EPS)
    g["got"] = _host(g["b"].pdhg_rays(K_MIXED, eps=EPS, ray_eps=EPS), ALL)
    return g


@pytest.fixture(scope="module")
def long_rows(LPBatch):
    return _join(LPBatch, [pr.infeasible(pg.cpu_planted(po.ragged_case(which=[4]))[0])])


def _off(got, n_inst, what):
    assert not got["ray_x"].any() and not got["ray_y"].any(), what
    assert np.array_equal(got["cert"].view(np.int32).reshape(-1, 4), np.tile(np.array([INF, 0, INF, 0], np.int32), (n_inst, 1))), what


# ---------------------------------------------------------------------------------------------------
# 1, 2. where nothing is stopped: the wide call's bits
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [0, 1, 64, 512])
def test_off_is_the_wide_call_on_plain_iterations(plain, K):  # noqa: F811
    b = plain["b"]
    for kw in (dict(check_every=0), dict(check_every=64, eps=0.0)):
        want = _bits(_host(b.pdhg_wide(K, **kw)))
        res = b.pdhg_rays(K, ray_eps=-1.0, **kw)
        got = _host(res, ALL)
        same_bits(_bits({k: got[k] for k in WIDE}), want, f"K = {K}, {kw}, ray_eps = -1")
        _off(got, b.n_inst, (K, kw))
        assert res.calls == 1


@pytest.mark.parametrize("rows", [64, None])
def test_off_is_the_wide_call_at_the_decisions(trace, rows):  # noqa: F811
    from mllp_amd.graph import LPPdhgRays, LPPdhgWide
    b = trace["b"]
    res = b.pdhg_rays(8192, eps=EPS, check_every=64, ray_eps=-1.0, rows_per_item=rows)
    assert isinstance(res, LPPdhgRays) and isinstance(res, LPPdhgWide)
    got = _host(res, ALL)
    same_bits(_bits({k: got[k] for k in WIDE}), trace["want"], f"8192 iterations, ray_eps = -1, rows_per_item = {rows}")
    _off(got, b.n_inst, rows)


def test_detection_moves_no_bit_of_an_instance_it_does_not_stop(trace):  # noqa: F811
    b = trace["b"]
    got = _host(b.pdhg_rays(8192, eps=EPS, check_every=64, ray_eps=EPS), ALL)
    same_bits(_bits({k: got[k] for k in WIDE}), trace["want"], "8192 iterations, ray_eps = 2^-10")
    assert not got["ray_x"].any() and not got["ray_y"].any()
    cert = got["cert"].reshape(-1, 4)
    print("cert of the feasible instances:", cert.tolist())
    assert np.isfinite(cert[:, [1, 3]]).all() and (np.minimum(cert[:, 0], cert[:, 2]) > EPS).all()         # looked at, and not stopped


# ---------------------------------------------------------------------------------------------------
# 3. the mixed batch
# ---------------------------------------------------------------------------------------------------
def test_the_mixed_batch_ends_as_the_oracle_ends_it(mixed):
    got = mixed["got"]
    for k, ((o32, _), code, lp) in enumerate(zip(mixed["oracle"], mixed["codes"], mixed["lps"])):
        part = _cut(mixed, got, k)
        print(k, lp["A"].shape, "oracle", o32["status"], "device", list(part["status"]), "cert", list(part["cert"]))
        assert o32["status"][0] == code and o32["status"][1] < K_MIXED          # the construction's answer, within the limit
        assert list(part["status"]) == o32["status"], (k, list(part["status"]), o32["status"])
        assert bool(part["ray_y"].any()) == (code == 4) and bool(part["ray_x"].any()) == (code == 5), k
        if code:        # the device's ray on its own, in fp64, from the data alone
            ok, q = pr.verify64(lp, code, part["ray_x"], part["ray_y"], EPS)
            assert ok, (k, code, q)
            assert min(part["cert"][0], part["cert"][2]) <= EPS
        # x, y and kkt are the step's output and its errors at every code
        assert all(abs(float(e) - w) <= 1e-4 * max(1.0, abs(w)) for e, w in zip(part["kkt"][:3], pg.errors64(lp["A"], lp["b"], lp["c"], part["x"], part["y"])))


# ---------------------------------------------------------------------------------------------------
# 4. the qualities
# ---------------------------------------------------------------------------------------------------
def _quality_units(got, want, words):
    """the largest deviation over `words` of a cert, in units of 2^-24 of the largest of the fp64 oracle's values there"""
    got, want = np.asarray(got, np.float64)[words], np.asarray(want, np.float64)[words]
    scale = np.abs(want).max(initial=0.0)
    return 0.0 if scale == 0.0 else float(np.abs(got - want).max() / (2.0 ** -24 * scale))


def _quality_runs(g, K):
    """per instance (fp32 oracle, fp64 oracle, qualifies) after K iterations at eps = ray_eps = 0, once per K"""
    if K not in g["quality"]:
        runs = []
        for lp in g["lps"]:
            o32, o64 = (pr.solve(lp["A"], lp["b"], lp["c"], K, eps=0.0, ray_eps=0.0, dtype=dt) for dt in (np.float32, np.float64))
            assert o32["status"][:2] == o64["status"][:2] == [6, K]          # small enough that nothing stops, which the oracle says
            runs.append((o32, o64, o32["status"] == o64["status"] and min(o32["margin"], o64["margin"]) >= MARGIN))
        g["quality"][K] = runs
    return g["quality"][K]


def _oracle_words(o32, o64):
    return np.isfinite(np.asarray(o32["cert"], np.float64)) & np.isfinite(np.asarray(o64["cert"], np.float64))


@pytest.mark.parametrize("K", [64, 512])
def test_the_qualities_are_the_oracles(mixed, K):
    """An instance is compared where the fp32 and the fp64 oracle took the same decisions up to K with a margin of at least 2^-7
    (all 27 at 64; 23 at 512, where four feasible instances have converged to the noise of fp32 and restart differently in the two
    oracles), over the words of its cert that are finite in both oracles and on the device: a quality is +inf where its
    denominator has the wrong sign, and a denominator at the noise level may have either.
    THE BAR is per instance: 8 x the deviation of the fp32 oracle from the fp64 oracle on THAT instance.  That deviation is one
    sample of the rounding error of one summation order, and a sample may fall far below what another order gives (0.5 units on
    instance 14 at K = 64), so it is held from below by a floor: the median of the 27 deviations at K = 64, times K / 64 --
    rounding errors of an iteration that has not gone unstable add up at most linearly in the iterations, which is how
    tests/test_pdhg_halpern.py scales its own bar with the iteration count.  The floor comes from the two oracles alone."""
    runs = _quality_runs(mixed, K)
    first = _quality_runs(mixed, 64)
    assert sum(ok for _, _, ok in runs) == (27 if K == 64 else 23) and all(ok for _, _, ok in first)
    floor = float(np.median([_quality_units(o32["cert"], o64["cert"], _oracle_words(o32, o64)) for o32, o64, _ in first])) * K / 64
    got = _host(mixed["b"].pdhg_rays(K, eps=0.0, ray_eps=0.0), ("cert", "status"))
    assert (got["status"][:, 0] == 6).all() and (got["status"][:, 1] == K).all()
    print(f"K = {K}: floor {floor:.1f} units (bar {8 * floor:.1f})")
    failed = []
    for k, (o32, o64, ok) in enumerate(runs):
        if not ok:
            continue
        cert = got["cert"][k]
        assert not np.isnan(cert).any() and np.isfinite(cert[[1, 3]]).all(), (k, cert)
        words = np.isfinite(cert) & _oracle_words(o32, o64)
        assert words[1] and words[3]
        d, u = _quality_units(o32["cert"], o64["cert"], words), _quality_units(cert, o64["cert"], words)
        bar = 8.0 * max(d, floor)
        print(f"K = {K}, instance {k}: fp32 oracle {d:.1f} units -> bar {bar:.1f}; device {u:.1f} units")
        if u > bar:
            failed.append((k, u, bar))
    assert not failed, (K, failed)


# ---------------------------------------------------------------------------------------------------
# 5. every tier of the paired evaluation
# ---------------------------------------------------------------------------------------------------
def test_the_long_rows_end_infeasible_through_every_tier(long_rows):
    lp = long_rows["lps"][0]
    rows, cols = np.diff(lp["A"].indptr), np.diff(sp.csc_matrix(lp["A"]).indptr)
    for lens in (rows, cols):       # both sweeps pass through the wave tier and the block tier
        assert (lens > 1024).any() and ((lens > 64) & (lens <= 1024)).any() and (lens <= 64).any()
    o32, _ = _oracles([lp], 4096, eps=EPS, ray_eps=EPS)[0]
    got = _host(long_rows["b"].pdhg_rays(4096, eps=EPS, ray_eps=EPS), ALL)
    print("oracle", o32["status"], "device", got["status"].tolist(), "cert", got["cert"].tolist())
    assert o32["status"][:2] == [4, 3200] and list(got["status"][0]) == o32["status"]
    ok, q = pr.verify64(lp, 4, got["ray_x"], got["ray_y"], EPS)
    assert ok and not got["ray_x"].any(), q


# ---------------------------------------------------------------------------------------------------
# 6. execution moves no bit
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [64, 128])
def test_rows_per_item_moves_no_bit(mixed, rows):
    got = _host(mixed["b"].pdhg_rays(K_MIXED, eps=EPS, ray_eps=EPS, rows_per_item=rows), ALL)
    same_bits(_bits(got), _bits(mixed["got"]), f"rows_per_item = {rows} against the default")


@pytest.mark.parametrize("k", [4, 8, 14, 25])
def test_an_instance_alone_has_its_bits_inside_the_batch(LPBatch, mixed, k):  # noqa: F811
    alone = _join(LPBatch, [mixed["lps"][k]])
    got = _host(alone["b"].pdhg_rays(K_MIXED, eps=EPS, ray_eps=EPS), ALL)
    assert got["status"][0, 0] == mixed["codes"][k] != 0
    same_bits(_bits(_cut(alone, got, 0)), _bits(_cut(mixed, mixed["got"], k)), f"instance {k} alone against inside the batch")


# ---------------------------------------------------------------------------------------------------
# 7. continuation, through the C ABI on the test's own buffers
# ---------------------------------------------------------------------------------------------------
def _scratch_bytes(b, rows=0):
    n = ctypes.c_int64(-1)
    _lib.check(_lib.lib().mllp_lp_pdhg_rays_scratch_bytes(b._h, rows, ctypes.byref(n)))
    return n.value


class Raw:
    """the outputs and the scratch of a sequence of C calls on one batch (Guarded, at the natural alignment of a float)"""

    def __init__(self, g, fill=PATTERNS["nan"], rows=0):
        c, b = g["c"], g["b"]
        K = len(c["inst_m"])
        self.b, self.rows = b, rows
        f = lambda n, name, shift, dtype=torch.float32: Guarded(n, dtype, "cuda", fill=fill, name=name, shift=shift)       # noqa: E731
        self.o = dict(x=f(c["N"], "x", 4), y=f(c["M"], "y", 8), dr=f(c["M"], "dr", 12), dc=f(c["N"], "dc", 8), ray_x=f(c["N"], "ray_x", 12),
                      ray_y=f(c["M"], "ray_y", 4), status=f(4 * K, "status", 4, torch.int32), kkt=f(6 * K, "kkt", 4), cert=f(4 * K, "cert", 8))
        self.scratch = f(_scratch_bytes(b, rows) // 4, "scratch", 4)

    def call(self, begin, end, check_every=64, eps=EPS, ray_eps=EPS):
        b = self.b
        rc = _lib.lib().mllp_lp_pdhg_rays(b._h, _lib.ptr(b.x1), _lib.ptr(b.x2), None, None, begin, end, check_every, eps, 0.9, 0.5, 10, 1, 1, 16.0,
                                          1, ray_eps, self.rows, *[self.o[k].ptr for k in ORDER[18:27]], self.scratch.ptr, _lib.current_stream())
        assert rc == 0, _lib.lib().mllp_last_error()
        torch.cuda.synchronize()
        for v in list(self.o.values()) + [self.scratch]:
            v.check()
        return {k: v.bits().view(np.int32) for k, v in self.o.items()}


@pytest.mark.parametrize("split", [(100, K_MIXED), (63, 65)])
def test_two_calls_give_the_single_calls_bits(mixed, split):
    K1, K2 = split
    single = Raw(mixed).call(0, K2)
    if K2 == K_MIXED:
        same_bits(single, _bits(mixed["got"]), "the C call on guarded buffers against LPBatch.pdhg_rays")
    two = Raw(mixed, rows=128)
    first = two.call(0, K1)
    assert (first["status"].reshape(-1, 4)[:, 0] == 6).all()
    same_bits(two.call(K1, K2), single, f"(0, {K1}) then ({K1}, {K2}) against (0, {K2})")


def test_a_stopped_instance_keeps_its_bits_and_polling_stops(mixed):
    want = _bits(mixed["got"])
    codes = want["status"].reshape(-1, 4)[:, 0]
    assert sorted(set(codes)) == [0, 4, 5] and len(codes) == 27
    r = Raw(mixed)
    at = r.call(0, 256)         # some have stopped at 192, of every code; others run
    st = at["status"].reshape(-1, 4)
    assert {0, 4, 5, 6} <= set(st[:, 0])
    for begin, end in ((256, 320), (320, K_MIXED), (K_MIXED, K_MIXED), (K_MIXED, K_MIXED + 100)):
        got = r.call(begin, end)
        for k in np.flatnonzero(st[:, 0] != 6):
            same_bits(_bits(_cut(mixed, got, k)), _bits(_cut(mixed, want, k)), f"instance {k} after ({begin}, {end})")
        if end >= K_MIXED:
            same_bits(got, want, f"every instance after ({begin}, {end})")
    last = int(want["status"].reshape(-1, 4)[:, 1].max())
    res = mixed["b"].pdhg_rays(8192, eps=EPS, ray_eps=EPS, poll_every=256)
    same_bits(_bits(_host(res, ALL)), want, "poll_every = 256 against the single call")
    assert res.calls == -(-last // 256) < 8192 // 256


# ---------------------------------------------------------------------------------------------------
# 8. contract details
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", list(PATTERNS))
def test_stale_state_is_refused_per_instance(mixed, fill):
    K = len(mixed["lps"])
    r = Raw(mixed, fill=PATTERNS[fill])
    got = r.call(64, 128)
    assert [list(s) for s in got["status"].reshape(-1, 4)] == [[9, 0, 0, 0]] * K
    assert all((got[k] == 0).all() for k in ALL if k != "status")
    # a real state that ended elsewhere, at every code; and one that continues
    r.call(0, 256)
    got = r.call(192, 320)
    assert [list(s) for s in got["status"].reshape(-1, 4)] == [[9, 0, 0, 0]] * K and all((got[k] == 0).all() for k in ALL if k != "status")
    same_bits(r.call(256, 320), Raw(mixed).call(0, 320), "the state still continues where it ended")


def test_every_refusal_writes_nothing(mixed):
    c, b = mixed["c"], mixed["b"]
    K, L, z = len(c["inst_m"]), _lib.lib(), ctypes.c_void_p(0)
    poison = lambda n: torch.full((n,), float("nan"), device="cuda")      # noqa: E731
    bufs = dict(x=poison(c["N"]), y=poison(c["M"]), dr=poison(c["M"]), dc=poison(c["N"]), ray_x=poison(c["N"] + 8), ray_y=poison(c["M"]),
                status=poison(4 * K).view(torch.int32), kkt=poison(6 * K), cert=poison(4 * K), scratch=poison(_scratch_bytes(b) // 4))
    x0, y0 = tb._dev(np.ones(c["N"], np.float32)), tb._dev(np.ones(c["M"], np.float32))
    ok = dict(g=b._h, x1=_lib.ptr(b.x1), x2=_lib.ptr(b.x2), x0=_lib.ptr(x0), y0=_lib.ptr(y0), iter_begin=0, iter_end=128, check_every=64, eps=EPS,
              step=0.9, beta=0.5, ruiz=10, pc=1, pw=1, span=16.0, reflect=1, ray_eps=EPS, rows=0, **{k: _lib.ptr(v) for k, v in bufs.items()})
    nan, inf = float("nan"), float("inf")
    bad = [dict(g=None), dict(x=z), dict(status=z), dict(iter_begin=-1), dict(iter_begin=129), dict(eps=nan), dict(step=0.0), dict(beta=1.0),
           dict(scratch=z), dict(ruiz=65), dict(span=0.5), dict(rows=96), dict(ray_eps=nan), dict(ray_eps=inf), dict(ray_eps=-inf),
           dict(x0=_lib.ptr(bufs["x"])), dict(y0=_lib.ptr(bufs["dr"])), dict(x0=_lib.ptr(bufs["ray_x"])), dict(y0=_lib.ptr(bufs["ray_x"])),
           dict(x0=ctypes.c_void_p(bufs["ray_x"].data_ptr() + 32)), dict(x0=_lib.ptr(bufs["ray_y"])), dict(y0=_lib.ptr(bufs["ray_y"])),
           dict(x0=_lib.ptr(bufs["cert"])), dict(y0=_lib.ptr(bufs["cert"])), dict(y0=ctypes.c_void_p(bufs["cert"].data_ptr() + 4))]
    before = {k: v.view(torch.int32).cpu().numpy().copy() for k, v in bufs.items()}
    for kw in bad:
        args = dict(ok, **kw)
        assert L.mllp_lp_pdhg_rays(*[args[k] for k in ORDER], _lib.current_stream()) == -1, kw
        assert b"mllp_lp_pdhg_rays:" in L.mllp_last_error(), kw
    torch.cuda.synchronize()
    same_bits({k: v.view(torch.int32).cpu().numpy() for k, v in bufs.items()}, before, "buffers after the refused calls")
    # the same arguments without a fault are accepted; every new output may be NULL (eps = ray_eps = 0: nothing stops in 128 iterations)
    assert L.mllp_lp_pdhg_rays(*[dict(ok, kkt=z, dr=z, dc=z, ray_x=z, ray_y=z, cert=z)[k] for k in ORDER], _lib.current_stream()) == 0
    assert L.mllp_lp_pdhg_rays(*[dict(ok, eps=0.0, ray_eps=0.0, rows=4096)[k] for k in ORDER], _lib.current_stream()) == 0
    torch.cuda.synchronize()
    assert (bufs["status"].view(K, 4)[:, 0] == 6).all() and not any(torch.isnan(bufs[k][:c["N"] if k == "ray_x" else None]).any() for k in ALL if k != "status")


def test_an_empty_instance_and_an_empty_side(LPBatch):  # noqa: F811
    c = tb.dense_case([np.zeros((0, 3)), tb.int_matrix(3, 6, 0.7, 12), np.zeros((2, 0))], 1)
    c["c"][:3] = [1.0, 2.0, 0.0]
    b = tb._build(LPBatch, c, tb._dev(c["c"]), tb._dev(c["b"]))
    x0 = tb._dev(np.ones(c["N"], np.float32))
    for K in (0, 128):
        for ray_eps in (-1.0, EPS):
            got = _host(b.pdhg_rays(K, eps=EPS, ray_eps=ray_eps, x0=x0), ALL)
            print(K, ray_eps, got["status"].tolist(), got["cert"].tolist())
            assert len(got["ray_x"]) == 9 and len(got["ray_y"]) == 5 and got["cert"].shape == (3, 4)
            if ray_eps < 0 or K == 0:
                same_bits(_bits({k: got[k] for k in WIDE}), _bits(_host(b.pdhg_wide(K, eps=EPS, x0=x0))), f"empty sides, {K} iterations")
                _off(got, 3, K)
    # three columns of cost 1, 2, 0 and no row: optimal at once.  Two rows of right-hand side b and no column: A'y = 0 for every
    # y, so the LP is infeasible where b != 0, and the rays say so as soon as y has moved
    assert got["status"][0, 0] == 0 and c["b"][-2:].any() and got["status"][2, 0] == 4 and got["ray_y"][-2:].any() and got["cert"][2, 0] == 0.0


@pytest.mark.parametrize("m", [3, 193])
def test_scratch_bytes_is_the_headers_closed_form(LPBatch, m):  # noqa: F811
    shapes = [(m, 2 * m + 6), (5, 12)]
    b = tb._build(LPBatch, tb.planted_shapes(shapes, 40))
    M, N = sum(s[0] for s in shapes), sum(s[1] for s in shapes)
    for rows in (0, 64, 128, 4096):
        assert _scratch_bytes(b, rows) == 4 * (27 * len(shapes) + 6 * N + 5 * M), (m, rows)
    from mllp_amd.graph import pdhg_rays_limits
    assert pdhg_rays_limits() == (1024, 64, 64, 4096)


# ---------------------------------------------------------------------------------------------------
# 9. the driver
# ---------------------------------------------------------------------------------------------------
def test_driver_reports_infeasible_and_unbounded(tmp_path, monkeypatch):
    """`rays: true` and `rays: {eps: E}` inside `report_solved: pdhg` select LPBatch.pdhg_rays (and imply `wide`) and add the two
    counts to train_log.json; without the key every log key is the one it was"""
    import json
    from mllp_amd import experiment
    from mllp_amd.graph import LPBatch as Batch
    cfg = ("train_data_type: 'planted'\ntrain_lr: 1.e-3\ntrain_iter: 1\nmethods:\n  - 'gs-topk'\nbatch_size: 3\nholdout: 0.25\n"
           "planted: {instances: 8, m: 20, n: 50, row_nnz: 4, seed: 5}\n")
    base = {"obj", "val_obj", "usable", "feasible", "optimal", "skipped"} | {f"planted{5 + i}" for i in range(8)}
    calls, inner = [], Batch.pdhg_rays

    def recorded(self, max_iters, **kw):
        calls.append({k: kw.get(k) for k in ("ray_eps", "rows_per_item", "poll_every", "reflect")})
        res = inner(self, max_iters, **kw)
        calls[-1]["codes"] = res.status[:, 0].cpu().tolist()
        return res
    monkeypatch.setattr(Batch, "pdhg_rays", recorded)
    blocks = {"pdhg: {iters: 2048, eps: 1.e-3, wide: true}": None,
              "pdhg: {iters: 2048, eps: 1.e-3, rays: false}": None,
              "pdhg: {iters: 2048, eps: 1.e-3, rays: true}": dict(ray_eps=2.0 ** -10, rows_per_item=None, poll_every=None, reflect=True),
              "pdhg: {iters: 2048, eps: 1.e-3, warm: false, rays: {eps: 1.e-2}, wide: {rows: 128, poll: 512}}":
                  dict(ray_eps=1e-2, rows_per_item=128, poll_every=512, reflect=True)}
    logs = {}
    for block, want in blocks.items():
        del calls[:]
        (tmp_path / "cfg.yaml").write_text(cfg + f"report_solved: {{feas_tol: 1.e-3, opt_tol: 1.e-3, max_m: 20, {block}}}\n")
        monkeypatch.chdir(tmp_path)
        assert experiment.main(["--cfg", str(tmp_path / "cfg.yaml")]) == 0
        log = json.load(open(tmp_path / "train_log.json"))
        keys = set(experiment.PDHG_KEYS) | (set(experiment.PDHG_RAY_KEYS) if want else set())
        assert set(log) == base | keys, block
        logs[block] = {k: log[k][0] for k in keys}
        if want is None:
            assert calls == []
            continue
        assert calls and all({k: v for k, v in call.items() if k != "codes"} == want for call in calls), (block, calls)
        codes = [code for call in calls for code in call["codes"]]
        assert logs[block]["pdhg_infeasible"] == codes.count(4) and logs[block]["pdhg_unbounded"] == codes.count(5)
    keys = list(blocks)
    assert [logs[keys[2]][k] for k in experiment.PDHG_KEYS] == [logs[keys[0]][k] for k in experiment.PDHG_KEYS]       # feasible instances: nothing moved
    assert logs[keys[2]]["pdhg_infeasible"] == logs[keys[2]]["pdhg_unbounded"] == 0
    for wrong in ({"rays": {"epsilon": 1e-3}}, {"rays": True, "wide": False}, {"rays": {"eps": -1.0}}, {"rays": True, "scaled": False}):
        with pytest.raises(ValueError):
            experiment.pdhg_counts(None, None, {"pdhg": {"iters": 5, "eps": 1e-3, "warm": False, **wrong}})
