"""CPU: the numpy oracle of mllp_lp_pdhg_rays (tests/pdhg_rays_oracle.py) does what THE RULE of include/mllp_hip.h says -- with
detection off, and on instances it never stops, it is tests/pdhg_halpern_oracle.py exactly; on LPs whose answer is known by
construction it ends with the code of the construction, at the iteration counts of DESIGN.md 4.26's table, in fp32 and fp64
alike, and every ray it returns passes a verification in fp64 from the data alone; optimal wins over a ray at the same check --
and the C ABI's new entry points exist, refuse what they must and report their limits without a GPU.  The device is held to
this oracle by tests/test_pdhg_rays.py.

THE TABLE (iterations at check_every 64, eps = ray_eps = 2^-10, defaults otherwise; bar: 4096 iterations).  The seeds are
tests/test_pdhg_halpern_oracle.py's.  Every case has an oracle margin of at least 2^-7 in both dtypes, which is asserted, so
the device is compared on all of them.
"""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

import pdhg_halpern_oracle as ph
import pdhg_oracle as pg
import pdhg_rays_oracle as pr
import planted_oracle as po
import test_basis_repair as tb
from mllp_amd import _lib

EPS = 2.0 ** -10
BAR = 4096
MARGIN = 2.0 ** -7
SHAPES = [(5, 12), (40, 100), (193, 400)]
SEEDS = (27, 22, 43)
NETLIB = ("afiro", "sc50a", "sc50b", "blend", "adlittle", "stocfor1")
KINDS = {"feasible": lambda inst: inst, "infeasible": pr.infeasible, "unbounded": pr.unbounded}
CODES = {"feasible": 0, "infeasible": 4, "unbounded": 5}
# {seed: per shape (feasible, infeasible, unbounded)}: the iterations at which the instance stops
TABLE = {27: [(192, 192, 192), (448, 192, 832), (512, 512, 704)],
         22: [(192, 256, 320), (384, 256, 704), (384, 384, 512)],
         43: [(192, 192, 128), (192, 192, 320), (384, 192, 576)]}
LONG = dict(feasible=(0, 2176), infeasible=(4, 3200), unbounded=(6, 4096))         # the long-row instance: (code, iterations)
SMALLEST_RAY_MARGIN = 2.0 ** -4         # measured: 0.108 (40 x 100, seed 22, unbounded)


@pytest.fixture(scope="module")
def planted():
    return {seed: pg.cpu_planted(tb.planted_shapes(SHAPES, seed)) for seed in SEEDS}


@pytest.fixture(scope="module")
def long_rows():
    return pg.cpu_planted(po.ragged_case(which=[4]))[0]


@pytest.fixture(scope="module")
def netlib():
    from mllp_amd.data import load_packed
    return [dict(name=i.name, A=sp.csr_matrix((i.values, i.indices, i.indptr), shape=(i.m, i.n)), b=i.rhs, c=i.coefs) for i in load_packed(NETLIB)]


def _same_run(a, z):
    """a run of this oracle against one of pdhg_halpern_oracle: x, y, status, kkt and every check"""
    assert np.array_equal(a["x"], z["x"]) and np.array_equal(a["y"], z["y"]) and a["status"] == z["status"] and a["kkt"] == z["kkt"]
    keep = ("it", "k", "e", "e_last", "w", "restart")
    assert [{f: k[f] for f in keep if f in k} for k in a["checks"]] == [{f: k[f] for f in keep if f in k} for k in z["checks"]]
    assert a["anchors"] == z["anchors"] and np.array_equal(a["dr"], z["dr"]) and np.array_equal(a["dc"], z["dc"])


# ---- 1. off, and where it never stops: the Halpern oracle --------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_without_a_stop_the_oracle_is_the_halpern_oracle(planted, dtype):
    for inst in planted[SEEDS[0]]:
        for lp in (inst, pr.infeasible(inst), pr.unbounded(inst)):
            for kw in (dict(), dict(reflect=False, primal_weight=False), dict(x0=np.linspace(-1, 1, lp["n"]), y0=np.ones(lp["m"]), check_every=48)):
                z = ph.solve(lp["A"], lp["b"], lp["c"], 640, eps=EPS, dtype=dtype, **kw)
                off = pr.solve(lp["A"], lp["b"], lp["c"], 640, eps=EPS, ray_eps=-1.0, dtype=dtype, **kw)
                _same_run(off, z)
                assert off["margin"] == z["margin"] and off["ray_margin"] == np.inf and off["cert"] == [np.inf, 0, np.inf, 0]
                assert not off["ray_x"].any() and not off["ray_y"].any() and all("qp" not in k and "unused" not in k for k in off["checks"])
        for kw in (dict(), dict(ray_eps=0.0)):      # detection on, a feasible instance: it is looked at and never stopped
            z = ph.solve(inst["A"], inst["b"], inst["c"], BAR, eps=EPS, dtype=dtype)
            on = pr.solve(inst["A"], inst["b"], inst["c"], BAR, eps=EPS, dtype=dtype, **kw)
            _same_run(on, z)
            assert on["status"][0] == 0 and all(("qp" in k) != ("unused" in k) for k in on["checks"]) and not on["ray_x"].any() and not on["ray_y"].any()
            last = [k for k in on["checks"] if "qp" in k][-1]
            assert [float(v) for v in on["cert"]] == [last[f] for f in ("qp", "by", "qd", "cx")]


# ---- 2. the table, and the certificates --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("seed", SEEDS)
def test_the_table(planted, seed, dtype):
    worst = np.inf
    for inst, row in zip(planted[seed], TABLE[seed]):
        for (kind, make), its in zip(KINDS.items(), row):
            lp = make(inst)
            r = pr.solve(lp["A"], lp["b"], lp["c"], BAR, eps=EPS, ray_eps=EPS, dtype=dtype)
            small = min([min(k["qp"], k["qd"]) for k in r["checks"] if "qp" in k] or [np.inf])
            print(seed, inst["m"], inst["n"], kind, r["status"], "margin", r["margin"], "rays", r["ray_margin"], "smallest quality", small)
            assert r["status"][:2] == [CODES[kind], its] and r["status"][3] == 0, (seed, inst["m"], kind, r["status"])
            assert r["margin"] >= MARGIN, (seed, inst["m"], kind, r["margin"])
            worst = min(worst, r["ray_margin"])
            if kind == "feasible":
                assert small > 32 * EPS and not r["ray_x"].any() and not r["ray_y"].any()        # measured: 0.056 at the least
                continue
            ok, q = pr.verify64(lp, r["status"][0], r["ray_x"], r["ray_y"], EPS)
            assert ok, (seed, inst["m"], kind, q)
            assert (kind == "infeasible") == bool(r["ray_y"].any()) and (kind == "unbounded") == bool(r["ray_x"].any())
            assert r["ray_x"].dtype == r["ray_y"].dtype == dtype
            # the certificate is the anchor-to-output direction of the deciding check, which was its last
            assert "qp" in r["checks"][-1] and r["checks"][-1]["it"] == its and min(r["cert"][0], r["cert"][2]) <= EPS
    assert worst >= SMALLEST_RAY_MARGIN, worst


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_long_rows(long_rows, dtype):
    for kind, make in KINDS.items():
        lp = make(long_rows)
        r = pr.solve(lp["A"], lp["b"], lp["c"], BAR, eps=EPS, ray_eps=EPS, dtype=dtype)
        print("long rows", kind, r["status"], "margin", r["margin"], "rays", r["ray_margin"], "cert", r["cert"])
        assert tuple(r["status"][:2]) == LONG[kind] and (kind == "unbounded" or r["margin"] >= MARGIN)
        if kind == "infeasible":
            assert pr.verify64(lp, 4, r["ray_x"], r["ray_y"], EPS)[0] and r["ray_margin"] >= 0.25
        if kind == "unbounded":     # not claimed: the displacement has not converged within the bar (qd 0.0014 against 0.00098)
            assert EPS < r["cert"][2] < 2 * EPS


def test_the_constructions_are_what_they_claim(planted):
    for inst in planted[SEEDS[1]]:
        A, b, c = sp.csr_matrix(inst["A"]), inst["b"], inst["c"]
        bad = pr.infeasible(inst)
        assert bad["A"].shape == (inst["m"] + 1, inst["n"]) and np.array_equal(bad["A"][-1].toarray(), A[0].toarray()) and bad["b"][-1] == np.float32(b[0] + 1)
        y = np.zeros(inst["m"] + 1)
        y[0], y[-1] = -1.0, 1.0       # the Farkas ray: A'y = 0, b'y = 1
        assert pr.verify64(bad, 4, None, y, 0.0) == (True, 0.0)
        free = pr.unbounded(inst)
        assert free["A"].shape == (inst["m"], inst["n"] + 1) and free["c"][-1] == np.float32(-c[0] - 1)
        d = np.zeros(inst["n"] + 1)
        d[0] = d[-1] = 1.0            # the recession ray: A d = 0, d >= 0, c'd = -1
        assert pr.verify64(free, 5, d, None, 0.0) == (True, 0.0)
        assert np.abs(free["A"] @ np.append(inst["xstar"], 0.0) - b).max() < 1e-5          # still feasible
        assert pr.verify64(free, 5, -d, None, 1.0)[0] is False and pr.verify64(bad, 4, None, -y, 1.0)[0] is False


def test_six_netlib_instances_end_as_the_halpern_rule_ends_them(netlib):
    for inst in netlib:
        z = ph.solve(inst["A"], inst["b"], inst["c"], 8192, eps=EPS, dtype=np.float32)
        r = pr.solve(inst["A"], inst["b"], inst["c"], 8192, eps=EPS, ray_eps=EPS, dtype=np.float32)
        small = min(min(k["qp"], k["qd"]) for k in r["checks"] if "qp" in k)
        print(inst["name"], r["status"], "smallest quality", small)
        assert r["status"] == z["status"] and r["status"][0] == 0 and np.array_equal(r["x"], z["x"]) and small > 2 * EPS


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_optimal_wins(planted, dtype):
    """one check, at 192 iterations, of an infeasible instance: with eps = 2^-10 its ray decides (code 4); with an eps that the
    errors of the same point pass, the same check ends with code 0 and the rays, which would have passed, are not looked at"""
    lp = pr.infeasible(planted[SEEDS[0]][1])
    kw = dict(check_every=192, ray_eps=0.25, dtype=dtype)
    ray = pr.solve(lp["A"], lp["b"], lp["c"], 192, eps=EPS, **kw)
    assert ray["status"] == [4, 192, 0, 0] and ray["cert"][0] <= 0.25 and ray["ray_y"].any()
    opt = pr.solve(lp["A"], lp["b"], lp["c"], 192, eps=1e6, **kw)
    assert opt["status"] == [0, 192, 0, 0] and opt["cert"] == [np.inf, 0, np.inf, 0] and not opt["ray_y"].any()
    assert opt["checks"][-1]["unused"] == [float(v) for v in ray["cert"]] and np.array_equal(opt["x"], ray["x"])


# ---- 3. the C ABI, without a GPU ---------------------------------------------------------------------------------------------
NEW = ("mllp_lp_pdhg_rays_limits", "mllp_lp_pdhg_rays_scratch_bytes", "mllp_lp_pdhg_rays")
ORDER = ("g", "x1", "x2", "x0", "y0", "iter_begin", "iter_end", "check_every", "eps", "step", "beta", "ruiz", "pc", "pw", "span", "reflect",
         "ray_eps", "rows", "x", "y", "dr", "dc", "ray_x", "ray_y", "status", "kkt", "cert", "scratch", "stream")
WIDE = tuple(k for k in ORDER if k not in ("ray_eps", "ray_x", "ray_y", "cert"))


def _sizes(M, N, n_inst):
    """a stand-in for a graph of which only the sizes are read: they are its first four 64-bit words (M, N, nnz, n_inst).  This
    leans on the private layout of csrc/internal.h's mllp_graph, which carries a note beside those words, and on the calls below
    reading nothing else of the graph before they return; tests/test_pdhg_rays.py repeats both checks on a real graph"""
    buf = (ctypes.c_int64 * 512)(M, N, 0, n_inst)
    _sizes.keep = getattr(_sizes, "keep", []) + [buf]
    return ctypes.cast(buf, ctypes.c_void_p)


def test_the_new_symbols_are_exported_and_bound():
    L = _lib.lib()
    header = open(_lib.HEADER_PATH).read()
    for name in NEW:
        assert name in _lib._PROTOTYPES and hasattr(L, name) and f"int {name}(" in header, name
    rays, wide = _lib._PROTOTYPES["mllp_lp_pdhg_rays"][1], _lib._PROTOTYPES["mllp_lp_pdhg_wide"][1]
    assert len(rays) == len(ORDER) == len(wide) + 4
    assert [t for k, t in zip(ORDER, rays) if k in WIDE] == wide            # the wide call's arguments in that call's order
    at = {k: t for k, t in zip(ORDER, rays)}
    assert at["ray_eps"] is ctypes.c_float and ORDER.index("ray_eps") == ORDER.index("reflect") + 1
    assert ORDER.index("ray_x") == ORDER.index("dc") + 1 and ORDER.index("ray_y") == ORDER.index("dc") + 2 and ORDER.index("cert") == ORDER.index("kkt") + 1
    assert _lib._PROTOTYPES["mllp_lp_pdhg_rays_scratch_bytes"] == _lib._PROTOTYPES["mllp_lp_pdhg_wide_scratch_bytes"]
    assert L.mllp_abi_version() == 6            # added without a bump


def test_the_limits_answer_without_a_gpu():
    lim = (ctypes.c_int64 * 4)()
    assert _lib.lib().mllp_lp_pdhg_rays_limits(lim) == 0 and list(lim) == [1024, 64, 64, 4096]
    from mllp_amd.graph import LPBatch, LPPdhgRays, LPPdhgWide, pdhg_rays_limits, pdhg_wide_limits
    assert pdhg_rays_limits() == pdhg_wide_limits() == (1024, 64, 64, 4096)
    assert hasattr(LPBatch, "pdhg_rays") and issubclass(LPPdhgRays, LPPdhgWide)
    assert _lib.lib().mllp_lp_pdhg_rays_limits(None) == -1 and b"mllp_lp_pdhg_rays_limits" in _lib.lib().mllp_last_error()
    # scratch bytes on a graph of sizes alone (a dummy whose first words are M, N, nnz, n_inst: nothing else is read): the closed form
    g, n = _sizes(M=3, N=5, n_inst=2), ctypes.c_int64(-7)
    for rows in (0, 64, 4096):
        assert _lib.lib().mllp_lp_pdhg_rays_scratch_bytes(g, rows, ctypes.byref(n)) == 0 and n.value == 4 * (27 * 2 + 6 * 5 + 5 * 3)
        assert _lib.lib().mllp_lp_pdhg_wide_scratch_bytes(g, rows, ctypes.byref(n)) == 0 and n.value == 4 * (21 * 2 + 6 * 5 + 5 * 3)
    for rows in (-64, 1, 96, 4160):
        n = ctypes.c_int64(-7)
        assert _lib.lib().mllp_lp_pdhg_rays_scratch_bytes(g, rows, ctypes.byref(n)) == -1 and n.value == -7
        assert b"mllp_lp_pdhg_rays_scratch_bytes: rows_per_item" in _lib.lib().mllp_last_error()
    assert _lib.lib().mllp_lp_pdhg_rays_scratch_bytes(None, 0, ctypes.byref(n)) == -1


def test_every_refusal_carries_the_wide_calls_words_under_this_calls_name():
    """the scalar checks come before the graph is read and before any HIP call, and a refused call dereferences no pointer:
    non-null dummies stand for the graph and the device buffers"""
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = dict(g=p, x1=p, x2=p, x0=None, y0=None, iter_begin=0, iter_end=10, check_every=64, eps=EPS, step=0.9, beta=0.5, ruiz=10, pc=1, pw=1, span=16.0,
              reflect=1, ray_eps=EPS, rows=0, x=p, y=p, dr=None, dc=None, ray_x=None, ray_y=None, status=p, kkt=None, cert=None, scratch=None, stream=None)
    nan, inf = float("nan"), float("inf")
    shared = [dict(g=None), dict(x1=None), dict(x2=None), dict(x=None), dict(y=None), dict(status=None), dict(iter_begin=-1), dict(iter_end=-1),
              dict(iter_begin=11), dict(iter_begin=5, iter_end=4), dict(check_every=-1), dict(eps=nan), dict(eps=inf), dict(eps=-1.0), dict(step=nan),
              dict(step=0.0), dict(step=1.5), dict(beta=nan), dict(beta=0.0), dict(beta=1.0), dict(ruiz=-1), dict(ruiz=65), dict(span=nan), dict(span=inf),
              dict(span=0.5), dict(rows=-64), dict(rows=1), dict(rows=96), dict(rows=4160), dict(rows=1 << 40), dict(ruiz=65, span=0.5),
              dict(beta=nan, ruiz=-1), dict(eps=nan, ray_eps=nan), dict(span=0.5, ray_eps=inf)]
    for kw in shared:
        args = dict(ok, **kw)
        assert L.mllp_lp_pdhg_rays(*[args[k] for k in ORDER]) == -1, kw
        mine = L.mllp_last_error()
        assert L.mllp_lp_pdhg_wide(*[args[k] for k in WIDE]) == -1, kw
        theirs = L.mllp_last_error()
        assert mine.startswith(b"mllp_lp_pdhg_rays: ") and theirs.startswith(b"mllp_lp_pdhg_wide: "), (kw, mine, theirs)
        assert mine.split(b": ", 1)[1].replace(b"mllp_lp_pdhg_rays", b"@") == theirs.split(b": ", 1)[1].replace(b"mllp_lp_pdhg_wide", b"@"), (kw, mine, theirs)
    for kw in (dict(ray_eps=nan), dict(ray_eps=inf), dict(ray_eps=-inf)):
        args = dict(ok, **kw)
        assert L.mllp_lp_pdhg_rays(*[args[k] for k in ORDER]) == -1 and b"mllp_lp_pdhg_rays: ray_eps" in L.mllp_last_error(), kw
    for kw in (dict(ray_eps=-1.0), dict(ray_eps=0.0), dict(ray_eps=-1e30)):
        args = dict(ok, x=None, **kw)           # (accepted values: the refusal is the null d_x, not ray_eps)
        assert L.mllp_lp_pdhg_rays(*[args[k] for k in ORDER]) == -1 and b"null argument" in L.mllp_last_error(), kw
    # the start may not lie on a new output (a graph of sizes alone, as above; the refusal comes before anything else is read)
    g = _sizes(M=3, N=5, n_inst=2)
    q = ctypes.cast((ctypes.c_float * 64)(), ctypes.c_void_p)
    for kw in (dict(x0=q, ray_x=q), dict(y0=q, ray_x=q), dict(x0=q, ray_y=q), dict(y0=q, ray_y=q), dict(x0=q, cert=q), dict(y0=q, cert=q),
               dict(x0=ctypes.c_void_p(q.value + 16), ray_x=q), dict(y0=ctypes.c_void_p(q.value + 8), ray_y=q), dict(x0=ctypes.c_void_p(q.value + 28), cert=q)):
        args = dict(ok, g=g, scratch=p, **kw)
        assert L.mllp_lp_pdhg_rays(*[args[k] for k in ORDER]) == -1 and b"mllp_lp_pdhg_rays: d_x0 or d_y0 overlaps an output" in L.mllp_last_error(), kw


def test_the_header_says_what_the_call_is():
    flat = " ".join(open(_lib.HEADER_PATH).read().replace("\n *", " ").split())
    assert "mllp_lp_pdhg_rays is under the MEMORY CONTRACT below as mllp_lp_pdhg is" in flat
    assert "mllp_lp_pdhg_wide is under the MEMORY CONTRACT below as mllp_lp_pdhg is" in flat            # ... beside its neighbour's
    assert "which is 4 (27 n_inst + 6 N + 5 M)" in flat and "which is 4 (21 n_inst + 6 N + 5 M)" in flat
    assert "qp <= ray_eps: code 4, primal infeasible" in flat and "Otherwise qd <= ray_eps: code 5, dual infeasible" in flat
    assert "With ray_eps < 0 nothing is evaluated and nothing changes" in flat
    assert "EXACTLY the launches of mllp_lp_pdhg_wide for the same arguments" in flat
    assert "The persistent calls (mllp_lp_pdhg, mllp_lp_pdhg_scaled, mllp_lp_pdhg_halpern) get no detection" in flat
    assert "|x|_1 >= 1 / qp >= 1 / ray_eps" in flat
