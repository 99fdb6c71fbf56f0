"""mllp_lp_pdhg_spectral under the stream contract of tests/test_stream_contract.py and under the header's MEMORY CONTRACT, in the
pattern of tests/test_pdhg_rays_stream.py: the row of the census, the Specs and the cells are added to the tables of the
imported module when this file is imported, which is at collection whenever the suite is collected as a whole (test_census
fails if tests/test_stream_contract.py is collected without this file, as it must for an export without a row).  The cells run
through that file's own test bodies: a delayed side stream with inputs that arrive late, and a capture replayed on a second
data set.  Variants: rows_per_item 64 and the default, both with power_iters = 40 and detection off (this call's default).

The instances and the limit ITER_END are tests/test_pdhg_wide_stream.py's.  THE ANCHOR is that file's, which is rule-independent
(code 0 within the limit at a multiple of check_every, the three errors recomputed in fp64 within eps (1 + 2^-6), the m largest
entries of x the planted basis, the final weight inside the clamp, the factors positive and finite); in addition the rays are
zeros, the cert words say that no ray was evaluated, the estimate is positive and not above the bound, and kkt[3] is
fdiv(step, estimate), bit for bit.

LAUNCHES.  The header's closed form: mllp_lp_pdhg_rays' launches, 40 + 2 ITER_END + 3 ITER_END / CHECK here, and 3 P + 1 more in
the set-up; with power_iters = 0 exactly that call's.  Both are captured and the nodes counted.

The memory contract: outputs and scratch poisoned with zeros, NaN or the largest float give the same bits on a call with
iter_begin = 0, over every buffer, d_norm included; the guard words around every buffer are intact; the inputs are unchanged;
and a NULL d_norm moves no other bit.
"""
import ctypes

import numpy as np
import pytest
import torch

import test_pdhg_halpern_stream as hs
import test_pdhg_rays_stream as rs
import test_pdhg_wide_stream as ws
import test_stream_contract as sc
from guarded import PATTERNS, Guarded, same_bits
from mllp_amd import _lib
from test_stream_contract import side  # noqa: F401  (the fixture of the cells)

FN = "mllp_lp_pdhg_spectral"
ITER_END, CHECK, EPS, SPAN, SHAPES = ws.ITER_END, ws.CHECK, ws.EPS, ws.SPAN, ws.SHAPES
POWER = 40
VARIANTS = {"rows64": 64, "default": 0}         # rows_per_item
SCRATCH_WORDS = 29 * len(SHAPES) + sum(6 * n + 5 * m for m, n in SHAPES)
OUTS = ("x", "y", "dr", "dc", "ray_x", "ray_y", "status", "kkt", "cert", "norm")
INF = np.float32(np.inf).view(np.int32)


def _make(variant):
    def make(case, config):
        import test_basis_repair as tb
        from mllp_amd.graph import LPBatch
        c = tb.planted_shapes(SHAPES, 40)
        b, _, st = tb._planted(LPBatch, c)
        n = ctypes.c_int64()
        _lib.check(_lib.lib().mllp_lp_pdhg_spectral_scratch_bytes(b._h, VARIANTS[variant], ctypes.byref(n)))
        assert n.value // 4 == SCRATCH_WORDS == rs.SCRATCH_WORDS + 2 * len(SHAPES)
        x0, y0 = hs._starts(c, 3)
        torch.cuda.synchronize()
        return sc.Plain(f"pdhg_spectral {variant}", b, hs._second, c=c, values=st["values"], labels=st["labels"], x1=sc._f32(st["x1"]),
                        x2=sc._f32(st["x2"]), x0=x0, y0=y0, rows=VARIANTS[variant], scratch_floats=SCRATCH_WORDS, h=b._h)
    return make


def _call(ctx, x1, x2, x0, y0, o, scratch, power=POWER, norm=True):
    outs = [o[k].ptr if k != "norm" or norm else None for k in OUTS]
    return _lib.lib().mllp_lp_pdhg_spectral(ctx.h, x1.ptr, x2.ptr, x0.ptr, y0.ptr, 0, ITER_END, CHECK, EPS, 0.9, 0.5, 10, 1, 1, SPAN, 1, -1.0, power,
                                           ctx.rows, *outs, scratch.ptr, sc._s())


def ep_pdhg_spectral(ctx, B):
    c, K = ctx.c, len(ctx.c["inst_m"])
    x1, x2, x0, y0 = B.ro("x1", ctx.x1), B.ro("x2", ctx.x2), B.ro("x0", ctx.x0), B.ro("y0", ctx.y0)
    o = dict(x=B.rw("x", c["N"]), y=B.rw("y", c["M"]), dr=B.rw("dr", c["M"]), dc=B.rw("dc", c["N"]), ray_x=B.rw("ray_x", c["N"]),
             ray_y=B.rw("ray_y", c["M"]), status=B.rw("status", 4 * K, dtype=torch.int32), kkt=B.rw("kkt", 6 * K), cert=B.rw("cert", 4 * K),
             norm=B.rw("norm", 2 * K))
    scratch = B.rw("scratch", ctx.scratch_floats)
    _lib.check(_call(ctx, x1, x2, x0, y0, o, scratch))
    return o


def anchor_pdhg_spectral(ctx):
    inner = ws.anchor_pdhg_wide(ctx)

    def check(out):
        inner({k: v for k, v in out.items() if k in ("x", "y", "dr", "dc", "status", "kkt")})
        K = len(ctx.c["inst_m"])
        assert not np.asarray(out["ray_x"]).any() and not np.asarray(out["ray_y"]).any()
        assert np.array_equal(np.asarray(out["cert"]).view(np.int32).reshape(K, 4), np.tile(np.array([INF, 0, INF, 0], np.int32), (K, 1)))
        norm = np.asarray(out["norm"]).view(np.float32).reshape(K, 2)
        eta = np.asarray(out["kkt"]).view(np.float32).reshape(K, 6)[:, 3]
        assert (norm[:, 0] > 0).all() and (norm[:, 0] <= norm[:, 1]).all() and np.isfinite(norm).all(), norm
        assert np.array_equal(eta, np.float32(0.9) / norm[:, 0]), (eta, norm)
    return check


CELLS = [(f"pdhg_spectral_{v}", ("own", f"pdhg_spectral_{v}", "-", "-")) for v in VARIANTS]
sc.LAUNCH[FN] = tuple(name for name, _ in CELLS)
for _v in VARIANTS:
    sc.SPECS[f"pdhg_spectral_{_v}"] = sc.Spec(ep_pdhg_spectral, anchor_pdhg_spectral, (FN,), not_finite=("status", "cert"))
    sc.OWN_MAKERS[f"pdhg_spectral_{_v}"] = _make(_v)
# (new lists: the parametrisation of that file's own tests keeps the lists it was given)
sc.LATE_CELLS = sc.LATE_CELLS + CELLS
sc.CAPTURE_CELLS = sc.CAPTURE_CELLS + CELLS


def test_the_census_has_the_row():
    header = open(_lib.HEADER_PATH).read()
    assert FN in sc.stream_prototypes(header)
    assert FN in sc.LAUNCH and sc.LAUNCH[FN] == ("pdhg_spectral_rows64", "pdhg_spectral_default")
    missing, stale = sc.census(header)
    assert FN not in missing and not stale
    # without the row the census names the call
    rows = dict(sc.LAUNCH)
    try:
        del sc.LAUNCH[FN]
        assert FN in sc.census(header)[0]
    finally:
        sc.LAUNCH.clear()
        sc.LAUNCH.update(rows)
    flat = sc._flat_text(header)
    assert "mllp_lp_pdhg_spectral is under the MEMORY CONTRACT below as mllp_lp_pdhg is" in flat      # a sentence of its own
    assert "mllp_lp_pdhg_rays is under the MEMORY CONTRACT below as mllp_lp_pdhg is" in flat          # ... beside its neighbour's
    assert "mllp_basis_simplex, mllp_lp_pdhg and mllp_optim_step call" in flat                        # ... and the pinned one stands


@pytest.mark.gpu
@pytest.mark.parametrize("cell", CELLS, ids=sc._id)
def test_late_inputs_on_a_delayed_side_stream(cell, side):  # noqa: F811
    sc.test_late_inputs_on_a_delayed_side_stream(cell, side)


@pytest.mark.gpu
@pytest.mark.parametrize("cell", CELLS, ids=sc._id)
def test_capture_then_replay_on_other_inputs(cell):
    sc.test_capture_then_replay_on_other_inputs(cell)


def _buffers(ctx, fill):
    c, K = ctx.c, len(ctx.c["inst_m"])
    g = lambda n, name, shift, dtype=torch.float32, **kw: Guarded(n, dtype, "cuda", name=name, shift=shift, **kw)      # noqa: E731
    ins = dict(x1=g(c["N"], "x1", 4, data=ctx.x1), x2=g(c["M"], "x2", 8, data=ctx.x2), x0=g(c["N"], "x0", 12, data=ctx.x0),
               y0=g(c["M"], "y0", 4, data=ctx.y0))
    outs = dict(x=g(c["N"], "x", 4, fill=fill), y=g(c["M"], "y", 8, fill=fill), dr=g(c["M"], "dr", 12, fill=fill), dc=g(c["N"], "dc", 8, fill=fill),
                ray_x=g(c["N"], "ray_x", 12, fill=fill), ray_y=g(c["M"], "ray_y", 4, fill=fill), status=g(4 * K, "status", 4, torch.int32, fill=fill),
                kkt=g(6 * K, "kkt", 4, fill=fill), cert=g(4 * K, "cert", 8, fill=fill), norm=g(2 * K, "norm", 12, fill=fill))
    return ins, outs, g(ctx.scratch_floats, "scratch", 4, fill=fill)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_the_captured_graph_has_the_stated_node_count(variant):
    """capture only: no graph is instantiated or replayed (the replay is the capture cell's)"""
    ctx = sc.resolve(("own", f"pdhg_spectral_{variant}", "-", "-"))
    ins, outs, scratch = _buffers(ctx, PATTERNS["zero"])
    torch.cuda.synchronize()
    counts = {}
    for name, run in (("spectral", lambda: _call(ctx, ins["x1"], ins["x2"], ins["x0"], ins["y0"], outs, scratch)),
                      ("no rounds", lambda: _call(ctx, ins["x1"], ins["x2"], ins["x0"], ins["y0"], outs, scratch, power=0)),
                      ("three rounds", lambda: _call(ctx, ins["x1"], ins["x2"], ins["x0"], ins["y0"], outs, scratch, power=3)),
                      ("rays", lambda: rs._call(ctx, ins["x1"], ins["x2"], ins["x0"], ins["y0"], outs, scratch, ray_eps=-1.0))):
        graph = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(graph):
            assert run() == 0
        counts[name] = rs._nodes(graph)
        del graph
    print(variant, counts)
    rays = 40 + 2 * ITER_END + 3 * (ITER_END // CHECK)
    assert counts["rays"] == counts["no rounds"] == rays
    assert counts["spectral"] == rays + 3 * POWER + 1 and counts["three rounds"] == rays + 3 * 3 + 1


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_memory_contract(variant):
    ctx = sc.resolve(("own", f"pdhg_spectral_{variant}", "-", "-"))
    runs = {}
    for name, fill in PATTERNS.items():
        ins, outs, scratch = _buffers(ctx, fill)
        assert _call(ctx, ins["x1"], ins["x2"], ins["x0"], ins["y0"], outs, scratch) == 0
        torch.cuda.synchronize()
        for v in list(ins.values()) + list(outs.values()) + [scratch]:
            v.check()
        runs[name] = {k: v.bits() for k, v in outs.items()}
    anchor_pdhg_spectral(ctx)(runs["zero"])
    for name in runs:
        same_bits(runs[name], runs["zero"], f"{variant}: outputs under {name} poison against zero poison")
    # a NULL d_norm: the buffer keeps its poison and no other bit moves
    ins, outs, scratch = _buffers(ctx, PATTERNS["nan"])
    before = outs["norm"].bits().copy()
    assert _call(ctx, ins["x1"], ins["x2"], ins["x0"], ins["y0"], outs, scratch, norm=False) == 0
    torch.cuda.synchronize()
    for v in list(ins.values()) + list(outs.values()) + [scratch]:
        v.check()
    assert np.array_equal(outs["norm"].bits(), before)
    same_bits({k: v.bits() for k, v in outs.items() if k != "norm"}, {k: v for k, v in runs["zero"].items() if k != "norm"}, f"{variant}: NULL d_norm")
