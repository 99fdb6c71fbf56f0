"""mllp_lp_pdhg_rays under the stream contract of tests/test_stream_contract.py and under the header's MEMORY CONTRACT, in the
pattern of tests/test_pdhg_wide_stream.py: the row of the census, the Specs and the cells are added to the tables of the
imported module when this file is imported, which is at collection whenever the suite is collected as a whole (test_census
fails if tests/test_stream_contract.py is collected without this file, as it must for an export without a row).  The cells run
through that file's own test bodies: a delayed side stream with inputs that arrive late, and a capture replayed on a second
data set.  Variants: rows_per_item 64 and the default, both with detection on (ray_eps = 2^-10).

The instances, the limit ITER_END and THE ANCHOR are tests/test_pdhg_wide_stream.py's: the two instances are feasible, detection
looks at them and stops neither, so the six outputs that the wide call has are that call's and its anchor holds; in addition the
rays are zeros and the cert words say that no ray came near ray_eps.

LAUNCHES.  The header promises exactly mllp_lp_pdhg_wide's launches for the same arguments: both calls are captured with the
same limits and the two graphs must have the same number of nodes, which is the closed form of that file's docstring.

The memory contract: outputs and scratch poisoned with zeros, NaN or the largest float give the same bits on a call with
iter_begin = 0, over every buffer, the three new ones included; the guard words around every buffer are intact; the inputs are
unchanged.
"""
import ctypes

import numpy as np
import pytest
import torch

import test_pdhg_halpern_stream as hs
import test_pdhg_wide_stream as ws
import test_stream_contract as sc
from guarded import PATTERNS, Guarded, same_bits
from mllp_amd import _lib
from test_stream_contract import side  # noqa: F401  (the fixture of the cells)

FN = "mllp_lp_pdhg_rays"
ITER_END, CHECK, EPS, SPAN, SHAPES = ws.ITER_END, ws.CHECK, ws.EPS, ws.SPAN, ws.SHAPES
RAY_EPS = 2.0 ** -10
VARIANTS = {"rows64": 64, "default": 0}         # rows_per_item
SCRATCH_WORDS = 27 * len(SHAPES) + sum(6 * n + 5 * m for m, n in SHAPES)
OUTS = ("x", "y", "dr", "dc", "ray_x", "ray_y", "status", "kkt", "cert")


def _make(variant):
    def make(case, config):
        import test_basis_repair as tb
        from mllp_amd.graph import LPBatch
        c = tb.planted_shapes(SHAPES, 40)
        b, _, st = tb._planted(LPBatch, c)
        n = ctypes.c_int64()
        _lib.check(_lib.lib().mllp_lp_pdhg_rays_scratch_bytes(b._h, VARIANTS[variant], ctypes.byref(n)))
        assert n.value // 4 == SCRATCH_WORDS == ws.SCRATCH_WORDS + 6 * len(SHAPES)
        x0, y0 = hs._starts(c, 3)
        torch.cuda.synchronize()
        return sc.Plain(f"pdhg_rays {variant}", b, hs._second, c=c, values=st["values"], labels=st["labels"], x1=sc._f32(st["x1"]),
                        x2=sc._f32(st["x2"]), x0=x0, y0=y0, rows=VARIANTS[variant], scratch_floats=SCRATCH_WORDS, h=b._h)
    return make


def _call(ctx, x1, x2, x0, y0, o, scratch, ray_eps=RAY_EPS):
    return _lib.lib().mllp_lp_pdhg_rays(ctx.h, x1.ptr, x2.ptr, x0.ptr, y0.ptr, 0, ITER_END, CHECK, EPS, 0.9, 0.5, 10, 1, 1, SPAN, 1, ray_eps, ctx.rows,
                                       *[o[k].ptr for k in OUTS], scratch.ptr, sc._s())


def ep_pdhg_rays(ctx, B):
    c, K = ctx.c, len(ctx.c["inst_m"])
    x1, x2, x0, y0 = B.ro("x1", ctx.x1), B.ro("x2", ctx.x2), B.ro("x0", ctx.x0), B.ro("y0", ctx.y0)
    o = dict(x=B.rw("x", c["N"]), y=B.rw("y", c["M"]), dr=B.rw("dr", c["M"]), dc=B.rw("dc", c["N"]), ray_x=B.rw("ray_x", c["N"]),
             ray_y=B.rw("ray_y", c["M"]), status=B.rw("status", 4 * K, dtype=torch.int32), kkt=B.rw("kkt", 6 * K), cert=B.rw("cert", 4 * K))
    scratch = B.rw("scratch", ctx.scratch_floats)
    _lib.check(_call(ctx, x1, x2, x0, y0, o, scratch))
    return o


def anchor_pdhg_rays(ctx):
    inner = ws.anchor_pdhg_wide(ctx)

    def check(out):
        inner({k: v for k, v in out.items() if k in ("x", "y", "dr", "dc", "status", "kkt")})
        K = len(ctx.c["inst_m"])
        cert = np.asarray(out["cert"]).view(np.float32).reshape(K, 4)
        assert not np.asarray(out["ray_x"]).any() and not np.asarray(out["ray_y"]).any()
        assert not np.isnan(cert).any() and np.isfinite(cert[:, [1, 3]]).all() and (np.minimum(cert[:, 0], cert[:, 2]) > RAY_EPS).all(), cert
    return check


CELLS = [(f"pdhg_rays_{v}", ("own", f"pdhg_rays_{v}", "-", "-")) for v in VARIANTS]
sc.LAUNCH[FN] = tuple(name for name, _ in CELLS)
for _v in VARIANTS:
    sc.SPECS[f"pdhg_rays_{_v}"] = sc.Spec(ep_pdhg_rays, anchor_pdhg_rays, (FN,), not_finite=("status", "cert"))
    sc.OWN_MAKERS[f"pdhg_rays_{_v}"] = _make(_v)
# (new lists: the parametrisation of that file's own tests keeps the lists it was given)
sc.LATE_CELLS = sc.LATE_CELLS + CELLS
sc.CAPTURE_CELLS = sc.CAPTURE_CELLS + CELLS


def test_the_census_has_the_row():
    header = open(_lib.HEADER_PATH).read()
    assert FN in sc.stream_prototypes(header)
    assert FN in sc.LAUNCH and sc.LAUNCH[FN] == ("pdhg_rays_rows64", "pdhg_rays_default")
    missing, stale = sc.census(header)
    assert FN not in missing and not stale
    flat = sc._flat_text(header)
    assert "mllp_lp_pdhg_rays is under the MEMORY CONTRACT below as mllp_lp_pdhg is" in flat          # a sentence of its own
    assert "mllp_lp_pdhg_wide is under the MEMORY CONTRACT below as mllp_lp_pdhg is" in flat          # ... beside its neighbour's
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
                kkt=g(6 * K, "kkt", 4, fill=fill), cert=g(4 * K, "cert", 8, fill=fill))
    return ins, outs, g(ctx.scratch_floats, "scratch", 4, fill=fill)


def _nodes(graph):
    """the nodes of a captured graph that was kept (hipGraphGetNodes with no array: the count alone)"""
    hip = ctypes.CDLL("libamdhip64.so")
    n = ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(ctypes.c_void_p(graph.raw_cuda_graph()), None, ctypes.byref(n)) == 0
    return n.value


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_the_captured_graph_has_the_wide_calls_node_count(variant):
    """capture only: neither graph is instantiated or replayed (the replay is the capture cell's)"""
    ctx = sc.resolve(("own", f"pdhg_rays_{variant}", "-", "-"))
    ins, outs, scratch = _buffers(ctx, PATTERNS["zero"])
    torch.cuda.synchronize()
    counts = {}
    for name, run in (("rays", lambda: _call(ctx, ins["x1"], ins["x2"], ins["x0"], ins["y0"], outs, scratch)),
                      ("off", lambda: _call(ctx, ins["x1"], ins["x2"], ins["x0"], ins["y0"], outs, scratch, ray_eps=-1.0)),
                      ("wide", lambda: ws._call(ctx, ins["x1"], ins["x2"], ins["x0"], ins["y0"], outs, scratch))):
        graph = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(graph):
            assert run() == 0
        counts[name] = _nodes(graph)
        del graph
    print(variant, counts)
    assert counts["rays"] == counts["off"] == counts["wide"] == 40 + 2 * ITER_END + 3 * (ITER_END // CHECK)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_memory_contract(variant):
    ctx = sc.resolve(("own", f"pdhg_rays_{variant}", "-", "-"))
    runs = {}
    for name, fill in PATTERNS.items():
        ins, outs, scratch = _buffers(ctx, fill)
        assert _call(ctx, ins["x1"], ins["x2"], ins["x0"], ins["y0"], outs, scratch) == 0
        torch.cuda.synchronize()
        for v in list(ins.values()) + list(outs.values()) + [scratch]:
            v.check()
        runs[name] = {k: v.bits() for k, v in outs.items()}
    anchor_pdhg_rays(ctx)(runs["zero"])
    for name in runs:
        same_bits(runs[name], runs["zero"], f"{variant}: outputs under {name} poison against zero poison")
    # ... and the six outputs that the wide call has are that call's bits on the same data
    ins, outs, scratch = _buffers(ctx, PATTERNS["nan"])
    assert ws._call(ctx, ins["x1"], ins["x2"], ins["x0"], ins["y0"], outs, scratch) == 0
    torch.cuda.synchronize()
    wide = ("x", "y", "dr", "dc", "status", "kkt")
    same_bits({k: runs["zero"][k] for k in wide}, {k: outs[k].bits() for k in wide}, f"{variant}: against mllp_lp_pdhg_wide")
