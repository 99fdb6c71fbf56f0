"""mllp_lp_pdhg_wide under the stream contract of tests/test_stream_contract.py and under the header's MEMORY CONTRACT, in
the pattern of tests/test_pdhg_halpern_stream.py: the row of the census, the Specs and the cells are added to the tables of the
imported module when this file is imported, which is at collection whenever the suite is collected as a whole (test_census
fails if tests/test_stream_contract.py is collected without this file, as it must for an export without a row).  The cells
run through that file's own test bodies: a delayed side stream with inputs that arrive late, and a capture replayed on a
second data set (c and b scaled by positive factors and another start, as in that file).  Variants: rows_per_item 64 (the
40 x 100 instance has two column items) and the default.

ITER_END.  A call is 2 launches per iteration and 3 per check, so the cells' limit sizes the captured graph.  The persistent
call (mllp_lp_pdhg_halpern, same options) stops these two instances, on either data set, after at most PERSISTENT_ITERS
iterations (192 and 320 on the first data set, 192 and 384 on the second: 384); the limit is the smallest multiple of 64 at or
above twice that: ITER_END = 768, which makes a graph of 40 + 2 ITER_END + 3 ITER_END / 64 = 1612 nodes.
test_the_limit_is_twice_the_persistent_calls_count holds the figure to the device.

THE ANCHOR of both data sets is tests/test_pdhg_halpern_stream.py's, rule-independent: code 0 within the limit at a multiple of
check_every, the three errors recomputed in fp64 within eps (1 + 2^-6), the m largest entries of x the planted basis, the final
weight inside the clamp, the factors positive and finite.

The memory contract: outputs and scratch poisoned with zeros, NaN or the largest float give the same bits on a call with
iter_begin = 0; the guard words around every buffer are intact; the inputs are unchanged.  (What a call with iter_begin > 0 makes
of such scratch is tests/test_pdhg_wide.py's: code 9 for every instance.)
"""
import ctypes

import pytest
import torch

import test_pdhg_halpern_stream as hs
import test_stream_contract as sc
from guarded import PATTERNS, Guarded, same_bits
from mllp_amd import _lib
from test_stream_contract import side  # noqa: F401  (the fixture of the cells)

FN = "mllp_lp_pdhg_wide"
PERSISTENT_ITERS = 384          # the most iterations of mllp_lp_pdhg_halpern on the two instances, over both data sets
ITER_END = -(-2 * PERSISTENT_ITERS // 64) * 64
CHECK, EPS, SPAN = hs.CHECK, hs.EPS, hs.SPAN
SHAPES = hs.SHAPES
VARIANTS = {"rows64": 64, "default": 0}         # rows_per_item
SCRATCH_WORDS = 21 * len(SHAPES) + sum(6 * n + 5 * m for m, n in SHAPES)


def _make(variant):
    def make(case, config):
        import test_basis_repair as tb
        from mllp_amd.graph import LPBatch
        c = tb.planted_shapes(SHAPES, 40)
        b, _, st = tb._planted(LPBatch, c)
        n = ctypes.c_int64()
        _lib.check(_lib.lib().mllp_lp_pdhg_wide_scratch_bytes(b._h, VARIANTS[variant], ctypes.byref(n)))
        assert n.value // 4 == SCRATCH_WORDS
        x0, y0 = hs._starts(c, 3)
        torch.cuda.synchronize()
        return sc.Plain(f"pdhg_wide {variant}", b, hs._second, c=c, values=st["values"], labels=st["labels"], x1=sc._f32(st["x1"]),
                        x2=sc._f32(st["x2"]), x0=x0, y0=y0, rows=VARIANTS[variant], scratch_floats=SCRATCH_WORDS, h=b._h)
    return make


def _call(ctx, x1, x2, x0, y0, o, scratch):
    return _lib.lib().mllp_lp_pdhg_wide(ctx.h, x1.ptr, x2.ptr, x0.ptr, y0.ptr, 0, ITER_END, CHECK, EPS, 0.9, 0.5, 10, 1, 1, SPAN, 1, ctx.rows,
                                       o["x"].ptr, o["y"].ptr, o["dr"].ptr, o["dc"].ptr, o["status"].ptr, o["kkt"].ptr, scratch.ptr, sc._s())


def ep_pdhg_wide(ctx, B):
    c, K = ctx.c, len(ctx.c["inst_m"])
    x1, x2, x0, y0 = B.ro("x1", ctx.x1), B.ro("x2", ctx.x2), B.ro("x0", ctx.x0), B.ro("y0", ctx.y0)
    o = dict(x=B.rw("x", c["N"]), y=B.rw("y", c["M"]), dr=B.rw("dr", c["M"]), dc=B.rw("dc", c["N"]),
             status=B.rw("status", 4 * K, dtype=torch.int32), kkt=B.rw("kkt", 6 * K))
    scratch = B.rw("scratch", ctx.scratch_floats)
    _lib.check(_call(ctx, x1, x2, x0, y0, o, scratch))
    return o


def anchor_pdhg_wide(ctx):
    inner = hs.anchor_pdhg_halpern(ctx)

    def check(out):
        K = len(ctx.c["inst_m"])
        assert (out["status"].reshape(K, 4)[:, 1] <= ITER_END).all()
        inner(out)                                  # (its own limit, 4096, lies above ITER_END)
    return check


CELLS = [(f"pdhg_wide_{v}", ("own", f"pdhg_wide_{v}", "-", "-")) for v in VARIANTS]
sc.LAUNCH[FN] = tuple(name for name, _ in CELLS)
for _v in VARIANTS:
    sc.SPECS[f"pdhg_wide_{_v}"] = sc.Spec(ep_pdhg_wide, anchor_pdhg_wide, (FN,), not_finite=("status",))
    sc.OWN_MAKERS[f"pdhg_wide_{_v}"] = _make(_v)
# (new lists: the parametrisation of that file's own tests keeps the lists it was given)
sc.LATE_CELLS = sc.LATE_CELLS + CELLS
sc.CAPTURE_CELLS = sc.CAPTURE_CELLS + CELLS


def test_the_census_has_the_row():
    header = open(_lib.HEADER_PATH).read()
    assert FN in sc.stream_prototypes(header)
    assert FN in sc.LAUNCH and sc.LAUNCH[FN] == ("pdhg_wide_rows64", "pdhg_wide_default")
    missing, stale = sc.census(header)
    assert FN not in missing and not stale
    flat = sc._flat_text(header)
    assert "mllp_lp_pdhg_wide is under the MEMORY CONTRACT below as mllp_lp_pdhg is" in flat          # a sentence of its own
    assert "mllp_lp_pdhg_halpern is under the MEMORY CONTRACT below as mllp_lp_pdhg is" in flat       # ... beside its neighbour's
    assert "mllp_basis_simplex, mllp_lp_pdhg and mllp_optim_step call" in flat                        # ... and the pinned one stands
    assert ITER_END % 64 == 0 and 2 * PERSISTENT_ITERS <= ITER_END < 2 * PERSISTENT_ITERS + 64 and ITER_END <= hs.MAX_ITERS


@pytest.mark.gpu
def test_the_limit_is_twice_the_persistent_calls_count():
    """PERSISTENT_ITERS is what mllp_lp_pdhg_halpern takes on these instances, on the data set that needs more"""
    ctx = sc.resolve(("own", "pdhg_wide_default", "-", "-"))
    most = 0
    x1, x2 = ctx.b.x1.clone(), ctx.b.x2.clone()
    try:
        for data in (ctx, hs._second(ctx)):
            ctx.b.x1.copy_(torch.tensor(data.x1, device="cuda"))
            ctx.b.x2.copy_(torch.tensor(data.x2, device="cuda"))
            ctx.b.invalidate_inputs()
            res = ctx.b.pdhg_halpern(hs.MAX_ITERS, eps=EPS, check_every=CHECK, weight_span=SPAN, x0=torch.tensor(data.x0, device="cuda"),
                                     y0=torch.tensor(data.y0, device="cuda"))
            status = res.status.cpu().numpy()
            print(data.case, [list(s) for s in status])
            assert (status[:, 0] == 0).all()
            most = max(most, int(status[:, 1].max()))
    finally:
        ctx.b.x1.copy_(x1)
        ctx.b.x2.copy_(x2)
        ctx.b.invalidate_inputs()
    assert most == PERSISTENT_ITERS, most


@pytest.mark.gpu
@pytest.mark.parametrize("cell", CELLS, ids=sc._id)
def test_late_inputs_on_a_delayed_side_stream(cell, side):  # noqa: F811
    sc.test_late_inputs_on_a_delayed_side_stream(cell, side)


@pytest.mark.gpu
@pytest.mark.parametrize("cell", CELLS, ids=sc._id)
def test_capture_then_replay_on_other_inputs(cell):
    sc.test_capture_then_replay_on_other_inputs(cell)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_memory_contract(variant):
    ctx = sc.resolve(("own", f"pdhg_wide_{variant}", "-", "-"))
    c, K = ctx.c, len(ctx.c["inst_m"])
    runs = {}
    for name, fill in PATTERNS.items():
        ins = dict(x1=Guarded(c["N"], device="cuda", data=ctx.x1, name="x1", shift=4), x2=Guarded(c["M"], device="cuda", data=ctx.x2, name="x2", shift=8),
                   x0=Guarded(c["N"], device="cuda", data=ctx.x0, name="x0", shift=12), y0=Guarded(c["M"], device="cuda", data=ctx.y0, name="y0", shift=4))
        outs = dict(x=Guarded(c["N"], device="cuda", fill=fill, name="x", shift=4), y=Guarded(c["M"], device="cuda", fill=fill, name="y", shift=8),
                    dr=Guarded(c["M"], device="cuda", fill=fill, name="dr", shift=12), dc=Guarded(c["N"], device="cuda", fill=fill, name="dc", shift=8),
                    status=Guarded(4 * K, torch.int32, "cuda", fill=fill, name="status", shift=4),
                    kkt=Guarded(6 * K, device="cuda", fill=fill, name="kkt", shift=4))
        scratch = Guarded(ctx.scratch_floats, device="cuda", fill=fill, name="scratch", shift=4)
        assert _call(ctx, ins["x1"], ins["x2"], ins["x0"], ins["y0"], outs, scratch) == 0
        torch.cuda.synchronize()
        for v in list(ins.values()) + list(outs.values()) + [scratch]:
            v.check()
        runs[name] = {k: v.bits() for k, v in outs.items()}
    anchor_pdhg_wide(ctx)(runs["zero"])
    for name in runs:
        same_bits(runs[name], runs["zero"], f"{variant}: outputs under {name} poison against zero poison")
    # ... and they are the persistent call's bits on the same buffers' worth of data
    res = ctx.b.pdhg_halpern(ITER_END, eps=EPS, check_every=CHECK, weight_span=SPAN, x0=torch.tensor(ctx.x0, device="cuda"),
                             y0=torch.tensor(ctx.y0, device="cuda"))
    torch.cuda.synchronize()
    want = {k: getattr(res, k).cpu().numpy().view("int32").reshape(-1) for k in ("x", "y", "dr", "dc", "status", "kkt")}
    same_bits(runs["zero"], want, f"{variant}: against mllp_lp_pdhg_halpern")
