"""mllp_lp_pdhg_halpern under the stream contract of tests/test_stream_contract.py and under the header's MEMORY CONTRACT, in
the pattern of tests/test_pdhg_halpern_stream.py: the row of the census, the Specs and the cells are added to the tables of the
imported module when this file is imported, which is at collection whenever the suite is collected as a whole (test_census
fails if tests/test_stream_contract.py is collected without this file, as it must for an export without a row).  The cells
run through that file's own test bodies: a delayed side stream with inputs that arrive late, and a capture replayed on a
second data set (c and b scaled by positive factors -- the planted basis stays the unique optimum, the weight's start moves
by a factor of 2 -- and another start).  Variants: "lds" (every instance keeps its five vectors in LDS) and "scratch"
(max_lds_words = 100: the 5 x 12 instance in LDS, the 40 x 100 one in the caller's scratch, so both launches run).  Both
variants need scratch: tc, tr and the anchor (xr, yr) of every instance live there.

THE ANCHOR of both data sets is rule-independent: code 0 within max_iters at a multiple of check_every, the three errors
recomputed in fp64 within eps (1 + 2^-6), the m largest entries of x the planted basis, the final weight inside the clamp
around the weight's start, the factors positive and finite, status[3] = 0.

The memory contract: outputs (d_dr and d_dc among them) and scratch poisoned with zeros, NaN or the largest float give the
same bits; the guard words around every buffer are intact; the inputs are unchanged.  Planted batches only.
"""
import ctypes

import numpy as np
import pytest
import torch

import pdhg_oracle as pg
import test_stream_contract as sc
from guarded import PATTERNS, Guarded, same_bits
from mllp_amd import _lib
from test_stream_contract import side  # noqa: F401  (the fixture of the cells)

FN = "mllp_lp_pdhg_halpern"
MAX_ITERS, CHECK, EPS, SPAN = 4096, 64, 2.0 ** -10, 16.0
SHAPES = [(5, 12), (40, 100)]
VARIANTS = {"lds": None, "scratch": 100}        # max_lds_words (None: the kernel's limit); 3 n + 2 m = 46 and 380
SIDE_WORDS = sum(2 * n + 2 * m for m, n in SHAPES)


def _starts(c, seed):
    x0, y0 = np.zeros(c["N"], np.float32), np.zeros(c["M"], np.float32)
    for k in range(len(c["inst_m"])):
        rng = np.random.default_rng(seed + k)
        x0[c["ptr_n"][k]:c["ptr_n"][k + 1]] = rng.uniform(-0.5, 1.0, c["inst_n"][k])
        y0[c["ptr_m"][k]:c["ptr_m"][k + 1]] = rng.uniform(-0.5, 0.5, c["inst_m"][k])
    return x0, y0


def _make(variant):
    def make(case, config):
        import test_basis_repair as tb
        from mllp_amd.graph import LPBatch, pdhg_halpern_limits
        c = tb.planted_shapes(SHAPES, 40)
        b, _, st = tb._planted(LPBatch, c)
        lds = pdhg_halpern_limits()[0] if VARIANTS[variant] is None else VARIANTS[variant]
        n = ctypes.c_int64()
        _lib.check(_lib.lib().mllp_lp_pdhg_halpern_scratch_bytes(b._h, lds, ctypes.byref(n)))
        assert n.value // 4 == SIDE_WORDS + (0 if variant == "lds" else 3 * 100 + 2 * 40)
        x0, y0 = _starts(c, 3)
        torch.cuda.synchronize()
        return sc.Plain(f"pdhg_halpern {variant}", b, _second, c=c, values=st["values"], labels=st["labels"], x1=sc._f32(st["x1"]),
                        x2=sc._f32(st["x2"]), x0=x0, y0=y0, lds=lds, scratch_floats=n.value // 4, h=b._h)
    return make


def _second(ctx):
    def make():
        x0, y0 = _starts(ctx.c, 4)
        return ctx.with_data(x1=sc._f32(ctx.x1 * 1.5), x2=sc._f32(ctx.x2 * 0.75), x0=x0, y0=y0)
    return sc._second(ctx, make)


def _call(ctx, x1, x2, x0, y0, o, scratch):
    return _lib.lib().mllp_lp_pdhg_halpern(ctx.h, x1.ptr, x2.ptr, x0.ptr, y0.ptr, MAX_ITERS, CHECK, EPS, 0.9, 0.5, 10, 1, 1, SPAN, 1, ctx.lds,
                                          o["x"].ptr, o["y"].ptr, o["dr"].ptr, o["dc"].ptr, o["status"].ptr, o["kkt"].ptr, scratch.ptr, sc._s())


def ep_pdhg_halpern(ctx, B):
    c, K = ctx.c, len(ctx.c["inst_m"])
    x1, x2, x0, y0 = B.ro("x1", ctx.x1), B.ro("x2", ctx.x2), B.ro("x0", ctx.x0), B.ro("y0", ctx.y0)
    o = dict(x=B.rw("x", c["N"]), y=B.rw("y", c["M"]), dr=B.rw("dr", c["M"]), dc=B.rw("dc", c["N"]),
             status=B.rw("status", 4 * K, dtype=torch.int32), kkt=B.rw("kkt", 6 * K))
    scratch = B.rw("scratch", ctx.scratch_floats)
    _lib.check(_call(ctx, x1, x2, x0, y0, o, scratch))
    return o


def anchor_pdhg_halpern(ctx):
    def check(out):
        c, K = ctx.c, len(ctx.c["inst_m"])
        status, kkt = out["status"].reshape(K, 4), sc.fl(out["kkt"]).reshape(K, 6)
        x, y, dr, dc = sc.fl(out["x"]), sc.fl(out["y"]), sc.fl(out["dr"]), sc.fl(out["dc"])
        assert np.isfinite(dr).all() and (dr > 0).all() and np.isfinite(dc).all() and (dc > 0).all()
        for k, inst in enumerate(pg.split(c, ctx.values, ctx.x1, ctx.x2, ctx.labels)):
            code, it, restarts, flag = status[k]
            assert code == 0 and it % CHECK == 0 and 0 < it <= MAX_ITERS and restarts >= 0 and flag == 0, (ctx.case, k, status[k])
            s, r = slice(c["ptr_n"][k], c["ptr_n"][k + 1]), slice(c["ptr_m"][k], c["ptr_m"][k + 1])
            errs = pg.errors64(inst["A"], inst["b"], inst["c"], x[s], y[r])
            assert max(errs) <= EPS * (1 + 2.0 ** -6) and max(kkt[k][:3]) <= EPS, (ctx.case, k, errs, kkt[k])
            assert np.array_equal(pg.topm(x[s], inst["m"]), inst["labels"]), (ctx.case, k)
            eta, w0, w = kkt[k][3:]
            assert 0 < eta and 0 < w0 and np.float32(w0) / np.float32(SPAN) <= w <= np.float32(w0) * np.float32(SPAN), (ctx.case, k, kkt[k])
    return check


CELLS = [(f"pdhg_halpern_{v}", ("own", f"pdhg_halpern_{v}", "-", "-")) for v in VARIANTS]
sc.LAUNCH[FN] = tuple(name for name, _ in CELLS)
for _v in VARIANTS:
    sc.SPECS[f"pdhg_halpern_{_v}"] = sc.Spec(ep_pdhg_halpern, anchor_pdhg_halpern, (FN,), not_finite=("status",))
    sc.OWN_MAKERS[f"pdhg_halpern_{_v}"] = _make(_v)
# (new lists: the parametrisation of that file's own tests keeps the lists it was given)
sc.LATE_CELLS = sc.LATE_CELLS + CELLS
sc.CAPTURE_CELLS = sc.CAPTURE_CELLS + CELLS


def test_the_census_has_the_row():
    header = open(_lib.HEADER_PATH).read()
    assert FN in sc.stream_prototypes(header)
    assert FN in sc.LAUNCH and sc.LAUNCH[FN] == ("pdhg_halpern_lds", "pdhg_halpern_scratch")
    missing, stale = sc.census(header)
    assert FN not in missing and not stale
    flat = sc._flat_text(header)
    assert "mllp_lp_pdhg_halpern is under the MEMORY CONTRACT below as mllp_lp_pdhg is" in flat      # a sentence of its own
    assert "mllp_lp_pdhg_scaled is under the MEMORY CONTRACT below as mllp_lp_pdhg is" in flat       # ... beside its neighbour's
    assert "mllp_basis_simplex, mllp_lp_pdhg and mllp_optim_step call" in flat                     # ... and the pinned one stands


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
    ctx = sc.resolve(("own", f"pdhg_halpern_{variant}", "-", "-"))
    c, K = ctx.c, len(ctx.c["inst_m"])
    runs = {}
    for name, fill in PATTERNS.items():
        ins = dict(x1=Guarded(c["N"], device="cuda", data=ctx.x1, name="x1", shift=4), x2=Guarded(c["M"], device="cuda", data=ctx.x2, name="x2", shift=8),
                   x0=Guarded(c["N"], device="cuda", data=ctx.x0, name="x0", shift=12), y0=Guarded(c["M"], device="cuda", data=ctx.y0, name="y0", shift=4))
        outs = dict(x=Guarded(c["N"], device="cuda", fill=fill, name="x", shift=4), y=Guarded(c["M"], device="cuda", fill=fill, name="y", shift=8),
                    dr=Guarded(c["M"], device="cuda", fill=fill, name="dr", shift=12), dc=Guarded(c["N"], device="cuda", fill=fill, name="dc", shift=8),
                    status=Guarded(4 * K, torch.int32, "cuda", fill=fill, name="status", shift=4),
                    kkt=Guarded(6 * K, device="cuda", fill=fill, name="kkt", shift=4))
        scratch = Guarded(max(ctx.scratch_floats, 1), device="cuda", fill=fill, name="scratch", shift=4)
        assert _call(ctx, ins["x1"], ins["x2"], ins["x0"], ins["y0"], outs, scratch) == 0
        torch.cuda.synchronize()
        for v in list(ins.values()) + list(outs.values()) + [scratch]:
            v.check()
        runs[name] = {k: v.bits() for k, v in outs.items()}
    anchor_pdhg_halpern(ctx)(runs["zero"])
    for name in runs:
        same_bits(runs[name], runs["zero"], f"{variant}: outputs under {name} poison against zero poison")
