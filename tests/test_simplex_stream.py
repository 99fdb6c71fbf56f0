"""mllp_basis_simplex under the stream contract of tests/test_stream_contract.py: its rows of the census, and its
late-input and capture cells.

That file's tables are the census of the header's launch functions, and a new launch function needs a row in LAUNCH, a Spec
and a cell of each kind.  They are added HERE, to the tables of the imported module, when this file is imported -- which
is at collection, before any test runs, whenever the suite is collected as a whole (test_census fails if
tests/test_stream_contract.py is collected without this file, as it must for an export without a row).  The cells run from
this file through that file's own test bodies, so the entry point gets exactly what every other launch function gets: a
delayed side stream with inputs that arrive late, and a capture replayed on a second data set.

THE ANCHOR of both data sets is rule-independent (tests/test_simplex.py): code 0 at the planted labels within max_pivots.
"""
import ctypes

import numpy as np
import pytest
import torch

import simplex_oracle as so
import test_stream_contract as sc
from mllp_amd import _lib
from test_stream_contract import side  # noqa: F401  (the fixture of the cells)

MAX_PIVOTS = 200
VARIANTS = {"lds": ([(5, 12), (40, 100)], [2, 6]), "scratch": ([(5, 12), (193, 400)], [2, 4])}


def _starts(c, mats, labels, seed, ks):
    start = np.zeros(c["N"], np.float32)
    for i, k in enumerate(ks):
        s = slice(c["ptr_n"][i], c["ptr_n"][i + 1])
        start[s], _ = so.perturbed_start(mats[i], labels[s], k, seed + i)
    return start


def _make_simplex(variant):
    def make(case, config):
        import test_basis_repair as tb
        from mllp_amd.graph import LPBatch
        shapes, ks = VARIANTS[variant]
        c = tb.planted_shapes(shapes, 40)
        b, mats, st = tb._planted(LPBatch, c)
        n = ctypes.c_int64()
        max_m = max(c["inst_m"])
        _lib.check(_lib.lib().mllp_basis_simplex_scratch_bytes(b._h, max_m, ctypes.byref(n)))
        assert n.value // 4 == sum(c["inst_n"]) + (193 * 193 if variant == "scratch" else 0)
        torch.cuda.synchronize()
        return sc.Plain(f"simplex {variant}", b, _simplex_b, c=c, mats=mats, labels=st["labels"], x1=sc._f32(st["x1"]), x2=sc._f32(st["x2"]),
                        start=_starts(c, mats, st["labels"], 40, ks), ks=ks, max_m=max_m, scratch_floats=n.value // 4, h=b._h)
    return make


def _simplex_b(ctx):
    """other c and b (scaled by positive factors: the planted basis stays the unique optimum) and another start"""
    def make():
        return ctx.with_data(x1=sc._f32(ctx.x1 * 1.5), x2=sc._f32(ctx.x2 * 0.75),
                             start=_starts(ctx.c, ctx.mats, ctx.labels, 50, [k + 1 for k in ctx.ks]))
    return sc._second(ctx, make)


def ep_simplex(ctx, B):
    c, K = ctx.c, len(ctx.c["inst_m"])
    x1, x2, start = B.ro("x1", ctx.x1), B.ro("x2", ctx.x2), B.ro("start", ctx.start)
    o = dict(basis=B.rw("basis", c["N"]), col_of_row=B.rw("col_of_row", c["M"], dtype=torch.int32),
             trace=B.rw("trace", 2 * K * MAX_PIVOTS, dtype=torch.int32), status=B.rw("status", 4 * K, dtype=torch.int32))
    scratch = B.rw("scratch", ctx.scratch_floats)
    _lib.check(_lib.lib().mllp_basis_simplex(ctx.h, x1.ptr, x2.ptr, start.ptr, 2.0 ** -12, 2.0 ** -10, 2.0 ** -10, 2.0 ** -10, 2.0 ** -4,
                                             MAX_PIVOTS, ctx.max_m, o["basis"].ptr, o["col_of_row"].ptr, o["trace"].ptr, o["status"].ptr,
                                             scratch.ptr, sc._s()))
    return o


def anchor_simplex(ctx):
    def check(out):
        c, K = ctx.c, len(ctx.c["inst_m"])
        status, trace = out["status"].reshape(K, 4), out["trace"].reshape(K, MAX_PIVOTS, 2)
        assert np.array_equal(sc.fl(out["basis"]), ctx.labels), ctx.case
        for k, m in enumerate(c["inst_m"]):
            code, nd, np_, rank = status[k]
            assert code == 0 and rank == m and 0 < nd + np_ <= MAX_PIVOTS, (ctx.case, k, status[k])
            assert (trace[k, :nd + np_] >= 0).all() and (trace[k, nd + np_:] == -1).all()
            r, s = slice(c["ptr_m"][k], c["ptr_m"][k + 1]), slice(c["ptr_n"][k], c["ptr_n"][k + 1])
            assert sorted(out["col_of_row"][r]) == sorted(np.flatnonzero(ctx.labels[s]))
    return check


CELLS = [(f"simplex_{v}", ("own", f"simplex_{v}", "-", "-")) for v in VARIANTS]
sc.LAUNCH["mllp_basis_simplex"] = tuple(name for name, _ in CELLS)
for _v in VARIANTS:
    sc.SPECS[f"simplex_{_v}"] = sc.Spec(ep_simplex, anchor_simplex, ("mllp_basis_simplex",), not_finite=("col_of_row", "trace", "status"))
    sc.OWN_MAKERS[f"simplex_{_v}"] = _make_simplex(_v)
# (new lists: the parametrisation of that file's own tests keeps the lists it was given)
sc.LATE_CELLS = sc.LATE_CELLS + CELLS
sc.CAPTURE_CELLS = sc.CAPTURE_CELLS + CELLS


def test_the_census_has_the_row():
    header = open(_lib.HEADER_PATH).read()
    assert "mllp_basis_simplex" in sc.stream_prototypes(header)
    assert sc.census(header) == ([], [])
    sc.test_every_launch_function_has_a_late_cell_and_a_capture_cell()


@pytest.mark.gpu
@pytest.mark.parametrize("cell", CELLS, ids=sc._id)
def test_late_inputs_on_a_delayed_side_stream(cell, side):  # noqa: F811
    sc.test_late_inputs_on_a_delayed_side_stream(cell, side)


@pytest.mark.gpu
@pytest.mark.parametrize("cell", CELLS, ids=sc._id)
def test_capture_then_replay_on_other_inputs(cell):
    sc.test_capture_then_replay_on_other_inputs(cell)
