"""mllp_basis_simplex_guarded under the stream contract of tests/test_stream_contract.py: its row of the census, and one
late-input and one capture cell per instantiation (T in LDS, T in scratch).

As tests/test_simplex_stream.py does for mllp_basis_simplex, the row, the Specs and the cells are added to the tables of the
imported module when this file is imported, which is at collection whenever the suite is collected as a whole
(test_census fails if tests/test_stream_contract.py is collected without this file, as it must for an export without a
row).  The cases, their second data set and THE ANCHOR are that file's: code 0 at the planted labels within max_pivots, which
is rule-independent and so holds with both guards on (R = 2, S = 2: every run here has two pivots or more, so every
instance is refactorized at least once).
"""
import numpy as np
import pytest
import torch

import test_simplex_stream as tss
import test_stream_contract as sc
from mllp_amd import _lib
from test_stream_contract import side  # noqa: F401  (the fixture of the cells)

MAX_PIVOTS = tss.MAX_PIVOTS
R, S = 2, 2
FN = "mllp_basis_simplex_guarded"


def ep_guarded(ctx, B):
    c, K = ctx.c, len(ctx.c["inst_m"])
    x1, x2, start = B.ro("x1", ctx.x1), B.ro("x2", ctx.x2), B.ro("start", ctx.start)
    o = dict(basis=B.rw("basis", c["N"]), col_of_row=B.rw("col_of_row", c["M"], dtype=torch.int32),
             trace=B.rw("trace", 2 * K * MAX_PIVOTS, dtype=torch.int32), status=B.rw("status", 4 * K, dtype=torch.int32),
             guard=B.rw("guard", 2 * K, dtype=torch.int32))
    scratch = B.rw("scratch", ctx.scratch_floats)
    _lib.check(_lib.lib().mllp_basis_simplex_guarded(ctx.h, x1.ptr, x2.ptr, start.ptr, 2.0 ** -12, 2.0 ** -10, 2.0 ** -10, 2.0 ** -10,
                                                     2.0 ** -4, MAX_PIVOTS, ctx.max_m, R, S, o["basis"].ptr, o["col_of_row"].ptr,
                                                     o["trace"].ptr, o["status"].ptr, o["guard"].ptr, scratch.ptr, sc._s()))
    return o


def anchor_guarded(ctx):
    plain = tss.anchor_simplex(ctx)

    def check(out):
        plain(out)
        K = len(ctx.c["inst_m"])
        status, guard = out["status"].reshape(K, 4), out["guard"].reshape(K, 2)
        assert np.array_equal(guard[:, 0], (status[:, 1] + status[:, 2]) // R) and (guard[:, 1] >= 0).all(), (ctx.case, guard)
        assert guard[:, 0].min() > 0, (ctx.case, "an instance was not refactorized")
    return check


CELLS = [(f"simplex_guarded_{v}", ("own", f"simplex_guarded_{v}", "-", "-")) for v in tss.VARIANTS]
sc.LAUNCH[FN] = tuple(name for name, _ in CELLS)
for _v in tss.VARIANTS:
    sc.SPECS[f"simplex_guarded_{_v}"] = sc.Spec(ep_guarded, anchor_guarded, (FN,), not_finite=("col_of_row", "trace", "status", "guard"))
    sc.OWN_MAKERS[f"simplex_guarded_{_v}"] = tss._make_simplex(_v)
# (new lists: the parametrisation of that file's own tests keeps the lists it was given)
sc.LATE_CELLS = sc.LATE_CELLS + CELLS
sc.CAPTURE_CELLS = sc.CAPTURE_CELLS + CELLS


def test_the_census_has_the_row():
    header = open(_lib.HEADER_PATH).read()
    assert FN in sc.stream_prototypes(header)
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
