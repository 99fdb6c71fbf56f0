"""mllp_optim_step under the stream contract of tests/test_stream_contract.py: its row of the census, and one late-input and
one capture cell per shape (n = 4721: one launch of one workgroup; n = 20481: partials, sliced update, tick).

As tests/test_simplex_stream.py does for mllp_basis_simplex, the row, the Specs and the cells are added to the tables of the
imported module when this file is imported, which is at collection whenever the suite is collected as a whole (test_census
fails if tests/test_stream_contract.py is collected without this file, as it must for an export without a row).

A cell is two steps with weight decay, a clip norm between the two steps' norms, W = 1, T = 3, r = 0.1, info and scratch.
THE ANCHOR is the fp64 oracle of tests/test_optim.py (AdamW + clip_grad_norm_ + LambdaLR) at that file's bars: parameters
and moments within four times the deviation of the same recipe in fp32 torch on the CPU, the norm and the rate of the last
step within the bounds derived there.
"""
import math

import numpy as np
import pytest
import torch

import test_optim as to
import test_stream_contract as sc
import test_topm_loss_stream  # noqa: F401  (its rows and those of the files it imports: the census below is whole)
from mllp_amd import _lib
from mllp_amd.graph import optim_scratch_floats
from test_stream_contract import side  # noqa: F401  (the fixture of the cells)

FN = "mllp_optim_step"
SIZES = {"optim_single": 4721, "optim_wide": 20481}
RULE = dict(wd=0.01, W=1, T=3, r=0.1)
FACTORS = [3.0, 0.3]


def _make_optim(kind):
    def make(case, config):
        n = SIZES[kind]
        seed = n + (0 if case == "-" else 100)
        p0 = np.random.default_rng(seed).standard_normal(n).astype(np.float32)
        second = (lambda ctx: sc.resolve(("own", kind, "b", "-"))) if case == "-" else None
        return sc.Plain(f"{kind} {case}", None, second, n=n, p0=p0, gs=to.make_grads(n, 2, seed + 1, FACTORS))
    return make


def ep_optim(ctx, B):
    """two steps from zero moments, each with its own gradient; step counter and schedule live in d_state"""
    n = ctx.n
    zeros = np.zeros(n, np.float32)
    P, m, v = B.io("params", ctx.p0), B.io("exp_avg", zeros), B.io("exp_avg_sq", zeros)
    st = B.io("state", np.array([0.0, to.LR, to.BETAS[0], to.BETAS[1], RULE["W"], RULE["T"], RULE["r"], 0.0], np.float32))
    info, scratch = B.rw("info", 4), B.rw("scratch", optim_scratch_floats(n))
    for k, g in enumerate(ctx.gs):
        G = B.ro(f"grads{k}", g)
        _lib.check(_lib.lib().mllp_optim_step(P.ptr, G.ptr, m.ptr, v.ptr, st.ptr, to.EPS, 1.0, RULE["wd"], math.sqrt(n), scratch.ptr,
                                              info.ptr, n, sc._s()))
    return {"params": P, "exp_avg": m, "exp_avg_sq": v, "state": st, "info": info}


def anchor_optim(ctx):
    kw = dict(wd=RULE["wd"], max_norm=math.sqrt(ctx.n), W=RULE["W"], T=RULE["T"], r=RULE["r"])
    r64, r32 = to.oracle_run(ctx.p0, ctx.gs, torch.float64, **kw), to.oracle_run(ctx.p0, ctx.gs, torch.float32, **kw)
    assert list(r64["clipped"]) == [True, False]

    def check(out):
        for what, k in (("params", "p"), ("exp_avg", "m"), ("exp_avg_sq", "v")):
            dev, allowed = np.abs(sc.fl(out[what]).astype(np.float64) - r64[k]).max(), 4 * np.abs(r32[k] - r64[k]).max()
            assert dev <= allowed, f"{ctx.case} {what}: {dev:.3e} against {allowed:.3e}"
        state, (norm, c, lr, skipped) = sc.fl(out["state"]), sc.fl(out["info"]).astype(np.float64)
        assert state[0] == 2.0 and skipped == 0.0 and c == 1.0
        assert abs(norm - r64["norm"][1]) <= (0.5 * ((1 + to.U) ** to.norm_path_length(ctx.n) - 1) + to.U) * r64["norm"][1]
        assert abs(lr - r64["lr"][1]) <= to.LR_BOUND_U * to.U * to.LR
    return check


CELLS = [(kind, ("own", kind, "-", "-")) for kind in SIZES]
sc.LAUNCH[FN] = tuple(SIZES)
for _kind in SIZES:
    sc.SPECS[_kind] = sc.Spec(ep_optim, anchor_optim, (FN,))
    sc.OWN_MAKERS[_kind] = _make_optim(_kind)
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
