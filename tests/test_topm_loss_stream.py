"""The soft top-m loss head under the stream contract of tests/test_stream_contract.py: the census rows of mllp_topm_loss,
mllp_topm_loss_math and mllp_gnn_loss_step_topm, their Specs, and one late-input and one capture cell for the head in each
tier (a_i in LDS; a_i formed again from the logits), for the math probe, and for the whole step on both paths.

As tests/test_simplex_guarded_stream.py does, the rows, the Specs and the cells are added to the tables of the imported module
when this file is imported, which is at collection whenever the suite is collected as a whole (test_census fails if
tests/test_stream_contract.py is collected without this file, as it must for an export without a row).  THE ANCHORS: the
head against tests/topm_oracle.py at its derived bounds (tests/test_topm_loss.py::anchor_topm_loss); the step against the fp64
model oracle driven by that head's dz, at the bars of tests/test_memory_contract.py::anchor_weighted; the probe at K_ULP.
"""
import numpy as np
import pytest

import fused_cases as fc
import test_memory_contract as mc
import test_simplex_guarded_stream  # noqa: F401  (its rows and those of tests/test_simplex_stream.py: the census below is whole)
import test_stream_contract as sc
import test_topm_loss as tl
import topm_oracle as to
from mllp_amd import _lib
from test_hip_parity import RTOL_ACT, RTOL_GRAD, close, grad_mask
from test_stream_contract import side  # noqa: F401  (the fixture of the cells)

TAU = 0.5
TIERS = ("lds", "global")


# ---- the head alone, once per tier ------------------------------------------------------------------------------------------
def _shapes(tier):
    lds_max, _ = tl.limits()
    return [(12, 5), (7, 0), (100, 40), (1025, 300)] if tier == "lds" else [(lds_max + 1, lds_max // 2), (3, 3)]


def _make_head(tier):
    def make(case, config):
        c = tl.make_case(_shapes(tier), 31, "other")
        ctx = tl.HeadCtx(f"topm_loss {tier}", c, TAU, tl.S_NOISY, _head_b)
        ctx.tier = tier
        return ctx
    return make


def _head_b(ctx):
    """other logits, weights and ids, labels with sum y = m, on the same graph"""
    def make():
        other = tl.HeadCtx(ctx.case + "+b", tl.make_case(_shapes(ctx.tier), 32, "m"), TAU, tl.S_NOISY, b=ctx.b)
        other.c["ids"] = other.c["ids"] + 3
        return other
    return sc._second(ctx, make)


# ---- the three library functions -------------------------------------------------------------------------------------------
def _math_grids(seed):
    rng = np.random.default_rng(seed)
    n = 4096
    return dict(exp=mc._f32(-rng.random(n) * 40.0), log1p=mc._f32(rng.random(n)), log=mc._f32(rng.random(n) * 4.0 + 2.0 ** -20))


def _make_math(case, config):
    return sc.Plain("topm_loss_math", None, lambda ctx: sc._second(ctx, lambda: ctx.with_data(**_math_grids(2))), **_math_grids(1))


def ep_math(ctx, B):
    out = {}
    for which, name in enumerate(("exp", "log1p", "log")):
        x, out[name] = B.ro("x_" + name, getattr(ctx, name)), B.rw("y_" + name, 4096)
        _lib.check(_lib.lib().mllp_topm_loss_math(which, 4096, x.ptr, out[name].ptr, sc._s()))
    return out


def anchor_math(ctx):
    def check(out):
        for name, f in (("exp", np.exp), ("log1p", np.log1p), ("log", np.log)):
            want = f(getattr(ctx, name).astype(np.float64))
            ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
            assert (np.abs(mc.fl(out[name]).astype(np.float64) - want) <= to.K_ULP * ulp).all(), name
    return check


# ---- the whole step --------------------------------------------------------------------------------------------------------
def ep_loss_step_topm(ctx, B):
    m = mc._model(ctx, B)
    y, z, ls, g = mc._loss_outputs(ctx, B)
    iw, pw, il, dz = B.ro("inst_weight", ctx.iw), B.ro("pos_weight", ctx.pw), B.rw("inst_loss", ctx.K), B.rw("dlogits", ctx.N)
    _lib.check(_lib.lib().mllp_gnn_loss_step_topm(ctx.h, m.P.ptr, m.x1.ptr, m.x2.ptr, y.ptr, iw.ptr, pw.ptr, None, TAU, 0.0, 0, 0,
                                                  m.ws.ptr, z.ptr, ls.ptr, il.ptr, g.ptr, dz.ptr, sc._s()))
    return {"logits": z, "loss": ls, "inst_loss": il, "grads": g, "dlogits": dz}


_STEP_REF = {}


def anchor_step_topm(ctx):
    """the fp64 model oracle's logits through the fp64 head, its dz back through the model oracle; the bars of
    tests/test_memory_contract.py::anchor_weighted"""
    r = mc.refs(ctx.case)
    if ctx.case not in _STEP_REF:
        res, loss, _, off = to.batch(r.step["logits"], np.asarray(r.ob.basis, np.float64), r.seg_n, r.seg_m, TAU, iw=ctx.iw, pw=ctx.pw)
        dz = np.concatenate([x["dz"] for x in res])
        _STEP_REF[ctx.case] = dict(loss=loss, inst_loss=np.array([x["L"] for x in res]), dz=dz,
                                   grads=fc.model_dt(r.sd, r.ob, np.float64, dlogits=dz)["grads"])
    ref = _STEP_REF[ctx.case]

    def check(out):
        keep = grad_mask()
        close(mc.fl(out["logits"]), r.step["logits"], RTOL_ACT, "logits")
        close(mc.fl(out["loss"]), np.array([ref["loss"]]), RTOL_ACT, "loss")
        close(mc.fl(out["inst_loss"]), ref["inst_loss"], RTOL_ACT, "inst_loss")
        close(mc.fl(out["dlogits"]), ref["dz"], 1e-5, "dlogits")
        close(mc.fl(out["grads"])[keep], ref["grads"][keep], RTOL_GRAD, "grads")
    return check


# ---- the tables ------------------------------------------------------------------------------------------------------------
HEAD_CELLS = [(f"topm_loss_{t}", ("own", f"topm_loss_{t}", "-", "-")) for t in TIERS]
MATH_CELLS = [("topm_loss_math", ("own", "topm_loss_math", "-", "-"))]
STEP_CELLS = [("loss_step_topm", ("model", "holes", config)) for config in ("fused", "generic")]
CELLS = HEAD_CELLS + MATH_CELLS + STEP_CELLS

sc.LAUNCH["mllp_topm_loss"] = tuple(name for name, _ in HEAD_CELLS)
sc.LAUNCH["mllp_topm_loss_math"] = ("topm_loss_math",)
sc.LAUNCH["mllp_gnn_loss_step_topm"] = ("loss_step_topm",)
for _t in TIERS:
    sc.SPECS[f"topm_loss_{_t}"] = sc.Spec(tl.ep_topm_loss, tl.anchor_topm_loss, ("mllp_topm_loss",))
    sc.OWN_MAKERS[f"topm_loss_{_t}"] = _make_head(_t)
sc.SPECS["topm_loss_math"] = sc.Spec(ep_math, anchor_math, ("mllp_topm_loss_math",))
sc.OWN_MAKERS["topm_loss_math"] = _make_math
sc.SPECS["loss_step_topm"] = sc.Spec(ep_loss_step_topm, anchor_step_topm, ("mllp_gnn_loss_step_topm",))
# (new lists: the parametrisation of that file's own tests keeps the lists it was given)
sc.LATE_CELLS = sc.LATE_CELLS + CELLS
sc.CAPTURE_CELLS = sc.CAPTURE_CELLS + CELLS


def test_the_census_has_the_rows():
    header = open(_lib.HEADER_PATH).read()
    names = sc.stream_prototypes(header)
    assert all(fn in names for fn in ("mllp_topm_loss", "mllp_topm_loss_math", "mllp_gnn_loss_step_topm"))
    assert "mllp_topm_loss_limits" not in names
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
