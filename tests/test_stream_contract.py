"""The stream contract of the C ABI (include/mllp_hip.h, "Conventions"), launch function by launch function:

  - every launch is asynchronous on the hipStream_t passed as `stream`;
  - no entry point synchronises (except the setup calls the header names);
  - all launch functions are hipGraph-capturable (no malloc / free / sync inside);
  - calls made while the stream is captured re-make the fused path's copies of the inputs inside the capture.

CENSUS (CPU).  Every prototype of the header with a `void* stream` parameter is either a row of LAUNCH (with the entry
points that run it) or a row of SETUP (with the header's sentence that lets it allocate or synchronise): a new export
without a row fails `test_census`, and every launch function must appear in a late-input cell and in a capture cell.

LATE INPUTS (GPU).  A cell is one entry point on one case and configuration.  The anchor runs on the default stream with
zero-filled buffers and is checked against the fp64 oracle of the test file that owns the entry point (bars imported or
cited, none introduced).  Then a non-blocking side stream S gets a delay (torch.cuda._sleep, one workgroup), and the entry
point runs on S through `LateBufs`: every buffer was created NaN-filled on the default stream, and BEHIND THE DELAY ON S the
inputs receive their bytes by a device-to-device copy and the outputs and workspaces are NaN-filled once more.  When the
entry point returns S must still be busy (so every call was queued while its inputs were NaN, and none synchronised); after
S.synchronize() every guard is intact, every read-only input unchanged and every output equals the anchor BIT FOR BIT.
Whatever the library had queued on another stream, or on its own second stream without an event from S, ran during the
delay on NaN inputs or had its result wiped by the late NaN fill.

CAPTURE (GPU).  The entry point runs eagerly on two data sets A and B (B: parameters x 1.25, other x1 / x2 / dlogits,
complemented labels; both checked against the oracle), is captured with torch.cuda.graph (default error mode: an allocation
or a synchronisation fails the capture) on buffers that hold A, through a `Bufs` that hands back existing buffers; then
the inputs are rewritten in place with B, the outputs NaN-filled, and two replays must each give the eager bits of B.

REPLAY BETWEEN EAGER CALLS (GPU, fused path).  eager X, capture on other buffers Y, eager X, replay Y, eager X: the eager
results are the same bits each time.  On the commit before this file the last one was computed on Y's inputs (the replay
rewrote the graph's renumbered copies behind the pointer cache); fused_bind now stops trusting the cache after a capture.

The side stream: torch.cuda.Stream(), hipStreamGetFlags = 1 (hipStreamNonBlocking), asserted in the `side` fixture.
The delay: HOST_MS_MEASURED below is the longest host time of an entry point on S, buffer staging included, on one MI355X:
3.56 ms (mllp_tconv_fwd + _bwd with 16 channels on grid: thirteen guarded buffers staged); the next are the same cell in the
other configurations (3.5 ms) and tconv with one channel on grid (1.7 ms); every whole-model call stays below 1.7 ms.  (The
fixture prints every cell's time at the end of the module.)  DELAY_MS = max(50, 4 x 3.56) = 50 ms, the floor; asserted
<= 500; _sleep is calibrated with events (2.40 M cycles per ms measured) and the calibrated sleep is timed once, so that a
miscalibration cannot pass for a hang.

FOUND.  (1) test_replay_between_eager_calls fails on the commit before this file (the last eager call computes on Y's inputs;
logits, loss and gradients all differ); fixed in fused_bind.  (2) The capture cells of mllp_angle_backward / _backward_inputs:
the zeros of the never-called gconv3 block were a hipMemsetAsync, and at replay the block came back holding the NaN the test
had just written on the launch stream (every replay at F = 256, the second replay at N = 257, F = 16): the memset node ran
ahead of the work queued in front of the graph.  angle.hip now writes those zeros with a launch of its own.  Nothing else:
no launch on stream 0, no missing fork, no hidden synchronisation in any cell.
"""
import copy
import ctypes
import dataclasses
import re
import time
import types

import numpy as np
import pytest
import torch

import fused_cases as fc
import test_memory_contract as mc
from guarded import NAN, Guarded, _bytes_of, same_bits
from mllp_amd import _lib
from oracle import spmm_form as o2
from test_hip_parity import RTOL_ACT, close
from test_memory_contract import CONFIGS, MODEL_EPS, Bufs, _f32, fl, get_ctx, refs

gpu = pytest.mark.gpu

# longest host time of one entry point on the side stream, staging included, and where (measured on one MI355X)
HOST_MS_MEASURED = (3.56, "tconv_cin16 on grid (stream_padded); the whole-model calls on grid stay below 1.7 ms, on holes below 1.4 ms")
DELAY_MS = max(50.0, 4.0 * HOST_MS_MEASURED[0])
DELAY_CEILING_MS = 500.0


# ---------------------------------------------------------------------------------------------------------------------
# 1. census
# ---------------------------------------------------------------------------------------------------------------------
SETUP = {   # function -> the header's sentence that allows it to allocate or synchronise
    "mllp_csr_transpose_device": "Allocates scratch and synchronises `stream` (not a launch function)",
    "mllp_graph_create_device": "no entry point synchronises except mllp_graph_create_* / mllp_graph_export",
    "mllp_graph_build_spmm_copy": "these three are not launch functions: they allocate, free and synchronise",
    "mllp_graph_build_stream_copy": "The four functions above are these with geom = 0",
    "mllp_graph_build_tiled": "not a launch function: allocates and synchronises `stream`",
    "mllp_graph_export_tiled": "mllp_graph_export_tiled (tests; a setup call beside mllp_graph_build_tiled, not a launch function)",
    "mllp_graph_plant_basis": "A SETUP call, not a launch function",
}
LAUNCH = {  # function -> the entry points (SPECS) that run it
    "mllp_graph_set_values": ("set_scale", "normalize"),
    "mllp_graph_scale_values": ("set_scale",),
    "mllp_graph_normalize": ("normalize",),
    "mllp_lp_certificate": ("certificate",),
    "mllp_basis_repair": ("repair_lds", "repair_scratch"),
    "mllp_spmm_csr_f32": ("spmm_0", "spmm_1"),
    "mllp_spmm_csr_bf16": ("spmm_bf16_0", "spmm_bf16_1"),
    "mllp_tconv_fwd": ("tconv_cin1", "tconv_cin16"),
    "mllp_tconv_bwd": ("tconv_cin1", "tconv_cin16"),
    "mllp_gnn_forward": ("forward", "forward_backward", "input_grads"),
    "mllp_gnn_backward": ("forward_backward",),
    "mllp_gnn_loss_step": ("loss_step",),
    "mllp_gnn_backward_inputs": ("backward_inputs",),
    "mllp_gnn_input_grads": ("input_grads",),
    "mllp_gnn_loss_step_inputs": ("loss_step_inputs",),
    "mllp_weighted_loss": ("weighted_loss",),
    "mllp_balanced_pos_weight": ("weighted_loss",),
    "mllp_gnn_loss_step_weighted": ("loss_step_weighted",),
    "mllp_adam_step": ("adam",),
    "mllp_gnn_train_step": ("train_step",),
    "mllp_gnn_train_step_small": ("small_loss", "small_adam"),
    "mllp_topm_metrics": ("topm",),
    "mllp_topm_select": ("topm",),
    "mllp_topm_select_dense": ("topm_dense",),
    "mllp_angle_forward": ("angle_forward", "angle_backward", "angle_backward_inputs"),
    "mllp_angle_backward": ("angle_backward",),
    "mllp_angle_backward_inputs": ("angle_backward_inputs",),
}


def stream_prototypes(header_text):
    """names of the prototypes that take a `void* stream`, in the header's order"""
    text = re.sub(r"/\*.*?\*/", " ", header_text, flags=re.S)
    return [m.group(1) for m in re.finditer(r"\bint\s+(mllp_\w+)\s*\(([^;{}]*)\)\s*;", text) if re.search(r"void\s*\*\s*stream\b", m.group(2))]


def census(header_text):
    """the rows that are missing and the rows that name no prototype (both empty: the tables and the header agree)"""
    names = stream_prototypes(header_text)
    assert len(names) == len(set(names))
    assert not set(SETUP) & set(LAUNCH)
    known = set(SETUP) | set(LAUNCH)
    return [n for n in names if n not in known], sorted(known - set(names))


def _flat_text(header_text):
    return " ".join(re.sub(r"\n\s*\*\s", " ", header_text).split())


def test_census():
    header = open(_lib.HEADER_PATH).read()
    missing, stale = census(header)
    assert not missing, f"prototypes with a `void* stream` and no row in LAUNCH or SETUP: {missing}"
    assert not stale, f"rows that name no prototype of the header: {stale}"
    text = _flat_text(header)
    for name, sentence in SETUP.items():
        assert sentence in text, f"{name}: the header no longer says: {sentence}"
    print(f"{len(LAUNCH)} launch functions, {len(SETUP)} setup functions")
    for conv in ("every launch is asynchronous on the hipStream_t passed as `stream`", "no entry point synchronises except",
                 "all launch functions are hipGraph-capturable (no malloc/free/sync inside)",
                 "calls on ONE graph must be stream-ordered",
                 "re-make the copies inside the capture and leave the cache empty"):
        assert conv in text, conv
    # a new export with a stream and without a row is found
    grown = header.replace("#ifdef __cplusplus\n}", "int mllp_new_thing(const mllp_graph_t* g, float* d_out,\n        void* stream);\n#ifdef __cplusplus\n}")
    assert census(grown)[0] == ["mllp_new_thing"]


def test_every_launch_function_has_a_late_cell_and_a_capture_cell():
    late = {c[0] for c in LATE_CELLS}
    cap = {c[0] for c in CAPTURE_CELLS}
    for fn, eps in LAUNCH.items():
        assert all(e in SPECS for e in eps), fn
        for e in eps:
            assert fn in SPECS[e].covers, (fn, e)
        assert late & set(eps), f"{fn}: no late-input cell"
        assert cap & set(eps), f"{fn}: no capture cell"
    for name, s in SPECS.items():
        for fn in s.covers:
            assert name in LAUNCH[fn], (name, fn)


# ---------------------------------------------------------------------------------------------------------------------
# buffers: late, handed back, refilled
# ---------------------------------------------------------------------------------------------------------------------
class LateBufs(Bufs):
    """every buffer NaN-filled on the default stream (synchronised); its data, or NaN once more, arrives on the CURRENT
    stream -- the delayed side stream -- by device-to-device copy from a staging tensor (kept alive here until the end)"""

    def __init__(self, side):
        super().__init__("nan")
        self.side, self.staged = side, []

    def _make(self, name, n, dtype, wide, data=None, fill=None, leavings=None):
        assert name not in self.all and torch.cuda.current_stream() == self.side
        dflt = torch.cuda.default_stream()
        with torch.cuda.stream(dflt):
            g = Guarded(max(int(n), 1), dtype, "cuda", fill=NAN, guard_fill=NAN, name=name)
            src = None if data is None else _bytes_of(np.asarray(data)).to("cuda")
            dflt.synchronize()
        if src is None:
            g.refill(fill=NAN)
        else:
            self.staged.append(src)
            g.refill(data=src)
        self.all[name] = g
        return g


class ReuseBufs(Bufs):
    """hands back the buffers another run made, by name: nothing is allocated and no device work is queued (poison_rw:
    outputs and scratch are NaN-filled again, on the current stream)"""

    def __init__(self, made, poison_rw=False):
        super().__init__("nan")
        self.made, self.poison_rw = made.all, poison_rw

    def _make(self, name, n, dtype, wide, data=None, fill=None, leavings=None):
        g = self.made[name]
        assert name not in self.all and g.n == max(int(n), 1) and g.dtype == dtype
        if data is None and self.poison_rw:
            g.refill(fill=NAN)
        self.all[name] = g
        return g

    def io(self, name, data, wide=False):
        g = self._make(name, np.asarray(data).size, torch.float32, wide, data=np.asarray(data))
        if self.poison_rw:
            g.refill(data=np.asarray(data))
            g.data = None
        return g


class RefillBufs(Bufs):
    """rewrites existing buffers in place with another data set (read-only inputs and in/out buffers get its data, outputs
    and scratch NaN) and remembers which is which, so that `again()` restores that state before the next replay"""

    def __init__(self, made):
        super().__init__("nan")
        self.made, self.data_of, self.in_out = made.all, {}, set()

    def _make(self, name, n, dtype, wide, data=None, fill=None, leavings=None):
        g = self.made[name]
        assert name not in self.all and g.n == max(int(n), 1) and g.dtype == dtype
        if data is None:
            g.refill(fill=NAN)
        else:
            self.data_of[name] = np.array(data, copy=True)
            g.refill(data=self.data_of[name])
        self.all[name] = g
        return g

    def io(self, name, data, wide=False):
        g = self.ro(name, data, wide)
        g.data = None
        self.in_out.add(name)
        return g

    def again(self):
        for name, g in self.all.items():
            if name not in self.data_of:
                g.refill(fill=NAN)
            elif name in self.in_out:
                g.refill(data=self.data_of[name])
                g.data = None


def finish(outs):
    """Guarded -> its bits; a callable (an export that synchronises) is called now"""
    return {k: (g.bits() if isinstance(g, Guarded) else g() if callable(g) else g) for k, g in outs.items()}


def eager(ctx, ep, B=None):
    B = B or Bufs("zero")
    ctx.b.invalidate_inputs()
    outs = ep(ctx, B)
    B.check()
    return finish(outs), B


# ---------------------------------------------------------------------------------------------------------------------
# the second data set of a context
# ---------------------------------------------------------------------------------------------------------------------
def _inst_b(inst, k):
    rng = np.random.default_rng(900 + k)
    pert = lambda a: a * (1.0 + 0.25 * rng.uniform(-1.0, 1.0, a.shape)) + 0.05 * rng.standard_normal(a.shape)  # noqa: E731
    return dataclasses.replace(inst, coefs=pert(np.asarray(inst.coefs, np.float64)), rhs=pert(np.asarray(inst.rhs, np.float64)),
                               basis=1 - np.asarray(inst.basis))


def _case_b(case):
    name = case + "+b"
    if name not in mc._CASES:
        mc._CASES[name] = [_inst_b(i, k) for k, i in enumerate(mc.case_instances(case))]
    return name


def _model_b(ctx):
    """a shallow copy on the SAME graph: parameters x 1.25, x1 / x2 / dlogits perturbed, labels complemented"""
    name = _case_b(ctx.case)
    key = (name, ctx.config, id(ctx))
    if key not in _B:
        if (name, "generic") not in mc._CTX:                      # refs(name) takes dz, inst_weight, pos_weight from it
            g = get_ctx(ctx.case, "generic")
            mc._CTX[(name, "generic")] = _fill_b(copy.copy(g), name)
        _B[key] = _fill_b(copy.copy(ctx), name)
    return _B[key]


def _fill_b(c, name):
    c.case, c.insts, c.data_seed = name, mc._CASES[name], 7
    c.flat = _f32(mc.case_flat(name))
    c.x1, c.x2, c.y = (_f32(np.concatenate([getattr(i, f) for i in c.insts])) for f in ("coefs", "rhs", "basis"))
    c.dz = mc._functional(c.N, seed=43)
    return c


_B, _OWN, _ANCHOR = {}, {}, {}


def ctx_b(ctx):
    return (getattr(ctx, "second", None) or _model_b)(ctx)


def test_the_second_data_set_exempts_no_tensor_either():
    """the per-tensor cap of tests/test_memory_contract.py (0) holds for the second data set of both cases (CPU)"""
    import grad_scales as gs
    for case in ("holes", "grid", "golden"):
        name = _case_b(case)
        insts = mc._CASES[name]
        sd = fc.golden_state({"weights_flat": mc.case_flat(name)})
        ob = o2.BatchCSR(insts)
        assert (ob.basis == 1 - o2.BatchCSR(mc.case_instances(case)).basis).all()
        for dz in (None, mc._functional(ob.N, seed=43)):
            assert len(gs.exempt_tensors(gs.yardstick(sd, ob, dlogits=dz))) <= mc.PER_TENSOR_CAP, name


# ---------------------------------------------------------------------------------------------------------------------
# 2. entry points the memory-contract file does not have (each: (ctx, B) -> outputs; no read-back, no synchronisation)
# ---------------------------------------------------------------------------------------------------------------------
def _s():
    return _lib.current_stream()


def ep_input_grads_late(ctx, B):
    """mc.ep_input_grads without its read-back: the parameter gradients are the head of the scratch buffer"""
    m, z, dz = mc._model(ctx, B), B.rw("logits", ctx.N), B.ro("dlogits", ctx.dz)
    dx1, dx2, dv = mc._input_grad_outputs(ctx, B)
    L, n = _lib.lib(), ctypes.c_int64()
    _lib.check(L.mllp_gnn_input_grads_scratch_bytes(ctx.h, ctypes.byref(n)))
    sc = B.rw("scratch", n.value // 4)
    _lib.check(L.mllp_gnn_forward(ctx.h, m.P.ptr, m.x1.ptr, m.x2.ptr, m.ws.ptr, z.ptr, _s()))
    _lib.check(L.mllp_gnn_input_grads(ctx.h, m.P.ptr, m.x1.ptr, m.x2.ptr, m.ws.ptr, dz.ptr, None, dx1.ptr, dx2.ptr, dv.ptr,
                                      sc.ptr, _s()))
    return {"logits": z, "grads": lambda: sc.bits()[:_lib.NUM_PARAMS], "dx1": dx1, "dx2": dx2, "dvalues": dv}


def ep_backward_inputs(ctx, B):
    """mllp_gnn_backward_inputs itself (generic path only), with a gradient buffer"""
    m, z, dz, g = mc._model(ctx, B), B.rw("logits", ctx.N), B.ro("dlogits", ctx.dz), B.rw("grads", _lib.NUM_PARAMS)
    dx1, dx2, dv = mc._input_grad_outputs(ctx, B)
    L = _lib.lib()
    _lib.check(L.mllp_gnn_forward(ctx.h, m.P.ptr, m.x1.ptr, m.x2.ptr, m.ws.ptr, z.ptr, _s()))
    _lib.check(L.mllp_gnn_backward_inputs(ctx.h, m.P.ptr, m.x1.ptr, m.x2.ptr, m.ws.ptr, dz.ptr, g.ptr, dx1.ptr, dx2.ptr, dv.ptr,
                                          None, _s()))
    return {"logits": z, "grads": g, "dx1": dx1, "dx2": dx2, "dvalues": dv}


def ep_train_step_late(ctx, B):
    """mc.ep_train_step (flags 0, then flags 1) without the read between its steps"""
    m = mc._model(ctx, B, params="io")
    y, z, ls, g = mc._loss_outputs(ctx, B)
    ea, es, st = mc._adam(ctx, B)
    for flags in (0, 1):
        _lib.check(_lib.lib().mllp_gnn_train_step(ctx.h, m.P.ptr, m.x1.ptr, m.x2.ptr, y.ptr, 1.0 / ctx.K, m.ws.ptr, z.ptr, ls.ptr,
                                                  g.ptr, ea.ptr, es.ptr, st.ptr, 1e-8, flags, _s()))
    return dict(params=m.P, exp_avg=ea, exp_avg_sq=es, state=st, logits=z, loss=ls, grads=g)


def _tconv_late(which):
    def ep(ctx, B):
        name, dst_is_var, cin, nd, ns, xs, xd, dh = mc._tconv_inputs(ctx, which)
        L, n = _lib.lib(), ctypes.c_int64()
        _lib.check(L.mllp_tconv_workspace_floats(ctx.h, int(dst_is_var), cin, ctypes.byref(n)))
        cp = B.ro("conv_params", ctx.flat[_lib.conv_param_slice(name)], wide=True)
        x_src, x_dst = B.ro("x_src", xs, wide=True), B.ro("x_dst", xd, wide=True)
        ws, h = B.rw("ws", n.value, wide=True), B.rw("h", nd * 16, wide=True)
        d, pg = B.io("dh", dh, wide=True), B.rw("param_grads", cp.n)
        out = {"h": h, "dh": d, "param_grads": pg}
        dxd = dxs = None
        if cin == 16:
            dxd, dxs = B.rw("dx_dst", nd * 16, wide=True), B.rw("dx_src", ns * 16, wide=True)
            out.update(dx_dst=dxd, dx_src=dxs)
        _lib.check(L.mllp_tconv_fwd(ctx.h, int(dst_is_var), cin, cp.ptr, x_src.ptr, x_dst.ptr, h.ptr, ws.ptr, _s()))
        _lib.check(L.mllp_tconv_bwd(ctx.h, int(dst_is_var), cin, cp.ptr, x_src.ptr, x_dst.ptr, h.ptr, ws.ptr, d.ptr,
                                    dxd.ptr if dxd else None, dxs.ptr if dxs else None, 0, pg.ptr, _s()))
        return out
    ep.__name__ = f"ep_tconv_{which}_late"
    return ep


# ---- batches of their own (the call rewrites the batch, or needs a copy the shared contexts do not attach) ------------------
def _second(ctx, make):
    if getattr(ctx, "second_ctx", None) is None:
        ctx.second_ctx = make()
    return ctx.second_ctx


def _rows_of(ctx):
    return np.repeat(np.arange(ctx.M), np.diff(ctx.b.export(0).astype(np.int64)))


def _make_set_scale(case, config):
    import test_set_values as ts
    c = mc.Ctx(case, config, mc.case_flat(case))
    assert c.skip is None
    c.v0 = ts._values(c.insts)
    rng = np.random.default_rng(21)
    c.v_new, c.rs, c.cs = ts._new_values(c.v0, 31), _f32(0.5 + 1.5 * rng.random(c.M)), _f32(0.5 + 1.5 * rng.random(c.N))
    c.second = _set_scale_b
    return c


def _set_scale_b(ctx):
    import test_set_values as ts

    def make():
        c = _fill_b(copy.copy(ctx), _case_b(ctx.case))
        rng = np.random.default_rng(22)
        c.v_new, c.rs, c.cs = ts._new_values(c.v0, 32), _f32(0.5 + 1.5 * rng.random(c.M)), _f32(0.5 + 1.5 * rng.random(c.N))
        return c
    return _second(ctx, make)


def ep_set_scale(ctx, B):
    """mllp_graph_set_values, a forward; mllp_graph_scale_values, a forward; then the plain arrays (exported afterwards)"""
    v, rs, cs = B.ro("values", ctx.v_new), B.ro("row_scale", ctx.rs), B.ro("col_scale", ctx.cs)
    m, z1, z2 = mc._model(ctx, B), B.rw("logits_set", ctx.N), B.rw("logits", ctx.N)
    L = _lib.lib()
    _lib.check(L.mllp_graph_set_values(ctx.h, v.ptr, _s()))
    _lib.check(L.mllp_gnn_forward(ctx.h, m.P.ptr, m.x1.ptr, m.x2.ptr, m.ws.ptr, z1.ptr, _s()))
    _lib.check(L.mllp_graph_scale_values(ctx.h, rs.ptr, cs.ptr, _s()))
    _lib.check(L.mllp_gnn_forward(ctx.h, m.P.ptr, m.x1.ptr, m.x2.ptr, m.ws.ptr, z2.ptr, _s()))
    return {"logits_set": z1, "logits": z2, "csr_values": lambda: ctx.b.export(2).view(np.int32),
            "csc_values": lambda: ctx.b.export(5).view(np.int32)}


def anchor_set_scale(ctx):
    """values: exact (tests/test_set_values.py: byte for byte (r a) s in fp32, the transposed orientation a permutation); the
    forwards: the fp64 oracle on instances that hold those values, at the bar of tests/test_hip_parity.py (RTOL_ACT)"""
    import test_set_values as ts
    sd = fc.golden_state({"weights_flat": ctx.flat})
    rows, idx = _rows_of(ctx), ctx.b.export(1).astype(np.int64)
    scaled = (ctx.rs[rows] * ctx.v_new) * ctx.cs[idx]
    assert scaled.dtype == np.float32
    want = [o2.gnn_forward_backward(sd, o2.BatchCSR(ts._with_values(ctx.insts, v)))["logits"] for v in (ctx.v_new, scaled)]

    def check(out):
        ts._same(fl(out["csr_values"]), scaled, "CSR(A) values after set + scale")
        ts._same(fl(out["csc_values"]), scaled[np.lexsort((rows, idx))], "CSR(A^T) values after set + scale")
        close(fl(out["logits_set"]), want[0], RTOL_ACT, "forward after set_values")
        close(fl(out["logits"]), want[1], RTOL_ACT, "forward after scale_values")
    return check


def _make_normalize(case, config):
    import test_normalize as tn
    pert, _ = tn._perturbed_list(mc.case_instances(case))
    assert not any(tn._knife_edge(p).any() for p in pert)
    name = case + "~normalize"
    mc._CASES[name] = pert
    c = mc.Ctx(name, config, mc.case_flat(case))
    c.v0 = np.concatenate([p.values for p in pert]).astype(np.float32)
    c.second = _normalize_b
    return c


def _normalize_b(ctx):
    import test_normalize as tn

    def make():
        pert, _ = tn._perturbed_list(mc.case_instances(ctx.case.split("~")[0]), seed=101)
        assert not any(tn._knife_edge(p).any() for p in pert)
        c = copy.copy(ctx)
        c.insts = pert
        c.v0 = np.concatenate([p.values for p in pert]).astype(np.float32)
        c.x1, c.x2 = (_f32(np.concatenate([getattr(p, f) for p in pert])) for f in ("coefs", "rhs"))
        return c
    return _second(ctx, make)


def ep_normalize_own(ctx, B):
    """the batch's values put back by mllp_graph_set_values (a launch function too), then mllp_graph_normalize: x1, x2 in
    place and both scale outputs"""
    v, x1, x2 = B.ro("values", ctx.v0), B.io("x1", ctx.x1), B.io("x2", ctx.x2)
    rs, os_ = B.rw("row_scale", ctx.M), B.rw("obj_scale", ctx.K)
    L = _lib.lib()
    _lib.check(L.mllp_graph_set_values(ctx.h, v.ptr, _s()))
    _lib.check(L.mllp_graph_normalize(ctx.h, x1.ptr, x2.ptr, 5.0, 0, rs.ptr, os_.ptr, _s()))
    return {"x1": x1, "x2": x2, "row_scale": rs, "obj_scale": os_, "values": lambda: ctx.b.export(2).view(np.int32)}


def anchor_normalize(ctx):
    """tests/test_normalize.py's fp64 statement of the rule at its bar, as tests/test_memory_contract.py::test_normalize"""
    import test_normalize as tn
    want = [np.concatenate([np.atleast_1d(tn._normalize_host(p, np.float64)[k]) for p in ctx.insts]) for k in range(5)]

    def check(out):
        for k, name in enumerate(("values", "x1", "x2", "row_scale", "obj_scale")):
            tn._close(fl(out[name]), want[k], f"{ctx.case} {name}")
    return check


def ep_certificate(ctx, B):
    rng = np.random.default_rng(61 + getattr(ctx, "data_seed", 0))
    x1, x2, basis = B.ro("x1", ctx.x1), B.ro("x2", ctx.x2), B.ro("basis", ctx.y)
    x, y = B.ro("x", _f32(rng.standard_normal(ctx.N) * (0.25 + ctx.y))), B.ro("y", _f32(rng.standard_normal(ctx.M)))
    L, n = _lib.lib(), ctypes.c_int64()
    _lib.check(L.mllp_lp_certificate_scratch_bytes(ctx.h, ctypes.byref(n)))
    sc, cert = B.rw("scratch", (n.value + 3) // 4), B.rw("cert", 6 * ctx.K)
    _lib.check(L.mllp_lp_certificate(ctx.h, x1.ptr, x2.ptr, x.ptr, y.ptr, basis.ptr, cert.ptr, sc.ptr, _s()))
    return {"cert": cert}


def anchor_certificate(ctx):
    """tests/test_planted.py::test_certificate_matches_the_oracle: planted_oracle.certificate and its bounds"""
    import planted_oracle as po
    from test_planted import _within
    rng = np.random.default_rng(61 + getattr(ctx, "data_seed", 0))
    x, y = _f32(rng.standard_normal(ctx.N) * (0.25 + ctx.y)), _f32(rng.standard_normal(ctx.M))
    ptr_m, ptr_n = (np.concatenate([[0], np.cumsum([getattr(i, f) for i in ctx.insts])]) for f in ("m", "n"))
    want, bound = po.certificate(ctx.b.export(0), ctx.b.export(1), ctx.b.export(2), ctx.x1, ctx.x2, x, y, ctx.y, ptr_m, ptr_n)

    def check(out):
        got = fl(out["cert"]).reshape(ctx.K, 6)
        fin = np.isfinite(want)
        assert np.array_equal(np.isinf(got), ~fin) and (got[~fin] > 0).all()
        _within(got[fin], want[fin], bound[fin], "certificate")
        assert list(got[:, 5]) == [float(ctx.y[ptr_n[k]:ptr_n[k + 1]].sum()) for k in range(ctx.K)]
    return check


class Plain:
    """a context without a whole-model batch: named data and, where there is one, the batch the calls run on"""
    config = "-"

    def __init__(self, case, b=None, second=None, **data):
        self.case, self.b, self.second = case, b or types.SimpleNamespace(invalidate_inputs=lambda: None), second
        self.__dict__.update(data)

    def with_data(self, **changed):
        """the second data set: the same context with some of its data replaced"""
        keep = {k: v for k, v in self.__dict__.items() if k not in ("case", "b", "second", "second_ctx")}
        return Plain(self.case + "+b", self.b, None, **{**keep, **changed})


def _make_repair(variant):
    def make(case, config):
        import test_basis_repair as tb
        from mllp_amd.graph import LPBatch
        if variant == "lds":                                       # every instance keeps its transform in LDS
            c = tb.dense_case(tb.repair_mats(), 1)
            b = tb._build(LPBatch, c, tb._dev(c["c"]), tb._dev(c["b"]))
            order, x1, x2, mats, st = tb.natural_order(c), c["c"], c["b"], c["mats"], None
        else:                                                       # m = threshold + 1: the transform in the caller's scratch
            c = tb.planted_shapes([(5, 12), (tb.LDS_MAX, 2 * tb.LDS_MAX + 16), (tb.LDS_MAX + 1, 2 * tb.LDS_MAX + 16)], 40)
            b, mats, st = tb._planted(LPBatch, c)
            order, x1, x2 = tb._labels_first(c, st["labels"]), st["x1"], st["x2"]
        n = ctypes.c_int64()
        max_m = max(c["inst_m"])
        _lib.check(_lib.lib().mllp_basis_repair_scratch_bytes(b._h, max_m, ctypes.byref(n)))
        assert (n.value > 0) == (variant == "scratch")
        torch.cuda.synchronize()
        return Plain(f"repair {variant}", b, _repair_b, c=c, variant=variant, order=order.astype(np.int32), x1=_f32(x1), x2=_f32(x2),
                     mats=mats, st=st, max_m=max_m, scratch_floats=n.value // 4, h=b._h)
    return make


def _repair_b(ctx):
    """other c and b (scaled by positive factors: what the planted checks need stays true) and another ranking: every
    instance's list reversed inside its basic and inside its nonbasic part (planted), or reversed behind the three injected
    columns (dense)"""
    def make():
        c, order = ctx.c, ctx.order.copy()
        x1, x2 = _f32(ctx.x1 * 1.5), _f32(ctx.x2 * 0.75)
        for k in range(len(c["inst_n"])):
            s, m = slice(c["ptr_n"][k], c["ptr_n"][k + 1]), c["inst_m"][k]
            seg = order[s].copy()
            order[s] = np.concatenate([seg[:m][::-1], seg[m:][::-1]] if ctx.variant == "scratch" else [seg[:3], seg[3:][::-1]])
        return ctx.with_data(order=order, x1=x1, x2=x2, st=None if ctx.st is None else dict(ctx.st, x1=x1, x2=x2))
    return _second(ctx, make)


def ep_repair(ctx, B):
    c, K = ctx.c, len(ctx.c["inst_m"])
    x1, x2, order = B.ro("x1", ctx.x1), B.ro("x2", ctx.x2), B.ro("order", ctx.order, dtype=torch.int32)
    o = dict(basis=B.rw("basis", c["N"]), col_of_row=B.rw("col_of_row", c["M"], dtype=torch.int32), x=B.rw("x", c["N"]),
             y=B.rw("y", c["M"]), status=B.rw("status", 4 * K, dtype=torch.int32), quality=B.rw("quality", 2 * K))
    sc = B.rw("scratch", ctx.scratch_floats)
    import test_basis_repair as tb
    _lib.check(_lib.lib().mllp_basis_repair(ctx.h, x1.ptr, x2.ptr, order.ptr, tb.TOL, ctx.max_m, o["basis"].ptr, o["col_of_row"].ptr,
                                            o["x"].ptr, o["y"].ptr, o["status"].ptr, o["quality"].ptr, sc.ptr, _s()))
    return o


def anchor_repair(ctx):
    """tests/test_basis_repair.py: the fp64 walk of the rule and the dense solve, at that file's bar (X_BAR)"""
    import test_basis_repair as tb
    c, K = ctx.c, len(ctx.c["inst_m"])
    walks = tb.oracle_walks(ctx.mats, c, ctx.order)

    def check(out):
        h = dict(basis=fl(out["basis"]), col_of_row=out["col_of_row"], x=fl(out["x"]), y=fl(out["y"]),
                 status=out["status"].reshape(K, 4), quality=fl(out["quality"]).reshape(K, 2))
        if ctx.variant == "scratch":                               # (its certificate reads c and b from the batch's own tensors)
            b, keep = ctx.b, (ctx.b.x1.clone(), ctx.b.x2.clone())
            b.x1.copy_(torch.from_numpy(ctx.x1))
            b.x2.copy_(torch.from_numpy(ctx.x2))
            try:
                tb._check_planted(b, c, ctx.mats, ctx.st, h, walks, ctx.case)
            finally:
                b.x1.copy_(keep[0])
                b.x2.copy_(keep[1])
        else:
            tb._check_against_walks(c, h, walks, ctx.case, x1=ctx.x1, x2=ctx.x2)
    return check


ADAM = dict(lr=3e-3, b1=0.8, b2=0.99, eps=1e-8, gscale=0.37)


def _make_adam(n, seed=None):
    """the data of tests/test_throughput_oracle.py::test_adam_step_against_fp64 (one sign per element keeps the moments away
    from cancellation; exact zeros included)"""
    rng = np.random.default_rng(n if seed is None else seed)
    p0 = (rng.choice([-1.0, 1.0], n) * rng.uniform(0.5, 1.5, n)).astype(np.float32)
    sign = rng.choice([-1.0, 1.0], n)
    gs = [(sign * np.abs(rng.standard_normal(n)) * (rng.random(n) >= 0.2)).astype(np.float32) for _ in range(2)]
    return Plain(f"adam {n}", None, (lambda ctx: resolve(("adam_b", n))) if seed is None else None, n=n, p0=p0, gs=gs)


def ep_adam(ctx, B):
    """two steps from zero moments, each with its own gradient; the step count lives in d_state"""
    n, a = ctx.n, ADAM
    P, m, v = B.io("params", ctx.p0), B.io("exp_avg", np.zeros(n, np.float32)), B.io("exp_avg_sq", np.zeros(n, np.float32))
    st = B.io("state", _f32([0.0, a["lr"], a["b1"], a["b2"]]))
    for k, g in enumerate(ctx.gs):
        G = B.ro(f"grads{k}", g)
        _lib.check(_lib.lib().mllp_adam_step(P.ptr, G.ptr, m.ptr, v.ptr, st.ptr, a["eps"], a["gscale"], n, _s()))
    return {"params": P, "exp_avg": m, "exp_avg_sq": v, "state": st}


def anchor_adam(ctx):
    """oracle/spmm_form.py::adam_step in fp64 on the fp32 values the kernel receives; the bars of
    tests/test_throughput_oracle.py::test_adam_step_against_fp64 (1e-6 parameters, 1e-5 moments, element by element)"""
    f = lambda x: float(np.float32(x))  # noqa: E731
    p, m, v = ctx.p0.astype(np.float64), np.zeros(ctx.n), np.zeros(ctx.n)
    for t, g in enumerate(ctx.gs, start=1):
        o2.adam_step(p, g.astype(np.float64) * f(ADAM["gscale"]), m, v, t, f(ADAM["lr"]), f(ADAM["b1"]), f(ADAM["b2"]), f(ADAM["eps"]))

    def check(out):
        for what, want, rtol in (("params", p, 1e-6), ("exp_avg", m, 1e-5), ("exp_avg_sq", v, 1e-5)):
            bad = np.abs(fl(out[what]).astype(np.float64) - want) > rtol * np.abs(want)
            assert not bad.any(), f"{ctx.case} {what}: {int(bad.sum())} elements off"
        assert float(fl(out["state"])[0]) == float(len(ctx.gs))
    return check


def _make_dense(seed):
    """one segment of 4999 logits with ties (three values), 1025 to select: past the 1024-key chunk of select.hip"""
    from test_predict import tied_inputs
    n, m = 4999, 1025
    z = tied_inputs(n, seed)["three_values"]
    z[:: 7] = np.random.default_rng(seed).standard_normal(len(z[:: 7])).astype(np.float32)
    return Plain(f"dense {seed}", None, (lambda ctx: resolve(("dense", 6))) if seed == 5 else None, n=n, m=m, z=z)


def ep_topm_dense(ctx, B):
    z = B.ro("logits", ctx.z)
    mask, index, stats = B.rw("mask", ctx.n, dtype=torch.uint8), B.rw("index", ctx.m, dtype=torch.int32), B.rw("stats", 2)
    _lib.check(_lib.lib().mllp_topm_select_dense(ctx.n, ctx.m, z.ptr, mask.ptr, index.ptr, stats.ptr, _s()))
    return {"mask": mask, "index": index, "stats": stats}


def anchor_topm_dense(ctx):
    """tests/test_predict.py::oracle_select: exact"""
    from test_predict import oracle_select
    mask, index, stats = oracle_select(ctx.z, [ctx.n], [ctx.m])

    def check(out):
        assert np.array_equal(out["mask"], mask) and np.array_equal(out["index"], index)
        assert np.array_equal(out["stats"], stats.reshape(-1).view(np.int32))
    return check


def _make_spmm_copy(kind):
    def make(case, config):
        c = mc.Ctx(case, "generic", mc.case_flat(case))
        for tr in (False, True):
            if kind == "streamed":
                assert c.b.build_spmm_copy(tr)["n_tiles"] > 0
            else:
                assert c.b.enable_tiled(tr, variant=0) is not None
        torch.cuda.synchronize()
        c.spmm_rtol = 2e-6       # the bar of the files that own these kernels (tests/test_stream_spmm.py::_check_orientation;
        return c                 # tests/test_hip_parity.py, the LDS-tiled product); on the plain arrays 1e-6
    return make


def _bf16_bits(a):
    """fp32 -> bf16 (round to nearest even) as int16 bit patterns, and the fp32 values those patterns stand for"""
    t = torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16)
    return t.view(torch.int16).numpy().copy(), t.float().numpy()


def _spmm_bf16(transpose):
    def ep(ctx, B):
        n_in, n_out = (ctx.M, ctx.N) if transpose else (ctx.N, ctx.M)
        bits, _ = _bf16_bits(np.random.default_rng(1 + getattr(ctx, "data_seed", 0)).standard_normal((n_in, 16)))
        H = B.ro("H", bits.reshape(-1), wide=True, dtype=torch.int16)
        Y = B.rw("Y", n_out * 16, wide=True)
        _lib.check(_lib.lib().mllp_spmm_csr_bf16(ctx.h, int(transpose), H.ptr, Y.ptr, _s()))
        return {"Y": Y}
    ep.__name__ = f"ep_spmm_bf16_{int(transpose)}"
    return ep


def anchor_spmm_bf16(ctx, transpose):
    """include/mllp_hip.h: the fp32 product of A with H rounded to bf16, exact-fp32 accumulation -- against the fp64 product
    with the SAME rounded features, at bound (a) of tests/test_hip_parity.py::test_bf16_feature_image_spmm (2e-6)"""
    ob = refs(ctx.case).ob
    n_in = ctx.M if transpose else ctx.N
    _, H = _bf16_bits(np.random.default_rng(1 + getattr(ctx, "data_seed", 0)).standard_normal((n_in, 16)))
    ptr, idx, val = (ob.cp, ob.ri, ob.cv) if transpose else (ob.rp, ob.ci, ob.va)
    want = o2.spmm(ptr, idx, val.astype(np.float32).astype(np.float64), H.astype(np.float64))
    return lambda out: close(fl(out["Y"]).reshape(want.shape), want, 2e-6, "A bf16(H)")


# ---- AngleModel -------------------------------------------------------------------------------------------------------------
ANGLE_SIZES = [(17, 16), (257, 16), (17, 256), (257, 256)]      # two of the sizes and both end widths of tests/test_angle_shapes.py


def _make_angle(N, F):
    import test_angle_shapes as ta
    model, Q, coefs, basis = ta._grid_case(N, F)
    g, _ = ta._graph(Q, coefs, basis)
    names = [n for n, _ in model.named_parameters()]
    shapes = [tuple(p.shape) for _, p in model.named_parameters()]
    dl = (torch.randn(N - 1, generator=torch.Generator().manual_seed(5)) / (N - 1)).numpy()
    return Plain(f"angle N={N} F={F}", None, _angle_b, N=N, F=F, cos=_f32(g.cos.numpy()), x=_f32(g.x.numpy()),
                 flat=_f32(model.flat_parameters().detach().numpy()), dl=_f32(dl), names=names, shapes=shapes,
                 ws_floats=ta._ws_floats(N, F))


def _angle_b(ctx):
    """parameters x 1.1, x and the logit gradient perturbed, another SYMMETRIC matrix in place of the cosines"""
    def make():
        rng = np.random.default_rng(77)
        R = rng.uniform(-0.2, 0.2, ctx.cos.shape)
        return ctx.with_data(cos=_f32(np.clip(ctx.cos + (R + R.T) / 2, -1.0, 1.0)), flat=_f32(ctx.flat * 1.1),
                             x=_f32(ctx.x * (1.0 + 0.1 * rng.uniform(-1, 1, ctx.x.shape))), dl=_f32(ctx.dl[::-1] * 1.5))
    return _second(ctx, make)


def _angle(mode):
    def ep(ctx, B):
        N, F, L = ctx.N, ctx.F, _lib.lib()
        cos, x, P = B.ro("cos", ctx.cos.reshape(-1)), B.ro("x", ctx.x.reshape(-1)), B.ro("params", ctx.flat, wide=True)
        ws, z = B.rw("ws", ctx.ws_floats, wide=True), B.rw("logits", N - 1)
        out = {"logits": z}
        _lib.check(L.mllp_angle_forward(N, F, cos.ptr, x.ptr, P.ptr, ws.ptr, z.ptr, _s()))
        if mode != "forward":
            dl, g = B.ro("dlogits", ctx.dl), B.rw("grads", ctx.flat.size)
            out["grads"] = g
        if mode == "backward":
            _lib.check(L.mllp_angle_backward(N, F, cos.ptr, x.ptr, P.ptr, ws.ptr, dl.ptr, g.ptr, _s()))
        if mode == "backward_inputs":
            dx, dcos = B.rw("dx", 2 * N), B.rw("dcos", N * N)
            out.update(dx=dx, dcos=dcos)
            _lib.check(L.mllp_angle_backward_inputs(N, F, cos.ptr, x.ptr, P.ptr, ws.ptr, dl.ptr, g.ptr, dx.ptr, dcos.ptr, _s()))
        return out
    ep.__name__ = f"ep_angle_{mode}"
    return ep


def anchor_angle(ctx):
    """angle_oracle.sweep_backward in fp64 (autograd's gradient of sum(logits * dlogits) for a symmetric matrix) at the bars
    of tests/test_angle_shapes.py::test_orientation_each_sweep_reads: RTOL_LOGITS, RTOL_GRAD against each tensor's maximum"""
    import angle_oracle as ao
    key = ("angle", id(ctx))
    if key not in _ANCHOR:
        sizes = [int(np.prod(s)) for s in ctx.shapes]
        sd = {n: t.reshape(s).double() for n, t, s in zip(ctx.names, torch.split(torch.from_numpy(ctx.flat), sizes), ctx.shapes)}
        A = torch.from_numpy(ctx.cos).double()
        assert torch.equal(A, A.T)
        _ANCHOR[key] = ao.sweep_backward(sd, torch.from_numpy(ctx.x).double(), A, A, A, torch.from_numpy(ctx.dl).double()), sizes
    (logits, dx, dcos, grads), sizes = _ANCHOR[key]

    def check(out):
        N = ctx.N
        ao.close(fl(out["logits"]), logits.numpy(), ao.RTOL_LOGITS, "logits")
        if "dx" in out:
            ao.close(fl(out["dx"]).reshape(N, 2), dx.numpy(), ao.RTOL_GRAD, "dx")
            ao.close(fl(out["dcos"]).reshape(N, N), dcos.numpy(), ao.RTOL_GRAD, "dcos")
        if "grads" in out:
            got = dict(zip(ctx.names, np.split(fl(out["grads"]), np.cumsum(sizes)[:-1])))
            for name in ctx.names:
                if name.startswith("gconv3"):
                    assert not got[name].any()
                elif name.endswith("lin_key.bias"):        # cancels in the softmax (the rule of test_angle_shapes._compare)
                    assert float(np.abs(got[name]).max()) <= 1e-6 * max(1.0, float(grads[name].abs().max()) * 1e6), name
                else:
                    ao.close(got[name], grads[name].numpy().reshape(-1), ao.RTOL_GRAD, name)
    return check


OWN_MAKERS = {"set_scale": _make_set_scale, "normalize": _make_normalize, "repair_lds": _make_repair("lds"),
              "repair_scratch": _make_repair("scratch"), "spmm_streamed": _make_spmm_copy("streamed"),
              "spmm_tiled": _make_spmm_copy("tiled")}
MAKERS = {"own": lambda kind, case, config: OWN_MAKERS[kind](case, config), "adam": lambda n: _make_adam(n),
          "adam_b": lambda n: _make_adam(n, seed=n + 1), "dense": lambda seed: _make_dense(seed), "angle": lambda N, F: _make_angle(N, F)}


def resolve(where):
    """a cell's context: ("model", case, config): the shared one of tests/test_memory_contract.py; ("own", kind, case, config),
    ("adam", n), ("dense", seed), ("angle", N, F): made here, once"""
    if where[0] == "model":
        return get_ctx(where[1], where[2])
    if where not in _OWN:
        _OWN[where] = MAKERS[where[0]](*where[1:])
    return _OWN[where]


# ---------------------------------------------------------------------------------------------------------------------
# the table of entry points
# ---------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Spec:
    ep: object                      # the entry point of the anchor run (may read back between its calls)
    anchor: object                  # ctx -> check(outputs)
    covers: tuple                   # the launch functions it runs
    late: object = None             # the same calls without a read-back or a synchronisation (default: ep)
    not_finite: tuple = ()          # outputs that are not floats, or may hold an infinity by their definition

    @property
    def queued(self):
        return self.late or self.ep


def _m(name, covers, late=None):
    ep, anchor = MODEL_EPS[name]
    return Spec(ep, anchor, tuple("mllp_" + c for c in covers), late)


SPECS = {
    "forward": _m("forward", ["gnn_forward"]),
    "forward_backward": _m("forward_backward", ["gnn_forward", "gnn_backward"]),
    "loss_step": _m("loss_step", ["gnn_loss_step"]),
    "loss_step_weighted": _m("loss_step_weighted", ["gnn_loss_step_weighted"]),
    "input_grads": _m("input_grads", ["gnn_forward", "gnn_input_grads"], ep_input_grads_late),
    "loss_step_inputs": _m("loss_step_inputs", ["gnn_loss_step_inputs"]),
    "train_step": _m("train_step", ["gnn_train_step"], ep_train_step_late),
    "backward_inputs": Spec(ep_backward_inputs, mc.anchor_input_grads, ("mllp_gnn_backward_inputs",)),
    "small_loss": Spec(mc.ep_small_loss, mc.anchor_loss_step, ("mllp_gnn_train_step_small",)),
    "small_adam": Spec(mc.ep_small_adam, lambda ctx: mc.anchor_train(ctx, 1), ("mllp_gnn_train_step_small",)),
    "tconv_cin1": Spec(mc._tconv("cin1"), lambda ctx: mc.anchor_tconv(ctx, "cin1"), ("mllp_tconv_fwd", "mllp_tconv_bwd"), _tconv_late("cin1")),
    "tconv_cin16": Spec(mc._tconv("cin16"), lambda ctx: mc.anchor_tconv(ctx, "cin16"), ("mllp_tconv_fwd", "mllp_tconv_bwd"), _tconv_late("cin16")),
    "weighted_loss": Spec(mc.ep_weighted_loss, mc.anchor_weighted_loss, ("mllp_weighted_loss", "mllp_balanced_pos_weight")),
    "topm": Spec(mc.ep_topm, mc.anchor_topm, ("mllp_topm_metrics", "mllp_topm_select"), not_finite=("stats", "index", "mask")),
    "spmm_0": Spec(mc._spmm(False), lambda ctx: mc.anchor_spmm(ctx, False, getattr(ctx, "spmm_rtol", 1e-6)), ("mllp_spmm_csr_f32",)),
    "spmm_1": Spec(mc._spmm(True), lambda ctx: mc.anchor_spmm(ctx, True, getattr(ctx, "spmm_rtol", 1e-6)), ("mllp_spmm_csr_f32",)),
    "spmm_bf16_0": Spec(_spmm_bf16(False), lambda ctx: anchor_spmm_bf16(ctx, False), ("mllp_spmm_csr_bf16",)),
    "spmm_bf16_1": Spec(_spmm_bf16(True), lambda ctx: anchor_spmm_bf16(ctx, True), ("mllp_spmm_csr_bf16",)),
    "set_scale": Spec(ep_set_scale, anchor_set_scale, ("mllp_graph_set_values", "mllp_graph_scale_values")),
    "normalize": Spec(ep_normalize_own, anchor_normalize, ("mllp_graph_set_values", "mllp_graph_normalize")),
    "certificate": Spec(ep_certificate, anchor_certificate, ("mllp_lp_certificate",), not_finite=("cert",)),
    "repair_lds": Spec(ep_repair, anchor_repair, ("mllp_basis_repair",), not_finite=("col_of_row", "status", "quality")),
    "repair_scratch": Spec(ep_repair, anchor_repair, ("mllp_basis_repair",), not_finite=("col_of_row", "status", "quality")),
    "adam": Spec(ep_adam, anchor_adam, ("mllp_adam_step",)),
    "topm_dense": Spec(ep_topm_dense, anchor_topm_dense, ("mllp_topm_select_dense",), not_finite=("stats", "index", "mask")),
    "angle_forward": Spec(_angle("forward"), anchor_angle, ("mllp_angle_forward",)),
    "angle_backward": Spec(_angle("backward"), anchor_angle, ("mllp_angle_forward", "mllp_angle_backward")),
    "angle_backward_inputs": Spec(_angle("backward_inputs"), anchor_angle, ("mllp_angle_forward", "mllp_angle_backward_inputs")),
}


def _cells():
    cells = []
    for case in ("holes", "grid"):
        for config in CONFIGS:
            for name in list(MODEL_EPS) + ["tconv_cin1", "tconv_cin16"]:
                cells.append((name, ("model", case, config)))
            if config != "fused":                                  # (mllp_gnn_backward_inputs refuses the fused path)
                cells.append(("backward_inputs", ("model", case, config)))
            if case == "holes":                                    # (grid is beyond the small step's limits)
                cells += [("small_loss", ("model", case, config)), ("small_adam", ("model", case, config))]
    for name in ("weighted_loss", "topm", "spmm_0", "spmm_1", "certificate"):
        cells.append((name, ("model", "holes", "generic")))
    for kind in ("spmm_streamed", "spmm_tiled"):
        cells += [("spmm_0", ("own", kind, "holes", "generic")), ("spmm_1", ("own", kind, "holes", "generic"))]
    cells += [("spmm_bf16_0", ("own", "spmm_tiled", "holes", "generic")), ("spmm_bf16_1", ("own", "spmm_tiled", "holes", "generic"))]
    cells += [("set_scale", ("own", "set_scale", "holes", "fused")), ("set_scale", ("own", "set_scale", "holes", "generic")),
              ("normalize", ("own", "normalize", "holes", "generic"))]
    cells += [("repair_lds", ("own", "repair_lds", "-", "-")), ("repair_scratch", ("own", "repair_scratch", "-", "-"))]
    cells += [("adam", ("adam", 4721)), ("adam", ("adam", 20000)), ("topm_dense", ("dense", 5))]
    for N, F in ANGLE_SIZES:
        cells += [(f"angle_{mode}", ("angle", N, F)) for mode in ("forward", "backward", "backward_inputs")]
    return cells


LATE_CELLS = _cells()
CAPTURE_CELLS = _cells()          # no launch function is exempt from capture: every entry point has a variant without a read-back


def _id(cell):
    return cell[0] + "-" + "-".join(str(v) for v in cell[1][1:])


def anchor_of(ctx, name):
    """the eager run on the default stream with zero-filled buffers, checked against the oracle once and shared"""
    key = (id(ctx), name)
    if key not in _ANCHOR:
        spec = SPECS[name]
        out, _ = eager(ctx, spec.ep)
        for k, v in out.items():
            if v.dtype == np.int32 and k not in spec.not_finite:
                assert np.isfinite(fl(v)).all(), f"{k} is not finite"
        spec.anchor(ctx)(out)
        _ANCHOR[key] = out
    return _ANCHOR[key]


# ---------------------------------------------------------------------------------------------------------------------
# 3. late inputs on a delayed side stream
# ---------------------------------------------------------------------------------------------------------------------
def _hip_runtime():
    """the HIP runtime this process already has loaded (the one torch uses), by its path in /proc/self/maps"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return ctypes.CDLL(line.split()[-1])
    raise AssertionError("no libamdhip64 is mapped into this process")


@pytest.fixture(scope="module")
def side():
    assert torch.cuda.is_available()
    _lib.lib()
    S = torch.cuda.Stream()
    flags = ctypes.c_uint(99)
    assert _hip_runtime().hipStreamGetFlags(ctypes.c_void_p(S.cuda_stream), ctypes.byref(flags)) == 0
    assert flags.value == 1, f"the side stream is not hipStreamNonBlocking (flags {flags.value})"
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(cycles):
        with torch.cuda.stream(S):
            e0.record()
            torch.cuda._sleep(cycles)
            e1.record()
        S.synchronize()
        return e0.elapsed_time(e1)
    timed(1_000_000)
    probe = 20_000_000
    per_ms = probe / timed(probe)
    assert DELAY_MS <= DELAY_CEILING_MS
    cycles = int(DELAY_MS * per_ms)
    got = timed(cycles)
    assert 0.8 * DELAY_MS <= got <= DELAY_CEILING_MS, f"a sleep of {cycles} cycles took {got:.1f} ms, asked for {DELAY_MS}"
    s = types.SimpleNamespace(stream=S, cycles=cycles, per_ms=per_ms, delay_ms=got, host_ms={})
    yield s
    if s.host_ms:
        worst = max(s.host_ms, key=s.host_ms.get)
        print(f"\n[stream contract] side stream flags {flags.value}; {per_ms:.0f} sleep cycles per ms; delay {got:.1f} ms; "
              f"longest host time on the side stream {s.host_ms[worst]:.2f} ms ({worst}); the five longest: "
              + ", ".join(f"{k} {v:.2f}" for k, v in sorted(s.host_ms.items(), key=lambda kv: -kv[1])[:5]))


@gpu
@pytest.mark.parametrize("cell", LATE_CELLS, ids=_id)
def test_late_inputs_on_a_delayed_side_stream(cell, side):
    name, where = cell
    ctx, spec = resolve(where), SPECS[name]
    anchor = anchor_of(ctx, name)
    B = LateBufs(side.stream)
    ctx.b.invalidate_inputs()
    torch.cuda.synchronize()
    with torch.cuda.stream(side.stream):
        torch.cuda._sleep(side.cycles)
        t0 = time.perf_counter()
        outs = spec.queued(ctx, B)
        side.host_ms[_id(cell)] = 1e3 * (time.perf_counter() - t0)
        still_busy = not side.stream.query()
    side.stream.synchronize()
    assert still_busy, (f"{_id(cell)}: the side stream was idle when the entry point returned after {side.host_ms[_id(cell)]:.1f} ms "
                        f"of host time: a call synchronised, or the delay of {side.delay_ms:.0f} ms is too short for this cell")
    B.check()
    got = finish(outs)
    same_bits(got, {k: anchor[k] for k in got}, f"{_id(cell)}: late inputs on the delayed side stream against the default stream")


# ---------------------------------------------------------------------------------------------------------------------
# 4. capture, and replay after every input changed
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("cell", CAPTURE_CELLS, ids=_id)
def test_capture_then_replay_on_other_inputs(cell):
    name, where = cell
    ctx, spec = resolve(where), SPECS[name]
    other = ctx_b(ctx)
    anchor_of(ctx, name)
    want = anchor_of(other, name)
    _, made = eager(ctx, spec.queued, Bufs("nan"))                 # the buffers, holding A; every lazy allocation is made
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = spec.queued(ctx, ReuseBufs(made))
    refill = RefillBufs(made)
    other.b.invalidate_inputs()
    spec.queued(other, refill)                                      # B in place (and an eager run on it, which may bind the inputs)
    for replay in (1, 2):
        refill.again()
        graph.replay()
        made.check()
        got = finish(outs)
        same_bits(got, {k: want[k] for k in got}, f"{_id(cell)}: replay {replay} on the second data set against the eager run on it")


# ---------------------------------------------------------------------------------------------------------------------
# 5. a replay between eager calls on the fused path
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ["loss_step", "forward"])
@pytest.mark.parametrize("case", ["holes", "golden"])
def test_replay_between_eager_calls(case, name):
    """eager X, capture on Y, eager X, replay Y, eager X: the pointers of X never change and nothing invalidates, so the
    library alone must notice that the replay rewrote its copies of the inputs"""
    ctx, spec = get_ctx(case, "fused"), SPECS[name]
    other = ctx_b(ctx)
    r1, want_y = anchor_of(ctx, name), anchor_of(other, name)
    first, X = eager(ctx, spec.ep, Bufs("nan"))
    same_bits(first, r1, "eager X")
    _, Y = eager(other, spec.ep, Bufs("nan"))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs_y = spec.ep(other, ReuseBufs(Y))

    def eager_x(what):
        outs = spec.ep(ctx, ReuseBufs(X, poison_rw=True))          # the same pointers, the same contents; outputs NaN again
        X.check()
        same_bits(finish(outs), r1, what)
    eager_x("eager X after the capture on Y")
    for g in Y.all.values():
        if g.data is None:
            g.refill(fill=NAN)
    graph.replay()
    Y.check()
    same_bits(finish(outs_y), want_y, "the replay on Y")
    eager_x("eager X after the replay on Y")
