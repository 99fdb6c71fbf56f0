"""The memory contract of the GNN side of the C ABI (include/mllp_hip.h, "Memory contract"), entry point by
entry point, through guarded buffers (tests/guarded.py) for EVERYTHING the caller owns, the workspace included:

  1. results do not depend on what the workspace, scratch and output buffers held before the call;
  2. nothing is written outside the documented extents, and no read-only input is written;
  3. results do not depend on bytes outside the extents (the guards change with every fill);
  4. between whole calls that carry nothing the workspace may be clobbered.

Every cell (case x configuration x entry point) runs the call with all caller-owned writable memory and all guards zeroed
(the ANCHOR, compared with the fp64 oracle the project already uses for that entry point, at the bars of the test files
that own them -- imported, not restated; no tolerance is introduced here), then again with everything filled with
0xFFFFFFFF (a NaN), with 0x7F7FFFFF (the largest finite float), with the LEAVINGS of another batch and other parameters run
through the same entry point, and once more with every buffer that needs only 4-byte alignment shifted by one float.  Each
of these must reproduce the anchor BIT FOR BIT (the library promises determinism without atomics: equality is the bar), every
guard word must be intact and every read-only input unchanged after every run.

Nothing here poisons between a forward and its backward, or before a flags-1 train step: the header forbids that use.
The per-tensor caps of the four cases are 0: measured on the CPU, the fp32 restatement exempts no tensor on any of them
(test_case_shapes_and_yardsticks asserts it).
"""
import ctypes
import types

import numpy as np
import pytest
import torch

import fused_cases as fc
import grad_scales as gs
from guarded import HUGE, NAN, ZERO, Guarded, same_bits
from mllp_amd import _lib
from mllp_amd._lib import conv_param_slice
from mllp_amd.data import SUBSET5, load_packed
from oracle import spmm_form as o2
from test_hip_parity import RTOL_ACT, RTOL_GRAD, close, grad_mask
from test_input_grads import oracle_input_grads
from test_input_grads_fused import RTOL_OUT, _bce_loss, _check_four
from test_normalize import _close as norm_close
from test_normalize import _knife_edge, _normalize_host, _perturbed_list
from test_predict import oracle_select
from test_weighted_loss import oracle_balanced, oracle_loss

gpu = pytest.mark.gpu
EINVAL = -1
CASES = ("holes", "grid", "golden", "one")
# stream: LPBatch.enable_stream_step() as a trainer calls it (a copy that pads beyond 2 entry slots per nonzero is dropped);
# stream_padded: every streamed copy kept whatever it pads -- the C ABI builds and uses them, so the contract covers them
CONFIGS = ("fused", "generic", "stream", "stream_padded", "tiled")
FILLS = ("nan", "huge", "leavings")
PATTERN = {"zero": ZERO, "nan": NAN, "huge": HUGE, "leavings": NAN}      # (leavings: the guards hold the NaN pattern)
PER_TENSOR_CAP = 0


# ---------------------------------------------------------------------------------------------------------------------
# the helper itself, on CPU tensors
# ---------------------------------------------------------------------------------------------------------------------
def test_guard_detects_and_locates_a_planted_word_before_and_after():
    for dtype, n in ((torch.float32, 37), (torch.uint8, 13), (torch.int32, 1)):
        for fill in (ZERO, NAN, HUGE):
            g = Guarded(n, dtype, fill=fill, guard_fill=fill, name="planted")
            assert g.view.data_ptr() % 256 == 0 and g.intact()
            words = g.raw.view(torch.int32)
            first_behind = (g.start + g.nbytes + 3) // 4
            words[g.start // 4 - 1] ^= 0x00400000                  # the word just before the inner buffer
            assert g.damage() == (-2, -2)                           # (little endian: bit 22 is in byte 2 of the word)
            with pytest.raises(AssertionError, match=r"first damaged byte -2 \(word -1\)"):
                g.intact()
            words[g.start // 4 - 1] ^= 0x00400000
            assert g.intact()
            words[first_behind] ^= 1                                # the first whole word behind it
            lo = 4 * first_behind - g.start
            assert g.damage() == (lo, lo) and lo - g.nbytes < 4
            words[-1] ^= 1                                          # ... and the very last guard word
            assert g.damage() == (lo, g.raw.numel() - 4 - g.start)
            with pytest.raises(AssertionError, match="planted: guard words overwritten"):
                g.check()
    g = Guarded(5, torch.uint8, fill=ZERO, guard_fill=HUGE)        # a byte behind an inner buffer that ends inside a word
    g.raw[g.start + 5] ^= 0x10
    assert g.damage() == (5, 5)


def test_untouched_nan_guards_count_as_intact():
    g = Guarded(100, fill=NAN, guard_fill=NAN)
    assert torch.isnan(g.raw.view(torch.float32)).all()           # as floats no word equals itself ...
    assert g.intact() and g.damage() is None                       # ... the comparison is on the bits
    g.view.fill_(1.0)                                               # writing the inner buffer is not damage
    assert g.intact()
    assert (g.bits() == np.float32(1.0).view(np.int32)).all()
    h = Guarded(100, fill=HUGE, guard_fill=HUGE, shift=4)
    assert h.view.data_ptr() % 256 == 4 and float(h.view[0]) == float(np.finfo(np.float32).max) and h.intact()
    e = Guarded(7, leavings=torch.tensor([1.0, -0.0]))
    assert e.bits().tolist() == [0x3F800000, -0x80000000] * 3 + [0x3F800000]
    same_bits({"a": e.bits()}, {"a": e.bits().copy()}, "equal")
    with pytest.raises(AssertionError, match="first at 1, last at 1"):
        other = e.bits().copy()
        other[1] = 0                                                # +0.0 for -0.0: equal as floats, not as bits
        same_bits({"a": other}, {"a": e.bits()}, "signed zero")


def test_changed_read_only_input_is_detected():
    x = np.arange(50, dtype=np.float32)
    g = Guarded(50, data=x, name="x1")
    assert g.check() and np.array_equal(g.numpy(), x)
    g.view[17] = np.nan
    with pytest.raises(AssertionError, match=r"x1: read-only input written, .* first at byte 7\d \(word 17\)"):
        g.check()
    g.view[17] = 17.0
    assert g.check()
    g.view[0] = -0.0                                                # 0.0 -> -0.0: equal as floats, a change all the same
    with pytest.raises(AssertionError, match="read-only input written"):
        g.unchanged()
    with pytest.raises(AssertionError, match="holds no given data"):
        Guarded(4).unchanged()


# ---------------------------------------------------------------------------------------------------------------------
# cases (tests/fused_cases.py), built once
# ---------------------------------------------------------------------------------------------------------------------
_CASES = {}


def case_instances(name):
    if name not in _CASES:
        sub = load_packed(SUBSET5)
        _CASES["golden"] = list(sub)
        _CASES["one"] = [i for i in sub if i.name == "afiro.mps"]
        _CASES["holes"] = [fc.holes_instance(3, 150, 230), fc.empty_instance(7, 9), fc.small_inst(np.array([[1.5]]), "one", 1),
                           fc.single_row_instance(300)]
        _CASES["grid"] = [fc.degree_grid(0)]          # N = M = 6585 > 1024 already: one replica is as far as needed
        _CASES["donor"] = [i for i in sub if i.name in ("kb2.mps", "sc50a.mps")]
    return _CASES[name]


def _golden_flat():
    import os
    return np.load(os.path.join(fc.ROOT, "tests", "golden", "subset5.npz"), allow_pickle=False)["weights_flat"]


def test_case_shapes_and_yardsticks():
    """The shapes the issue asks for, and the per-tensor cap of every case from the fp32 restatement alone (CPU)."""
    lim = (ctypes.c_int64 * 4)()
    assert _lib.lib().mllp_gnn_small_step_limits(lim) == 0
    dims = {}
    for name in CASES:
        insts = case_instances(name)
        dims[name] = M, N, nnz = sum(i.m for i in insts), sum(i.n for i in insts), sum(i.nnz for i in insts)
        assert nnz > 0
    M, N, nnz = dims["holes"]
    assert M + N <= 2048 and nnz <= 8192 and M + N <= lim[0] and nnz <= lim[1] and M % 16 and N % 16
    h = case_instances("holes")
    deg_r, deg_c = fc.degrees(h[0])
    assert (deg_r == 0).any() and (deg_c == 0).any() and h[1].nnz == 0 and (h[2].m, h[2].n) == (1, 1) and h[3].m == 1
    M, N, _ = dims["grid"]
    c = fc.constants()
    assert M > 1024 and N > 1024 and all(v % 1024 and v % 64 for v in (M, N))
    for deg in fc.degrees(case_instances("grid")[0]):
        for T in c["T16"] + c["T1"]:
            assert {T - 1, T, T + 1} <= set(deg.tolist())
    assert dims["one"][1] < 64 and sum(dims["one"][:2]) <= 2048
    assert [i.name for i in case_instances("golden")] == list(SUBSET5)
    sd = {k: v for k, v in fc.golden_state({"weights_flat": _golden_flat()}).items()}
    for name in CASES:
        ob = o2.BatchCSR(case_instances(name))
        for dz in (None, _functional(ob.N)):
            assert len(gs.exempt_tensors(gs.yardstick(sd, ob, dlogits=dz))) <= PER_TENSOR_CAP, name
    for name in CASES:                                              # normalize: no row on the knife edge of the cap
        pert, _ = _perturbed_list(case_instances(name))
        assert not any(_knife_edge(p).any() for p in pert), name


def _functional(n, seed=41):
    return (np.random.default_rng(seed).standard_normal(n) / max(n, 1)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# the misaligned-pointer refusals need no GPU: they come before any HIP call (and before the graph is looked at)
# ---------------------------------------------------------------------------------------------------------------------
def _aligned_calls(L, p):
    """name -> (call(args), positions of the pointers that are accessed in 16-byte pieces); every pointer argument is `p`"""
    f, i = 1.0, 0
    return {
        "mllp_gnn_forward": (lambda a: L.mllp_gnn_forward(*a, None), [p] * 6, (1, 2, 3, 4)),
        "mllp_gnn_backward": (lambda a: L.mllp_gnn_backward(*a, None), [p] * 7, (1, 2, 3, 4)),
        "mllp_gnn_loss_step": (lambda a: L.mllp_gnn_loss_step(*a[:5], f, *a[5:], None), [p] * 9, (1, 2, 3, 5)),
        "mllp_gnn_loss_step_weighted": (lambda a: L.mllp_gnn_loss_step_weighted(*a, None), [p] * 13, (1, 2, 3, 7)),
        "mllp_gnn_backward_inputs": (lambda a: L.mllp_gnn_backward_inputs(*a, None), [p] * 11, (1, 2, 3, 4)),
        "mllp_gnn_input_grads": (lambda a: L.mllp_gnn_input_grads(*a, None), [p] * 11, (1, 2, 3, 4)),
        "mllp_gnn_loss_step_inputs": (lambda a: L.mllp_gnn_loss_step_inputs(*a[:5], f, *a[5:], None), [p] * 12, (1, 2, 3, 5)),
        "mllp_gnn_train_step": (lambda a: L.mllp_gnn_train_step(*a[:5], f, *a[5:], 1e-8, i, None), [p] * 12, (1, 2, 3, 5)),
        "mllp_gnn_train_step_small": (lambda a: L.mllp_gnn_train_step_small(*a[:5], f, *a[5:], 1e-8, None), [p] * 12, (1, 2, 3, 5)),
        "mllp_tconv_fwd": (lambda a: L.mllp_tconv_fwd(a[0], 0, 16, *a[1:], None), [p] * 6, (1, 2, 3, 4, 5)),
        "mllp_tconv_bwd": (lambda a: L.mllp_tconv_bwd(a[0], 0, 16, *a[1:9], 0, a[9], None), [p] * 10, (1, 2, 3, 4, 5, 6, 7, 8)),
        "mllp_spmm_csr_f32": (lambda a: L.mllp_spmm_csr_f32(a[0], 0, a[1], a[2], None), [p] * 3, (1, 2)),
    }


def test_misaligned_16_byte_pointers_are_refused_before_any_hip_call():
    """Host memory that is never dereferenced stands for every pointer, the graph included: the refusal comes first.  One
    float off (the natural alignment of a float) is refused with MLLP_EINVAL and a message that says why; the null checks
    keep their own message."""
    L = _lib.lib()
    room = ctypes.create_string_buffer(1 << 12)
    base = (ctypes.addressof(room) + 255) // 256 * 256
    p, off = ctypes.c_void_p(base), ctypes.c_void_p(base + 4)
    for name, (call, args, wide) in _aligned_calls(L, p).items():
        for k in wide:
            a = list(args)
            a[k] = off
            assert call(a) == EINVAL, (name, k)
            msg = L.mllp_last_error()
            assert name.encode() in msg and b"misaligned" in msg and b"16-byte" in msg, (name, k, msg)
        a = list(args)
        a[wide[0]] = None
        assert call(a) == EINVAL and b"null" in L.mllp_last_error(), name


# ---------------------------------------------------------------------------------------------------------------------
# GPU: contexts (one batch per case x configuration, built once) and references (one per case, computed once)
# ---------------------------------------------------------------------------------------------------------------------
_CTX, _REFS, _LEAVINGS = {}, {}, {}


def _stream():
    return _lib.current_stream()


def _f32(a):
    return np.ascontiguousarray(np.asarray(a), dtype=np.float32)


class Ctx:
    """one batch on one configuration, with its inputs as fp32 host arrays (device copies are made per run, guarded)"""

    def __init__(self, case, config, flat):
        from mllp_amd.graph import LPBatch
        _lib.lib()
        assert torch.cuda.is_available()
        self.case, self.config, self.insts = case, config, case_instances(case)
        self.b = b = LPBatch.from_instances(self.insts)
        self.skip = None
        b.set_path(2 if config == "fused" else 1)
        if config in ("stream", "stream_padded"):
            info = b.enable_stream_step() if config == "stream" else b.enable_stream_step(max_slots_per_nnz=float("inf"))
            self.copies = {k: ("dropped" if v.get("dropped") else "kept") for k, v in info.items()}
            kept = [k for k, v in info.items() if not v.get("dropped")]
            if not kept:
                self.skip = (f"{case}: enable_stream_step() keeps no copy (every geometry pads beyond 2 entry slots per "
                             "nonzero and is dropped): the cell would repeat the plain generic one")
        if config == "tiled":
            info = b.enable_tiled_step()
            self.copies = {k: ("none" if v is None else "attached") for k, v in info.items()}
            if not [k for k, v in info.items() if v is not None]:
                self.skip = f"{case}: enable_tiled_step() attaches no copy: the cell would repeat the plain generic one"
        self.h, self.M, self.N, self.nnz, self.K = b._h, b.M, b.N, b.nnz, b.n_inst
        self.flat = _f32(flat)
        self.x1, self.x2, self.y = (_f32(np.concatenate([getattr(i, f) for i in self.insts])) for f in ("coefs", "rhs", "basis"))
        n = ctypes.c_int64()
        _lib.check(_lib.lib().mllp_gnn_workspace_bytes(self.h, ctypes.byref(n)))
        assert n.value % 64 == 0
        self.ws_floats = n.value // 4
        self.dz = _functional(self.N)
        rng = np.random.default_rng(17)
        self.iw = _f32(rng.random(self.K) * 2.0)
        if self.K > 1:
            self.iw[1] = 0.0                                        # a held-out instance
        self.pw = _f32(0.5 + 3.0 * rng.random(self.K))


def case_flat(case):
    """the parameters a case runs with: the golden ones; x 1.25 for the donor of the leavings and for the second data set
    ("+b") of tests/test_stream_contract.py"""
    flat = _golden_flat()
    return flat * 1.25 if case == "donor" or case.endswith("+b") else flat


def get_ctx(case, config):
    key = (case, config)
    if key not in _CTX:
        _CTX[key] = Ctx(case, config, case_flat(case))
    c = _CTX[key]
    if c.skip:
        pytest.skip(c.skip)
    return c


def refs(case):
    """the fp64 references of a case: computed on first use, shared, never modified"""
    if case in _REFS:
        return _REFS[case]
    insts, flat = case_instances(case), case_flat(case)
    sd = fc.golden_state({"weights_flat": flat})
    ob = o2.BatchCSR(insts)
    seg_n, ib = [i.n for i in insts], 1.0 / len(insts)
    r = types.SimpleNamespace(sd=sd, ob=ob, seg_n=seg_n, seg_m=[i.m for i in insts], flat=flat)
    r.step = o2.gnn_forward_backward(sd, ob)
    r.yard = gs.yardstick(sd, ob)
    c = get_ctx(case, "generic")
    dz = c.dz.astype(np.float64)
    r.dz = fc.model_dt(sd, ob, np.float64, dlogits=dz)
    r.yard_dz = gs.yardstick(sd, ob, dlogits=dz)
    r.wl = oracle_loss(r.step["logits"], ob.basis, seg_n, c.iw, c.pw)
    r.wl_grads = fc.model_dt(sd, ob, np.float64, dlogits=r.wl["dz"])["grads"]
    r.ig_loss = oracle_input_grads(flat, insts, _bce_loss(insts, ib))
    rt = torch.tensor(dz)
    r.ig_dz = oracle_input_grads(flat, insts, lambda z: (z.reshape(-1) * rt).sum())
    # two Adam steps of the reference's loop on this batch (oracle.spmm_form.adam_step), fp64
    P, m, v = np.asarray(flat, np.float64).copy(), np.zeros(len(flat)), np.zeros(len(flat))
    r.adam_losses = []
    for step in (1, 2):
        sdk = fc.golden_state({"weights_flat": P})
        rr = o2.gnn_forward_backward(sdk, ob)
        r.adam_losses.append(rr["loss"])
        o2.adam_step(P, rr["grads"], m, v, step)
    r.adam_params = P
    _REFS[case] = r
    return r


class Bufs:
    """the guarded buffers of one run: ro = read-only input (checked unchanged), io = in/out with given data, rw = output or
    scratch, filled by the run's mode.  wide=True: a pointer the header wants 16-byte aligned (never shifted)."""

    def __init__(self, fill, leavings=None, shift=0):
        self.fill, self.leavings, self.shift, self.all = fill, leavings or {}, shift, {}

    def _make(self, name, n, dtype, wide, **kw):
        assert name not in self.all
        g = Guarded(max(int(n), 1), dtype, "cuda", guard_fill=PATTERN[self.fill], shift=0 if wide else self.shift, name=name, **kw)
        self.all[name] = g
        return g

    def ro(self, name, data, wide=False, dtype=torch.float32):
        return self._make(name, np.asarray(data).size, dtype, wide, data=np.asarray(data))

    def io(self, name, data, wide=False):
        g = self.ro(name, data, wide)
        g.data = None
        return g

    def rw(self, name, n, wide=False, dtype=torch.float32):
        if self.fill == "leavings" and name in self.leavings:
            return self._make(name, n, dtype, wide, leavings=self.leavings[name])
        return self._make(name, n, dtype, wide, fill=PATTERN[self.fill])

    def poison(self, name, pattern=NAN):
        self.all[name].refill(fill=pattern)

    def check(self):
        torch.cuda.synchronize()
        for g in self.all.values():
            g.check()


def execute(ctx, ep, fill, shift=0):
    """one run of an entry point through fresh guarded buffers: extents checked, outputs returned as integer arrays"""
    leav = None
    if fill == "leavings":
        key = (ep.__name__, ctx.config)
        if key not in _LEAVINGS:                                   # another batch, other parameters, the same entry point
            _, donor = execute(get_ctx("donor", "fused" if ctx.config == "fused" else "generic"), ep, "zero")
            _LEAVINGS[key] = {k: g.view.clone() for k, g in donor.all.items()}
        leav = _LEAVINGS[key]
    B = Bufs(fill, leav, shift)
    ctx.b.invalidate_inputs()                                      # (the fused path keys its copies of the inputs on pointer values)
    outs = ep(ctx, B)
    B.check()
    return {k: (g.bits() if isinstance(g, Guarded) else g) for k, g in outs.items()}, B


def fl(bits):
    return np.ascontiguousarray(bits).view(np.float32)


def all_finite(out, skip=()):
    for k, v in out.items():
        if v.dtype == np.int32 and k not in skip:
            assert np.isfinite(fl(v)).all(), f"{k} is not finite"


def contract(ctx, ep, anchor_check, skip_finite=()):
    """the anchor against the oracle, then every fill and the shifted run against the anchor, bit for bit"""
    anchor, _ = execute(ctx, ep, "zero")
    all_finite(anchor, skip_finite)
    anchor_check(anchor)
    for fill in FILLS:
        got, _ = execute(ctx, ep, fill)
        same_bits(got, anchor, f"{ctx.case} {ctx.config} {ep.__name__}: {fill}-filled buffers against zero-filled ones")
    got, _ = execute(ctx, ep, "nan", shift=4)
    same_bits(got, anchor, f"{ctx.case} {ctx.config} {ep.__name__}: 4-byte pointers shifted by one float")
    return anchor


# ---- the bars, from the files that own them ---------------------------------------------------------------------------
def check_step(out, r, yard, what, loss=True):
    close(fl(out["logits"]), r["logits"], RTOL_ACT, f"{what} logits")
    if loss:
        ls = float(fl(out["loss"])[0])
        assert abs(ls - r["loss"]) <= RTOL_ACT * abs(r["loss"]), f"{what} loss {ls} vs {r['loss']}"
    if "grads" in out:
        g = fl(out["grads"])
        close(g[grad_mask()], r["grads"][grad_mask()], RTOL_GRAD, f"{what} grads")
        gs.close_per_tensor(g, r["grads"], yard, f"{what} grads", max_exempt=PER_TENSOR_CAP)
        assert not g[conv_param_slice("gconv3_s2w")].any()


# ---- entry points: each takes (ctx, B), queues its calls and returns its outputs ---------------------------------------
def _model(ctx, B, params="ro"):
    P = (B.ro if params == "ro" else B.io)("params", ctx.flat, wide=True)
    return types.SimpleNamespace(P=P, x1=B.ro("x1", ctx.x1, wide=True), x2=B.ro("x2", ctx.x2, wide=True),
                                 ws=B.rw("ws", ctx.ws_floats, wide=True))


def ep_forward(ctx, B):
    m, z = _model(ctx, B), B.rw("logits", ctx.N)
    _lib.check(_lib.lib().mllp_gnn_forward(ctx.h, m.P.ptr, m.x1.ptr, m.x2.ptr, m.ws.ptr, z.ptr, _stream()))
    return {"logits": z}


def ep_forward_backward(ctx, B):
    m, z, dz, g = _model(ctx, B), B.rw("logits", ctx.N), B.ro("dlogits", ctx.dz), B.rw("grads", _lib.NUM_PARAMS)
    L = _lib.lib()
    _lib.check(L.mllp_gnn_forward(ctx.h, m.P.ptr, m.x1.ptr, m.x2.ptr, m.ws.ptr, z.ptr, _stream()))
    _lib.check(L.mllp_gnn_backward(ctx.h, m.P.ptr, m.x1.ptr, m.x2.ptr, m.ws.ptr, dz.ptr, g.ptr, _stream()))
    return {"logits": z, "grads": g}


def _loss_outputs(ctx, B):
    return B.ro("labels", ctx.y), B.rw("logits", ctx.N), B.rw("loss", 1), B.rw("grads", _lib.NUM_PARAMS)


def ep_loss_step(ctx, B):
    m = _model(ctx, B)
    y, z, ls, g = _loss_outputs(ctx, B)
    _lib.check(_lib.lib().mllp_gnn_loss_step(ctx.h, m.P.ptr, m.x1.ptr, m.x2.ptr, y.ptr, 1.0 / ctx.K, m.ws.ptr, z.ptr, ls.ptr,
                                             g.ptr, _stream()))
    return {"logits": z, "loss": ls, "grads": g}


def ep_loss_step_weighted(ctx, B):
    m = _model(ctx, B)
    y, z, ls, g = _loss_outputs(ctx, B)
    iw, pw, il, dz = B.ro("inst_weight", ctx.iw), B.ro("pos_weight", ctx.pw), B.rw("inst_loss", ctx.K), B.rw("dlogits", ctx.N)
    _lib.check(_lib.lib().mllp_gnn_loss_step_weighted(ctx.h, m.P.ptr, m.x1.ptr, m.x2.ptr, y.ptr, iw.ptr, pw.ptr, m.ws.ptr, z.ptr,
                                                      ls.ptr, il.ptr, g.ptr, dz.ptr, _stream()))
    return {"logits": z, "loss": ls, "inst_loss": il, "grads": g, "dlogits": dz}


def _input_grad_outputs(ctx, B):
    return B.rw("dx1", ctx.N), B.rw("dx2", ctx.M), B.rw("dvalues", ctx.nnz)


def ep_input_grads(ctx, B):
    """after a forward; d_grads = NULL, so the parameter gradients go to the scratch buffer"""
    m, z, dz = _model(ctx, B), B.rw("logits", ctx.N), B.ro("dlogits", ctx.dz)
    dx1, dx2, dv = _input_grad_outputs(ctx, B)
    L, n = _lib.lib(), ctypes.c_int64()
    _lib.check(L.mllp_gnn_input_grads_scratch_bytes(ctx.h, ctypes.byref(n)))
    sc = B.rw("scratch", n.value // 4)
    _lib.check(L.mllp_gnn_forward(ctx.h, m.P.ptr, m.x1.ptr, m.x2.ptr, m.ws.ptr, z.ptr, _stream()))
    _lib.check(L.mllp_gnn_input_grads(ctx.h, m.P.ptr, m.x1.ptr, m.x2.ptr, m.ws.ptr, dz.ptr, None, dx1.ptr, dx2.ptr, dv.ptr,
                                      sc.ptr, _stream()))
    torch.cuda.synchronize()
    return {"logits": z, "grads": sc.bits()[:_lib.NUM_PARAMS], "dx1": dx1, "dx2": dx2, "dvalues": dv}


def ep_loss_step_inputs(ctx, B):
    m = _model(ctx, B)
    y, z, ls, g = _loss_outputs(ctx, B)
    dx1, dx2, dv = _input_grad_outputs(ctx, B)
    _lib.check(_lib.lib().mllp_gnn_loss_step_inputs(ctx.h, m.P.ptr, m.x1.ptr, m.x2.ptr, y.ptr, 1.0 / ctx.K, m.ws.ptr, z.ptr,
                                                    ls.ptr, g.ptr, dx1.ptr, dx2.ptr, dv.ptr, _stream()))
    return {"logits": z, "loss": ls, "grads": g, "dx1": dx1, "dx2": dx2, "dvalues": dv}


def _adam(ctx, B):
    zeros = np.zeros(_lib.NUM_PARAMS, np.float32)
    return B.io("exp_avg", zeros), B.io("exp_avg_sq", zeros), B.io("state", _f32([0.0, 1e-3, 0.9, 0.999]))


def _train_steps(ctx, B, second_flags, poison_between):
    m = _model(ctx, B, params="io")
    y, z, ls, g = _loss_outputs(ctx, B)
    ea, es, st = _adam(ctx, B)
    L = _lib.lib()
    step = lambda flags: _lib.check(L.mllp_gnn_train_step(ctx.h, m.P.ptr, m.x1.ptr, m.x2.ptr, y.ptr, 1.0 / ctx.K, m.ws.ptr, z.ptr,  # noqa: E731
                                                          ls.ptr, g.ptr, ea.ptr, es.ptr, st.ptr, 1e-8, flags, _stream()))
    step(0)
    torch.cuda.synchronize()
    first = {"logits1": z.bits(), "loss1": ls.bits(), "grads1": g.bits()}
    if poison_between:
        B.poison("ws")
    step(second_flags)
    return dict(first, params=m.P, exp_avg=ea, exp_avg_sq=es, state=st, logits=z, loss=ls, grads=g)


def ep_train_step(ctx, B):
    """two consecutive steps, flags 0 then 1 (the second takes the folded weights the first left in the workspace)"""
    return _train_steps(ctx, B, 1, False)


def _small(mode):
    def ep(ctx, B):
        m = _model(ctx, B, params="io" if mode == "adam" else "ro")
        y, z, ls, g = _loss_outputs(ctx, B)
        ea, es, st = _adam(ctx, B) if mode == "adam" else (None, None, None)
        ptr = lambda t: None if t is None else t.ptr  # noqa: E731
        _lib.check(_lib.lib().mllp_gnn_train_step_small(ctx.h, m.P.ptr, m.x1.ptr, m.x2.ptr, y.ptr, 1.0 / ctx.K, m.ws.ptr, z.ptr,
                                                        ls.ptr, g.ptr, ptr(ea), ptr(es), ptr(st), 1e-8, _stream()))
        out = {"logits": z, "loss": ls, "grads": g}
        if mode == "adam":
            out.update(params=m.P, exp_avg=ea, exp_avg_sq=es, state=st)
        return out
    ep.__name__ = f"ep_small_{mode}"
    return ep


ep_small_loss, ep_small_adam = _small("loss"), _small("adam")


# ---- anchors ------------------------------------------------------------------------------------------------------------
def anchor_forward(ctx):
    r = refs(ctx.case)
    return lambda out: check_step(out, r.step, r.yard, f"{ctx.case} {ctx.config} forward", loss=False)


def anchor_forward_backward(ctx):
    r = refs(ctx.case)
    return lambda out: check_step(out, r.dz, r.yard_dz, f"{ctx.case} {ctx.config} forward + backward", loss=False)


def anchor_loss_step(ctx):
    r = refs(ctx.case)
    return lambda out: check_step(out, r.step, r.yard, f"{ctx.case} {ctx.config} loss step")


def anchor_weighted(ctx):
    """the bars of tests/test_weighted_loss.py::test_whole_step_both_paths, and its 1e-5 for dlogits"""
    r = refs(ctx.case)

    def check(out):
        ref, keep = r.wl, grad_mask()
        close(fl(out["logits"]), r.step["logits"], RTOL_ACT, "logits")
        close(fl(out["loss"]), np.array([ref["loss"]]), RTOL_ACT, "loss")
        close(fl(out["inst_loss"]), ref["inst_loss"], RTOL_ACT, "inst_loss")
        close(fl(out["dlogits"]), ref["dz"], 1e-5, "dlogits")
        close(fl(out["grads"])[keep], r.wl_grads[keep], RTOL_GRAD, "grads")
        off = np.concatenate([[0], np.cumsum(r.seg_n)])
        for k in np.flatnonzero(ctx.iw == 0):
            assert not fl(out["dlogits"])[off[k]:off[k + 1]].any()      # weight 0: exactly no gradient
    return check


def _four(out):
    return tuple(torch.from_numpy(fl(out[k]).copy()) for k in ("grads", "dx1", "dx2", "dvalues"))


def anchor_input_grads(ctx):
    r = refs(ctx.case)

    def check(out):
        close(fl(out["logits"]), r.step["logits"], RTOL_OUT, "logits")
        _check_four(_four(out), r.ig_dz[1:], f"{ctx.case} {ctx.config} input_grads")
    return check


def anchor_loss_step_inputs(ctx):
    r = refs(ctx.case)

    def check(out):
        check_step(out, r.step, r.yard, f"{ctx.case} {ctx.config} loss_step_inputs")
        assert abs(float(fl(out["loss"])[0]) - r.ig_loss[0]) < RTOL_OUT * abs(r.ig_loss[0])
        _check_four(_four(out), r.ig_loss[1:], f"{ctx.case} {ctx.config} loss_step_inputs")
    return check


def anchor_train(ctx, steps):
    """first step: the loss step's bars; the trajectory: the bars of test_small_step.test_reference_loop_20_adam_steps
    (every loss within 1e-5 relative, the parameters that receive gradient within 1e-4 absolute)"""
    r = refs(ctx.case)

    def check(out):
        if steps == 2:
            check_step(dict(logits=out["logits1"], loss=out["loss1"], grads=out["grads1"]), r.step, r.yard, "first step")
        else:
            check_step(out, r.step, r.yard, "the step")
        got = [float(fl(out["loss1"])[0]), float(fl(out["loss"])[0])] if steps == 2 else [float(fl(out["loss"])[0])]
        np.testing.assert_allclose(got, r.adam_losses[:steps], rtol=1e-5, atol=0)
        assert float(fl(out["state"])[0]) == float(steps)
        if steps == 2:
            dw = np.abs(fl(out["params"]).astype(np.float64) - r.adam_params)[grad_mask()]
            assert dw.max() < 1e-4
        unused = conv_param_slice("gconv3_s2w")
        assert np.array_equal(fl(out["params"])[unused], ctx.flat[unused])
        assert not fl(out["exp_avg"])[unused].any() and not fl(out["exp_avg_sq"])[unused].any()
    return check


MODEL_EPS = {
    "forward": (ep_forward, anchor_forward),
    "forward_backward": (ep_forward_backward, anchor_forward_backward),
    "loss_step": (ep_loss_step, anchor_loss_step),
    "loss_step_weighted": (ep_loss_step_weighted, anchor_weighted),
    "input_grads": (ep_input_grads, anchor_input_grads),
    "loss_step_inputs": (ep_loss_step_inputs, anchor_loss_step_inputs),
    "train_step": (ep_train_step, lambda ctx: anchor_train(ctx, 2)),
}


@gpu
@pytest.mark.parametrize("name", list(MODEL_EPS))
@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("case", CASES)
def test_whole_model_calls(case, config, name):
    ctx = get_ctx(case, config)
    ep, anchor = MODEL_EPS[name]
    contract(ctx, ep, anchor(ctx))


@gpu
@pytest.mark.parametrize("mode", ["loss", "adam"])
@pytest.mark.parametrize("case", ["holes", "one"])
def test_small_step(case, mode):
    ctx = get_ctx(case, "generic")          # (the kernel reads the plain arrays, whatever path is set)
    assert ctx.b.small_step_fits()
    if mode == "loss":
        contract(ctx, ep_small_loss, anchor_loss_step(ctx))
    else:
        contract(ctx, ep_small_adam, anchor_train(ctx, 1))


# ---- clause 4: the workspace clobbered between whole calls --------------------------------------------------------------
def _loss_step_then_forward(poison):
    def ep(ctx, B):
        out = ep_loss_step(ctx, B)
        if poison:
            B.poison("ws")
        z2, a = B.rw("logits2", ctx.N), B.all
        _lib.check(_lib.lib().mllp_gnn_forward(ctx.h, a["params"].ptr, a["x1"].ptr, a["x2"].ptr, a["ws"].ptr, z2.ptr, _stream()))
        return {"logits": z2}
    ep.__name__ = "ep_loss_step_then_forward"
    return ep


@gpu
@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("case", CASES)
def test_forward_after_a_loss_step_on_a_clobbered_workspace(case, config):
    ctx = get_ctx(case, config)
    anchor, _ = execute(ctx, ep_forward, "zero")
    anchor_forward(ctx)(anchor)
    got, _ = execute(ctx, _loss_step_then_forward(True), "zero")
    same_bits(got, anchor, "forward after loss_step + 0xFFFFFFFF over the workspace")


@gpu
@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("case", CASES)
def test_train_step_flags_0_on_a_clobbered_workspace(case, config):
    """step, poison, step with flags 0 == step, step with flags 1 on an untouched workspace: parameters, moments, step
    count, loss, logits (and gradients), bit for bit"""
    ctx = get_ctx(case, config)
    carried, _ = execute(ctx, ep_train_step, "zero")
    anchor_train(ctx, 2)(carried)

    def ep_poisoned(c, B):
        return _train_steps(c, B, 0, True)
    got, _ = execute(ctx, ep_poisoned, "zero")
    same_bits(got, carried, "step, poison, step(flags 0) against step, step(flags 1)")


@gpu
@pytest.mark.parametrize("path", ["fused", "generic"])
@pytest.mark.parametrize("case", ["holes", "one"])
def test_loss_step_after_a_small_step_on_a_clobbered_workspace(case, path):
    ctx = get_ctx(case, path)
    anchor, _ = execute(ctx, ep_loss_step, "zero")
    anchor_loss_step(ctx)(anchor)

    def ep(c, B):
        m = _model(c, B)
        y = B.ro("labels", c.y)
        z0, l0, g0 = B.rw("logits0", c.N), B.rw("loss0", 1), B.rw("grads0", _lib.NUM_PARAMS)
        L = _lib.lib()
        _lib.check(L.mllp_gnn_train_step_small(c.h, m.P.ptr, m.x1.ptr, m.x2.ptr, y.ptr, 1.0 / c.K, m.ws.ptr, z0.ptr, l0.ptr,
                                               g0.ptr, None, None, None, 1e-8, _stream()))
        B.poison("ws")
        z, ls, g = B.rw("logits", c.N), B.rw("loss", 1), B.rw("grads", _lib.NUM_PARAMS)
        _lib.check(L.mllp_gnn_loss_step(c.h, m.P.ptr, m.x1.ptr, m.x2.ptr, y.ptr, 1.0 / c.K, m.ws.ptr, z.ptr, ls.ptr, g.ptr,
                                        _stream()))
        return {"logits": z, "loss": ls, "grads": g}
    got, _ = execute(ctx, ep, "zero")
    same_bits(got, anchor, "loss_step after train_step_small + 0xFFFFFFFF over the workspace")


# ---- the calls beside the model -----------------------------------------------------------------------------------------
def ep_weighted_loss(ctx, B):
    r = refs(ctx.case)
    z, y = B.ro("logits", _f32(r.step["logits"])), B.ro("labels", ctx.y)
    iw, pw = B.ro("inst_weight", ctx.iw), B.ro("pos_weight", ctx.pw)
    dz, il, ls, bal = B.rw("dlogits", ctx.N), B.rw("inst_loss", ctx.K), B.rw("loss", 1), B.rw("balanced", ctx.K)
    L = _lib.lib()
    _lib.check(L.mllp_weighted_loss(ctx.h, z.ptr, y.ptr, iw.ptr, pw.ptr, dz.ptr, il.ptr, ls.ptr, _stream()))
    _lib.check(L.mllp_balanced_pos_weight(ctx.h, y.ptr, bal.ptr, _stream()))
    return {"dlogits": dz, "inst_loss": il, "loss": ls, "balanced": bal}


def ep_topm(ctx, B):
    r = refs(ctx.case)
    z, y = B.ro("logits", _f32(r.step["logits"])), B.ro("labels", ctx.y)
    L, n = _lib.lib(), ctypes.c_int64()
    _lib.check(L.mllp_metrics_scratch_bytes(ctx.h, ctypes.byref(n)))
    sc, met = B.rw("scratch", n.value // 4), B.rw("metrics", 2 * ctx.K)
    mask, index, stats = B.rw("mask", ctx.N, dtype=torch.uint8), B.rw("index", ctx.M, dtype=torch.int32), B.rw("stats", 2 * ctx.K)
    _lib.check(L.mllp_topm_metrics(ctx.h, z.ptr, y.ptr, sc.ptr, met.ptr, _stream()))
    _lib.check(L.mllp_topm_select(ctx.h, z.ptr, mask.ptr, index.ptr, stats.ptr, _stream()))
    return {"metrics": met, "mask": mask, "index": index, "stats": stats}


def anchor_weighted_loss(ctx):
    """bars of tests/test_weighted_loss.py: test_kernel_alone_against_oracle, test_balanced_pos_weight (one ulp)"""
    r = refs(ctx.case)

    def check_wl(out):
        close(fl(out["inst_loss"]), r.wl["inst_loss"], RTOL_ACT, "inst_loss")
        close(fl(out["loss"]), np.array([r.wl["loss"]]), RTOL_ACT, "loss")
        close(fl(out["dlogits"]), r.wl["dz"], 1e-5, "dlogits")
        want = oracle_balanced(r.ob.basis, r.seg_n).astype(np.float32)
        ulp = np.abs(out["balanced"].astype(np.int64) - want.view(np.int32).astype(np.int64))
        assert ulp.max() <= 1, ulp
    return check_wl


def anchor_topm(ctx):
    """metrics as tests/test_hip_parity.py::test_whole_model_against_golden checks them; selection: exact"""
    r = refs(ctx.case)

    def check_topm(out):
        z = _f32(r.step["logits"])
        met, off = fl(out["metrics"]).reshape(-1, 2), np.concatenate([[0], np.cumsum(r.seg_n)])
        for k, i in enumerate(ctx.insts):
            order = np.argsort(-z[off[k]:off[k + 1]].astype(np.float64), kind="stable")[:i.m]
            tp = float(i.basis[order].sum())
            assert met[k, 0] == tp, i.name
            f1 = 0.0 if tp == 0 else 2 * tp / (2 * tp + (len(order) - tp) + (i.basis.sum() - tp))
            assert abs(met[k, 1] - f1) < 1e-5
        mask, index, stats = oracle_select(z, r.seg_n, r.seg_m)
        assert np.array_equal(out["mask"], mask) and np.array_equal(out["index"], index)
        assert np.array_equal(out["stats"], stats.reshape(-1).view(np.int32))
    assert all(i.m <= i.n for i in ctx.insts)
    return check_topm


@gpu
@pytest.mark.parametrize("case", CASES)
def test_loss_head_metrics_and_selection(case):
    ctx = get_ctx(case, "generic")
    contract(ctx, ep_weighted_loss, anchor_weighted_loss(ctx))
    contract(ctx, ep_topm, anchor_topm(ctx), skip_finite=("stats", "index"))


TCONVS = {"cin1": ("gconv1_w2s", True, 1), "cin16": ("gconv2_s2w", False, 16)}
TCONV_KEYS = ("lin_key.weight", "lin_key.bias", "lin_query.weight", "lin_query.bias", "lin_value.weight", "lin_value.bias",
              "lin_edge.weight", "lin_skip.weight", "lin_skip.bias")


def _tconv_inputs(ctx, which):
    name, dst_is_var, cin = TCONVS[which]
    nd, ns = (ctx.N, ctx.M) if dst_is_var else (ctx.M, ctx.N)
    seed = getattr(ctx, "data_seed", 0)     # the second data set of tests/test_stream_contract.py: other inputs, and dh x 0.25
    rng = np.random.default_rng(3 + seed)   # beside its parameters x 1.25 (lin_key.bias's bar is absolute, its noise scales with dh)
    return name, dst_is_var, cin, nd, ns, _f32(rng.standard_normal((ns, cin))), _f32(rng.standard_normal((nd, cin))), \
        _f32(rng.standard_normal((nd, 16)) * (0.25 if seed else 1.0))


def _tconv(which):
    def ep(ctx, B):
        name, dst_is_var, cin, nd, ns, xs, xd, dh = _tconv_inputs(ctx, which)
        L, n = _lib.lib(), ctypes.c_int64()
        _lib.check(L.mllp_tconv_workspace_floats(ctx.h, int(dst_is_var), cin, ctypes.byref(n)))
        cp = B.ro("conv_params", ctx.flat[conv_param_slice(name)], wide=True)
        x_src, x_dst = B.ro("x_src", xs, wide=True), B.ro("x_dst", xd, wide=True)
        ws, h = B.rw("ws", n.value, wide=True), B.rw("h", nd * 16, wide=True)
        _lib.check(L.mllp_tconv_fwd(ctx.h, int(dst_is_var), cin, cp.ptr, x_src.ptr, x_dst.ptr, h.ptr, ws.ptr, _stream()))
        torch.cuda.synchronize()
        d = B.io("dh", dh, wide=True)
        pg = B.rw("param_grads", cp.n)
        out = {"h": h, "h_before_bwd": h.bits(), "dh": d, "param_grads": pg}
        dxd = dxs = None
        if cin == 16:
            dxd, dxs = B.rw("dx_dst", nd * 16, wide=True), B.rw("dx_src", ns * 16, wide=True)
            out.update(dx_dst=dxd, dx_src=dxs)
        _lib.check(L.mllp_tconv_bwd(ctx.h, int(dst_is_var), cin, cp.ptr, x_src.ptr, x_dst.ptr, h.ptr, ws.ptr, d.ptr,
                                    dxd.ptr if dxd else None, dxs.ptr if dxs else None, 0, pg.ptr, _stream()))
        return out
    ep.__name__ = f"ep_tconv_{which}"
    return ep


def anchor_tconv(ctx, which, reads_h=True):
    """the bars of tests/test_hip_parity.py::test_single_layer_forward_backward (reads_h: the entry point read h back
    between the forward and the backward)"""
    r = refs(ctx.case)
    name, dst_is_var, cin, nd, ns, xs, xd, dh = _tconv_inputs(ctx, which)
    p = o2.conv_params(r.sd, name)
    ptr, idx, val, _, _ = r.ob.orient(dst_is_var)
    f64 = lambda a: a.astype(np.float64)  # noqa: E731
    h_ref, saved = o2.conv_fwd(p, ptr, idx, val, f64(xs), f64(xd))
    grads, dxd, dxs, inter = o2.conv_bwd(p, ptr, idx, val, f64(xs), f64(xd), saved, f64(dh), need_input_grads=(cin == 16))

    def check(out):
        close(fl(out["h"]).reshape(nd, 16), h_ref, RTOL_ACT, "h")
        if reads_h:
            assert np.array_equal(out["h"], out["h_before_bwd"])        # d_h_out is an input of the backward
        close(fl(out["dh"]).reshape(nd, 16), inter["g"], 1e-7, "masked dh")
        if cin == 16:
            close(fl(out["dx_dst"]).reshape(nd, 16), dxd, RTOL_GRAD, "dx_dst")
            close(fl(out["dx_src"]).reshape(ns, 16), dxs, RTOL_GRAD, "dx_src")
        pg, o3 = fl(out["param_grads"]), 0
        for key in TCONV_KEYS:
            ref = np.asarray(grads[key]).reshape(-1)
            if key == "lin_key.bias":
                assert np.abs(pg[o3:o3 + ref.size]).max() < 1e-5
            else:
                close(pg[o3:o3 + ref.size], ref, RTOL_GRAD, key)
            o3 += ref.size
        assert o3 == pg.size
    return check


@gpu
@pytest.mark.parametrize("which", list(TCONVS))
@pytest.mark.parametrize("config", CONFIGS[1:])
@pytest.mark.parametrize("case", CASES)
def test_single_conv(case, config, which):
    """mllp_tconv_fwd + _bwd on one workspace"""
    ctx = get_ctx(case, config)
    contract(ctx, _tconv(which), anchor_tconv(ctx, which))


def _spmm(transpose):
    def ep(ctx, B):
        n_in, n_out = (ctx.M, ctx.N) if transpose else (ctx.N, ctx.M)
        H = B.ro("H", _f32(np.random.default_rng(1 + getattr(ctx, "data_seed", 0)).standard_normal((n_in, 16))), wide=True)
        Y = B.rw("Y", n_out * 16, wide=True)
        _lib.check(_lib.lib().mllp_spmm_csr_f32(ctx.h, int(transpose), H.ptr, Y.ptr, _stream()))
        return {"Y": Y}
    ep.__name__ = f"ep_spmm_{int(transpose)}"
    return ep


def anchor_spmm(ctx, transpose, rtol=1e-6):
    """the bar of tests/test_hip_parity.py::test_spmm_both_orientations"""
    ob = refs(ctx.case).ob
    n_in = ctx.M if transpose else ctx.N
    H = _f32(np.random.default_rng(1 + getattr(ctx, "data_seed", 0)).standard_normal((n_in, 16))).astype(np.float64)
    ptr, idx, val = (ob.cp, ob.ri, ob.cv) if transpose else (ob.rp, ob.ci, ob.va)
    want = o2.spmm(ptr, idx, val.astype(np.float32).astype(np.float64), H)
    return lambda out: close(fl(out["Y"]).reshape(want.shape), want, rtol, "A H")


@gpu
@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_spmm(case, transpose):
    ctx = get_ctx(case, "generic")
    contract(ctx, _spmm(transpose), anchor_spmm(ctx, transpose))


def ep_normalize(ctx, B):
    """x1, x2 in place and both scale outputs, on a batch of its own (the call rewrites the batch's values)"""
    from mllp_amd.graph import LPBatch
    pert, _ = _perturbed_list(ctx.insts)
    b = LPBatch.from_instances(pert)
    x1, x2 = B.io("x1", _f32(np.concatenate([p.coefs for p in pert]))), B.io("x2", _f32(np.concatenate([p.rhs for p in pert])))
    rs, os_ = B.rw("row_scale", ctx.M), B.rw("obj_scale", ctx.K)
    _lib.check(_lib.lib().mllp_graph_normalize(b._h, x1.ptr, x2.ptr, 5.0, 0, rs.ptr, os_.ptr, _stream()))
    torch.cuda.synchronize()
    return {"x1": x1, "x2": x2, "row_scale": rs, "obj_scale": os_, "values": b.export(2).view(np.int32)}


@gpu
@pytest.mark.parametrize("case", CASES)
def test_normalize(case):
    """against tests/test_normalize.py's fp64 statement of the rule, at its bar (1e-5 of each tensor's maximum)"""
    ctx = get_ctx(case, "generic")
    pert, _ = _perturbed_list(ctx.insts)
    want = [np.concatenate([np.atleast_1d(_normalize_host(p, np.float64)[k]) for p in pert]) for k in range(5)]

    def check(out):
        for k, name in enumerate(("values", "x1", "x2", "row_scale", "obj_scale")):
            norm_close(fl(out[name]), want[k], f"{case} {name}")
    contract(ctx, ep_normalize, check)


# ---- alignment: the refusal writes nothing ------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("config", ["fused", "generic"])
def test_misaligned_workspace_is_refused_and_nothing_is_written(config):
    """a real graph, sentinel-filled outputs and workspace: MLLP_EINVAL, every byte as it was; the batch works afterwards.
    (No misaligned pointer ever reaches a kernel: the refusal is the whole call.)"""
    ctx = get_ctx("one", config)
    L = _lib.lib()
    B = Bufs("huge", shift=4)
    m = _model(ctx, B)
    off_ws = B.rw("ws_off", ctx.ws_floats + 1)                    # a buffer of the right size, one float off
    assert off_ws.view.data_ptr() % 16 == 4 and m.ws.view.data_ptr() % 16 == 0
    off_x1 = B.ro("x1_off", ctx.x1)
    y, z, ls, g = _loss_outputs(ctx, B)
    dz = B.ro("dlogits", ctx.dz)
    ea, es, st = _adam(ctx, B)
    before = {k: v.bits() for k, v in B.all.items()}
    s = _stream()
    calls = {
        "forward": lambda ws, x1: L.mllp_gnn_forward(ctx.h, m.P.ptr, x1, m.x2.ptr, ws, z.ptr, s),
        "backward": lambda ws, x1: L.mllp_gnn_backward(ctx.h, m.P.ptr, x1, m.x2.ptr, ws, dz.ptr, g.ptr, s),
        "loss_step": lambda ws, x1: L.mllp_gnn_loss_step(ctx.h, m.P.ptr, x1, m.x2.ptr, y.ptr, 1.0, ws, z.ptr, ls.ptr, g.ptr, s),
        "loss_step_weighted": lambda ws, x1: L.mllp_gnn_loss_step_weighted(ctx.h, m.P.ptr, x1, m.x2.ptr, y.ptr, None, None, ws,
                                                                           z.ptr, ls.ptr, None, g.ptr, z.ptr, s),
        "input_grads": lambda ws, x1: L.mllp_gnn_input_grads(ctx.h, m.P.ptr, x1, m.x2.ptr, ws, dz.ptr, g.ptr, None, None, None,
                                                             None, s),
        "loss_step_inputs": lambda ws, x1: L.mllp_gnn_loss_step_inputs(ctx.h, m.P.ptr, x1, m.x2.ptr, y.ptr, 1.0, ws, z.ptr, ls.ptr,
                                                                       g.ptr, None, None, None, s),
        "train_step": lambda ws, x1: L.mllp_gnn_train_step(ctx.h, m.P.ptr, x1, m.x2.ptr, y.ptr, 1.0, ws, z.ptr, ls.ptr, g.ptr,
                                                           ea.ptr, es.ptr, st.ptr, 1e-8, 0, s),
        "train_step_small": lambda ws, x1: L.mllp_gnn_train_step_small(ctx.h, m.P.ptr, x1, m.x2.ptr, y.ptr, 1.0, ws, z.ptr, ls.ptr,
                                                                       g.ptr, ea.ptr, es.ptr, st.ptr, 1e-8, s),
    }
    for name, call in calls.items():
        for ws, x1 in ((off_ws.ptr, m.x1.ptr), (m.ws.ptr, off_x1.ptr)):
            assert call(ws, x1) == EINVAL, name
            assert b"misaligned" in L.mllp_last_error(), name
    B.check()
    same_bits({k: v.bits() for k, v in B.all.items()}, before, "refused calls wrote something")
    anchor, _ = execute(ctx, ep_loss_step, "zero")
    anchor_loss_step(ctx)(anchor)
