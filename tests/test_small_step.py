"""The one-launch training step of a small batch (mllp_gnn_train_step_small, csrc/small_step.hip): limits without a GPU;
on the GPU the loss step against the fp64 oracle, the reference's per-instance Adam loop, bitwise repeatability and
capture, refusals, the library's forgotten state.  (No trainer or driver option uses the call: DESIGN.md section 4.8.)"""
import ctypes
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fused_cases as fc  # noqa: E402
import grad_scales as gs  # noqa: E402
from mllp_amd import _lib  # noqa: E402
from mllp_amd._lib import conv_param_slice  # noqa: E402
from mllp_amd.data import SUBSET5, LPInstance, load_packed  # noqa: E402
from oracle import pyg_restatement as o1  # noqa: E402
from oracle import spmm_form as o2  # noqa: E402
from test_hip_parity import RTOL_ACT, RTOL_GRAD, close, grad_mask  # noqa: E402

FLOOR_NODES, FLOOR_NNZ = 2048, 8192
MLLP_EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _limits(lib):
    out = (ctypes.c_int64 * 4)()
    assert lib.mllp_gnn_small_step_limits(out) == 0
    return list(out)


# ---- without a GPU ---------------------------------------------------------------------------------------------------
def test_limits_answer_and_respect_the_floor(lib):
    nodes, nnz, threads, lds = _limits(lib)
    assert nodes >= FLOOR_NODES and nnz >= FLOOR_NNZ
    assert threads in (768, 1024)
    assert 0 < lds <= 160 * 1024
    assert lib.mllp_gnn_small_step_limits(None) == MLLP_EINVAL and b"null" in lib.mllp_last_error()
    from mllp_amd.graph import small_step_limits
    assert small_step_limits() == dict(max_nodes=nodes, max_nnz=nnz, threads=threads, lds_bytes=lds)


def test_null_arguments_are_refused_without_a_gpu(lib):
    fits = ctypes.c_int(7)
    assert lib.mllp_gnn_small_step_fits(None, ctypes.byref(fits)) == MLLP_EINVAL and b"null" in lib.mllp_last_error()
    assert lib.mllp_gnn_train_step_small(None, None, None, None, None, 1.0, None, None, None, None, None, None, None, 1e-8,
                                         None) == MLLP_EINVAL
    assert b"null" in lib.mllp_last_error()


def test_netlib_instances_of_the_floor_are_eligible(lib):
    nodes, nnz = _limits(lib)[:2]
    insts = load_packed()
    assert len(insts) == 97
    floor = [i for i in insts if i.m + i.n <= FLOOR_NODES and i.nnz <= FLOOR_NNZ]
    eligible = [i for i in insts if i.m + i.n <= nodes and i.nnz <= nnz]
    assert len(floor) >= 50                     # most of Netlib is small: the median instance has 4 756 nonzeros
    assert {i.name for i in floor} <= {i.name for i in eligible}


# ---- on the GPU ------------------------------------------------------------------------------------------------------
def _sd(golden):
    return {k: v.numpy() for k, v in o1.unflatten_state(torch.tensor(golden["weights_flat"])).items()}


def _params(sd):
    flat = o1.flatten_state({k: torch.as_tensor(v) for k, v in sd.items()}).numpy()
    return torch.tensor(flat, dtype=torch.float32, device="cuda")


from fused_cases import SMALL_CASE_NAMES as CASE_NAMES  # noqa: E402
from fused_cases import SMALL_PER_TENSOR_CAPS as PER_TENSOR_CAPS  # noqa: E402
from fused_cases import small_inst as _inst  # noqa: E402
from fused_cases import small_long as _long  # noqa: E402
from fused_cases import small_step_cases as _cases  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    _lib.lib()
    assert torch.cuda.is_available()
    from mllp_amd.graph import LPBatch
    return LPBatch


@pytest.fixture(scope="module")
def oracle_cases(golden, subset5):
    """name -> (sd, instances, oracle result, per-tensor yardstick): computed once, shared, never modified"""
    out = {}
    for name, sd, insts in _cases(golden, subset5):
        ob = o2.BatchCSR(insts)
        out[name] = (sd, insts, o2.gnn_forward_backward(sd, ob), gs.yardstick(sd, ob) if name in PER_TENSOR_CAPS else None)
    assert list(out) == CASE_NAMES
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_loss_step_against_oracle(dev, oracle_cases, name):
    """Loss-step mode (no optimizer buffers) against oracle.spmm_form.gnn_forward_backward in fp64: logits and loss at
    1e-5, gradients at 5e-5, max-norm relative (test_hip_parity's bars)."""
    sd, insts, r, yard = oracle_cases[name]
    b = dev.from_instances(insts)
    assert b.small_step_fits(), f"{name}: M + N = {b.M + b.N}, nnz = {b.nnz} is beyond the limits"
    p = _params(sd)
    p0 = p.clone()
    loss, logits, grads = b.train_step_small(p)
    torch.cuda.synchronize()
    assert torch.equal(p, p0)                               # the loss step leaves the parameters alone
    lg, ls, g = logits.cpu().numpy(), float(loss[0]), grads.cpu().numpy()
    scale = max(float(np.abs(r["logits"]).max()), 1e-30)
    print(f"{name}: logits {np.abs(lg - r['logits']).max() / scale:.2e}, loss {abs(ls - r['loss']) / abs(r['loss']):.2e}, "
          f"grads {np.abs(g - r['grads']).max() / np.abs(r['grads']).max():.2e}")
    close(lg, r["logits"], RTOL_ACT, f"{name} logits")
    assert abs(ls - r["loss"]) <= RTOL_ACT * abs(r["loss"]), f"{name} loss {ls} vs {r['loss']}"
    close(g, r["grads"], RTOL_GRAD, f"{name} grads")
    if yard is not None:
        gs.close_per_tensor(g, r["grads"], yard, f"{name} grads", max_exempt=PER_TENSOR_CAPS[name])
    unused = conv_param_slice("gconv3_s2w")
    assert not g[unused].any()


def _adam_buffers(p):
    return (torch.zeros_like(p), torch.zeros_like(p), torch.tensor([0.0, 1e-3, 0.9, 0.999], device=p.device))


@pytest.mark.gpu
def test_reference_loop_20_adam_steps(dev, golden, subset5):
    """The reference's loop (one Adam step per instance, linear_program_experiment.py:123-144): 20 steps cycling over the
    five golden singles against the oracle's adam_step trajectory in fp64, through the one-launch step and through
    mllp_gnn_train_step.  Tolerance of test_hip_parity.test_cfg2_trajectory_100_adam_steps_vs_oracle: every loss within
    1e-5 relative, the parameters that receive gradient (grad_mask) within 1e-4 absolute."""
    flat = np.asarray(golden["weights_flat"], dtype=np.float64)
    P, m, v = flat.copy(), np.zeros_like(flat), np.zeros_like(flat)
    batches = [o2.BatchCSR([i]) for i in subset5]
    want = []
    for step in range(1, 21):
        sd = {k: t.numpy() for k, t in o1.unflatten_state(torch.tensor(P)).items()}
        r = o2.gnn_forward_backward(sd, batches[(step - 1) % 5])
        want.append(r["loss"])
        o2.adam_step(P, r["grads"], m, v, step)
    singles = [dev.from_instances([i]) for i in subset5]
    assert all(b.small_step_fits() for b in singles)
    unused, keep = conv_param_slice("gconv3_s2w"), grad_mask()
    for which in ("small", "train_step"):
        p = torch.tensor(flat, dtype=torch.float32, device="cuda")
        p0 = p.clone()
        ea, es, st = _adam_buffers(p)
        got = []
        for step in range(20):
            b = singles[step % 5]
            if which == "small":
                loss, _, grads = b.train_step_small(p, ea, es, st)
            else:
                loss, _, grads = b.train_step(p, ea, es, st)
            got.append(float(loss[0]))
        dw = np.abs(p.cpu().numpy().astype(np.float64) - P)[keep]
        print(f"{which}: loss deviation {np.max(np.abs(np.array(got) - want) / np.abs(want)):.2e}, max |dw| {dw.max():.2e}")
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=0)
        assert dw.max() < 1e-4
        assert float(st[0]) == 20.0
        assert torch.equal(p[unused], p0[unused])           # never called: zero gradient, zero moments, no movement
        assert not grads[unused].any() and not ea[unused].any() and not es[unused].any()


def _step_bytes(b, flat, n=1, capture=False):
    p = torch.tensor(flat, dtype=torch.float32, device="cuda")
    ea, es, st = _adam_buffers(p)
    logits, loss = torch.empty(b.N, device="cuda"), torch.zeros(1, device="cuda")
    grads = torch.empty(_lib.NUM_PARAMS, device="cuda")
    run = lambda: b.train_step_small(p, ea, es, st, logits=logits, loss=loss, grads=grads)  # noqa: E731
    if capture:
        b.workspace()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            run()
        for _ in range(n):
            g.replay()
    else:
        for _ in range(n):
            run()
    torch.cuda.synchronize()
    return [t.cpu().numpy().tobytes() for t in (logits, loss, grads, p, ea, es, st)]


@pytest.mark.gpu
def test_bitwise_repeatable_and_capturable(dev, golden, subset5):
    flat = golden["weights_flat"]
    for insts in ([subset5[0]], [_long(False)], subset5[1:4]):
        b = dev.from_instances(insts)
        first = _step_bytes(b, flat, n=2)
        assert first == _step_bytes(b, flat, n=2)
        assert first == _step_bytes(b, flat, n=2, capture=True)


def _args(b, p, ea, es, st, logits, loss, grads):
    return (b._h, _lib.ptr(p), _lib.ptr(b.x1), _lib.ptr(b.x2), _lib.ptr(b.labels), 1.0, _lib.ptr(b.workspace()),
            _lib.ptr(logits), _lib.ptr(loss), _lib.ptr(grads), _lib.ptr(ea), _lib.ptr(es), _lib.ptr(st), 1e-8,
            _lib.current_stream())


@pytest.mark.gpu
def test_refusals(dev, golden, lib):
    max_nodes, max_nnz = _limits(lib)[:2]
    rng = np.random.default_rng(0)
    # max_nnz + 1 nonzeros on few nodes; max_nodes + 1 nodes with few nonzeros
    rows = 16
    degs = [(max_nnz + 1) // rows + (1 if i < (max_nnz + 1) % rows else 0) for i in range(rows)]
    too_dense = _inst(fc.block_of(degs, max(degs) + 5, rng), "dense", 1)
    m = 8
    too_wide = _inst(sp.csr_matrix((np.ones(m), (np.arange(m), np.arange(m))), shape=(m, max_nodes + 1 - m)), "wide", 2)
    p = torch.tensor(golden["weights_flat"], dtype=torch.float32, device="cuda")
    p0 = p.clone()
    ea, es, st = _adam_buffers(p)
    for inst, limit in ((too_dense, max_nnz), (too_wide, max_nodes)):
        b = dev.from_instances([inst])
        assert b.nnz == max_nnz + 1 or b.M + b.N == max_nodes + 1          # one above a limit, within the other
        assert not b.small_step_fits()
        logits, loss, grads = torch.empty(b.N, device="cuda"), torch.zeros(1, device="cuda"), torch.zeros(4721, device="cuda")
        assert lib.mllp_gnn_train_step_small(*_args(b, p, ea, es, st, logits, loss, grads)) == MLLP_EINVAL
        assert str(limit).encode() in lib.mllp_last_error()
        with pytest.raises(_lib.MllpError):
            b.train_step_small(p, ea, es, st)
        torch.cuda.synchronize()
        assert torch.equal(p, p0) and float(st[0]) == 0.0 and not grads.any()
    b = dev.from_instances(load_packed(["afiro.mps"]))
    logits, loss, grads = torch.empty(b.N, device="cuda"), torch.zeros(1, device="cuda"), torch.zeros(4721, device="cuda")
    for given in ((ea, None, None), (None, es, st), (ea, es, None), (ea, None, st)):
        assert lib.mllp_gnn_train_step_small(*_args(b, p, *given, logits, loss, grads)) == MLLP_EINVAL
    torch.cuda.synchronize()
    assert torch.equal(p, p0)


@pytest.mark.gpu
def test_no_stale_state_after_a_small_step(dev, golden, subset5):
    flat = golden["weights_flat"]

    def run(with_small):
        b = dev.from_instances(subset5[:2])
        p = torch.tensor(flat, dtype=torch.float32, device="cuda")
        ea, es, st = _adam_buffers(p)
        b.train_step(p, ea, es, st, param_gen=0)            # leaves the next step's folded weights in the workspace
        if with_small:
            q = p.clone()
            b.train_step_small(q)                           # loss step on a copy: p itself is unchanged
        loss, logits, grads = b.train_step(p, ea, es, st, param_gen=1)
        torch.cuda.synchronize()
        return [t.cpu().numpy().tobytes() for t in (loss, logits, grads, p, ea, es)]

    assert run(True) == run(False)
    b = dev.from_instances(subset5[:2])
    p = torch.tensor(flat, dtype=torch.float32, device="cuda")
    logits = b.forward(p)
    b.train_step_small(p)
    with pytest.raises(_lib.MllpError, match="forward"):
        b.backward(p, torch.ones_like(logits))


@pytest.mark.gpu
def test_library_drops_its_folded_weights_record(dev, golden, subset5, lib):
    """The C ABI itself, without LPBatch's own book-keeping: after mllp_gnn_train_step has left the next step's folded
    weights in the workspace, a one-launch Adam step on the same workspace and parameters moves the parameters; a following
    mllp_gnn_train_step that CLAIMS current folds (flags bit 0) must fold again and give the bytes of a flags = 0 call."""
    flat = golden["weights_flat"]

    def run(flags):
        b = dev.from_instances(subset5[:2])
        p = torch.tensor(flat, dtype=torch.float32, device="cuda")
        ea, es, st = _adam_buffers(p)
        logits, loss = torch.empty(b.N, device="cuda"), torch.zeros(1, device="cuda")
        grads = torch.zeros(_lib.NUM_PARAMS, device="cuda")
        args = _args(b, p, ea, es, st, logits, loss, grads)
        step = lambda f: lib.mllp_gnn_train_step(*args[:-1], f, args[-1])  # noqa: E731
        assert step(0) == 0
        assert step(1) == 0                                 # honoured: the record holds
        assert lib.mllp_gnn_train_step_small(*args) == 0
        assert step(flags) == 0
        torch.cuda.synchronize()
        return [t.cpu().numpy().tobytes() for t in (loss, logits, grads, p, ea, es)]

    assert run(1) == run(0)
