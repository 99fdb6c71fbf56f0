"""Gradients of AngleModel with respect to its inputs: x [N, 2] (node features) and the cosine matrix cos [N, N] (the edge
attributes: cos[i, j] belongs to the reference's edge j -> i), through `AngleModel` / `AngleGraph` and through the C ABI
`mllp_angle_backward_inputs`.

Oracles (tests/angle_oracle.py): fp64 autograd through the oracle's literal TransformerConv on the explicit N (N - 1) edge
list (as tests/test_angle.py), and, where that list is too large (25fv47: 3.5 M edges), a dense fp64 restatement of the same
model that this file first checks against the edge-list oracle on the small cases.  Tolerance as tests/test_angle.py:
max|diff| / max|ref| <= 1e-5 for logits, 5e-5 for gradients.  The host-only test at the top runs without a GPU.
"""
import ctypes

import numpy as np
import pytest
import torch

from angle_oracle import RTOL_GRAD, RTOL_LOGITS, close
from angle_oracle import oracle as _oracle
from mllp_amd import _lib

gpu = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------
# host only
# ---------------------------------------------------------------------------------------------------
def test_angle_backward_inputs_rejects_bad_arguments_without_gpu():
    """null required arguments, a bad size or a bad feat_dim: MLLP_EINVAL with a message, before any HIP call"""
    L = _lib.lib()
    assert L.mllp_angle_backward_inputs(52, 32, None, None, None, None, None, None, None, None, None) == -1
    assert b"null" in L.mllp_last_error()
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.mllp_angle_backward_inputs(52, 32, p, p, p, p, p, None, p, p, None) == -1       # d_grads is required
    assert b"null" in L.mllp_last_error()
    assert L.mllp_angle_backward_inputs(1, 32, p, p, p, p, p, p, None, None, None) == -1
    assert b"size" in L.mllp_last_error()
    assert L.mllp_angle_backward_inputs(52, 24, p, p, p, p, p, p, None, None, None) == -1
    assert b"feat_dim" in L.mllp_last_error()


# ---------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------
def _graph(case):
    from mllp_amd.angle import build_graph_from_Q_sets, dense_instance_tensors
    from mllp_amd.data import load_packed
    if case in ("afiro_F256", "25fv47_F256"):
        inst = load_packed([case.split("_")[0]])[0]
        Q, coefs, basis = dense_instance_tensors(inst)
        F = 256
    else:                                                   # N = 299: not a multiple of 4 or 16; a zero Q row
        rng = np.random.default_rng(11)
        Q, _ = np.linalg.qr(rng.standard_normal((299, 40)))
        Q[17] = 0.0
        coefs = rng.standard_normal(299)
        basis = (rng.random(298) < 0.3).astype(np.int32)
        F = 64
    g = build_graph_from_Q_sets(Q, coefs, torch.device("cuda"), case, basis)
    return g, torch.tensor(basis, dtype=torch.float, device="cuda"), F


def _model(F, seed=7):
    from mllp_amd.angle import AngleModel
    from mllp_amd.model import set_seed
    set_seed(seed)
    return AngleModel(feat_dim=F).to("cuda")


def _run(model, g, y, x_grad=True, cos_grad=True):
    """model(g) + BCE + backward with the requested inputs as leaves: (logits, x.grad, cos.grad, flat parameter grads)"""
    model.zero_grad(set_to_none=True)
    g.x = g.x.detach().requires_grad_(x_grad)
    g.cos = g.cos.detach().requires_grad_(cos_grad)
    logits = model(g)
    torch.nn.functional.binary_cross_entropy_with_logits(logits, y).backward()
    pg = torch.cat([p.grad.reshape(-1) for p in model.parameters()])
    return logits.detach(), g.x.grad, g.cos.grad, pg


def _check_params(model, ref):
    for name, p in model.named_parameters():
        if name.startswith("gconv3"):                      # never called by forward (reference :198)
            assert ref[name] is None and float(p.grad.abs().max()) == 0.0
        elif name.endswith("lin_key.bias"):                # cancels in the softmax: rounding noise on both sides
            assert float(p.grad.abs().max()) <= 1e-6 * max(1.0, float(ref[name].abs().max()) * 1e6)
        else:
            close(p.grad.cpu().numpy(), ref[name].numpy(), RTOL_GRAD, name)


@gpu
@pytest.mark.parametrize("case", ["afiro_F256", "random_N299_F64"])
def test_input_grads_vs_edge_list_oracle(case):
    g, y, F = _graph(case)
    model = _model(F)
    logits, dx, dcos, _ = _run(model, g, y)
    z, rdx, rdcos, rparams = _oracle(model, g, y, dense=False)
    close(logits.cpu().numpy(), z.numpy(), RTOL_LOGITS, "logits")
    _check_params(model, rparams)
    assert dx.shape == (g.num_nodes, 2) and dcos.shape == (g.num_nodes, g.num_nodes)
    close(dx.cpu().numpy(), rdx.numpy(), RTOL_GRAD, "dx")
    close(dcos.cpu().numpy(), rdcos.numpy(), RTOL_GRAD, "dcos")
    assert bool((dcos.diagonal() == 0).all())
    # the dense restatement used at full size is the same function as the edge-list oracle
    dz_, ddx, ddcos, dparams = _oracle(model, g, y, dense=True)
    close(dz_.numpy(), z.numpy(), 1e-12, "dense logits")
    close(ddx.numpy(), rdx.numpy(), 1e-10, "dense dx")
    close(ddcos.numpy(), rdcos.numpy(), 1e-10, "dense dcos")
    for name, t in rparams.items():
        if t is not None and not name.endswith("lin_key.bias"):
            close(dparams[name].numpy(), t.numpy(), 1e-9, "dense " + name)


@gpu
def test_input_grads_full_size_vs_dense_oracle():
    """25fv47, N = 1 877, F = 256: several X ranges per group of Y nodes, rows not 16-byte aligned; the weight-gradient
    GEMM runs with 7 K splits"""
    g, y, F = _graph("25fv47_F256")
    model = _model(F)
    logits, dx, dcos, _ = _run(model, g, y)
    z, rdx, rdcos, rparams = _oracle(model, g, y, dense=True)
    close(logits.cpu().numpy(), z.numpy(), RTOL_LOGITS, "logits")
    _check_params(model, rparams)
    close(dx.cpu().numpy(), rdx.numpy(), RTOL_GRAD, "dx")
    close(dcos.cpu().numpy(), rdcos.numpy(), RTOL_GRAD, "dcos")
    assert bool((dcos.diagonal() == 0).all())


@gpu
def test_inputs_path_keeps_logits_and_parameter_grads_bitwise():
    from mllp_amd.angle import _AngleFunction
    g, y, F = _graph("random_N299_F64")
    model = _model(F)
    l0, dx0, dc0, pg0 = _run(model, g, y, x_grad=False, cos_grad=False)
    assert dx0 is None and dc0 is None
    l1, dx1, dc1, pg1 = _run(model, g, y)
    assert torch.equal(l0, l1) and torch.equal(pg0, pg1)
    # the C call: both outputs NULL is mllp_angle_backward; with outputs, d_grads is unchanged
    L, N = _lib.lib(), g.num_nodes
    flat = model.flat_parameters().detach().contiguous()
    ws = g.workspace(F)
    logits = torch.empty(N - 1, device="cuda")
    dl = torch.randn(N - 1, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    args = (N, F, _lib.ptr(g.cos), _lib.ptr(g.x), _lib.ptr(flat), _lib.ptr(ws))
    _lib.check(L.mllp_angle_forward(*args, _lib.ptr(logits), _lib.current_stream()))
    ref, a, b = (torch.full_like(flat, float("nan")) for _ in range(3))
    dx, dcos = torch.empty(N, 2, device="cuda"), torch.empty(N, N, device="cuda")
    _lib.check(L.mllp_angle_backward(*args, _lib.ptr(dl), _lib.ptr(ref), _lib.current_stream()))
    _lib.check(L.mllp_angle_backward_inputs(*args, _lib.ptr(dl), _lib.ptr(a), None, None, _lib.current_stream()))
    _lib.check(L.mllp_angle_backward_inputs(*args, _lib.ptr(dl), _lib.ptr(b), _lib.ptr(dx), _lib.ptr(dcos),
                                            _lib.current_stream()))
    torch.cuda.synchronize()
    assert torch.equal(a, ref) and torch.equal(b, ref)
    assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(dcos).all())
    # with nothing requiring grad, the old Function runs: same logits, bit for bit
    assert torch.equal(_AngleFunction.apply(model.flat_parameters(), g, F).detach(), l0)


@gpu
def test_partial_requests_and_determinism():
    g, y, F = _graph("random_N299_F64")
    model = _model(F)
    _, dx, dc, _ = _run(model, g, y)
    _, dx2, dc2, _ = _run(model, g, y)
    assert torch.equal(dx, dx2) and torch.equal(dc, dc2)      # run to run, bit for bit
    _, dxa, dca, _ = _run(model, g, y, x_grad=True, cos_grad=False)
    assert dca is None and torch.equal(dxa, dx)
    _, dxb, dcb, _ = _run(model, g, y, x_grad=False, cos_grad=True)
    assert dxb is None and torch.equal(dcb, dc)


@gpu
def test_symmetry_requirement_no_grad_behaviour_and_token():
    g, y, F = _graph("afiro_F256")
    model = _model(F)
    # nothing requires grad: no input gradient, the plain Function's logits
    logits = model(g)
    assert g.x.grad is None and g.cos.grad is None and not g.x.requires_grad
    with torch.no_grad():
        g.cos = g.cos.detach().requires_grad_(True)
        assert torch.equal(model(g), logits.detach())        # grad mode off: the plain path even with a leaf
    # a non-symmetric cos with requires_grad is refused
    cos = g.cos.detach().clone()
    cos[0, 1] += 0.25
    g.cos = cos.requires_grad_(True)
    with pytest.raises(ValueError, match="symmetric"):
        model(g)
    # a backward after another forward on the same graph
    g.cos = (cos + cos.T).mul_(0.5).requires_grad_(True)
    first = model(g)
    model(g)
    with pytest.raises(RuntimeError, match="another forward"):
        first.sum().backward()
