"""Gradients of the model with respect to its inputs: x1 (objective coefficients), x2 (right-hand sides) and
edge_attr (the entries a_ij of A), through `GNNModel` / `BipartiteData` and through `LPBatch.backward_inputs`
(C ABI `mllp_gnn_backward_inputs`), against fp64 autograd through the oracle `oracle.pyg_restatement.gnn_forward`.

Tolerance as tests/test_hip_parity.py: max|diff| / max|ref| < 5e-5 for gradients (lin_key.bias excluded from the
parameter gradients: it is rounding noise on both sides).  The host-only tests at the top run without a GPU.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

from mllp_amd import _lib  # noqa: E402
from mllp_amd.data import load_packed  # noqa: E402
from mllp_amd.model import csr_to_edge_order, edge_order_to_csr  # noqa: E402
from oracle import pyg_restatement as o1  # noqa: E402

RTOL_GRAD = 5e-5
gpu = pytest.mark.gpu


def close(got, want, rtol, what=""):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, f"{what}: {got.shape} vs {want.shape}"
    assert np.isfinite(got).all(), what
    scale = max(float(np.abs(want).max()), 1e-30)
    err = float(np.abs(got - want).max()) / scale
    assert err < rtol, f"{what}: max|diff|/max|ref| = {err:.3e} >= {rtol}"


def grad_mask():
    keep, off = np.ones(_lib.NUM_PARAMS, bool), 0
    for k, s in o1.state_dict_spec():
        c = int(np.prod(s))
        if k.endswith("lin_key.bias"):
            keep[off:off + c] = False
        off += c
    return keep


def oracle_input_grads(flat, instances, loss_fn):
    """fp64 autograd through the oracle on the block-diagonal batch of `instances` (fp32 inputs, as the model sees
    them): (loss, dx1 [N], dx2 [M], dvalues [nnz] in CSR order, parameter gradients)."""
    sd = {k: v.detach().double().requires_grad_(True) for k, v in o1.unflatten_state(torch.tensor(flat)).items()}
    ei, x1, x2, ea = o1.batch_graphs([o1.instance_graph(i, torch.float32) for i in instances])
    x1, x2, ea = (t.double().requires_grad_(True) for t in (x1, x2, ea))
    z = o1.gnn_forward(sd, ei, x1, x2, ea)
    loss = loss_fn(z)
    params = list(sd.values())
    g = torch.autograd.grad(loss, [x1, x2, ea] + params, allow_unused=True)
    pg = torch.cat([(t if t is not None else torch.zeros_like(p)).reshape(-1) for t, p in zip(g[3:], params)])
    return float(loss.detach()), g[0].reshape(-1).numpy(), g[1].reshape(-1).numpy(), g[2].reshape(-1).numpy(), pg.numpy()


def _functional(n, seed):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


# ---------------------------------------------------------------------------------------------------
# host only
# ---------------------------------------------------------------------------------------------------
def test_csr_order_helpers_invert_the_sort():
    """the map from CSR-order values back to the caller's edge order, on a random edge list, against numpy"""
    rng = np.random.default_rng(7)
    m, n = 40, 60
    pairs = rng.choice(m * n, size=500, replace=False)
    con, var = pairs // n, pairs % n                     # distinct (constraint, variable) pairs, random order
    vals = rng.standard_normal(500)
    order = edge_order_to_csr(var, con)
    # CSR order: by constraint, then by variable (numpy's reference: a stable sort on the composite key)
    np.testing.assert_array_equal(order, np.argsort(con * n + var, kind="stable"))
    csr = torch.from_numpy(vals[order])
    back = csr_to_edge_order(csr, torch.from_numpy(order)).numpy()
    np.testing.assert_array_equal(back, vals)
    want = np.empty_like(vals)
    for k, e in enumerate(order):
        want[e] = vals[order][k]
    np.testing.assert_array_equal(back, want)


def test_backward_inputs_rejects_null_arguments_without_gpu():
    """null required arguments: MLLP_EINVAL with a message, before any HIP call"""
    L = _lib.lib()
    assert L.mllp_gnn_backward_inputs(None, None, None, None, None, None, None, None, None, None, None, None) == -1
    assert b"null" in L.mllp_last_error()
    n = ctypes.c_int64()
    assert L.mllp_gnn_input_grads_scratch_bytes(None, ctypes.byref(n)) == -1


# ---------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def weights(golden):
    flat = golden["weights_flat"]
    return flat, torch.tensor(flat, dtype=torch.float32, device="cuda")


@pytest.fixture(scope="module")
def model(weights):
    from mllp_amd.model import GNNModel
    m = GNNModel().to("cuda")
    m.load_flat(weights[1])
    return m


def _graph(inst, x1=True, x2=True, ea=True):
    from mllp_amd.model import build_graph_from_weights_sets
    name, constrs, w, coefs, rhs, basis = inst.as_reference_tuple()
    g = build_graph_from_weights_sets(constrs, w, rhs, coefs, torch.device("cuda"))
    g.x1.requires_grad_(x1)
    g.x2.requires_grad_(x2)
    g.edge_attr.requires_grad_(ea)
    return g


def _bce(basis):
    t = torch.tensor(np.asarray(basis), dtype=torch.float64)
    return lambda z: o1.bce_with_logits(z, t)


def _param_grads(model):
    return torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1)
                      for p in model.parameters()]).cpu().numpy()


@gpu
def test_afiro_dropin_input_grads(subset5, golden, weights, model):
    """x1.grad, x2.grad, edge_attr.grad through GNNModel + BCE + .backward(); parameter grads still the golden ones"""
    afiro = [i for i in subset5 if i.name == "afiro.mps"][0]
    g = _graph(afiro)
    model.zero_grad()
    z = model(g)
    obj = torch.nn.functional.binary_cross_entropy_with_logits(z, torch.tensor(afiro.basis, dtype=torch.float,
                                                                               device="cuda"))
    obj.backward()
    _, dx1, dx2, dv, _ = oracle_input_grads(weights[0], [afiro], _bce(afiro.basis))
    assert g.x1.grad is not None and g.x1.grad.shape == g.x1.shape
    assert g.x2.grad.shape == g.x2.shape and g.edge_attr.grad.shape == g.edge_attr.shape
    close(g.x1.grad.cpu().numpy().reshape(-1), dx1, RTOL_GRAD, "dL/dx1")
    close(g.x2.grad.cpu().numpy().reshape(-1), dx2, RTOL_GRAD, "dL/dx2")
    close(g.edge_attr.grad.cpu().numpy().reshape(-1), dv, RTOL_GRAD, "dL/dedge_attr")
    close(_param_grads(model)[grad_mask()], golden["afiro_grads"][grad_mask()], RTOL_GRAD, "parameter grads")
    model.zero_grad()


@gpu
def test_afiro_random_functional_and_batch_path_restored(subset5, weights, model):
    """a random linear functional of the logits; the batch's own path setting survives the pair"""
    afiro = [i for i in subset5 if i.name == "afiro.mps"][0]
    g = _graph(afiro)
    assert g.lp_batch().path == 0
    r = _functional(afiro.n, 11)
    z = model(g)
    assert g.lp_batch().path == 0
    (z * r.float().cuda()).sum().backward()
    assert g.lp_batch().path == 0
    _, dx1, dx2, dv, _ = oracle_input_grads(weights[0], [afiro], lambda z: (z * r).sum())
    close(g.x1.grad.cpu().numpy().reshape(-1), dx1, RTOL_GRAD, "dx1")
    close(g.x2.grad.cpu().numpy().reshape(-1), dx2, RTOL_GRAD, "dx2")
    close(g.edge_attr.grad.cpu().numpy().reshape(-1), dv, RTOL_GRAD, "dvalues")
    model.zero_grad()
    # nothing requires grad: the parameter-only Function, as before
    g2 = _graph(afiro, False, False, False)
    assert type(model(g2).grad_fn).__name__ == "_GNNFunctionBackward"


@gpu
def test_subset5_batched_each_graph_gets_its_slice(subset5, weights, model):
    from mllp_amd.model import BipartiteData
    graphs = [_graph(i) for i in subset5]
    b = BipartiteData.batch(graphs)
    z = model(b)
    basis = np.concatenate([i.basis for i in subset5])
    obj = torch.nn.functional.binary_cross_entropy_with_logits(z, torch.tensor(basis, dtype=torch.float, device="cuda"))
    obj.backward()
    _, dx1, dx2, dv, _ = oracle_input_grads(weights[0], subset5, _bce(basis))
    n0 = m0 = e0 = 0
    for g, inst in zip(graphs, subset5):
        close(g.x1.grad.cpu().numpy().reshape(-1), dx1[n0:n0 + inst.n], RTOL_GRAD, f"{inst.name} dx1")
        close(g.x2.grad.cpu().numpy().reshape(-1), dx2[m0:m0 + inst.m], RTOL_GRAD, f"{inst.name} dx2")
        close(g.edge_attr.grad.cpu().numpy().reshape(-1), dv[e0:e0 + inst.nnz], RTOL_GRAD, f"{inst.name} dvalues")
        n0, m0, e0 = n0 + inst.n, m0 + inst.m, e0 + inst.nnz
    model.zero_grad()


@gpu
def test_shuffled_edge_order_permutes_edge_grads(subset5, model):
    from mllp_amd.model import BipartiteData
    inst = [i for i in subset5 if i.name == "adlittle.mps"][0]
    g = _graph(inst, True, True, True)
    model(g).sum().backward()
    perm = torch.randperm(inst.nnz, generator=torch.Generator().manual_seed(3)).to("cuda")
    ea = g.edge_attr.detach()[perm].clone().requires_grad_(True)
    x1 = g.x1.detach().clone().requires_grad_(True)
    gs = BipartiteData(g.edge_index[:, perm], x1, g.x2.detach().clone(), ea)
    model(gs).sum().backward()
    assert torch.equal(ea.grad, g.edge_attr.grad[perm])
    assert torch.equal(x1.grad, g.x1.grad)
    model.zero_grad()


@gpu
def test_only_some_inputs(subset5, weights, model):
    """autograd.grad w.r.t. edge_attr alone, and w.r.t. x1 and x2 alone (the null-pointer outputs)"""
    inst = [i for i in subset5 if i.name == "blend.mps"][0]
    _, dx1, dx2, dv, _ = oracle_input_grads(weights[0], [inst], _bce(inst.basis))
    y = torch.tensor(inst.basis, dtype=torch.float, device="cuda")
    g = _graph(inst, False, False, True)
    obj = torch.nn.functional.binary_cross_entropy_with_logits(model(g), y)
    (gea,) = torch.autograd.grad(obj, g.edge_attr)
    close(gea.cpu().numpy().reshape(-1), dv, RTOL_GRAD, "edge_attr alone")
    g = _graph(inst, True, True, False)
    obj = torch.nn.functional.binary_cross_entropy_with_logits(model(g), y)
    gx1, gx2 = torch.autograd.grad(obj, [g.x1, g.x2])
    close(gx1.cpu().numpy().reshape(-1), dx1, RTOL_GRAD, "x1 with x2")
    close(gx2.cpu().numpy().reshape(-1), dx2, RTOL_GRAD, "x2 with x1")
    g = _graph(inst, False, True, False)
    (gx2,) = torch.autograd.grad(torch.nn.functional.binary_cross_entropy_with_logits(model(g), y), g.x2)
    close(gx2.cpu().numpy().reshape(-1), dx2, RTOL_GRAD, "x2 alone")


def _batch_input_grads(LPBatch, instances, flat_gpu, r):
    b = LPBatch.from_instances(instances)
    b.set_path(1)
    b.forward(flat_gpu)
    return b, b.backward_inputs(flat_gpu, r.float().cuda())


@gpu
@pytest.mark.parametrize("name", ["d6cube.mps", "80bau3b.mps"])
def test_skew_and_empty_rows_and_columns(name, weights):
    """d6cube: a 6 184-nonzero row and 11 empty rows; 80bau3b: 127 variables with no nonzero"""
    from mllp_amd.graph import LPBatch
    inst = load_packed([name])
    r = _functional(inst[0].n, 5)
    _, (grads, dx1, dx2, dv) = _batch_input_grads(LPBatch, inst, weights[1], r)
    _, ox1, ox2, odv, opg = oracle_input_grads(weights[0], inst, lambda z: (z * r).sum())
    close(dx1.cpu().numpy(), ox1, RTOL_GRAD, f"{name} dx1")
    close(dx2.cpu().numpy(), ox2, RTOL_GRAD, f"{name} dx2")
    close(dv.cpu().numpy(), odv, RTOL_GRAD, f"{name} dvalues")
    close(grads.cpu().numpy()[grad_mask()], opg[grad_mask()], RTOL_GRAD, f"{name} parameter grads")


@pytest.fixture(scope="module")
def netlib(weights):
    from mllp_amd.graph import LPBatch
    inst = load_packed()
    r = _functional(sum(i.n for i in inst), 9)
    b, out = _batch_input_grads(LPBatch, inst, weights[1], r)
    oracle = oracle_input_grads(weights[0], inst, lambda z: (z * r).sum())
    return inst, r, b, [t.cpu() for t in out], oracle


@gpu
def test_full_netlib_batch_input_grads(netlib):
    """all 97 instances (1.07 M nonzeros, every row tier, rows split over workgroups) on path 1"""
    inst, r, b, (grads, dx1, dx2, dv), (_, ox1, ox2, odv, _) = netlib
    d = b.dims()
    assert d["nnz"] == 1074147 and d["A_block"] > 0 and d["At_block"] > 0 and d["A_split"] > 0 and d["At_split"] > 0
    close(dx1.numpy(), ox1, RTOL_GRAD, "netlib dx1")
    close(dx2.numpy(), ox2, RTOL_GRAD, "netlib dx2")
    close(dv.numpy(), odv, RTOL_GRAD, "netlib dvalues")


@gpu
@pytest.mark.parametrize("copies", ["tiled", "streamed"])
def test_reblocked_copies_leave_input_grads_on_the_oracle(netlib, weights, copies):
    """with the training step's LDS-tiled or streamed copies attached the forward and the parameter backward run on
    them; the post-pass walks the plain CSR and still matches the oracle"""
    from mllp_amd.graph import LPBatch
    inst, r, _, (grads, dx1, dx2, dv), (_, ox1, ox2, odv, _) = netlib
    b = LPBatch.from_instances(inst)
    if copies == "tiled":
        b.enable_tiled_step()
    else:
        info = b.enable_stream_step(max_slots_per_nnz=1e9)
        assert not any(v.get("dropped") for v in info.values())
    b.set_path(1)
    b.forward(weights[1])
    _, x1c, x2c, dvc = b.backward_inputs(weights[1], r.float().cuda())
    close(x1c.cpu().numpy(), ox1, RTOL_GRAD, f"{copies} dx1")
    close(x2c.cpu().numpy(), ox2, RTOL_GRAD, f"{copies} dx2")
    close(dvc.cpu().numpy(), odv, RTOL_GRAD, f"{copies} dvalues")


@gpu
def test_backward_inputs_is_deterministic_and_keeps_parameter_grads(netlib, weights):
    """same parameter gradients as mllp_gnn_backward bit for bit; two calls give the same bits; d_grads = NULL
    with the scratch buffer gives the same input gradients"""
    inst, r, b, (grads, dx1, dx2, dv), _ = netlib
    flat_gpu, dl = weights[1], r.float().cuda()
    b.forward(flat_gpu)
    assert torch.equal(b.backward(flat_gpu, dl).cpu(), grads)
    b.forward(flat_gpu)
    g2, x1b, x2b, dvb = b.backward_inputs(flat_gpu, dl)
    assert torch.equal(g2.cpu(), grads)
    assert torch.equal(x1b.cpu(), dx1) and torch.equal(x2b.cpu(), dx2) and torch.equal(dvb.cpu(), dv)
    L = _lib.lib()
    n = ctypes.c_int64()
    _lib.check(L.mllp_gnn_input_grads_scratch_bytes(b._h, ctypes.byref(n)))
    scratch = torch.empty(n.value // 4, device="cuda")
    x1c = torch.empty(b.N, device="cuda")
    dvc = torch.empty(b.nnz, device="cuda")
    _lib.check(L.mllp_gnn_backward_inputs(b._h, _lib.ptr(flat_gpu), _lib.ptr(b.x1), _lib.ptr(b.x2),
                                          _lib.ptr(b.workspace()), _lib.ptr(dl), None, _lib.ptr(x1c), None,
                                          _lib.ptr(dvc), _lib.ptr(scratch), _lib.current_stream()))
    assert torch.equal(x1c.cpu(), dx1) and torch.equal(dvc.cpu(), dv)
    assert torch.equal(scratch[:_lib.NUM_PARAMS].cpu(), grads)


@gpu
def test_gradients_at_current_values(subset5, weights, model):
    """x1 changed in place after a first forward: the next forward / backward is taken at the new values"""
    inst = [i for i in subset5 if i.name == "sc50a.mps"][0]
    g = _graph(inst)
    model(g).sum().backward()
    with torch.no_grad():
        g.x1.mul_(-1.5).add_(0.25)
        g.edge_attr.mul_(0.5)
    g.x1.grad = g.x2.grad = g.edge_attr.grad = None
    model(g).sum().backward()
    x1_new = g.x1.detach().cpu().numpy().reshape(-1).astype(np.float64)
    ea_new = g.edge_attr.detach().cpu().numpy().reshape(-1).astype(np.float64)
    sd = {k: v.detach().double().requires_grad_(True) for k, v in o1.unflatten_state(torch.tensor(weights[0])).items()}
    ei, x1, x2, ea = o1.instance_graph(inst, torch.float32)
    x1 = torch.tensor(x1_new).reshape(-1, 1).requires_grad_(True)
    ea = torch.tensor(ea_new).reshape(-1, 1).requires_grad_(True)
    x2 = x2.double().requires_grad_(True)
    o1.gnn_forward(sd, ei, x1, x2, ea).sum().backward()
    close(g.x1.grad.cpu().numpy().reshape(-1), x1.grad.numpy().reshape(-1), RTOL_GRAD, "dx1 at new values")
    close(g.x2.grad.cpu().numpy().reshape(-1), x2.grad.numpy().reshape(-1), RTOL_GRAD, "dx2 at new values")
    close(g.edge_attr.grad.cpu().numpy().reshape(-1), ea.grad.numpy().reshape(-1), RTOL_GRAD, "dvalues at new values")
    model.zero_grad()


@gpu
def test_backward_after_another_forward_still_raises(subset5, model):
    inst = [i for i in subset5 if i.name == "kb2.mps"][0]
    g = _graph(inst)
    z1 = model(g)
    model(g)
    with pytest.raises(RuntimeError, match="another forward"):
        z1.sum().backward()
    model.zero_grad()


@gpu
def test_fused_forward_is_an_error_not_a_fault(subset5, weights):
    from mllp_amd.graph import LPBatch
    b = LPBatch.from_instances(subset5[:2])
    b.set_path(2)
    flat_gpu = weights[1]
    b.forward(flat_gpu)
    L = _lib.lib()
    dl = torch.ones(b.N, device="cuda")
    out = [torch.empty(k, device="cuda") for k in (_lib.NUM_PARAMS, b.N, b.M, b.nnz)]
    rc = L.mllp_gnn_backward_inputs(b._h, _lib.ptr(flat_gpu), _lib.ptr(b.x1), _lib.ptr(b.x2), _lib.ptr(b.workspace()),
                                    _lib.ptr(dl), *[_lib.ptr(t) for t in out], None, _lib.current_stream())
    assert rc == -1 and b"fused" in L.mllp_last_error()
    torch.cuda.synchronize()
    # the graph is still usable: the generic pair on the same batch
    b.set_path(1)
    b.forward(flat_gpu)
    grads, dx1, dx2, dv = b.backward_inputs(flat_gpu, dl)
    torch.cuda.synchronize()
    assert torch.isfinite(dv).all() and torch.isfinite(dx1).all()
