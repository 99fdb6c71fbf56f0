"""Input gradients on the fused latency-regime path (`mllp_gnn_input_grads`, `mllp_gnn_loss_step_inputs`;
`LPBatch.input_grads`, `LPBatch.loss_step_inputs`; mllp_amd/csrc/fused_input_grads.hip), against fp64 autograd through the
oracle `oracle.pyg_restatement.gnn_forward`, used exactly as tests/test_input_grads.py uses it.

Tolerance as there: max|diff| / max|ref| < 5e-5 per output array for gradients (lin_key.bias left out of the parameter
gradients: it is rounding noise on both sides), 1e-5 for loss and logits.  The host-only test at the top runs without a GPU.

The row kernel of the post-pass tiers rows at FUSED_T1[1] and FUSED_T1[2] nonzeros (16-lane group / wavefront /
workgroup), the thresholds of the fused layer-1 sweeps, so the degree grids of tests/fused_cases.py cross its tier edges
as well as those of the sweeps that wrote the records.
"""
import ctypes
import dataclasses
import itertools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from mllp_amd import _lib
from mllp_amd.data import SUBSET5, load_packed
from oracle import mps_norm
from oracle import pyg_restatement as o1
import fused_cases as fc
from test_input_grads import close, grad_mask, oracle_input_grads

RTOL_GRAD = 5e-5
RTOL_OUT = 1e-5
gpu = pytest.mark.gpu


def _functional(n, seed):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _bce_loss(instances, inv_batch):
    """L = inv_batch * sum_k mean_i BCE(z_i, y_i) over the instances k"""
    off = np.concatenate([[0], np.cumsum([i.n for i in instances])])
    ys = [torch.tensor(np.asarray(i.basis), dtype=torch.float64) for i in instances]

    def f(z):
        z = z.reshape(-1)
        return inv_batch * sum(torch.nn.functional.binary_cross_entropy_with_logits(z[off[k]:off[k + 1]], ys[k])
                               for k in range(len(instances)))
    return f


def _oracle_logits(flat, instances):
    sd = {k: v.double() for k, v in o1.unflatten_state(torch.tensor(flat)).items()}
    ei, x1, x2, ea = o1.batch_graphs([o1.instance_graph(i, torch.float32) for i in instances])
    with torch.no_grad():
        return o1.gnn_forward(sd, ei, x1.double(), x2.double(), ea.double()).reshape(-1).numpy()


def _check_four(got, want, what):
    grads, dx1, dx2, dv = got
    ox1, ox2, odv, opg = want
    close(dx1.cpu().numpy(), ox1, RTOL_GRAD, f"{what} dx1")
    close(dx2.cpu().numpy(), ox2, RTOL_GRAD, f"{what} dx2")
    close(dv.cpu().numpy(), odv, RTOL_GRAD, f"{what} dvalues")
    close(grads.cpu().numpy()[grad_mask()], opg[grad_mask()], RTOL_GRAD, f"{what} parameter grads")


def _same(a, b, what):
    for k, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), f"{what}: output {k} differs in bits"


# ---------------------------------------------------------------------------------------------------
# host only
# ---------------------------------------------------------------------------------------------------
def test_new_exports_reject_null_arguments_without_gpu():
    """1. null required arguments: MLLP_EINVAL with a message, before any HIP call; d_grads and d_scratch both null too"""
    L = _lib.lib()
    assert L.mllp_gnn_input_grads(None, None, None, None, None, None, None, None, None, None, None, None) == -1
    assert b"mllp_gnn_input_grads" in L.mllp_last_error() and b"null" in L.mllp_last_error()
    assert L.mllp_gnn_loss_step_inputs(None, None, None, None, None, 1.0, None, None, None, None, None, None, None, None) == -1
    assert b"mllp_gnn_loss_step_inputs" in L.mllp_last_error() and b"null" in L.mllp_last_error()
    # every required pointer present (host memory that is never dereferenced: the checks come first) but one
    room = ctypes.create_string_buffer(1 << 16)
    p = ctypes.c_void_p(ctypes.addressof(room))
    for missing in range(6):
        args = [p] * 6
        args[missing] = None
        assert L.mllp_gnn_input_grads(*args, p, p, p, p, p, None) == -1, missing
        assert b"null" in L.mllp_last_error()
    assert L.mllp_gnn_input_grads(p, p, p, p, p, p, None, p, p, p, None, None) == -1
    assert b"d_scratch" in L.mllp_last_error()
    for missing in range(9):          # graph, params, x1, x2, labels, workspace, logits, loss, grads
        args = [p] * 9
        args[missing] = None
        assert L.mllp_gnn_loss_step_inputs(*args[:5], 1.0, *args[5:], p, p, p, None) == -1, missing
        assert b"null" in L.mllp_last_error()


# ---------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def LPBatch():
    from mllp_amd.graph import LPBatch
    return LPBatch


@pytest.fixture(scope="module")
def weights(golden):
    flat = golden["weights_flat"]
    return flat, torch.tensor(flat, dtype=torch.float32, device="cuda")


def _fused_batch(LPBatch, instances, path=2):
    b = LPBatch.from_instances(instances)
    if path:
        b.set_path(path)
    return b


def _forward_input_grads(LPBatch, instances, flat_gpu, r, path=2, **kw):
    b = _fused_batch(LPBatch, instances, path)
    b.forward(flat_gpu)
    return b, b.input_grads(flat_gpu, r.float().cuda(), **kw)


@pytest.fixture(scope="module")
def golden_functional(subset5, weights):
    """the functional, the fused batch result and the oracle of the five golden instances as one batch"""
    from mllp_amd.graph import LPBatch
    r = _functional(sum(i.n for i in subset5), 21)
    b, out = _forward_input_grads(LPBatch, subset5, weights[1], r)
    oracle = oracle_input_grads(weights[0], subset5, lambda z: (z * r).sum())
    return r, b, out, oracle


@gpu
def test_golden_batch_against_oracle_and_single_instances(LPBatch, subset5, weights, golden_functional):
    """2. forward + input_grads with L = sum r z on the five golden instances as one batch; every instance alone gives
    the batch's slices within the same bar (block-diagonal independence)"""
    r, b, out, oracle = golden_functional
    assert [i.name for i in subset5] == list(SUBSET5)
    _check_four(out, oracle[1:], "subset5")
    _, dx1, dx2, dv = (t.cpu().numpy() for t in out)
    n0 = m0 = e0 = 0
    for inst in subset5:
        _, (_, sx1, sx2, sdv) = _forward_input_grads(LPBatch, [inst], weights[1], r[n0:n0 + inst.n])
        close(dx1[n0:n0 + inst.n], sx1.cpu().numpy(), RTOL_GRAD, f"{inst.name} dx1 slice")
        close(dx2[m0:m0 + inst.m], sx2.cpu().numpy(), RTOL_GRAD, f"{inst.name} dx2 slice")
        close(dv[e0:e0 + inst.nnz], sdv.cpu().numpy(), RTOL_GRAD, f"{inst.name} dvalues slice")
        n0, m0, e0 = n0 + inst.n, m0 + inst.m, e0 + inst.nnz


@gpu
@pytest.mark.parametrize("path", [2, 0])
def test_loss_step_inputs_against_oracle_and_loss_step(LPBatch, subset5, weights, path):
    """3. loss, logits and all four gradients against the oracle; loss, logits and grads bit for bit those of loss_step on a
    second batch of the same instances.  Path 0 is the default selection: it reaches the fused pass without set_path."""
    b = _fused_batch(LPBatch, subset5, path)
    loss, logits, grads, dx1, dx2, dv = b.loss_step_inputs(weights[1])
    ib = 1.0 / len(subset5)
    oloss, ox1, ox2, odv, opg = oracle_input_grads(weights[0], subset5, _bce_loss(subset5, ib))
    assert abs(float(loss) - oloss) < RTOL_OUT * abs(oloss), (float(loss), oloss)
    close(logits.cpu().numpy(), _oracle_logits(weights[0], subset5), RTOL_OUT, "logits")
    _check_four((grads, dx1, dx2, dv), (ox1, ox2, odv, opg), f"loss step path {path}")
    b2 = _fused_batch(LPBatch, subset5, path)
    _same((loss, logits, grads), b2.loss_step(weights[1]), "loss_step_inputs against loss_step")
    if path != 2:
        return
    # the generic path answers the same call (its own post-pass), against the same oracle
    b1 = _fused_batch(LPBatch, subset5, 1)
    l1, z1, g1, x1g, x2g, dvg = b1.loss_step_inputs(weights[1])
    _check_four((g1, x1g, x2g, dvg), (ox1, ox2, odv, opg), "loss step path 1")
    _same((l1, z1, g1), _fused_batch(LPBatch, subset5, 1).loss_step(weights[1]), "path 1 against loss_step")


@gpu
@pytest.mark.parametrize("name", ["d6cube.mps", "80bau3b.mps"])
def test_skew_and_empty_rows_and_columns(LPBatch, name, weights):
    """4. d6cube: a 6 184-nonzero row (workgroup tier of the row kernel, a split block row of the fused sweeps) and 11
    empty rows; 80bau3b: 127 variables with no nonzero"""
    inst = load_packed([name])
    r = _functional(inst[0].n, 5)
    _, out = _forward_input_grads(LPBatch, inst, weights[1], r)
    _check_four(out, oracle_input_grads(weights[0], inst, lambda z: (z * r).sum())[1:], name)


@gpu
@pytest.mark.parametrize("n_inst", [1, 2])
@pytest.mark.parametrize("variant", [0, 1])
def test_degree_grids_cross_every_tier_edge(LPBatch, weights, variant, n_inst):
    """5. rows AND columns with the degrees on both sides of every threshold of FUSED_T16 and FUSED_T1 (and so of the row
    kernel's own tiers, which are FUSED_T1[1] and FUSED_T1[2]), as one and as two instances"""
    c = fc.constants()
    insts = fc.grid_batch(variant, n_inst)
    for deg in fc.degrees(insts[0]):
        for T in (c["T1"][1], c["T1"][2]):
            assert {T - 1, T, T + 1} <= set(deg.tolist())
    r = _functional(sum(i.n for i in insts), 30 + variant)
    _, out = _forward_input_grads(LPBatch, insts, weights[1], r)
    _check_four(out, oracle_input_grads(weights[0], insts, lambda z: (z * r).sum())[1:], f"grid{variant} x {n_inst}")


@gpu
def test_same_bits_where_the_code_is_the_same(LPBatch, subset5, weights, golden_functional):
    """6. path 1: input_grads is backward_inputs bit for bit; path 2: grads of input_grads are those of backward"""
    r, b, out, _ = golden_functional
    flat_gpu, dl = weights[1], r.float().cuda()
    b1 = _fused_batch(LPBatch, subset5, 1)
    b1.forward(flat_gpu)
    want = b1.backward_inputs(flat_gpu, dl)
    b1.forward(flat_gpu)
    _same(b1.input_grads(flat_gpu, dl), want, "path 1")
    b.forward(flat_gpu)
    assert torch.equal(b.backward(flat_gpu, dl), out[0])


@gpu
def test_determinism_partial_outputs_guards_and_scratch(LPBatch, subset5, weights, golden_functional):
    """7. two calls give the same bits; every subset of {x1, x2, values} gives the bits of the all-three call for what it
    computes; guard words around every output stay intact; d_grads = NULL with the scratch buffer gives the same"""
    r, b, out, _ = golden_functional
    flat_gpu, dl = weights[1], r.float().cuda()
    b.forward(flat_gpu)
    _same(b.input_grads(flat_gpu, dl), out, "second call")
    for x1, x2, values in itertools.product([False, True], repeat=3):
        b.forward(flat_gpu)
        got = b.input_grads(flat_gpu, dl, x1=x1, x2=x2, values=values)
        assert torch.equal(got[0], out[0])
        for k, on in ((1, x1), (2, x2), (3, values)):
            assert (got[k] is None) == (not on)
            if on:
                assert torch.equal(got[k], out[k]), (x1, x2, values, k)
    L = _lib.lib()
    G, SENT = 16, -12345.0
    bufs = [torch.full((n + 2 * G,), SENT, device="cuda") for n in (_lib.NUM_PARAMS, b.N, b.M, b.nnz)]
    views = [t[G:-G] for t in bufs]
    b.forward(flat_gpu)
    _lib.check(L.mllp_gnn_input_grads(b._h, _lib.ptr(flat_gpu), _lib.ptr(b.x1), _lib.ptr(b.x2), _lib.ptr(b.workspace()),
                                      _lib.ptr(dl), *[_lib.ptr(v) for v in views], None, _lib.current_stream()))
    _same(views, out, "guarded buffers")
    for t in bufs:
        assert (t[:G] == SENT).all() and (t[-G:] == SENT).all()
    n = ctypes.c_int64()
    _lib.check(L.mllp_gnn_input_grads_scratch_bytes(b._h, ctypes.byref(n)))
    scratch = torch.empty(n.value // 4, device="cuda")
    outs = [torch.empty_like(t) for t in out[1:]]
    b.forward(flat_gpu)
    _lib.check(L.mllp_gnn_input_grads(b._h, _lib.ptr(flat_gpu), _lib.ptr(b.x1), _lib.ptr(b.x2), _lib.ptr(b.workspace()),
                                      _lib.ptr(dl), None, *[_lib.ptr(t) for t in outs], _lib.ptr(scratch),
                                      _lib.current_stream()))
    _same([scratch[:_lib.NUM_PARAMS]] + outs, out, "d_grads = NULL")


@gpu
def test_loss_step_inputs_under_graph_capture(LPBatch, subset5, weights):
    """8. after one eager call (which builds the position map) the call is captured and replayed twice: the eager bits"""
    b = _fused_batch(LPBatch, subset5)
    flat_gpu = weights[1]
    eager = [t.clone() for t in b.loss_step_inputs(flat_gpu)]
    torch.cuda.synchronize()
    static = [torch.zeros_like(t) for t in eager]
    loss, logits, grads = static[:3]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = b.loss_step_inputs(flat_gpu, logits=logits, loss=loss, grads=grads)
    for _ in range(2):
        for t in cap:
            t.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        _same(cap, eager, "replay")


def _as_seen(inst, values=None, coefs=None, rhs=None):
    """the instance with the fp32 arrays the device holds, as fp64"""
    f = lambda new, old: (old if new is None else new.detach().cpu().numpy()).astype(np.float32).astype(np.float64)
    return dataclasses.replace(inst, values=f(values, inst.values), coefs=f(coefs, inst.coefs), rhs=f(rhs, inst.rhs))


@gpu
def test_gradients_at_current_values_through_update_and_normalize(LPBatch, subset5, weights):
    """9. kb2 on the default path: set_values with perturbed coefficients, loss_step_inputs against the oracle on the
    perturbed instance; normalize(), loss_step_inputs again against the oracle on oracle.mps_norm.normalize of it"""
    inst = [i for i in subset5 if i.name == "kb2.mps"][0]
    rng = np.random.default_rng(17)
    new = (inst.values * np.exp2(rng.uniform(-1.0, 1.0, inst.nnz))).astype(np.float32)
    b = LPBatch.from_instances([inst])
    assert b.path == 0
    b.loss_step_inputs(weights[1])
    b.set_values(torch.tensor(new, device="cuda"))
    pert = _as_seen(inst, values=torch.tensor(new))
    loss, logits, grads, dx1, dx2, dv = b.loss_step_inputs(weights[1])
    oloss, *want = oracle_input_grads(weights[0], [pert], _bce_loss([pert], 1.0))
    assert abs(float(loss) - oloss) < RTOL_OUT * abs(oloss)
    _check_four((grads, dx1, dx2, dv), want, "kb2 perturbed")
    # the rule in fp64 (no slack columns to add: the instance has them already); no row sits on the cap's edge
    A = sp.csr_matrix((pert.values, pert.indices, pert.indptr), shape=(pert.m, pert.n))
    nrm = np.sqrt(np.asarray(A.multiply(A).sum(1)).ravel())
    ratio = np.abs(pert.rhs) / np.where(nrm > 0, nrm, 1.0)
    assert (np.abs(ratio - 5.0) > 1e-3).all()
    B, c, rhs = mps_norm.normalize({"rows": [], "rtype": {}, "ranges": {}}, A, pert.coefs, pert.rhs)
    assert np.array_equal(B.indptr, pert.indptr) and np.array_equal(B.indices, pert.indices)
    normed = dataclasses.replace(pert, values=B.data.astype(np.float32).astype(np.float64),
                                 coefs=c.astype(np.float32).astype(np.float64), rhs=rhs.astype(np.float32).astype(np.float64))
    b.normalize()
    close(b.export(2), normed.values, RTOL_OUT, "normalized values")
    loss, logits, grads, dx1, dx2, dv = b.loss_step_inputs(weights[1])
    oloss, *want = oracle_input_grads(weights[0], [normed], _bce_loss([normed], 1.0))
    assert abs(float(loss) - oloss) < RTOL_OUT * abs(oloss)
    close(logits.cpu().numpy(), _oracle_logits(weights[0], [normed]), RTOL_OUT, "logits after normalize")
    _check_four((grads, dx1, dx2, dv), want, "kb2 normalized")


@gpu
def test_refusals_write_nothing_and_leave_the_batch_usable(LPBatch, subset5, weights):
    """10. no forward on the workspace; a set_path between forward and call; set_values after the forward: RuntimeError,
    the sentinel-filled outputs unchanged, and the batch works afterwards"""
    flat_gpu = weights[1]
    b = _fused_batch(LPBatch, subset5[:2])
    dl = torch.ones(b.N, device="cuda")
    L = _lib.lib()
    SENT = -777.0
    outs = [torch.full((n,), SENT, device="cuda") for n in (_lib.NUM_PARAMS, b.N, b.M, b.nnz)]

    def refused(what):
        rc = L.mllp_gnn_input_grads(b._h, _lib.ptr(flat_gpu), _lib.ptr(b.x1), _lib.ptr(b.x2), _lib.ptr(b.workspace()),
                                    _lib.ptr(dl), *[_lib.ptr(t) for t in outs], None, _lib.current_stream())
        assert rc == -1, what
        torch.cuda.synchronize()
        for t in outs:
            assert (t == SENT).all(), what
        with pytest.raises(RuntimeError):
            b.input_grads(flat_gpu, dl)

    refused("no forward")
    b.forward(flat_gpu)
    b.set_path(1)
    refused("fused forward, generic call")
    b.forward(flat_gpu)
    b.set_path(2)
    refused("generic forward, fused call")
    b.forward(flat_gpu)
    b.set_values(torch.tensor(b.export(2), device="cuda"))
    refused("set_values after the forward")
    b.forward(flat_gpu)
    got = b.input_grads(flat_gpu, dl)
    _, want = _forward_input_grads(LPBatch, subset5[:2], flat_gpu, dl.double().cpu())
    _same(got, want, "after the refusals")
