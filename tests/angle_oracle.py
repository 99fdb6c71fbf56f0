"""Oracles of AngleModel shared by tests/test_angle.py, tests/test_angle_input_grads.py and tests/test_angle_shapes.py
(a plain helper module like tests/oracle_trainer.py).

* `edge_forward`: the oracle's literal TransformerConv (oracle/pyg_restatement.py) on the explicit N (N - 1) edge list.
* `dense_conv` / `dense_forward`: the same model on the complete graph as dense matrices, in any CPU dtype.  It is licensed
  by its equality with the edge-list form (1e-9 .. 1e-12 in fp64: test_input_grads_vs_edge_list_oracle on the GPU cases,
  test_dense_restatement_equals_edge_list_oracle_at_the_tails at N = 2 and 17 without a GPU) and used where the edge list
  is too large.  Its fp32 run is the yardstick of the row-wise tolerances of tests/test_angle_shapes.py.
* `oracle_grads`: autograd of either form: logits, loss, dx, dcos, every parameter gradient.
* `sweep_backward`: the kernels' hand-derived backward with the cosine matrix of each sweep as an argument of its own (what a
  non-symmetric matrix gives).
* `close` (tensor-max-normalised) and `close_rows` (row-wise) comparisons.
* the two host formulas of mllp_amd/csrc/angle.hip that decide what a size reaches (ranges of X blocks per attention
  sweep, K splits of the weight-gradient GEMM, the carve of the workspace), restated in Python.
"""
import math

import numpy as np
import torch

from oracle import pyg_restatement as o1

RTOL_LOGITS, RTOL_GRAD = 1e-5, 5e-5
ROW_FLOOR = 1e-3              # a row's scale is at least this fraction of the tensor's max |ref|


def close(got, want, rtol, what=""):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, f"{what}: {got.shape} vs {want.shape}"
    assert np.isfinite(got).all(), what
    err = float(np.abs(got - want).max()) / max(float(np.abs(want).max()), 1e-30)
    assert err <= rtol, f"{what}: max|diff|/max|ref| = {err:.3e} > {rtol}"


def row_ratio(got, want):
    """(worst row-wise ratio, its row): max over rows of max|got - ref| / max(row max|ref|, ROW_FLOOR tensor max|ref|)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and got.ndim == 2, (got.shape, want.shape)
    scale = np.maximum(np.abs(want).max(axis=1), ROW_FLOOR * max(float(np.abs(want).max()), 1e-300))
    ratio = np.abs(got - want).max(axis=1) / scale
    row = int(np.argmax(ratio))
    return float(ratio[row]), row


def close_rows(got, want, tol, what=""):
    assert np.isfinite(np.asarray(got)).all(), what
    ratio, row = row_ratio(got, want)
    assert ratio <= tol, f"{what}: row {row}: max|diff| / max(row max|ref|, floor) = {ratio:.3e} > {tol:.3e}"


# ---------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------
def edge_forward(sd, x, ei, ea):
    """reference linear_program_methods.py:195-200 with the oracle's literal TransformerConv on the edge list"""
    h = torch.relu(o1.transformer_conv(sd, "gconv1", x, x, ei, ea))
    h = torch.relu(o1.transformer_conv(sd, "gconv2", h, h, ei, ea))
    h = torch.relu(o1.transformer_conv(sd, "gconv2", h, h, ei, ea))
    return (h @ sd["fc.weight"].T + sd["fc.bias"]).squeeze(-1)[:-1]


def dense_scores(sd, prefix, X, A):
    """L_ij of one layer (target i, source j), diagonal -inf"""
    W = lambda name: sd[f"{prefix}.{name}"]
    F = W("lin_query.weight").shape[0]
    Q = X @ W("lin_query.weight").T + W("lin_query.bias")
    K = X @ W("lin_key.weight").T + W("lin_key.bias")
    we = W("lin_edge.weight")[:, 0]
    S = (Q @ K.T + (Q @ we)[:, None] * A) / math.sqrt(F)
    return S.masked_fill(torch.eye(A.shape[0], dtype=torch.bool), float("-inf"))


def dense_conv(sd, prefix, X, A):
    """the same TransformerConv on the complete graph as dense matrices: target i (row), source j (column),
    A[i, j] = attribute of edge j -> i, no self loops; softmax as torch_geometric.utils.softmax"""
    W = lambda name: sd[f"{prefix}.{name}"]
    V = X @ W("lin_value.weight").T + W("lin_value.bias")
    we = W("lin_edge.weight")[:, 0]
    S = dense_scores(sd, prefix, X, A)
    P = (S - S.detach().amax(dim=1, keepdim=True)).exp()
    P = P / (P.sum(dim=1, keepdim=True) + 1e-16)
    A0 = A.masked_fill(torch.eye(A.shape[0], dtype=torch.bool), 0.0)      # (P is 0 there: keeps a non-finite diagonal out)
    return P @ V + (P * A0).sum(dim=1, keepdim=True) * we[None, :] + X @ W("lin_skip.weight").T + W("lin_skip.bias")


def dense_forward(sd, x, A, dtype=None):
    """logits [N - 1] of the dense restatement; with `dtype` everything is cast first (torch.float64 or torch.float32)"""
    if dtype is not None:
        sd = {k: v.to(dtype) for k, v in sd.items()}
        x, A = x.to(dtype), A.to(dtype)
    h = torch.relu(dense_conv(sd, "gconv1", x, A))
    h = torch.relu(dense_conv(sd, "gconv2", h, A))
    h = torch.relu(dense_conv(sd, "gconv2", h, A))
    return (h @ sd["fc.weight"].T + sd["fc.bias"]).squeeze(-1)[:-1]


def oracle_grads(state_dict, x, cos, y, dense=True, dtype=torch.float64, edge_index=None):
    """CPU autograd of mean BCE(logits, y): (logits, loss, dx [N, 2], dcos [N, N] with zero diagonal,
    {name: parameter gradient or None}); `dense=False` runs the edge-list form (needs edge_index)"""
    sd = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in state_dict.items()}
    x = x.detach().cpu().to(dtype).requires_grad_(True)
    N = x.shape[0]
    if dense:
        A = cos.detach().cpu().to(dtype).requires_grad_(True)
        z = dense_forward(sd, x, A)
    else:
        ei = edge_index.cpu()
        ea = cos.detach().cpu().to(dtype)[ei[1], ei[0]].unsqueeze(-1).requires_grad_(True)
        z = edge_forward(sd, x, ei, ea)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(z, y.detach().cpu().to(dtype))
    names = list(sd)
    grads = torch.autograd.grad(loss, [x, A if dense else ea] + [sd[k] for k in names], allow_unused=True)
    if dense:
        dcos = grads[1]
    else:
        dcos = torch.zeros(N, N, dtype=dtype)
        dcos[ei[1], ei[0]] = grads[1][:, 0]
    return z.detach(), loss.detach(), grads[0], dcos, dict(zip(names, grads[2:]))


def oracle(model, g, y, dense):
    """fp64 autograd: (logits, dx [N, 2], dcos [N, N] with zero diagonal, {name: parameter gradient})"""
    z, _, dx, dcos, params = oracle_grads(model.state_dict(), g.x, g.cos, y, dense, torch.float64,
                                          None if dense else g.edge_index)
    return z, dx, dcos, params


def sweep_backward(sd, x, A_f, A_q, A_kv, dlogits):
    """The kernels' hand-derived backward (mllp_amd/csrc/angle.hip) as dense matrices in the dtype of its
    arguments, with the matrix each sweep reads as an argument of its own, all indexed [target i][source j]: A_f the
    forward, A_q the query sweep (dQ, r, dcos), A_kv the key / value sweep (dK, dV); the backward sweeps recompute the
    attention weights from the forward's row maximum and row sum.  With A_f = A_q = A_kv it is autograd's gradient of
    sum(logits * dlogits) (tests/test_angle_shapes.py checks that without a GPU).
    Returns (logits, dx, dcos, {name: parameter gradient})."""
    N = x.shape[0]
    eye = torch.eye(N, dtype=torch.bool)
    off = lambda A: A.masked_fill(eye, 0.0)
    layers, h = [], x
    for prefix in ("gconv1", "gconv2", "gconv2"):
        W = lambda name: sd[f"{prefix}.{name}"]
        we = W("lin_edge.weight")[:, 0]
        sc = 1.0 / math.sqrt(we.shape[0])
        Q = h @ W("lin_query.weight").T + W("lin_query.bias")
        K = h @ W("lin_key.weight").T + W("lin_key.bias")
        V = h @ W("lin_value.weight").T + W("lin_value.bias")
        qe = Q @ we
        L = ((Q @ K.T + qe[:, None] * off(A_f)) * sc).masked_fill(eye, float("-inf"))
        m = L.amax(dim=1)
        E = (L - m[:, None]).exp()
        inv = 1.0 / (E.sum(dim=1) + 1e-16)
        P = E * inv[:, None]
        Oa, s = P @ V, (P * off(A_f)).sum(dim=1)
        H = torch.relu(Oa + s[:, None] * we[None, :] + h @ W("lin_skip.weight").T + W("lin_skip.bias"))
        layers.append((prefix, h, Q, K, V, qe, m, inv, Oa, s, H, we, sc))
        h = H
    logits = (h @ sd["fc.weight"].T + sd["fc.bias"]).squeeze(-1)[:-1]
    grads = {k: torch.zeros_like(v) for k, v in sd.items()}
    grads["fc.weight"] = (dlogits[:, None] * h[:-1]).sum(dim=0)[None, :]
    grads["fc.bias"] = dlogits.sum()[None]
    dH = torch.zeros_like(h)
    dH[:-1] = dlogits[:, None] * sd["fc.weight"][0][None, :]
    dcos = torch.zeros_like(A_f)
    for prefix, X, Q, K, V, qe, m, inv, Oa, s, H, we, sc in reversed(layers):
        W = lambda name: sd[f"{prefix}.{name}"]
        dO = dH * (H > 0)
        u = dO @ we
        D = (dO * Oa).sum(dim=1) + u * s

        def sweep(A):
            A0 = off(A)
            P = (((Q @ K.T + qe[:, None] * A0) * sc - m[:, None]).exp() * inv[:, None]).masked_fill(eye, 0.0)
            return P, P * (dO @ V.T + u[:, None] * A0 - D[:, None]) * sc, A0
        Pq, dzq, Aq0 = sweep(A_q)
        r = (dzq * Aq0).sum(dim=1)
        dQ = dzq @ K + r[:, None] * we[None, :]
        dcos = dcos + dzq * qe[:, None] + Pq * u[:, None]
        Pk, dzk, _ = sweep(A_kv)
        dV, dK = Pk.T @ dO, dzk.T @ Q
        for lin, d in (("lin_query", dQ), ("lin_key", dK), ("lin_value", dV), ("lin_skip", dO)):
            grads[f"{prefix}.{lin}.weight"] = grads[f"{prefix}.{lin}.weight"] + d.T @ X
            grads[f"{prefix}.{lin}.bias"] = grads[f"{prefix}.{lin}.bias"] + d.sum(dim=0)
        grads[f"{prefix}.lin_edge.weight"] = grads[f"{prefix}.lin_edge.weight"] + (dO.T @ s + Q.T @ r)[:, None]
        dH = dO @ W("lin_skip.weight") + dQ @ W("lin_query.weight") + dK @ W("lin_key.weight") + dV @ W("lin_value.weight")
    return logits, dH, dcos, grads


# ---------------------------------------------------------------------------------------------------
# host formulas of mllp_amd/csrc/angle.hip
# ---------------------------------------------------------------------------------------------------
ATT_W, GK = 4, 32             # Y blocks of 16 nodes per workgroup; K step of the GEMM tile


def n_xblocks(N):
    return (N + 15) // 16


def attn_ranges(N):
    """ranges of X blocks the workspace is sized for"""
    nb = n_xblocks(N)
    yg = (nb + ATT_W - 1) // ATT_W
    return max(1, min(min(nb, 32), 256 // min(yg, 256)))


def xb_per_range(N):
    R = attn_ranges(N)
    return (n_xblocks(N) + R - 1) // R


def launched_ranges(N):
    """ranges the attention sweeps actually launch (blockIdx.y), <= attn_ranges"""
    return (n_xblocks(N) + xb_per_range(N) - 1) // xb_per_range(N)


def gemm_ksplits(K):
    return max(1, min(32, K // 256))


def kchunk(K):
    ks = gemm_ksplits(K)
    return ((K + ks - 1) // ks + GK - 1) // GK * GK


def _up(x):
    return (x + 63) & ~63


def angle_ws_floats(N, F):
    R, ks = attn_ranges(N), gemm_ksplits(N)
    return (3 * (6 * _up(N * F) + 4 * _up(N)) + 5 * _up(N * F) + 3 * _up(N) + 2 * _up(R * N * F) + _up(R * N * 4)
            + _up(4 * ks * F * (F + 1)))
