"""CPU tests of the oracle itself: golden vectors, analytic known answers, and agreement of the
literal edge-list form (oracle #1, torch autograd) with the SpMM form (oracle #2, hand backward)."""
import json
import os

import numpy as np
import pytest
import torch

from mllp_amd.data import SUBSET5, LPInstance, load_packed
from oracle import pyg_restatement as o1
from oracle import spmm_form as o2

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _sd_from_flat(flat, dtype=torch.float64):
    return o1.unflatten_state(torch.tensor(np.asarray(flat), dtype=dtype))


def test_param_count_and_keys():
    spec = o1.state_dict_spec()
    assert sum(int(np.prod(s)) for _, s in spec) == 4721
    assert spec[0][0] == "gconv1_w2s.lin_key.weight" and spec[-1][0] == "fc.bias"
    assert sum(int(np.prod(s)) for k, s in spec if k.startswith("gconv1_w2s.")) == 144
    assert sum(int(np.prod(s)) for k, s in spec if k.startswith("gconv3_s2w.")) == 1104


def test_loader_digest_matches_pack():
    """The packed fixture is byte-identical to what the reference loader returned (digest made by
    tests/golden/make_golden.py through the imported reference loader)."""
    import hashlib
    with open(os.path.join(ROOT, "tests", "golden", "loader_digest.json")) as fh:
        dig = json.load(fh)
    inst = load_packed()
    assert len(inst) == 97 and sorted(dig) == [i.name for i in inst]
    assert sum(i.nnz for i in inst) == 1074147 and sum(i.m for i in inst) == 102466 and sum(i.n for i in inst) == 263910
    for i in inst:
        h = hashlib.sha256()
        for a in (i.indptr.astype(np.int64), i.indices.astype(np.int32), i.values.astype(np.float64),
                  i.coefs.astype(np.float64), i.rhs.astype(np.float64), i.basis.astype(np.int32)):
            h.update(np.ascontiguousarray(a).tobytes())
        assert dig[i.name]["sha256"] == h.hexdigest(), i.name


def test_golden_inputs_equal_pack(golden, subset5):
    for i in subset5:
        k = i.name.replace(".mps", "")
        np.testing.assert_array_equal(golden[f"{k}_indptr"], i.indptr)
        np.testing.assert_array_equal(golden[f"{k}_indices"], i.indices)
        np.testing.assert_array_equal(golden[f"{k}_values"], i.values)
        np.testing.assert_array_equal(golden[f"{k}_coefs"], i.coefs)
        np.testing.assert_array_equal(golden[f"{k}_basis"], i.basis)


def test_oracle_reproduces_golden(golden, subset5):
    sd = _sd_from_flat(golden["weights_flat"])
    loss, logits, grads = o1.batch_loss_and_grads(sd, subset5, torch.float64)
    np.testing.assert_allclose(float(loss), float(golden["batch_loss"]), rtol=1e-12)
    np.testing.assert_allclose(torch.cat(logits).numpy(), golden["batch_logits"], rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(grads.numpy(), golden["batch_grads"], rtol=1e-9, atol=1e-14)


def test_graph_build_literal_equals_vectorised(subset5):
    for inst in subset5:
        name, constrs, w, coefs, rhs, basis = inst.as_reference_tuple()
        a = o1.build_graph_literal(constrs, w, rhs, coefs)
        b = o1.build_graph(constrs, w, rhs, coefs)
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and torch.equal(x, y)
        assert a[0].shape == (2, inst.nnz) and a[0].dtype == torch.long   # [var ; constr], CSR order
        assert a[1].shape == (inst.n, 1) and a[2].shape == (inst.m, 1) and a[3].dtype == torch.float32


def test_batch_equals_per_instance_loop(golden, subset5):
    """Block-diagonal batching (BipartiteData.__inc__) must not couple instances."""
    sd = _sd_from_flat(golden["weights_flat"])
    graphs = [o1.instance_graph(i, torch.float64) for i in subset5]
    zb = o1.gnn_forward(sd, *o1.batch_graphs(graphs))
    zs = torch.cat([o1.gnn_forward(sd, *g) for g in graphs])
    np.testing.assert_allclose(zb.numpy(), zs.numpy(), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(zs[138:138 + 51].numpy(), golden["afiro_logits"], rtol=1e-11, atol=1e-13)


def _toy_sd(seed=0):
    return o1.init_state(seed, torch.float64)


def test_known_answer_single_edge_and_zero_degree():
    """deg(i) == 1  =>  alpha = 1  =>  out_i = v_j + a*w_e + skip_i ;  deg(i) == 0  =>  out_i = skip_i."""
    sd = _toy_sd(1)
    p = "gconv2_s2w"
    xs, xd = torch.randn(3, 16, dtype=torch.float64), torch.randn(4, 16, dtype=torch.float64)
    ei = torch.tensor([[2, 0], [1, 3]])          # edges 2->1 and 0->3 ; destinations 0 and 2 are isolated
    ea = torch.tensor([[0.7], [-0.3]], dtype=torch.float64)
    out = o1.transformer_conv(sd, p, xs, xd, ei, ea)
    skip = xd @ sd[f"{p}.lin_skip.weight"].T + sd[f"{p}.lin_skip.bias"]
    val = xs @ sd[f"{p}.lin_value.weight"].T + sd[f"{p}.lin_value.bias"]
    we = sd[f"{p}.lin_edge.weight"][:, 0]
    np.testing.assert_allclose(out[0].numpy(), skip[0].numpy(), rtol=1e-13)
    np.testing.assert_allclose(out[2].numpy(), skip[2].numpy(), rtol=1e-13)
    np.testing.assert_allclose(out[1].numpy(), (val[2] + 0.7 * we + skip[1]).numpy(), rtol=1e-13)
    np.testing.assert_allclose(out[3].numpy(), (val[0] - 0.3 * we + skip[3]).numpy(), rtol=1e-13)


def test_known_answer_equal_logits_is_mean():
    """query == 0 (zero query weight and bias)  =>  all logits equal  =>  mean aggregation."""
    sd = _toy_sd(2)
    p = "gconv2_w2s"
    sd[f"{p}.lin_query.weight"].zero_()
    sd[f"{p}.lin_query.bias"].zero_()
    xs, xd = torch.randn(5, 16, dtype=torch.float64), torch.randn(1, 16, dtype=torch.float64)
    ei = torch.tensor([[0, 1, 2, 3, 4], [0, 0, 0, 0, 0]])
    ea = torch.randn(5, 1, dtype=torch.float64)
    out = o1.transformer_conv(sd, p, xs, xd, ei, ea)
    val = xs @ sd[f"{p}.lin_value.weight"].T + sd[f"{p}.lin_value.bias"] + ea * sd[f"{p}.lin_edge.weight"][:, 0]
    skip = xd @ sd[f"{p}.lin_skip.weight"].T + sd[f"{p}.lin_skip.bias"]
    np.testing.assert_allclose(out[0].numpy(), (val.mean(0) + skip[0]).numpy(), rtol=1e-12)


def test_edge_permutation_invariance(subset5):
    sd = _toy_sd(3)
    ei, x1, x2, ea = o1.instance_graph(subset5[1], torch.float64)
    perm = torch.randperm(ei.shape[1], generator=torch.Generator().manual_seed(5))
    z0 = o1.gnn_forward(sd, ei, x1, x2, ea)
    z1 = o1.gnn_forward(sd, ei[:, perm], x1, x2, ea[perm])
    np.testing.assert_allclose(z0.numpy(), z1.numpy(), rtol=1e-11, atol=1e-13)


def test_spmm_form_equals_literal_form(golden, subset5):
    """oracle #2 (refactored forward + hand-derived backward) == oracle #1 (autograd), fp64."""
    flat = golden["weights_flat"]
    sd_np = {k: v.numpy() for k, v in _sd_from_flat(flat).items()}
    r = o2.gnn_forward_backward(sd_np, o2.BatchCSR(subset5))
    np.testing.assert_allclose(r["logits"], golden["batch_logits"], rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(r["loss"], float(golden["batch_loss"]), rtol=1e-12)
    np.testing.assert_allclose(r["grads"], golden["batch_grads"], rtol=1e-8, atol=1e-15)
    # the never-called gconv3_s2w receives no gradient (reference methods.py:248)
    spec, off = o1.state_dict_spec(), 0
    for k, s in spec:
        c = int(np.prod(s))
        if k.startswith("gconv3_s2w"):
            assert not r["grads"][off:off + c].any()
        off += c


def test_spmm_form_with_empty_rows_and_long_rows():
    """zero-degree rows/columns and one long row, random weights: #1 == #2 incl. gradients."""
    rng = np.random.default_rng(7)
    m, n = 9, 40
    dense = (rng.random((m, n)) < 0.15) * rng.standard_normal((m, n))
    dense[3, :] = 0.0              # empty constraint row
    dense[:, 5] = 0.0              # empty variable column
    dense[6, :] = rng.standard_normal(n) * (np.arange(n) != 5)   # long row
    import scipy.sparse as sp
    A = sp.csr_matrix(dense)
    A.sort_indices()
    inst = LPInstance("toy", A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data,
                      rng.standard_normal(n), np.abs(rng.standard_normal(m)), (rng.random(n) < 0.4).astype(np.int32))
    sd = o1.init_state(11, torch.float64)
    loss, logits, grads = o1.batch_loss_and_grads(sd, [inst, inst], torch.float64)
    r = o2.gnn_forward_backward({k: v.numpy() for k, v in sd.items()}, o2.BatchCSR([inst, inst]))
    np.testing.assert_allclose(r["logits"], torch.cat(logits).numpy(), rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(r["grads"], grads.numpy(), rtol=1e-8, atol=1e-15)


def test_reference_trainer_golden(golden, subset5):
    sd = _sd_from_flat(golden["weights_flat"])
    afiro = [i for i in subset5 if i.name == "afiro.mps"][0]
    tr = o1.ReferenceTrainer(sd, lr=1e-3, dtype=torch.float64)
    losses = [tr.step(afiro)[0] for _ in range(3)]
    np.testing.assert_allclose(losses, golden["afiro_adam3_losses"], rtol=1e-11)
    np.testing.assert_allclose(o1.flatten_state(tr.sd).detach().numpy(), golden["afiro_adam3_weights"], rtol=1e-9, atol=1e-12)
    # flat Adam of oracle #2 follows torch.optim.Adam
    flat = golden["weights_flat"].copy()
    m, v = np.zeros_like(flat), np.zeros_like(flat)
    for step in range(1, 4):
        r = o2.gnn_forward_backward({k: t.numpy() for k, t in _sd_from_flat(flat).items()}, o2.BatchCSR([afiro]))
        o2.adam_step(flat, r["grads"], m, v, step, lr=1e-3)
    np.testing.assert_allclose(flat, golden["afiro_adam3_weights"], rtol=1e-8, atol=1e-11)


def test_topk_metrics_matches_sklearn():
    from sklearn.metrics import f1_score
    rng = np.random.default_rng(0)
    z, y = rng.standard_normal(50), (rng.random(50) < 0.4).astype(np.int32)
    tp, f1 = o1.topk_metrics(z, 17, y)
    pred = np.zeros(50)
    pred[np.argsort(-z)[:17]] = 1
    assert tp == pred @ y and abs(f1 - f1_score(y, pred)) < 1e-12


# ---- identities the throughput-regime GPU tests (tests/test_throughput_oracle.py) rely on -------------------------------
def _sd_np(golden):
    return {k: v.numpy() for k, v in _sd_from_flat(golden["weights_flat"]).items()}


def test_dlogits_equal_to_the_bce_gradient_gives_the_default_gradients(golden, subset5):
    sd, b = _sd_np(golden), o2.BatchCSR(subset5)
    r = o2.gnn_forward_backward(sd, b)
    dz = b.wnode * (1.0 / (1.0 + np.exp(-r["logits"])) - b.basis)
    r2 = o2.gnn_forward_backward(sd, b, dlogits=dz)
    assert r2["loss"] == r["loss"]
    np.testing.assert_array_equal(r2["logits"], r["logits"])
    np.testing.assert_array_equal(r2["grads"], r["grads"])


def test_dlogits_on_one_instance_equal_that_instance_alone(golden, subset5):
    """Block-diagonal batching: a dL/dz that is nonzero on instance k only gives instance k's own gradients, and the
    logits of the batch cut at instance k are the logits of the instance alone."""
    sd, b = _sd_np(golden), o2.BatchCSR(subset5)
    full = o2.gnn_forward_backward(sd, b, want_grads=False)
    off = np.concatenate([[0], np.cumsum(b.inst_n)])
    rng = np.random.default_rng(17)
    for k, inst in enumerate(subset5):
        alone = o2.gnn_forward_backward(sd, o2.BatchCSR([inst]), want_grads=False)
        np.testing.assert_allclose(full["logits"][off[k]:off[k + 1]], alone["logits"], rtol=1e-12, atol=1e-14)
        dz_k = rng.standard_normal(inst.n) / inst.n
        dz = np.zeros(b.N)
        dz[off[k]:off[k + 1]] = dz_k
        gb = o2.gnn_forward_backward(sd, b, dlogits=dz)["grads"]
        ga = o2.gnn_forward_backward(sd, o2.BatchCSR([inst]), dlogits=dz_k)["grads"]
        scale = np.abs(ga).max()
        assert scale > 0
        assert np.abs(gb - ga).max() <= 1e-12 * scale, inst.name


def test_replicated_batch_has_the_same_loss_and_gradients(golden, subset5):
    """loss = (1/B) sum_k mean-BCE(k): subset5 repeated three times in a shuffled order trains exactly like subset5."""
    sd = _sd_np(golden)
    order = np.random.default_rng(23).permutation(3 * len(subset5))
    rep = [subset5[i % len(subset5)] for i in order]
    r1 = o2.gnn_forward_backward(sd, o2.BatchCSR(subset5))
    r3 = o2.gnn_forward_backward(sd, o2.BatchCSR(rep))
    np.testing.assert_allclose(r3["loss"], r1["loss"], rtol=1e-12)
    assert np.abs(r3["grads"] - r1["grads"]).max() <= 1e-12 * np.abs(r1["grads"]).max()


def test_cut_instance_returns_every_netlib_instance():
    from batch_slices import cut_instance
    inst = load_packed()
    b = o2.BatchCSR(inst)
    for k, i in enumerate(inst):
        c = cut_instance(b.rp, b.ci, b.va, b.x1, b.x2, b.basis, b.inst_m, b.inst_n, k, name=i.name)
        assert (c.m, c.n, c.nnz) == (i.m, i.n, i.nnz), i.name
        for a, w in ((c.indptr, i.indptr), (c.indices, i.indices), (c.values, i.values), (c.coefs, i.coefs),
                     (c.rhs, i.rhs), (c.basis, i.basis)):
            assert a.dtype == w.dtype and np.array_equal(a, w), i.name
