"""The weighted loss head (mllp_weighted_loss, mllp_balanced_pos_weight, mllp_gnn_loss_step_weighted; LPBatch.weighted_loss,
.balanced_pos_weight, .loss_step_weighted, .evaluate; LPTrainer(pos_weight=...)) against an fp64 numpy oracle written here
from the formulas of include/mllp_hip.h:

    sp_i = max(-z_i, 0) + log1p(exp(-|z_i|))
    l_i  = (1 - y_i) z_i + (1 + (pw_k - 1) y_i) sp_i
    L_k  = (1 / n_k) sum_i l_i                                   0 for n_k = 0, not multiplied by w_k
    dz_i = (w_k / n_k) ((1 - y_i) - (1 + (pw_k - 1) y_i) (1 - sigmoid(z_i)))
    loss = sum_k w_k L_k

The oracle itself is checked on the CPU against torch.nn.functional.binary_cross_entropy_with_logits(pos_weight=...) in
fp64.  Bars: losses 1e-5 and gradients 5e-5, max-norm relative (`close`, RTOL_ACT, RTOL_GRAD of tests/test_hip_parity.py);
dlogits 1e-5 of max |ref|; the three-step Adam trajectory 1e-5 relative per loss (tests/test_small_step.py).

Measured on MI355X (max |got - ref| / max |ref|): see DESIGN.md, "Weighted loss head".
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import fused_cases as fc
from mllp_amd import _lib
from oracle import pyg_restatement as o1
from oracle import spmm_form as o2
from test_hip_parity import RTOL_ACT, RTOL_GRAD, close, grad_mask

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
MLLP_EINVAL = -1
NEW_SYMBOLS = ("mllp_weighted_loss", "mllp_balanced_pos_weight", "mllp_gnn_loss_step_weighted")


# ---- the oracle -------------------------------------------------------------------------------------------------------
def oracle_loss(z, y, seg_n, w=None, pw=None):
    """fp64: dict(inst_loss [K], loss, dz [N]) for logits z, labels y, segments of seg_n columns"""
    z, y = np.asarray(z, np.float64), np.asarray(y, np.float64)
    K = len(seg_n)
    w = np.ones(K) if w is None else np.asarray(w, np.float64)
    pw = np.ones(K) if pw is None else np.asarray(pw, np.float64)
    off = np.concatenate([[0], np.cumsum(seg_n)]).astype(np.int64)
    L, dz, loss = np.zeros(K), np.zeros(z.shape[0]), 0.0
    for k in range(K):
        zz, yy, n = z[off[k]:off[k + 1]], y[off[k]:off[k + 1]], int(seg_n[k])
        if n == 0:
            continue
        e = np.exp(-np.abs(zz))
        sp = np.maximum(-zz, 0.0) + np.log1p(e)
        c = 1.0 + (pw[k] - 1.0) * yy
        L[k] = ((1.0 - yy) * zz + c * sp).sum() / n
        one_minus_sig = np.where(zz >= 0, e / (1.0 + e), 1.0 / (1.0 + e))
        dz[off[k]:off[k + 1]] = (w[k] / n) * ((1.0 - yy) - c * one_minus_sig)
    for k in range(K):                      # instance order
        loss += w[k] * L[k]
    return dict(inst_loss=L, loss=loss, dz=dz)


def oracle_balanced(y, seg_n):
    off = np.concatenate([[0], np.cumsum(seg_n)]).astype(np.int64)
    out = np.ones(len(seg_n))
    for k, n in enumerate(seg_n):
        P = float(np.asarray(y[off[k]:off[k + 1]], np.float64).sum())
        if 0.0 < P < n:
            out[k] = (n - P) / P
    return out


# ---- CPU --------------------------------------------------------------------------------------------------------------
def test_oracle_equals_torch_bce_with_logits_pos_weight():
    F = torch.nn.functional
    rng = np.random.default_rng(0)
    seg_n = [1, 7, 0, 130, 33]
    N = sum(seg_n)
    z = rng.standard_normal(N) * 4.0
    z[:6] = [0.0, -0.0, 30.0, -30.0, 88.0, -88.0]
    z[-2:] = [1e4, -1e4]
    y = (rng.random(N) < 0.3).astype(np.float64)
    y[10:40] = rng.random(30)                       # any label in [0, 1]
    w, pw = rng.random(len(seg_n)) * 2.0, 0.25 + rng.random(len(seg_n)) * 7.75
    w[1] = 0.0
    got = oracle_loss(z, y, seg_n, w, pw)
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    yt = torch.tensor(y, dtype=torch.float64)
    off = np.concatenate([[0], np.cumsum(seg_n)])
    Ls = [F.binary_cross_entropy_with_logits(zt[off[k]:off[k + 1]], yt[off[k]:off[k + 1]],
                                             pos_weight=torch.full((seg_n[k],), pw[k], dtype=torch.float64))
          if seg_n[k] else torch.zeros((), dtype=torch.float64) for k in range(len(seg_n))]
    loss = sum(float(w[k]) * Ls[k] for k in range(len(seg_n)))
    loss.backward()
    np.testing.assert_allclose(got["inst_loss"], [float(v.detach()) for v in Ls], rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(got["loss"], float(loss.detach()), rtol=1e-13)
    np.testing.assert_allclose(got["dz"], zt.grad.numpy(), rtol=1e-12, atol=1e-16)
    assert np.isfinite(got["dz"]).all() and np.isfinite(got["inst_loss"]).all()
    # unweighted: the loss the library has always computed (oracle/spmm_form.py)
    plain = oracle_loss(z, y, seg_n)
    bce = np.maximum(z, 0) - z * y + np.log1p(np.exp(-np.abs(z)))
    want = [bce[off[k]:off[k + 1]].mean() if seg_n[k] else 0.0 for k in range(len(seg_n))]
    np.testing.assert_allclose(plain["inst_loss"], want, rtol=1e-13, atol=1e-15)


def _header_args(name):
    src = open(_lib.HEADER_PATH).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in include/mllp_hip.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_symbols_header_and_ctypes_signatures():
    L = _lib.lib()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), f"{name} is not exported"
        args = _header_args(name)
        res, argtypes = _lib._PROTOTYPES[name]
        assert res is ctypes.c_int and len(argtypes) == len(args), name
        assert all("*" in a for a in args) and all(t is ctypes.c_void_p for t in argtypes), name
        assert getattr(L, name).argtypes == argtypes
    doc = open(_lib.HEADER_PATH).read()
    assert "linear_program_experiment.py:41" in doc and "139-141" in doc
    assert "weighted_loss.o" in open(os.path.join(ROOT, "mllp_amd", "csrc", "Makefile")).read()


def test_null_arguments_are_refused_without_a_device():
    L = _lib.lib()
    fake = ctypes.create_string_buffer(4096)          # never dereferenced: every check below fails first
    p, nul = ctypes.c_void_p(ctypes.addressof(fake)), ctypes.c_void_p(0)
    for args in ((nul, p, p), (p, nul, p), (p, p, nul)):
        assert L.mllp_weighted_loss(*args, nul, nul, p, p, p, nul) == MLLP_EINVAL
        assert b"mllp_weighted_loss" in L.mllp_last_error() and b"null" in L.mllp_last_error()
    assert L.mllp_weighted_loss(p, p, p, p, p, nul, nul, nul, nul) == MLLP_EINVAL
    assert b"null outputs" in L.mllp_last_error()
    for args in ((nul, p, p), (p, nul, p), (p, p, nul)):
        assert L.mllp_balanced_pos_weight(*args, nul) == MLLP_EINVAL
        assert b"mllp_balanced_pos_weight" in L.mllp_last_error() and b"null" in L.mllp_last_error()
    # the step: g, params, x1, x2, labels | inst_weight, pos_weight (optional) | ws, logits | loss, inst_loss (optional) |
    # grads, dlogits
    required = (0, 1, 2, 3, 4, 7, 8, 11, 12)
    for miss in required:
        args = [nul if i == miss else p for i in range(13)]
        assert L.mllp_gnn_loss_step_weighted(*args, nul) == MLLP_EINVAL, miss
        assert b"mllp_gnn_loss_step_weighted" in L.mllp_last_error() and b"null" in L.mllp_last_error()


# ---- GPU --------------------------------------------------------------------------------------------------------------
N_K = [0, 1, 63, 64, 65, 1023, 1024, 1025, 4097]
K_ZEROS, K_ONES, K_W0 = 2, 7, 5                       # the all-zero-label, all-one-label and weight-0 instances
PLANTS = [0.0, -0.0, 30.0, -30.0, 88.0, -88.0, 1e4, -1e4]


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def dev():
    _lib.lib()
    assert torch.cuda.is_available()
    from mllp_amd.graph import LPBatch
    return LPBatch


@pytest.fixture(scope="module")
def case1(dev):
    """The kernel-alone case: instances without nonzeros, computed once and never modified."""
    rng = np.random.default_rng(11)
    insts = []
    for k, n in enumerate(N_K):
        it = fc.empty_instance(1, n, seed=k)
        it.name = f"seg{k}_{n}"
        it.basis = (np.zeros(n) if k == K_ZEROS else np.ones(n) if k == K_ONES else rng.random(n) < 0.3).astype(np.int32)
        insts.append(it)
    off = np.concatenate([[0], np.cumsum(N_K)])
    z = rng.standard_normal(off[-1]).astype(np.float32)
    j = 0
    for k, n in enumerate(N_K):
        if n:
            z[off[k]], z[off[k + 1] - 1] = PLANTS[(2 * j) % 8], PLANTS[(2 * j + 1) % 8]
            j += 1
    w = (rng.random(len(N_K)) * 2.0).astype(np.float32)
    w[K_W0] = 0.0
    pw = (0.25 + rng.random(len(N_K)) * 7.75).astype(np.float32)
    y = np.concatenate([i.basis for i in insts]).astype(np.float64)
    ref = oracle_loss(z, y, N_K, w, pw)
    b = dev.from_instances(insts)
    g = lambda a: torch.tensor(a, dtype=torch.float32, device="cuda")  # noqa: E731
    return dict(insts=insts, off=off, z=z, w=w, pw=pw, y=y, ref=ref, b=b, zt=g(z), wt=g(w), pwt=g(pw))


@pytest.mark.gpu
def test_kernel_alone_against_oracle(case1):
    c = case1
    b, ref, off = c["b"], c["ref"], c["off"]
    r = b.weighted_loss(c["zt"], c["wt"], c["pwt"])
    torch.cuda.synchronize()
    L, loss, dz = r["inst_loss"].cpu().numpy(), r["loss"].cpu().numpy(), r["dlogits"].cpu().numpy()
    print(f"inst_loss {fc.rel_err(L, ref['inst_loss']):.2e}, loss {abs(float(loss[0]) - ref['loss']) / abs(ref['loss']):.2e}, "
          f"dlogits {fc.rel_err(dz, ref['dz']):.2e}")
    assert np.isfinite(L).all() and np.isfinite(loss).all() and np.isfinite(dz).all()
    close(L, ref["inst_loss"], RTOL_ACT, "inst_loss")
    close(loss, np.array([ref["loss"]]), RTOL_ACT, "loss")
    close(dz, ref["dz"], 1e-5, "dlogits")
    assert L[0] == 0.0                                                  # n_k = 0
    k = K_W0
    assert not dz[off[k]:off[k + 1]].any()                              # w_k = 0: exactly no gradient ...
    assert abs(L[k] - ref["inst_loss"][k]) <= RTOL_ACT * abs(ref["inst_loss"][k]) and L[k] > 0.1       # ... and its loss
    # each output alone (loss alone: the one-workgroup launch), and in pairs: the bits of the call for all three
    for want in ("loss", "inst_loss", "dlogits", ("loss", "dlogits"), ("loss", "inst_loss"), ("inst_loss", "dlogits")):
        one = b.weighted_loss(c["zt"], c["wt"], c["pwt"], want=want)
        names = (want,) if isinstance(want, str) else want
        for name in ("loss", "inst_loss", "dlogits"):
            if name in names:
                assert _bits(one[name]) == _bits(r[name]), (want, name)
            else:
                assert one[name] is None
    # the C ABI with d_loss and no d_inst_loss (one workgroup takes the instances in turn): the same bits again
    lo, dz1 = torch.zeros(1, device="cuda"), torch.zeros(b.N, device="cuda")
    for dzp in (None, dz1):
        _lib.check(_lib.lib().mllp_weighted_loss(b._h, _lib.ptr(c["zt"]), _lib.ptr(b.labels), _lib.ptr(c["wt"]), _lib.ptr(c["pwt"]),
                                                 _lib.ptr(dzp), None, _lib.ptr(lo), _lib.current_stream()))
        assert _bits(lo) == _bits(r["loss"])
    assert _bits(dz1) == _bits(r["dlogits"])
    # NULL weights are ones
    ones = torch.ones(b.n_inst, device="cuda")
    a, e = b.weighted_loss(c["zt"]), b.weighted_loss(c["zt"], ones, ones)
    for name in ("loss", "inst_loss", "dlogits"):
        assert _bits(a[name]) == _bits(e[name]), name
    plain = oracle_loss(c["z"], c["y"], N_K)
    close(a["inst_loss"].cpu().numpy(), plain["inst_loss"], RTOL_ACT, "unweighted inst_loss")
    close(a["dlogits"].cpu().numpy(), plain["dz"], 1e-5, "unweighted dlogits")
    # a float broadcasts
    f = b.weighted_loss(c["zt"], 0.5, 3.0)
    h = b.weighted_loss(c["zt"], ones * 0.5, ones * 3.0)
    for name in ("loss", "inst_loss", "dlogits"):
        assert _bits(f[name]) == _bits(h[name]), name
    with pytest.raises(ValueError):
        b.weighted_loss(c["zt"], want=())
    with pytest.raises(ValueError):
        b.weighted_loss(c["zt"], pos_weight="balance")


@pytest.mark.gpu
def test_batch_independence_and_repeatability(dev, case1):
    c = case1
    b, off = c["b"], c["off"]
    r1, r2 = (b.weighted_loss(c["zt"], c["wt"], c["pwt"]) for _ in range(2))
    for name in ("loss", "inst_loss", "dlogits"):
        assert _bits(r1[name]) == _bits(r2[name]), name
    for k, inst in enumerate(c["insts"]):
        s = dev.from_instances([inst])
        one = s.weighted_loss(c["zt"][off[k]:off[k + 1]].contiguous(), c["wt"][k:k + 1].contiguous(),
                              c["pwt"][k:k + 1].contiguous())
        assert _bits(one["inst_loss"]) == _bits(r1["inst_loss"][k:k + 1]), inst.name
        assert _bits(one["dlogits"]) == _bits(r1["dlogits"][off[k]:off[k + 1]]), inst.name


@pytest.mark.gpu
def test_balanced_pos_weight(dev, case1):
    c = case1
    b = c["b"]
    pw = b.balanced_pos_weight()
    assert b.balanced_pos_weight() is pw                                # computed once
    got = pw.cpu().numpy()
    want = oracle_balanced(c["y"], N_K).astype(np.float32)
    assert got.dtype == np.float32 and got.shape == want.shape
    ulp = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    assert ulp.max() <= 1, ulp
    assert got[0] == 1.0 and got[K_ZEROS] == 1.0 and got[K_ONES] == 1.0
    assert (got[[k for k in range(len(N_K)) if k not in (0, K_ZEROS, K_ONES, 1)]] > 1.0).all()      # positives are the minority
    # 'balanced' is that tensor
    r = b.weighted_loss(c["zt"], c["wt"], "balanced")
    e = b.weighted_loss(c["zt"], c["wt"], pw)
    assert _bits(r["dlogits"]) == _bits(e["dlogits"]) and _bits(r["loss"]) == _bits(e["loss"])
    # rebinding the labels drops the cached weights
    s = dev.from_instances(c["insts"][3:5])
    first = s.balanced_pos_weight()
    s.labels = 1.0 - s.labels
    second = s.balanced_pos_weight()
    assert second is not first
    np.testing.assert_allclose(second.cpu().numpy(), 1.0 / first.cpu().numpy(), rtol=3e-7)


# ---- the whole step ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def weights(golden):
    flat = golden["weights_flat"]
    return flat, fc.golden_state(golden), torch.tensor(flat, dtype=torch.float32, device="cuda")


@pytest.fixture(scope="module")
def step_refs(golden, subset5):
    """name -> instances, weights w, and the fp64 oracle: logits of model_dt, the loss head above on them with balanced
    pos_weight, gradients of model_dt driven by the oracle's dz.  Computed once, shared, never modified."""
    sd = fc.golden_state(golden)
    out = {}
    for name, insts, seed in (("subset5", list(subset5), 5), ("ragged", fc.ragged_batch(), 6)):
        rng = np.random.default_rng(seed)
        ob = o2.BatchCSR(insts)
        seg_n = [i.n for i in insts]
        w = (rng.random(len(insts)) * 2.0).astype(np.float32)
        w[1] = 0.0
        z64 = fc.model_dt(sd, ob, np.float64)["logits"]
        ref = oracle_loss(z64, ob.basis, seg_n, w, oracle_balanced(ob.basis, seg_n))
        grads = fc.model_dt(sd, ob, np.float64, dlogits=ref["dz"])["grads"]
        out[name] = dict(insts=insts, ob=ob, seg_n=seg_n, w=w, z64=z64, ref=ref, grads=grads)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("name", ["subset5", "ragged"])
def test_whole_step_both_paths(dev, weights, step_refs, name, path):
    c = step_refs[name]
    p = weights[2]
    b = dev.from_instances(c["insts"]).set_path(path)
    z_fwd = b.forward(p).clone()
    wt = torch.tensor(c["w"], device="cuda")
    loss, logits, grads, inst_loss = b.loss_step_weighted(p, wt, "balanced")
    torch.cuda.synchronize()
    assert _bits(logits) == _bits(z_fwd)                               # the forward of this path, bit for bit
    L, ls, g = inst_loss.cpu().numpy(), loss.cpu().numpy(), grads.cpu().numpy()
    ref, keep = c["ref"], grad_mask()
    print(f"{name} path {path}: loss {abs(float(ls[0]) - ref['loss']) / abs(ref['loss']):.2e}, inst_loss "
          f"{fc.rel_err(L, ref['inst_loss']):.2e}, grads {fc.rel_err(g[keep], c['grads'][keep]):.2e}")
    close(ls, np.array([ref["loss"]]), RTOL_ACT, "loss")
    close(L, ref["inst_loss"], RTOL_ACT, "inst_loss")
    close(g[keep], c["grads"][keep], RTOL_GRAD, "grads")


@pytest.mark.gpu
@pytest.mark.parametrize("path", [1, 2])
def test_consistent_with_the_unweighted_step(dev, subset5, weights, path):
    p = weights[2]
    b = dev.from_instances(subset5).set_path(path)
    l0, z0, g0 = (t.clone() for t in b.loss_step(p))
    loss, logits, grads, inst_loss = b.loss_step_weighted(p, 1.0 / b.n_inst)
    torch.cuda.synchronize()
    assert _bits(logits) == _bits(z0)
    keep = grad_mask()
    print(f"path {path}: loss {abs(float(loss[0]) - float(l0[0])) / abs(float(l0[0])):.2e}, grads "
          f"{fc.rel_err(grads.cpu().numpy()[keep], g0.cpu().numpy()[keep]):.2e}")
    close(loss.cpu().numpy(), l0.cpu().numpy(), RTOL_ACT, "loss")
    close(grads.cpu().numpy()[keep], g0.cpu().numpy()[keep], RTOL_GRAD, "grads")
    close(inst_loss.sum().reshape(1).cpu().numpy() / b.n_inst, l0.cpu().numpy(), RTOL_ACT, "mean of inst_loss")
    # the workspace record is that of forward + backward: the input gradients of the same loss may follow
    g2, dx1, dx2, dv = b.input_grads(p, b.last_dlogits)
    torch.cuda.synchronize()
    assert _bits(g2) == _bits(grads)
    assert dx1.shape == (b.N,) and dx2.shape == (b.M,) and dv.shape == (b.nnz,)
    assert all(bool(torch.isfinite(t).all()) for t in (dx1, dx2, dv)) and bool(dx1.any())


@pytest.mark.gpu
def test_capture_and_replay(dev, subset5, weights):
    p = weights[2]
    b = dev.from_instances(subset5)
    wt = torch.rand(b.n_inst, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    bufs = [torch.zeros(b.N, device="cuda"), torch.zeros(1, device="cuda"), torch.zeros(b.n_inst, device="cuda"),
            torch.zeros(_lib.NUM_PARAMS, device="cuda")]
    run = lambda: b.loss_step_weighted(p, wt, "balanced", bufs[0], bufs[1], bufs[2], bufs[3])  # noqa: E731
    run()
    torch.cuda.synchronize()
    eager = [_bits(t) for t in bufs + [b.last_dlogits]]
    for t in bufs:
        t.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert [_bits(t) for t in bufs + [b.last_dlogits]] == eager


@pytest.mark.gpu
def test_trainer(dev, subset5, weights, golden):
    from mllp_amd.trainer import LPTrainer
    flat, _, p = weights
    # pos_weight=None is the trainer without the argument, bit for bit
    a, n = LPTrainer(p, lr=1e-3, with_metrics=True), LPTrainer(p, lr=1e-3, with_metrics=True, pos_weight=None)
    ba, bn = dev.from_instances(subset5), dev.from_instances(subset5)
    for _ in range(3):
        la, _ = a.step(ba)
        ln, _ = n.step(bn)
        assert _bits(la) == _bits(ln)
    torch.cuda.synchronize()
    assert _bits(a.params) == _bits(n.params) and _bits(a.opt.m) == _bits(n.opt.m) and _bits(a.opt.v) == _bits(n.opt.v)
    # 'balanced': three Adam steps against the fp64 trajectory driven by the oracle
    ob = o2.BatchCSR(list(subset5))
    seg_n = [i.n for i in subset5]
    pw, w = oracle_balanced(ob.basis, seg_n), np.full(len(seg_n), 1.0 / len(seg_n))
    P = np.asarray(flat, dtype=np.float64).copy()
    m, v, want = np.zeros_like(P), np.zeros_like(P), []
    for step in (1, 2, 3):
        sd = {k: t.numpy() for k, t in o1.unflatten_state(torch.tensor(P)).items()}
        ref = oracle_loss(fc.model_dt(sd, ob, np.float64)["logits"], ob.basis, seg_n, w, pw)
        want.append(ref["loss"])
        o2.adam_step(P, fc.model_dt(sd, ob, np.float64, dlogits=ref["dz"])["grads"], m, v, step)
    t = LPTrainer(p, lr=1e-3, with_metrics=True, pos_weight="balanced")
    bt = dev.from_instances(subset5)
    got = [float(t.step(bt)[0][0]) for _ in range(3)]
    dev_rel = np.max(np.abs(np.array(got) - want) / np.abs(want))
    print(f"balanced trajectory: loss deviation {dev_rel:.2e}; losses {got}")
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=0)
    assert float(t.opt.state[0]) == 3.0
    close(t.inst_loss_of(bt).cpu().numpy(), ref["inst_loss"], RTOL_ACT, "inst_loss of the last step")
    # evaluate: no step
    before = [_bits(x) for x in (t.params, t.opt.m, t.opt.v, t.opt.state)]
    held = dev.from_instances(subset5[:2])
    ev = t.evaluate(held)
    torch.cuda.synchronize()
    assert [_bits(x) for x in (t.params, t.opt.m, t.opt.v, t.opt.state)] == before
    assert set(ev) == {"logits", "inst_loss", "metrics"}
    assert _bits(ev["logits"]) == _bits(held.forward(t.params))
    assert _bits(ev["metrics"]) == _bits(held.topm_metrics(ev["logits"]))
    assert _bits(ev["inst_loss"]) == _bits(held.weighted_loss(ev["logits"], None, "balanced", want="inst_loss")["inst_loss"])
    assert ev["inst_loss"].shape == (2,) and ev["metrics"].shape == (2, 2)
