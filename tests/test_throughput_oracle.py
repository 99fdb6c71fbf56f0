"""GPU tests of the throughput regime against the fp64 oracle (oracle/spmm_form.py).

A batch of >= 32 M nonzeros runs other code than the Netlib headline: the generic sweeps at the throughput tier thresholds
(graph.cpp::choose_tiers), the streamed / LDS-tiled copies that LPTrainer attaches, and a head kernel that loops over many
grid-stride rounds.  The oracle cannot run a 34 M-nonzero batch directly, but two exact identities make it unnecessary
(tests/test_oracle.py checks both on the CPU): replicating every instance of a batch leaves the loss and the gradients
unchanged, and a dL/dz that is nonzero on one instance only gives that instance's own gradients.  So:

  a. Netlib-97 x 32 (34.4 M nonzeros, 8.4 M variables: 32 grid-stride rounds of the head kernel) against ONE oracle run of
     Netlib-97, in every copy configuration, and one LPTrainer step against the oracle's Adam step;
  b. the device-generated synthetic batch (configs[3] geometry) cut into instances, three of which go to the oracle;
  c. every composition of the streamed / tiled copies on small ragged batches and Netlib-97;
  d. the multi-workgroup Adam kernels (n > 16 384) against an fp64 restatement.

Tolerances are those of tests/test_hip_parity.py: 1e-5 for logits and losses, 5e-5 for gradients, lin_key.bias masked.
"""
import resource
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import grad_scales as gs  # noqa: E402
from batch_slices import cut_instance  # noqa: E402
from mllp_amd.data import LPInstance, load_packed  # noqa: E402
from oracle import pyg_restatement as o1  # noqa: E402
from oracle import spmm_form as o2  # noqa: E402
from fused_cases import ragged_batch as _ragged_batch  # noqa: E402
from test_hip_parity import RTOL_ACT, RTOL_GRAD, close, close_elementwise, grad_mask  # noqa: E402

REPLICAS = 32
STREAM_COPIES = [(tr, g) for tr in (False, True) for g in (1, 2, 3, 4)]


@pytest.fixture(scope="module")
def LPBatch():
    from mllp_amd import _lib
    _lib.lib()                      # fail loudly: no fallback
    assert torch.cuda.is_available()
    from mllp_amd.graph import LPBatch as cls
    assert cls.default_path == 0
    return cls


@pytest.fixture(scope="module")
def weights(golden):
    flat = golden["weights_flat"]
    sd = {k: v.numpy() for k, v in o1.unflatten_state(torch.tensor(flat)).items()}
    return flat, sd, torch.tensor(flat, dtype=torch.float32, device="cuda")


@pytest.fixture(scope="module")
def netlib():
    return load_packed()


@pytest.fixture(scope="module")
def netlib_oracle(netlib, weights):
    t0 = time.perf_counter()
    r = o2.gnn_forward_backward(weights[1], o2.BatchCSR(netlib))
    print(f"\n[oracle] Netlib-97: {time.perf_counter() - t0:.1f} s")
    return r


def _detach_copies(b):
    b.disable_stream_step()
    for tr in (False, True):
        for v in (1, 2, 3, 4):
            b.disable_tiled(tr, variant=v)
    b._streams = None


def _cid(c):
    return f"{'At' if c[0] else 'A'}_g{c[1]}"


def _check_topm_rule(b, z, insts, met):
    """the kernel's documented rule: m largest logits, ties at the threshold taken in index order"""
    for k, (zk, i) in enumerate(zip(b.logits_per_instance(z), insts)):
        order = np.argsort(-zk.astype(np.float64), kind="stable")[:i.m]
        tp = float(i.basis[order].sum())
        assert met[k, 0] == tp, (k, i.name)
        f1 = 0.0 if tp == 0 else 2 * tp / (2 * tp + (i.m - tp) + (i.basis.sum() - tp))
        assert abs(met[k, 1] - f1) < 1e-5, (k, i.name)


# ---------------------------------------------------------------------------------------------------------------------
# a. Netlib-97 x 32
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def netlib32(LPBatch, netlib):
    order = np.random.default_rng(2024).permutation(len(netlib) * REPLICAS) % len(netlib)
    insts = [netlib[j] for j in order]
    t0 = time.perf_counter()
    b = LPBatch.from_instances(insts)
    print(f"\n[netlib32] {b.n_inst} instances, nnz {b.nnz}, N {b.N}, M {b.M}: built in {time.perf_counter() - t0:.1f} s")
    where = [np.flatnonzero(order == j) for j in range(len(netlib))]        # batch positions of the replicas of j
    return b, insts, order, where


def test_netlib32_is_in_the_throughput_regime(netlib32, netlib, LPBatch):
    from mllp_amd.trainer import LPTrainer
    b, insts, order, where = netlib32
    assert b.nnz == REPLICAS * 1074147 and b.nnz >= LPTrainer.TILED_NNZ_MIN
    assert LPBatch.default_path == 0 and not getattr(b, "_tiled", None) and not getattr(b, "_streams", None)
    # the throughput tier thresholds (wave tier above 1 024 entries, chunks above 16 384): no Netlib row is chunked or
    # split here, while the latency thresholds chunk and split some (test_hip_parity.py::test_full_netlib_batch)
    rl = np.concatenate([np.diff(i.indptr) for i in insts])
    cl = np.concatenate([np.bincount(i.indices, minlength=i.n) for i in insts])
    d = b.dims()
    assert d["A_block"] == 0 and d["At_block"] == 0 and d["A_split"] == 0 and d["At_split"] == 0, d
    assert d["A_wave"] == int((rl > 1024).sum()) > 0 and d["At_wave"] == int((cl > 1024).sum()) > 0, d


def _netlib32_config(b, mode):
    """Attach the copies of one configuration; returns a printable table.  Measured on an MI355X (entry slots per nonzero,
    bytes; the default rule drops a copy above 2 slots per nonzero): A geometries 1-4 2.63 / 3.02 / 2.87 / 2.74 (dropped),
    A^T 1.46 / 1.52 / 1.49 / 1.79 (kept); all eight copies together take 4.8 GiB."""
    _detach_copies(b)
    lines = []
    if mode in ("streamed_default", "streamed_all"):
        t0 = time.perf_counter()
        if mode == "streamed_default":
            infos = b.enable_stream_step()
        else:
            from mllp_amd import _lib
            infos = {}
            for tr, g in STREAM_COPIES:
                try:
                    infos[(tr, g)] = b.build_stream_copy(tr, g)
                except _lib.MllpError as e:          # reported, not skipped: the configuration runs without this copy
                    infos[(tr, g)] = dict(entry_slots=0, bytes=0, failed=str(e))
        b._streams = infos
        lines.append(f"copies built in {time.perf_counter() - t0:.1f} s")
        for (tr, g), i in sorted(infos.items()):
            state = ("DOES NOT FIT: " + i["failed"]) if "failed" in i else ("dropped" if i.get("dropped") else "kept")
            lines.append(f"  {_cid((tr, g)):6s} entry_slots/nnz {i['entry_slots'] / b.nnz:7.3f}  "
                         f"{i['bytes'] / 2 ** 20:9.1f} MiB  {state}")
    elif mode == "tiled":
        infos = b.enable_tiled_step()
        for k, i in sorted(infos.items()):
            assert i is not None, k
            lines.append(f"  tiled A{'t' if k[0] else ''} variant {k[1]}: {i['n_tb']} (tile, block) pairs")
    return lines


@pytest.mark.parametrize("mode", ["generic", "streamed_default", "streamed_all", "tiled"])
def test_netlib32_step_against_oracle(netlib32, netlib, netlib_oracle, weights, mode):
    b, insts, order, where = netlib32
    r = netlib_oracle
    flat, sd, flat_gpu = weights
    lines = _netlib32_config(b, mode)
    print(f"\n[netlib32 {mode}]\n" + "\n".join(lines))
    if mode == "streamed_all":
        assert not any(i.get("dropped") for i in b._streams.values())
        if any("failed" in i for i in b._streams.values()):
            import warnings
            warnings.warn(f"netlib32 streamed_all: a copy did not fit: {lines}")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loss, logits, grads = [t.clone() for t in b.loss_step(flat_gpu)]
    torch.cuda.synchronize()
    free, total = torch.cuda.mem_get_info()
    print(f"  first loss_step {1e3 * (time.perf_counter() - t0):.1f} ms; device memory in use {(total - free) / 2 ** 30:.2f} GiB, "
          f"host peak RSS {resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2 ** 20:.2f} GiB")
    # replicas leave the loss (1/B) sum_k mean-BCE and the gradients unchanged: one oracle run of Netlib-97
    close(loss.cpu().numpy(), [r["loss"]], RTOL_ACT, f"{mode}: loss")
    keep = grad_mask()
    close(grads.cpu().numpy()[keep], r["grads"][keep], RTOL_GRAD, f"{mode}: gradients")
    z = logits.cpu().numpy()
    off = np.concatenate([[0], np.cumsum([i.n for i in netlib])])
    zs, zr = b.logits_per_instance(z), [r["logits"][off[j]:off[j + 1]] for j in range(len(netlib))]
    for j, inst in enumerate(netlib):
        got = np.stack([zs[k] for k in where[j]])
        want = np.broadcast_to(zr[j], got.shape)
        close(got, want, RTOL_ACT, f"{mode}: logits of the {REPLICAS} replicas of {inst.name}")
        close_elementwise(got, want, RTOL_ACT, f"{mode}: logits of the {REPLICAS} replicas of {inst.name}, element-wise")
    fwd = b.forward(flat_gpu)
    assert torch.equal(fwd, logits), f"{mode}: forward-only logits differ from loss_step's"
    l2, z2, g2 = b.loss_step(flat_gpu)
    assert torch.equal(l2, loss) and torch.equal(z2, logits) and torch.equal(g2, grads), f"{mode}: not run-to-run exact"
    _check_topm_rule(b, z, insts, b.topm_metrics(logits).cpu().numpy())


def test_netlib32_trainer_step_equals_oracle_adam(netlib32, netlib_oracle, weights):
    """LPTrainer(tiled_copies="auto") attaches the streamed copies itself and runs forward + loss + backward + Adam in one
    library call over 8.4 M variables; parameters after the step == o2.adam_step on the oracle gradients."""
    from mllp_amd.trainer import LPTrainer
    b, insts, order, where = netlib32
    r = netlib_oracle
    flat, sd, flat_gpu = weights
    _detach_copies(b)
    lr = 1e-3
    tr = LPTrainer(flat_gpu, lr=lr, tiled_copies="auto")
    loss, _ = tr.step(b)
    assert sorted(k for k, i in b._streams.items()) == STREAM_COPIES
    print("\n[netlib32 trainer] " + ", ".join(f"{_cid(k)} {'dropped' if i.get('dropped') else 'kept'}"
                                              for k, i in sorted(b._streams.items())))
    close(loss.cpu().numpy(), [r["loss"]], RTOL_ACT, "trainer loss")
    want = flat.astype(np.float64).copy()
    o2.adam_step(want, r["grads"], np.zeros_like(want), np.zeros_like(want), 1, lr=lr)
    got = tr.params.cpu().numpy().astype(np.float64)
    # the first Adam step moves a parameter by lr * g / (|g| + eps), about lr * sign(g): its sign is pinned only where the
    # gradient is pinned, i.e. |g| above the gradient tolerance (5e-5 of the largest); below that (and lin_key.bias) the
    # step is only bounded by lr
    g = np.abs(r["grads"])
    pinned = grad_mask() & (g >= RTOL_GRAD * g.max())
    print(f"  {int(pinned.sum())} parameters pinned, {int((~pinned).sum())} bounded by lr")
    np.testing.assert_allclose(got[pinned], want[pinned], rtol=1e-4, atol=1e-5)
    assert (np.abs(got - flat) <= lr * 1.001 + 1e-6).all()
    # every parameter: the step applied the fp64 Adam step to the gradients it computed, and those are the oracle's
    g_dev = tr._plans[b.token]["grads"].cpu().numpy().astype(np.float64)
    close(g_dev[grad_mask()], r["grads"][grad_mask()], RTOL_GRAD, "trainer gradients")
    own = flat.astype(np.float32).astype(np.float64)
    o2.adam_step(own, g_dev, np.zeros_like(own), np.zeros_like(own), 1, lr=float(np.float32(lr)))
    np.testing.assert_allclose(got, own, rtol=1e-6, atol=1e-7)
    assert float(tr.opt.state[0]) == 1.0
    tr.release(b)


# ---------------------------------------------------------------------------------------------------------------------
# b. the device-generated synthetic batch
# ---------------------------------------------------------------------------------------------------------------------
SYN_INST, SYN_CUT, SYN_BWD = 17, (0, 8, 16), (0, 16)


@pytest.fixture(scope="module")
def synthetic(LPBatch, weights):
    from mllp_amd.graph import synthetic_batch
    sb = synthetic_batch(SYN_INST, seed=4321)
    assert sb.nnz >= 32 << 20 and sb.N == 340000
    ptr, idx, val = sb.export(0), sb.export(1), sb.export(2)
    x1, x2, y = sb.x1.cpu().numpy(), sb.x2.cpu().numpy(), sb.labels.cpu().numpy()
    cut = {k: cut_instance(ptr, idx, val, x1, x2, y, sb.inst_m, sb.inst_n, k) for k in SYN_CUT}
    del ptr, idx, val
    sd = weights[1]
    ref, dz = {}, np.zeros(sb.N, np.float32)
    t0 = time.perf_counter()
    for k, inst in cut.items():
        ref[k] = o2.gnn_forward_backward(sd, o2.BatchCSR([inst]), want_grads=False)
        if k in SYN_BWD:
            z = ref[k]["logits"]
            dz_k = ((1.0 / (1.0 + np.exp(-z)) - inst.basis) / (inst.n * SYN_INST)).astype(np.float32)
            dz[sb._n_off[k]:sb._n_off[k + 1]] = dz_k
            ref[k]["grads"] = o2.gnn_forward_backward(sd, o2.BatchCSR([inst]), dlogits=dz_k.astype(np.float64))["grads"]
    print(f"\n[oracle] synthetic instances {SYN_CUT}: {time.perf_counter() - t0:.1f} s")
    return sb, cut, ref, dz


@pytest.mark.parametrize("mode", ["streamed", "generic"])
def test_synthetic_batch_against_oracle(synthetic, weights, mode):
    sb, cut, ref, dz = synthetic
    flat, sd, flat_gpu = weights
    _detach_copies(sb)
    if mode == "streamed":
        infos = sb.enable_stream_step()
        print(f"\n[synthetic streamed] " + ", ".join(f"{_cid(k)} {i['entry_slots'] / sb.nnz:.3f}" for k, i in sorted(infos.items())))
        assert not any(i.get("dropped") for i in infos.values()), infos
    loss, logits, grads = sb.loss_step(flat_gpu)
    z = logits.cpu().numpy().astype(np.float64)
    for k in SYN_CUT:
        got, want = z[sb._n_off[k]:sb._n_off[k + 1]], ref[k]["logits"]
        close(got, want, RTOL_ACT, f"{mode}: logits of instance {k}")
        close_elementwise(got, want, RTOL_ACT, f"{mode}: logits of instance {k}, element-wise")
    # the loss from the GPU's own logits, in fp64: (1/B) sum_k mean-BCE(k)
    y = sb.labels.cpu().numpy().astype(np.float64)
    bce = np.maximum(z, 0) - z * y + np.log1p(np.exp(-np.abs(z)))
    want_loss = sum(bce[sb._n_off[k]:sb._n_off[k + 1]].mean() for k in range(SYN_INST)) / SYN_INST
    close(loss.cpu().numpy(), [want_loss], RTOL_ACT, f"{mode}: loss vs fp64 BCE of the GPU's logits")
    # backward from a dL/dz that is nonzero on instances 0 and 16 only == the sum of their oracle gradients
    sb.forward(flat_gpu)
    g = sb.backward(flat_gpu, torch.tensor(dz, device="cuda")).cpu().numpy()
    want = sum(ref[k]["grads"] for k in SYN_BWD)
    keep = grad_mask()
    close(g[keep], want[keep], RTOL_GRAD, f"{mode}: gradients of dz on instances {SYN_BWD}")
    # a dense dz: d fc.bias = sum dz, the head's reduction over 1 024 blocks of partials
    sb.forward(flat_gpu)
    gen = torch.Generator(device="cuda").manual_seed(99)
    dzd = (torch.rand(sb.N, device="cuda", generator=gen) - 0.3) / sb.N
    g = sb.backward(flat_gpu, dzd)
    close(g[4720:].cpu().numpy(), [float(dzd.double().sum())], RTOL_ACT, f"{mode}: fc.bias gradient of a dense dz")


# ---------------------------------------------------------------------------------------------------------------------
# c. compositions of the copies on small batches
# ---------------------------------------------------------------------------------------------------------------------
COMPOSITIONS = ([("none", (), False), ("streamed_all", tuple(STREAM_COPIES), False)]
                + [(f"only_{_cid(c)}", (c,), False) for c in STREAM_COPIES]
                + [(f"all_but_{_cid(c)}", tuple(x for x in STREAM_COPIES if x != c), False) for c in STREAM_COPIES]
                + [("tiled", (), True), ("streamed_and_tiled", tuple(STREAM_COPIES), True)])


@pytest.fixture(scope="module")
def small_batches(LPBatch, weights, netlib, netlib_oracle):
    cache = {}

    def get(name):
        if name not in cache:
            insts = _ragged_batch() if name == "ragged" else netlib
            ob = o2.BatchCSR(insts)
            r = netlib_oracle if name == "netlib97" else o2.gnn_forward_backward(weights[1], ob)
            dz = (np.random.default_rng(5).standard_normal(ob.N) / max(ob.N, 1)).astype(np.float32)
            rd = o2.gnn_forward_backward(weights[1], ob, dlogits=dz.astype(np.float64))
            b = LPBatch.from_instances(insts)
            b.set_path(1)
            # per-tensor yardsticks (tests/grad_scales.py) of the loss step and of dz; Netlib-97 stays on the global check (its
            # fp32 restatement sums 8 M terms one after the other and is no yardstick)
            yards = (gs.yardstick(weights[1], ob), gs.yardstick(weights[1], ob, dz.astype(np.float64))) if name == "ragged" else None
            cache[name] = (b, r, dz, rd["grads"], yards)
        return cache[name]
    return get


@pytest.mark.parametrize("comp", COMPOSITIONS, ids=[c[0] for c in COMPOSITIONS])
@pytest.mark.parametrize("batch", ["ragged", "netlib97"])
def test_copy_composition_against_oracle(small_batches, weights, batch, comp):
    name, streams, tiled = comp
    b, r, dz, grads_dz, yards = small_batches(batch)
    flat, sd, flat_gpu = weights
    _detach_copies(b)
    if streams == tuple(STREAM_COPIES):
        infos = b.enable_stream_step(max_slots_per_nnz=float("inf"))
        assert not any(i.get("dropped") for i in infos.values())
    else:
        for tr, g in streams:
            assert b.build_stream_copy(tr, g)["n_tiles"] > 0
    if tiled:
        for k, i in b.enable_tiled_step().items():
            assert i is not None, k
    keep = grad_mask()
    z = b.forward(flat_gpu).clone()
    close(z.cpu().numpy(), r["logits"], RTOL_ACT, f"{batch} {name}: forward logits")
    close_elementwise(z.cpu().numpy(), r["logits"], RTOL_ACT, f"{batch} {name}: forward logits, element-wise")
    loss, logits, grads = [t.clone() for t in b.loss_step(flat_gpu)]
    assert torch.equal(logits, z)
    close(loss.cpu().numpy(), [r["loss"]], RTOL_ACT, f"{batch} {name}: loss")
    close(grads.cpu().numpy()[keep], r["grads"][keep], RTOL_GRAD, f"{batch} {name}: gradients")
    g = b.backward(flat_gpu, torch.tensor(dz, device="cuda")).clone()
    close(g.cpu().numpy()[keep], grads_dz[keep], RTOL_GRAD, f"{batch} {name}: gradients of a random dz")
    if yards is not None:                       # every tensor on its own scale; the reference exempts none on this batch
        gs.close_per_tensor(grads.cpu().numpy(), r["grads"], yards[0], f"{batch} {name}: gradients", max_exempt=0)
        gs.close_per_tensor(g.cpu().numpy(), grads_dz, yards[1], f"{batch} {name}: gradients of a random dz", max_exempt=0)
    if streams and tiled:                       # the streamed copies take precedence: same bits as without the tiled ones
        for tr in (False, True):
            for v in (1, 2, 3, 4):
                b.disable_tiled(tr, variant=v)
        assert torch.equal(b.loss_step(flat_gpu)[2], grads)
        b.forward(flat_gpu)
        assert torch.equal(b.backward(flat_gpu, torch.tensor(dz, device="cuda")), g)


# ---------------------------------------------------------------------------------------------------------------------
# d. Adam over many workgroups (n > 16 384: adam_wide_kernel + adam_tick_kernel)
# ---------------------------------------------------------------------------------------------------------------------
def _angle256_params():
    from mllp_amd.angle import AngleModel
    return sum(p.numel() for p in AngleModel(256).parameters())


ADAM_NS = [1, 4096, 16384, 16385, 4096 * 7 + 13, "angle256"]
ADAM_PAD = 4096 + 5
SENTINEL = (777.25, -3.5, 12.5, 5.0)          # params, m, v, grads past n


def _adam_buffers(n, p0):
    bufs = []
    for s, init in zip(SENTINEL, (p0, 0.0, 0.0, 0.0)):
        t = torch.full((n + ADAM_PAD,), s, dtype=torch.float32, device="cuda")
        if np.ndim(init):
            t[:n].copy_(torch.from_numpy(init))
        else:
            t[:n].fill_(init)
        bufs.append(t)
    return bufs


@pytest.mark.parametrize("n", ADAM_NS, ids=[str(v) for v in ADAM_NS])
def test_adam_step_against_fp64(n):
    from mllp_amd.graph import adam_step
    n = _angle256_params() if n == "angle256" else n
    rng = np.random.default_rng(n)
    p0 = (rng.choice([-1.0, 1.0], n) * rng.uniform(0.5, 1.5, n)).astype(np.float32)
    sign = rng.choice([-1.0, 1.0], n)
    # one sign per element keeps m away from cancellation (a relative bound holds element by element); exact zeros included
    gs = [(sign * np.abs(rng.standard_normal(n)) * (rng.random(n) >= 0.2)).astype(np.float32) for _ in range(6)]
    lr, b1, b2, eps, gscale = 3e-3, 0.8, 0.99, 1e-8, 0.37
    P, M, V, G = _adam_buffers(n, p0)
    state = torch.tensor([0.0, lr, b1, b2], dtype=torch.float32, device="cuda")
    for gt in gs:
        G[:n].copy_(torch.from_numpy(gt))
        adam_step(P[:n], G[:n], M[:n], V[:n], state, eps, gscale)
    torch.cuda.synchronize()
    # fp64 restatement with the fp32 values the kernel receives
    f = lambda x: float(np.float32(x))
    lr_, b1_, b2_, eps_, gs_ = f(lr), f(b1), f(b2), f(eps), f(gscale)
    p, m, v = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    for t, gt in enumerate(gs, start=1):
        g = gt.astype(np.float64) * gs_
        m = b1_ * m + (1 - b1_) * g
        v = b2_ * v + (1 - b2_) * g * g
        p = p - (lr_ / (1 - b1_ ** t)) * m / (np.sqrt(v) / np.sqrt(1 - b2_ ** t) + eps_)
    got = [t.cpu().numpy().astype(np.float64) for t in (P, M, V, G)]
    for what, a, want, rtol in (("params", got[0], p, 1e-6), ("m", got[1], m, 1e-5), ("v", got[2], v, 1e-5)):
        bad = np.abs(a[:n] - want) > rtol * np.abs(want)
        assert not bad.any(), f"n={n} {what}: {int(bad.sum())} elements off (first at {int(np.flatnonzero(bad)[0])})"
    assert float(state[0]) == 6.0
    for what, a, s in zip(("params", "m", "v", "grads"), got, SENTINEL):
        assert (a[n:] == s).all(), f"n={n}: {what} past n were written"
    # three steps captured in one graph (single stream), replayed twice == six eager steps, bit for bit
    Gs = [_adam_buffers(n, p0)[3] for _ in range(3)]
    for Gk, gt in zip(Gs, gs):
        Gk[:n].copy_(torch.from_numpy(gt))
    eager, graph = _adam_buffers(n, p0), _adam_buffers(n, p0)
    st_e, st_g = [torch.tensor([0.0, lr, b1, b2], dtype=torch.float32, device="cuda") for _ in range(2)]
    for _ in range(2):
        for Gk in Gs:
            adam_step(eager[0][:n], Gk[:n], eager[1][:n], eager[2][:n], st_e, eps, gscale)
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        for Gk in Gs:
            adam_step(graph[0][:n], Gk[:n], graph[1][:n], graph[2][:n], st_g, eps, gscale)
    cg.replay()
    cg.replay()
    torch.cuda.synchronize()
    for a, e in zip(graph[:3], eager[:3]):
        assert torch.equal(a, e), f"n={n}: replayed graph differs from eager steps"
    assert torch.equal(st_g, st_e) and float(st_g[0]) == 6.0
