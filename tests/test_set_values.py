"""mllp_graph_set_values / mllp_graph_scale_values: new coefficients a_ij on an unchanged sparsity pattern, refreshed in
place on the device (mllp_amd/csrc/set_values.hip).  The yardstick throughout is a FRESH batch built from the new values
by the ordinary builders; every launch path is deterministic, so every comparison is exact (bytes), not a tolerance.
Inputs: the 97 Netlib instances, and a small ragged batch with empty rows, an instance without nonzeros and rows longer
than a wavefront's register set."""
import ctypes
import dataclasses
import re

import numpy as np
import pytest
import torch

from mllp_amd import _lib

gpu = pytest.mark.gpu
EINVAL = -1


# ---------------------------------------------------------------------------------------------------
# CPU: the ABI surface
# ---------------------------------------------------------------------------------------------------
NEW = ("mllp_graph_set_values", "mllp_graph_set_values_bytes", "mllp_graph_scale_values")


def test_new_exports_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), f"{name} is not declared in include/mllp_hip.h"
        assert hasattr(L, name), f"{name} is not exported by libmllp_hip.so"
        assert name in _lib._PROTOTYPES, f"{name} has no ctypes prototype"
    assert _lib.lib().mllp_abi_version() == 6 and _lib.ABI_VERSION == 6
    assert re.search(r"#define\s+MLLP_ABI_VERSION\s+6\b", open(_lib.HEADER_PATH).read())


def test_null_arguments_are_refused_with_a_message():
    L = _lib.lib()
    for call in (lambda: L.mllp_graph_set_values(None, None, None),
                 lambda: L.mllp_graph_scale_values(None, None, None, None),
                 lambda: L.mllp_graph_set_values_bytes(None, None)):
        L.mllp_graph_dims(None, (ctypes.c_int64 * 12)())          # (some other message first)
        assert call() == EINVAL
        assert b"null" in L.mllp_last_error()


# ---------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def LPBatch():
    _lib.lib()
    assert torch.cuda.is_available()
    from mllp_amd.graph import LPBatch as cls
    return cls


def _ragged():
    from mllp_amd.data import LPInstance
    from test_stream_attn import _ragged_instance
    return [_ragged_instance(11, 700, 900), _ragged_instance(12, 3, 5), _ragged_instance(13, 1300, 2300, {7: 900, 40: 130}),
            LPInstance("empty", np.zeros(6, np.int64), np.zeros(0, np.int32), np.zeros(0), np.zeros(4), np.zeros(5),
                       np.zeros(4, np.int32)),
            _ragged_instance(14, 90, 60)]


@pytest.fixture(scope="module")
def datasets():
    from mllp_amd.data import load_packed
    netlib = load_packed()
    assert len(netlib) == 97
    return {"netlib": netlib, "ragged": _ragged()}


def _values(insts):
    """The batch's values in CSR(A) order (instances are consecutive row blocks), as the fp32 the library stores."""
    return np.concatenate([i.values for i in insts]).astype(np.float32)


def _new_values(v0, seed):
    """v0 (1 + u / 2), u uniform in [-1, 1], with a handful of entries exactly 0.0 and exactly -v0."""
    rng = np.random.default_rng(seed)
    v = (v0 * (1.0 + 0.5 * rng.uniform(-1.0, 1.0, v0.size)).astype(np.float32)).astype(np.float32)
    pick = rng.choice(v0.size, size=min(12, v0.size), replace=False)
    v[pick[:6]] = 0.0
    v[pick[6:]] = -v0[pick[6:]]
    return v


def _with_values(insts, v):
    out, off = [], 0
    for i in insts:
        out.append(dataclasses.replace(i, values=v[off:off + i.nnz].astype(np.float64)))
        off += i.nnz
    assert off == v.size
    return out


def _dev(v):
    return torch.tensor(v, dtype=torch.float32, device="cuda")


def _params(seed=5):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(_lib.NUM_PARAMS, generator=g) * 0.2).to("cuda")


def _plain(b):
    return [b.export(k) for k in range(7)]


def _same(a, b, what):
    if isinstance(a, torch.Tensor):
        a, b = a.cpu().numpy(), b.cpu().numpy()
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{what}: bytes differ"


def _same_lists(xs, ys, what):
    assert len(xs) == len(ys), what
    for k, (x, y) in enumerate(zip(xs, ys)):
        _same(x, y, f"{what}[{k}]")


@gpu
@pytest.mark.parametrize("data", ["netlib", "ragged"])
def test_plain_arrays_hold_the_new_values_and_nothing_else_moved(LPBatch, datasets, data):
    insts = datasets[data]
    v0 = _values(insts)
    v1 = _new_values(v0, 1)
    b0 = LPBatch.from_instances(insts)
    before = _plain(b0)
    _same(before[2], v0, "export(2) is the instances' values in order")
    assert b0.set_values_bytes() == 4 * b0.nnz              # the A^T map alone: no copy is attached
    b0.set_values(_dev(v1))
    b1 = LPBatch.from_instances(_with_values(insts, v1))
    after = _plain(b0)
    _same(after[2], v1, "export(2) after set_values")
    _same_lists(after, _plain(b1), "export(k) against a fresh build")
    for k in (0, 1, 3, 4, 6):
        _same(after[k], before[k], f"export({k}) must not move")
    assert (v1 == 0).sum() >= 6 and b0.nnz == b1.nnz        # explicit zeros stay in the pattern


def _model_outputs(b, params, path):
    """logits, loss / logits / gradients of loss_step, parameters and Adam state after one train_step."""
    b.set_path(path)
    out = [b.forward(params).clone()]
    loss, logits, grads = b.loss_step(params)
    out += [loss.clone(), logits.clone(), grads.clone()]
    p, m, v = params.clone(), torch.zeros_like(params), torch.zeros_like(params)
    state = torch.tensor([0.0, 1e-3, 0.9, 0.999], device="cuda")
    b.train_step(p, m, v, state)
    torch.cuda.synchronize()
    return out + [p, m, v, state]


@gpu
@pytest.mark.parametrize("data", ["netlib", "ragged"])
@pytest.mark.parametrize("path", [1, 2])
def test_both_whole_model_paths_match_a_fresh_build(LPBatch, datasets, data, path):
    insts = datasets[data]
    v1 = _new_values(_values(insts), 2)
    params = _params()
    b0 = LPBatch.from_instances(insts)
    b0.set_path(path)
    b0.forward(params)                                      # binds the inputs (the fused path's gathered copies) first
    b0.set_values(_dev(v1))
    b1 = LPBatch.from_instances(_with_values(insts, v1))
    _same_lists(_model_outputs(b0, params, path), _model_outputs(b1, params, path), f"path {path}")


def _attach_all(b):
    """Every copy kind in both orientations: the device-built LDS-tiled variants, streamed geometries 0-3, the lane copy.
    Returns what is attached (a variant the matrix does not qualify for is skipped, the same for every batch)."""
    tiled = [k for k, info in b.enable_tiled_all().items() if info is not None]
    for tr in (False, True):
        for geom in range(5):
            b.build_stream_copy(tr, geom)
    return tiled


def _copies(b, tiled):
    out = []
    for tr in (False, True):
        for geom in range(5):
            if b.stream_copy_info(tr, geom)["n_tiles"]:
                out += list(b.export_stream_copy(tr, geom))
    for tr, v in tiled:
        out += list(b.export_tiled(tr, v).values())
    return out


def _sweeps(b, params):
    """Single-layer sweeps of both orientations (plain SpMM, 1- and 16-channel conv forward and backward) and a loss_step,
    on whatever copies are attached."""
    g = torch.Generator().manual_seed(9)
    out = []
    for tr in (False, True):
        n_in = b.M if tr else b.N
        out.append(b.spmm(torch.randn(n_in, 16, generator=g).to("cuda"), tr))
    for dst_is_var in (0, 1):
        n_dst, n_src = (b.N, b.M) if dst_is_var else (b.M, b.N)
        for cin in (1, 16):
            cp = (torch.randn(144 if cin == 1 else 1104, generator=g) * 0.3).to("cuda")
            xs, xd = torch.randn(n_src, cin, generator=g).to("cuda"), torch.randn(n_dst, cin, generator=g).to("cuda")
            dh = torch.randn(n_dst, 16, generator=g).to("cuda")
            ws = b.tconv_workspace(dst_is_var, cin)
            h = b.tconv_fwd(dst_is_var, cin, cp, xs, xd, ws)
            pg, dxd, dxs, dhm = b.tconv_bwd(dst_is_var, cin, cp, xs, xd, h, ws, dh)
            out += [h, pg, dhm] + [t for t in (dxd, dxs) if t is not None]
    b.set_path(1)
    out += [t.clone() for t in b.loss_step(params)]
    torch.cuda.synchronize()
    return out


@gpu
@pytest.mark.parametrize("data", ["netlib", "ragged"])
def test_every_copy_kind_is_refreshed(LPBatch, datasets, data):
    insts = datasets[data]
    v1 = _new_values(_values(insts), 3)
    b0 = LPBatch.from_instances(insts)
    tiled = _attach_all(b0)
    assert tiled, "no LDS-tiled copy could be attached"
    no_copies = 4 * b0.nnz
    assert b0.set_values_bytes() > no_copies + 4 * b0.nnz * len(tiled) - 1
    b0.set_values(_dev(v1))
    b1 = LPBatch.from_instances(_with_values(insts, v1))
    assert _attach_all(b1) == tiled
    _same_lists(_copies(b0, tiled), _copies(b1, tiled), "copies after set_values against copies built from the new values")
    _same_lists(_plain(b0), _plain(b1), "export(k)")
    params = _params()
    _same_lists(_sweeps(b0, params), _sweeps(b1, params), "sweeps on the refreshed copies")


@gpu
def test_copies_built_after_and_maps_remade(LPBatch, datasets):
    insts = datasets["ragged"]
    v0 = _values(insts)
    v1, v2 = _new_values(v0, 4), _new_values(v0, 5)
    b0 = LPBatch.from_instances(insts)
    b0.set_values(_dev(v1))
    tiled = _attach_all(b0)                                 # built AFTER the values changed
    b1 = LPBatch.from_instances(_with_values(insts, v1))
    _attach_all(b1)
    _same_lists(_copies(b0, tiled), _copies(b1, tiled), "copies built after set_values")
    b0.set_values(_dev(v1))                                 # maps of all copies made here ...
    for tr in (False, True):
        for geom in (1, 4):
            b0.drop_stream_copy(tr, geom)                   # ... some freed with their copies ...
            b0.build_stream_copy(tr, geom)
    b0.set_values(_dev(v2))                                 # ... and made again
    b2 = LPBatch.from_instances(_with_values(insts, v2))
    _attach_all(b2)
    _same_lists(_copies(b0, tiled), _copies(b2, tiled), "drop + rebuild + set_values")
    _same_lists(_plain(b0), _plain(b2), "export(k)")


@gpu
@pytest.mark.parametrize("data", ["netlib", "ragged"])
def test_round_trip_restores_every_byte(LPBatch, datasets, data):
    insts = datasets[data]
    v0 = _values(insts)
    params = _params()
    b0 = LPBatch.from_instances(insts)
    tiled = _attach_all(b0)

    def snapshot():
        out = _plain(b0) + _copies(b0, tiled)
        for path in (1, 2):
            b0.set_path(path)
            out.append(b0.forward(params).clone())
        return out

    start = snapshot()
    b0.set_values(_dev(_new_values(v0, 6)))
    moved = snapshot()
    assert not np.array_equal(moved[2], start[2]) and not torch.equal(moved[-1], start[-1])
    b0.set_values(_dev(v0))
    _same_lists(snapshot(), start, "after set_values(v1), set_values(v0)")


@gpu
def test_backward_needs_a_new_forward(LPBatch, datasets):
    insts = datasets["ragged"]
    v1 = _new_values(_values(insts), 7)
    params = _params()
    b1 = LPBatch.from_instances(_with_values(insts, v1))
    for path in (1, 2):
        b0 = LPBatch.from_instances(insts)
        b0.set_path(path)
        b1.set_path(path)
        dl = torch.randn(b0.N, generator=torch.Generator().manual_seed(3)).to("cuda")
        b0.forward(params)
        b0.set_values(_dev(v1))
        with pytest.raises(_lib.MllpError, match="forward"):
            b0.backward(params, dl)
        _same(b0.forward(params), b1.forward(params), "logits")
        _same(b0.backward(params, dl), b1.backward(params, dl), "gradients after a new forward")


@gpu
def test_borrowed_tiled_copy_is_refused(LPBatch, datasets):
    insts = datasets["ragged"]
    v0 = _values(insts)
    v1 = _new_values(v0, 8)
    b0 = LPBatch.from_instances(insts)
    assert b0.enable_tiled(False, variant=1, builder="torch") is not None
    before = _plain(b0) + list(b0.export_tiled(False, 1).values())
    with pytest.raises(_lib.MllpError, match="mllp_graph_build_tiled"):
        b0.set_values(_dev(v1))
    with pytest.raises(_lib.MllpError, match="mllp_graph_build_tiled"):
        b0.rescale(torch.full((b0.M,), 2.0, device="cuda"))
    _same_lists(_plain(b0) + list(b0.export_tiled(False, 1).values()), before, "a refused call writes nothing")
    b0.disable_tiled(False, 1)
    b0.set_values(_dev(v1))
    _same(b0.export(2), v1, "after disable_tiled")
    _same(b0.export(5), LPBatch.from_instances(_with_values(insts, v1)).export(5), "A^T values")


@gpu
def test_captured_set_values_replays_from_its_source_buffer(LPBatch, datasets):
    """ONE capture, ONE replay (a runtime failure of the capture itself is a finding about the machine, not retried)."""
    insts = datasets["netlib"]
    v0 = _values(insts)
    v1, v2 = _new_values(v0, 9), _new_values(v0, 10)
    params = _params()
    b0 = LPBatch.from_instances(insts)
    b0.forward(params)                                      # fused path (by size), inputs bound
    src = _dev(v1)
    b0.set_values(src)                                      # eager: builds the maps
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        b0.set_values(src)
    src.copy_(_dev(v2))
    graph.replay()
    torch.cuda.synchronize()
    _same(b0.export(2), v2, "export(2) after the replay")
    b2 = LPBatch.from_instances(_with_values(insts, v2))
    _same(b0.forward(params), b2.forward(params), "logits after the replay")


@gpu
@pytest.mark.parametrize("data", ["netlib", "ragged"])
def test_input_gradients_after_a_refresh(LPBatch, datasets, data):
    insts = datasets[data]
    v1 = _new_values(_values(insts), 11)
    params = _params()
    b0 = LPBatch.from_instances(insts)
    b1 = LPBatch.from_instances(_with_values(insts, v1))
    got = []
    for b in (b0, b1):
        b.set_path(1)
        dl = torch.randn(b.N, generator=torch.Generator().manual_seed(4)).to("cuda")
        if b is b0:
            b.forward(params)
            b.backward_inputs(params, dl)                   # at_pos made by the input-gradient pass, reused by set_values
            b.set_values(_dev(v1))
        b.forward(params)
        got.append(list(b.backward_inputs(params, dl)))
    _same_lists(got[0], got[1], "grads, dL/dx1, dL/dx2, dL/da")


@gpu
@pytest.mark.parametrize("data", ["netlib", "ragged"])
def test_rescale(LPBatch, datasets, data):
    insts = datasets[data]
    params = _params()
    g = torch.Generator().manual_seed(12)
    b0 = LPBatch.from_instances(insts)
    r = (0.5 + 1.5 * torch.rand(b0.M, generator=g)).to("cuda")
    s = (0.5 + 1.5 * torch.rand(b0.N, generator=g)).to("cuda")
    ptr, idx = torch.tensor(b0.export(0).astype(np.int64), device="cuda"), torch.tensor(b0.export(1).astype(np.int64), device="cuda")
    row = torch.repeat_interleave(torch.arange(b0.M, device="cuda"), ptr[1:] - ptr[:-1])
    for rs, cs in ((r, s), (r, None), (None, s), (None, None)):
        b = LPBatch.from_instances(insts)
        b.forward(params)
        v0, x1, x2 = torch.tensor(b.export(2), device="cuda"), b.x1.clone(), b.x2.clone()
        rr = rs if rs is not None else torch.ones(b.M, device="cuda")
        ss = cs if cs is not None else torch.ones(b.N, device="cuda")
        want = (rr[row] * v0) * ss[idx]
        b.rescale(rs, cs)
        _same(b.export(2), want.cpu().numpy(), f"values, row scale {rs is not None}, column scale {cs is not None}")
        _same(b.x1, x1 * ss, "x1 = c s")
        _same(b.x2, x2 * rr, "x2 = b r")
        fresh = LPBatch.from_instances(_with_values(insts, want.cpu().numpy()))
        fresh.x1.copy_(b.x1)
        fresh.x2.copy_(b.x2)
        _same_lists(_plain(b), _plain(fresh), "export(k)")
        for path in (1, 2):
            b.set_path(path)
            fresh.set_path(path)
            _same(b.forward(params), fresh.forward(params), f"logits on path {path}")


@gpu
def test_sgd_on_edge_attr_refreshes_instead_of_rebuilding(datasets):
    """The loop the feature is for: SGD on edge_attr through GNNModel.  Forcing a rebuild before every forward (what every
    step cost before) gives the same edge_attr and the same loss after every step, exactly; without forcing, the batch
    object is never replaced."""
    from mllp_amd.model import BipartiteData, GNNModel, build_graph_from_weights_sets
    five = sorted(datasets["netlib"], key=lambda i: i.nnz)[:5]
    model = GNNModel().to("cuda")
    model.load_flat(_params(21))

    def run(force_rebuild):
        graphs, labels = [], []
        for inst in five:
            name, constrs, w, coefs, rhs, basis = inst.as_reference_tuple()
            graphs.append(build_graph_from_weights_sets(constrs, w, rhs, coefs, torch.device("cuda")))
            labels.append(torch.tensor(np.asarray(basis), dtype=torch.float32, device="cuda"))
        g = BipartiteData.batch(graphs)
        g.edge_attr = g.edge_attr.detach().clone().requires_grad_(True)
        y = torch.cat(labels)
        opt = torch.optim.SGD([g.edge_attr], lr=0.5)
        trace, ids = [], set()
        for _ in range(5):
            if force_rebuild:
                g._lp_batch = None
            opt.zero_grad()
            loss = torch.nn.functional.binary_cross_entropy_with_logits(model(g), y)
            loss.backward()
            opt.step()
            ids.add(id(g._lp_batch))
            trace += [loss.detach().clone(), g.edge_attr.detach().clone()]
        return trace, ids

    kept, ids = run(False)
    rebuilt, _ = run(True)
    assert len(ids) == 1, "the LPBatch was replaced although only edge_attr changed"
    assert not torch.equal(kept[1], kept[-1]), "the steps did not move edge_attr"
    _same_lists(kept, rebuilt, "loss and edge_attr after every step")
