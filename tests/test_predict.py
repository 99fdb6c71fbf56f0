"""The predicted basis: mllp_topm_select / mllp_topm_select_dense, LPBatch.predict_basis, GNNModel.predict,
AngleModel.predict and the linear_program_predict command line.

The expected result is defined here, without the code under test: `orderable` maps a float32 to the uint32 key whose
unsigned order is the order of the selection (negative floats: all bits flipped; the others: sign bit set; so
-0.0 < +0.0 and every bit pattern has its place), `oracle_select` takes a STABLE argsort of the descending keys of each
segment and keeps the first min(m, n): equal keys stay in index order, which is the tie rule.  The order is total, so
every comparison below is exact: integers, and the two statistics as bit patterns.  No tolerance anywhere.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from mllp_amd import _lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
gpu = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------
def orderable(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def oracle_select(z, seg_n, seg_m):
    """(mask uint8 [sum n], index int32 [sum m], stats float32 [segments, 2]) as include/mllp_hip.h defines them."""
    z = np.ascontiguousarray(z, dtype=np.float32)
    n_off = np.concatenate([[0], np.cumsum(seg_n)]).astype(np.int64)
    m_off = np.concatenate([[0], np.cumsum(seg_m)]).astype(np.int64)
    mask = np.zeros(n_off[-1], np.uint8)
    index = np.full(m_off[-1], -1, np.int32)
    stats = np.zeros((len(seg_n), 2), np.float32)
    for k, (n, m) in enumerate(zip(seg_n, seg_m)):
        zk = z[n_off[k]:n_off[k + 1]]
        order = np.argsort(~orderable(zk), kind="stable")          # descending keys, equal keys in index order
        t = min(m, n)
        sel = np.sort(order[:t])
        mask[n_off[k] + sel] = 1
        index[m_off[k]:m_off[k] + t] = sel
        stats[k, 0] = zk[order[t - 1]] if t > 0 else np.inf
        stats[k, 1] = zk[order[t]] if t < n else -np.inf
    return mask, index, stats


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_prediction(pred, z, seg_n, seg_m, what=""):
    mask, index, stats = oracle_select(z, seg_n, seg_m)
    if pred.mask is not None:
        got = pred.mask.cpu().numpy()
        assert got.dtype == np.uint8 and got.shape == mask.shape, what
        assert np.array_equal(got, mask), f"{what}: mask differs in {int((got != mask).sum())} places"
    if pred.index is not None:
        got = pred.index.cpu().numpy()
        assert got.dtype == np.int32 and got.shape == index.shape, what
        assert np.array_equal(got, index), f"{what}: index differs in {int((got != index).sum())} places"
    if pred.stats is not None:
        got = pred.stats.cpu().numpy()
        assert got.shape == stats.shape, what
        assert np.array_equal(bits(got), bits(stats)), f"{what}: stats differ: {got[bits(got) != bits(stats)][:4]}"


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8).reshape(-1), b.contiguous().view(torch.uint8).reshape(-1))


def test_oracle_equals_torch_topk_without_ties():
    """the oracle against torch.topk on the CPU, on input where the tie rule cannot matter"""
    rng = np.random.default_rng(3)
    seg_n, seg_m = [1, 7, 64, 1000, 3001], [1, 3, 64, 377, 1500]
    z = rng.permutation(np.linspace(-4.0, 4.0, sum(seg_n))).astype(np.float32)      # all distinct
    assert np.unique(z).size == z.size
    mask, index, stats = oracle_select(z, seg_n, seg_m)
    n_off, m_off = np.concatenate([[0], np.cumsum(seg_n)]), np.concatenate([[0], np.cumsum(seg_m)])
    for k, (n, m) in enumerate(zip(seg_n, seg_m)):
        zk = torch.tensor(z[n_off[k]:n_off[k + 1]])
        val, idx = torch.topk(zk, k=m)
        want = np.zeros(n, np.uint8)
        want[idx.numpy()] = 1
        assert np.array_equal(mask[n_off[k]:n_off[k + 1]], want)
        assert np.array_equal(index[m_off[k]:m_off[k + 1]], np.sort(idx.numpy()))
        assert stats[k, 0] == float(val[-1])
        rest = zk[torch.tensor(want == 0)]
        assert stats[k, 1] == (float(rest.max()) if rest.numel() else -np.inf)


def test_oracle_order_is_the_documented_one():
    z = np.array([0.0, -0.0, np.inf, -np.inf, 1.0, 1.0, -1.0], np.float32)
    key = orderable(z)
    assert key[1] < key[0] and key[3] < key[6] < key[1] and key[0] < key[4] == key[5] < key[2]
    mask, index, stats = oracle_select(z, [7], [2])
    assert index.tolist() == [2, 4] and mask.tolist() == [0, 0, 1, 0, 1, 0, 0]       # the first of the two 1.0
    assert bits(stats).tolist() == bits(np.array([[1.0, 1.0]], np.float32)).tolist()   # a tie: equal bit patterns


# ---------------------------------------------------------------------------------------------------
# without a GPU: the ABI refuses bad calls before any HIP call; the command line fails loudly
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_abi_version_is_6(L):
    assert L.mllp_abi_version() == 6 == _lib.ABI_VERSION


def test_select_refuses_bad_arguments_without_gpu(L):
    fake = ctypes.c_void_p(4096)            # never dereferenced: the checks come first
    assert L.mllp_topm_select(None, fake, fake, fake, fake, None) == -1
    assert b"mllp_topm_select" in L.mllp_last_error() and b"null" in L.mllp_last_error()
    assert L.mllp_topm_select(fake, None, fake, fake, fake, None) == -1
    assert b"null" in L.mllp_last_error()
    assert L.mllp_topm_select(fake, fake, None, None, None, None) == -1
    assert b"outputs" in L.mllp_last_error()


def test_select_dense_refuses_bad_arguments_without_gpu(L):
    fake = ctypes.c_void_p(4096)
    assert L.mllp_topm_select_dense(10, 3, None, fake, fake, fake, None) == -1
    assert b"mllp_topm_select_dense" in L.mllp_last_error() and b"null" in L.mllp_last_error()
    assert L.mllp_topm_select_dense(10, 3, fake, None, None, None, None) == -1
    assert b"outputs" in L.mllp_last_error()
    assert L.mllp_topm_select_dense(-1, 3, fake, fake, fake, fake, None) == -1
    assert b"negative" in L.mllp_last_error()
    assert L.mllp_topm_select_dense(10, -3, fake, fake, fake, fake, None) == -1
    assert b"negative" in L.mllp_last_error()


def _yaml(tmp_path, method="gs-topk", device="cuda", batch_size=0, extra=""):
    p = tmp_path / "cfg.yaml"
    p.write_text(f"train_data_type: 'netlib'\ntrain_lr: 1.e-3\ntrain_iter: 1\nverbose: True\ndevice: '{device}'\n"
                 f"batch_size: {batch_size}\n{extra}methods:\n  - '{method}'\n")
    return str(p)


def _cli(tmp_path, cfg, model):
    return ["--cfg", cfg, "--model", str(model), "--mps", os.path.join(ROOT, "tests", "golden", "mps"),
            "--out", str(tmp_path / "out")]


def test_cli_fails_loudly(tmp_path):
    import linear_program_predict
    from mllp_amd import predict
    assert linear_program_predict.main is predict.main
    model = tmp_path / "w.pt"
    model.write_bytes(b"")
    with pytest.raises(FileNotFoundError, match="--model"):
        predict.main(_cli(tmp_path, _yaml(tmp_path), tmp_path / "missing.pt"))
    with pytest.raises(NotImplementedError, match="no-such-method"):
        predict.main(_cli(tmp_path, _yaml(tmp_path, method="no-such-method"), model))
    with pytest.raises(NotImplementedError, match="invariant"):
        predict.main(_cli(tmp_path, _yaml(tmp_path, method="invariant"), model))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        predict.main(_cli(tmp_path, _yaml(tmp_path, device="cpu"), model))
    with pytest.raises(FileNotFoundError, match="--mps"):
        predict.main(["--cfg", _yaml(tmp_path), "--model", str(model), "--mps", str(tmp_path / "nowhere"),
                      "--out", str(tmp_path / "out")])
    with pytest.raises(SystemExit):                                     # argparse: --model is required
        predict.main(["--cfg", _yaml(tmp_path), "--mps", "x", "--out", "y"])
    assert not (tmp_path / "out").exists()


# ---------------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def netlib():
    from mllp_amd.data import load_packed
    from mllp_amd.graph import LPBatch
    _lib.lib()
    assert torch.cuda.is_available()
    return LPBatch.from_instances(load_packed())


@pytest.fixture(scope="module")
def five(subset5):
    from mllp_amd.graph import LPBatch
    _lib.lib()
    assert torch.cuda.is_available()
    return LPBatch.from_instances(subset5)


def _randn(n, seed):
    return torch.tensor(np.random.default_rng(seed).standard_normal(n).astype(np.float32), device="cuda")


def tied_inputs(n, seed=5):
    """name -> float32 [n]: logits with ties on purpose"""
    rng = np.random.default_rng(seed)
    three = np.array([-0.5, 0.25, 1.5], np.float32)[rng.integers(0, 3, n)]
    zeros = np.where(rng.random(n) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    infs = np.round(rng.standard_normal(n).astype(np.float32), 1)
    infs[rng.random(n) < 0.05] = np.inf
    infs[rng.random(n) < 0.05] = -np.inf
    return {"three_values": three, "all_equal": np.full(n, 0.75, np.float32), "signed_zeros": zeros, "infinities": infs}


def _correct_from_mask(batch, pred):
    y = batch.labels.cpu().numpy()
    mask = pred.mask.cpu().numpy()
    off = np.concatenate([[0], np.cumsum(batch.inst_n)])
    return np.asarray([float((mask[off[k]:off[k + 1]] * y[off[k]:off[k + 1]]).sum()) for k in range(batch.n_inst)],
                      np.float32)


@gpu
def test_random_logits_five_instances(five):
    z = _randn(five.N, 1)
    assert_prediction(five.predict_basis(z), z.cpu().numpy(), five.inst_n, five.inst_m, "subset5")


@gpu
def test_random_logits_netlib(netlib):
    assert min(netlib.inst_n) < 1024 and max(netlib.inst_n) > 16 * 1024      # below one chunk, and many chunks
    z = _randn(netlib.N, 2)
    pred = netlib.predict_basis(z)
    assert_prediction(pred, z.cpu().numpy(), netlib.inst_n, netlib.inst_m, "netlib")
    parts = pred.split()
    assert len(parts) == netlib.n_inst and all(p.size == min(m, n) for p, m, n in zip(parts, netlib.inst_m, netlib.inst_n))
    mask, off = pred.mask.cpu().numpy(), np.concatenate([[0], np.cumsum(netlib.inst_n)])
    assert all(np.array_equal(np.flatnonzero(mask[off[k]:off[k + 1]]), p) for k, p in enumerate(parts))


@gpu
@pytest.mark.parametrize("kind", ["three_values", "all_equal", "signed_zeros", "infinities"])
def test_ties_netlib(netlib, kind):
    """ties everywhere, in segments of up to 29 351 columns: the threshold's tie group runs across wavefront and
    1024-column chunk boundaries, and the lowest indices must win; and the existing metrics kernel counts the same set"""
    z = tied_inputs(netlib.N)[kind]
    zt = torch.tensor(z, device="cuda")
    pred = netlib.predict_basis(zt)
    assert_prediction(pred, z, netlib.inst_n, netlib.inst_m, kind)
    met = netlib.topm_metrics(zt).cpu().numpy()
    assert np.array_equal(_correct_from_mask(netlib, pred), met[:, 0])


@gpu
@pytest.mark.parametrize("m", [1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4999, 5000, 7000])
def test_tie_cut_at_wavefront_and_chunk_boundaries(m):
    """one segment of 5000 equal logits with a few larger and smaller ones mixed in: the cut through the tie group falls
    on, before and behind multiples of 64 and 1024"""
    from mllp_amd.graph import topm_select_dense
    z = np.full(5000, 2.0, np.float32)
    z[[0, 100, 1024, 4095]] = 3.0
    z[[1, 63, 1023, 2048]] = -1.0
    pred = topm_select_dense(torch.tensor(z, device="cuda"), m)
    assert pred.index.numel() == m
    assert_prediction(pred, z, [5000], [m], f"m={m}")


@gpu
def test_degenerate_segments():
    """m = 0, m >= n, a zero-column instance and an instance without nonzeros, in one batch"""
    import scipy.sparse as sp
    from mllp_amd.data import LPInstance
    from mllp_amd.graph import LPBatch
    rng = np.random.default_rng(7)

    def dense_inst(name, m, n):
        A = sp.csr_matrix((rng.random((m, n)) < 0.3) * rng.standard_normal((m, n)))
        A.sort_indices()
        return LPInstance(name, A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data, rng.standard_normal(n),
                          np.abs(rng.standard_normal(m)), (rng.random(n) < 0.4).astype(np.int32))
    toy = dense_inst("toy", 9, 40)
    wide = dense_inst("m_gt_n", 12, 5)                                   # m >= n: every column is selected
    square = dense_inst("m_eq_n", 6, 6)
    norows = LPInstance("m0", np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0), rng.standard_normal(7),
                        np.zeros(0), np.zeros(7, np.int32))              # m = 0: nothing is selected
    nocols = LPInstance("n0", np.zeros(4, np.int64), np.zeros(0, np.int32), np.zeros(0), np.zeros(0), np.ones(3),
                        np.zeros(0, np.int32))                            # a zero-column instance
    nonz = LPInstance("nonz", np.zeros(3, np.int64), np.zeros(0, np.int32), np.zeros(0), rng.standard_normal(4),
                      np.ones(2), np.array([1, 0, 0, 1], np.int32))
    insts = [toy, norows, wide, nocols, square, nonz, toy]
    b = LPBatch.from_instances(insts, tier_wave=4, tier_block=16)
    assert b.inst_m == [9, 0, 12, 3, 6, 2, 9] and b.inst_n == [40, 7, 5, 0, 6, 4, 40]
    z = _randn(b.N, 9)
    pred = b.predict_basis(z)
    assert_prediction(pred, z.cpu().numpy(), b.inst_n, b.inst_m, "degenerate")
    st = pred.stats.cpu().numpy()
    assert st[1, 0] == np.inf and st[1, 1] == float(z.cpu().numpy()[40:47].max())      # m = 0
    assert st[2, 1] == -np.inf and st[4, 1] == -np.inf                                  # every column selected
    assert st[3, 0] == np.inf and st[3, 1] == -np.inf                                   # empty segment
    assert [p.tolist() for p in pred.split()][1:5] == [[], [0, 1, 2, 3, 4], [], [0, 1, 2, 3, 4, 5]]


@gpu
def test_each_output_alone_and_twice(netlib):
    z = torch.tensor(tied_inputs(netlib.N, seed=8)["three_values"], device="cuda") + 0.5 * (_randn(netlib.N, 4) > 1.0)
    full = netlib.predict_basis(z)
    again = netlib.predict_basis(z)
    assert_prediction(full, z.cpu().numpy(), netlib.inst_n, netlib.inst_m, "full call")
    for name in ("mask", "index", "stats"):
        assert same_bits(getattr(full, name), getattr(again, name)), name                 # two calls: bitwise equal
        alone = netlib.predict_basis(z, want=(name,))
        assert all(getattr(alone, other) is None for other in ("mask", "index", "stats") if other != name)
        assert same_bits(getattr(full, name), getattr(alone, name)), name
    with pytest.raises(ValueError):
        netlib.predict_basis(z, want=())
    with pytest.raises(ValueError):
        netlib.predict_basis(z, want=("mask", "labels"))
    with pytest.raises(ValueError):
        netlib.predict_basis(z[:-1].contiguous())


@gpu
def test_model_logits_agree_with_metrics(netlib, golden):
    """Netlib logits from forward with the golden weights: the oracle, and correct_k of mllp_topm_metrics"""
    flat = torch.tensor(golden["weights_flat"], dtype=torch.float32, device="cuda")
    logits = netlib.forward(flat)
    pred = netlib.predict_basis(logits)
    assert_prediction(pred, logits.cpu().numpy(), netlib.inst_n, netlib.inst_m, "model logits")
    met = netlib.topm_metrics(logits).cpu().numpy()
    assert np.array_equal(_correct_from_mask(netlib, pred), met[:, 0])
    # GNNModel.predict: the same through the module surface, and no gradient state is made
    from mllp_amd.model import GNNModel
    model = GNNModel()
    model.load_flat(golden["weights_flat"])
    got = model.to("cuda").predict(netlib)
    for name in ("mask", "index", "stats"):
        assert same_bits(getattr(got, name), getattr(pred, name)), name
    assert all(p.grad is None for p in model.parameters())


@gpu
@pytest.mark.parametrize("name", ["afiro", "25fv47"])
def test_angle_model_predict(name):
    from mllp_amd.angle import AngleModel, build_graph_from_Q_sets, dense_instance_tensors
    from mllp_amd.data import load_packed
    from mllp_amd.model import set_seed
    set_seed(7)
    inst = load_packed([name])[0]
    Q, coefs, basis = dense_instance_tensors(inst)
    g = build_graph_from_Q_sets(Q, coefs, torch.device("cuda"), name, basis)
    model = AngleModel(feat_dim=32).to("cuda")
    pred = model.predict(g)
    with torch.no_grad():
        logits = model(g)
    assert logits.numel() == g.var_num == inst.n
    assert pred.index.numel() == g.basis_num and pred.mask.numel() == inst.n
    assert_prediction(pred, logits.cpu().numpy(), [inst.n], [g.basis_num], name)
    assert len(pred.split()) == 1 and pred.split()[0].size == min(g.basis_num, inst.n)


@gpu
def test_command_line_end_to_end(tmp_path, golden, subset5):
    import linear_program_predict
    from mllp_amd.graph import LPBatch
    from mllp_amd.model import GNNModel
    from mllp_amd.mps import read_mps
    model = GNNModel()
    model.load_flat(golden["weights_flat"])
    weights = str(tmp_path / "linear_program_netlib_gs-topk.pt")
    torch.save(model.state_dict(), weights)
    labels = tmp_path / "labels"
    labels.mkdir()
    for inst in subset5:
        np.save(str(labels / (inst.name + "_basis.npy")), inst.basis)
    mps_dir = os.path.join(ROOT, "tests", "golden", "mps")
    out = tmp_path / "out"
    rc = linear_program_predict.main(["--cfg", _yaml(tmp_path, batch_size=0), "--model", weights, "--mps", mps_dir,
                                      "--out", str(out), "--labels", str(labels)])
    assert rc == 0
    files = sorted(f for f in os.listdir(mps_dir) if f.endswith(".mps"))
    assert len(files) == 5
    assert sorted(os.listdir(str(out))) == sorted([f + "_basis_pred.npy" for f in files] + ["predictions.json"])
    by_name = {i.name: i for i in subset5}
    insts = []
    for f in files:
        inst, _ = read_mps(os.path.join(mps_dir, f), normalize=True)
        inst.basis = by_name[f].basis
        insts.append(inst)
    flat = torch.tensor(golden["weights_flat"], dtype=torch.float32, device="cuda")
    b = LPBatch.from_instances(insts)
    logits = b.forward(flat)
    mask, _, stats = oracle_select(logits.cpu().numpy(), b.inst_n, b.inst_m)
    met = b.topm_metrics(logits).cpu().numpy()
    with open(str(out / "predictions.json")) as fh:
        table = json.load(fh)
    off = np.concatenate([[0], np.cumsum(b.inst_n)])
    for k, f in enumerate(files):
        got = np.load(str(out / (f + "_basis_pred.npy")))
        assert got.dtype == np.int32 and got.shape == (b.inst_n[k],)
        assert np.array_equal(got, mask[off[k]:off[k + 1]].astype(np.int32)), f
        rec = table[f]
        assert rec["m"] == b.inst_m[k] and rec["n"] == b.inst_n[k]
        assert np.float32(float(rec["threshold"])) == stats[k, 0] and np.float32(float(rec["runner_up"])) == stats[k, 1]
        assert np.float32(float(rec["margin"])) == stats[k, 0] - stats[k, 1]
        assert rec["correct"] == float(met[k, 0]) and np.float32(rec["f1"]) == met[k, 1]
    # batch_size 2, no labels: three batches; each file equals the oracle on the logits of the batch it was in
    out2 = tmp_path / "out2"
    linear_program_predict.main(["--cfg", _yaml(tmp_path, batch_size=2), "--model", weights, "--mps", mps_dir,
                                 "--out", str(out2)])
    for i in range(0, 5, 2):
        bb = LPBatch.from_instances(insts[i:i + 2])
        mk, _, _ = oracle_select(bb.forward(flat).cpu().numpy(), bb.inst_n, bb.inst_m)
        o = np.concatenate([[0], np.cumsum(bb.inst_n)])
        for j, f in enumerate(files[i:i + 2]):
            assert np.array_equal(np.load(str(out2 / (f + "_basis_pred.npy"))), mk[o[j]:o[j + 1]].astype(np.int32)), f
    with open(str(out2 / "predictions.json")) as fh:
        assert "correct" not in json.load(fh)[files[0]]


@gpu
def test_command_line_angle_net(tmp_path):
    """method angleNet: AngleModel on the dense angle graph of the instance read from the .mps file"""
    import linear_program_predict
    from mllp_amd.angle import AngleModel, build_graph_from_Q_sets, dense_instance_tensors
    from mllp_amd.model import set_seed
    from mllp_amd.mps import read_mps
    set_seed(11)
    model = AngleModel(feat_dim=32).to("cuda")
    weights = str(tmp_path / "linear_program_netlib_angleNet.pt")
    torch.save(model.state_dict(), weights)
    mps = os.path.join(ROOT, "tests", "golden", "mps", "afiro.mps")
    out = tmp_path / "out"
    assert linear_program_predict.main(["--cfg", _yaml(tmp_path, method="angleNet", extra="angle_feat_dim: 32\n"),
                                        "--model", weights, "--mps", mps, "--out", str(out)]) == 0
    inst, _ = read_mps(mps, normalize=True)
    inst.basis = np.zeros(inst.n, np.int32)
    Q, coefs, basis = dense_instance_tensors(inst)
    g = build_graph_from_Q_sets(Q, coefs, torch.device("cuda"), inst.name, basis)
    with torch.no_grad():
        logits = model(g).cpu().numpy()
    mask, _, stats = oracle_select(logits, [inst.n], [g.basis_num])
    assert np.array_equal(np.load(str(out / "afiro.mps_basis_pred.npy")), mask.astype(np.int32))
    with open(str(out / "predictions.json")) as fh:
        rec = json.load(fh)["afiro.mps"]
    assert rec["m"] == g.basis_num and rec["n"] == inst.n
    assert np.float32(float(rec["threshold"])) == stats[0, 0] and np.float32(float(rec["runner_up"])) == stats[0, 1]
