"""mllp_graph_normalize / LPBatch.normalize: the reference's normalization of a resident batch on the device
(mllp_amd/csrc/normalize.hip; the rule is oracle/mps_norm.py `normalize`).

The yardstick is the reference's own data.  data/netlib_norm.npz (byte-identical to the reference's normalized tensors) is a
FIXED POINT of the stage: every row has unit norm, or right-hand side +5 and norm < 1, or is empty, and every objective has
unit norm.  The stage cancels a positive row scaling and a positive objective scaling, so "multiply rows by r_i and the
objective by 3 in fp64 on the host, normalize on the device" must give back the pack.  The gate is the project's bar: 1e-5 of
each tensor's maximum.

KNIFE EDGE (a condition on the inputs, not a tolerance): a row with |b| / ||row|| equal to the cap to within rounding falls on
either side of `> cap` in fp32, and with b < 0 the two sides differ by the sign of the whole row.  Such rows (b < 0, the
ratio within 5e-4 relative of 5) are computed in fp64 from the fixture on the CPU; the fixtures of the GPU tests against the
pack (subset5, d6cube) have none, the full Netlib pack has 61 of 102 466 rows (25fv47, ken-07, ken-11), which are masked.

Measured on MI355X (every test prints its worst deviation and the fraction of the gate it is): against the pack, over the seven
cases and the full Netlib batch, values 1.7e-7, x1 1.2e-7, x2 8.8e-7 and row scales 4.6e-7 absolute, each below 0.02 of its gate;
the reduction tails 6.7e-8 on scales of up to 2.3, 0.003 of the gate."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

from mllp_amd import _lib
from mllp_amd.data import SUBSET5, LPInstance, load_packed

gpu = pytest.mark.gpu
EINVAL = -1
CAP = 5.0
BAR = 1e-5              # of each tensor's maximum
EDGE = 5e-4             # relative half-width of the knife edge around the cap


# ---------------------------------------------------------------------------------------------------
# shared host data (computed once, never modified)
# ---------------------------------------------------------------------------------------------------
def _rows(inst):
    return np.repeat(np.arange(inst.m), np.diff(inst.indptr))


def _row_sq(inst, values=None, dtype=np.float64):
    v = (inst.values if values is None else values).astype(dtype)
    q = np.zeros(inst.m, dtype)
    nz = np.diff(inst.indptr) > 0
    if v.size:
        q[nz] = np.add.reduceat(v * v, inst.indptr[:-1][nz].astype(np.int64))
    return q


def _knife_edge(inst):
    """fp64: rows with b < 0 whose |b| / ||row|| is within EDGE (relative) of the cap."""
    nrm = np.sqrt(_row_sq(inst))
    ratio = np.abs(inst.rhs) / np.where(nrm > 0, nrm, 1.0)
    return (inst.rhs < 0) & (np.abs(ratio - CAP) <= EDGE * CAP)


def _normalize_host(inst, dtype):
    """The stage of oracle/mps_norm.py:121-128 on an instance's arrays, in `dtype` throughout (fp64: the rule; fp32: the
    restatement whose distance from fp64 is the yardstick).  Returns (values, coefs, rhs, row scale, objective scale)."""
    v, b, c = inst.values.astype(dtype), inst.rhs.astype(dtype), inst.coefs.astype(dtype)
    one, cap = dtype(1), dtype(CAP)
    q = _row_sq(inst, dtype=dtype)
    nrm = np.sqrt(q)
    s = np.where(nrm > 0, one / np.where(nrm > 0, nrm, one), one).astype(dtype)
    over = np.abs(b * s) > cap
    s = np.where(over, cap / np.where(over, b, one), s).astype(dtype)
    cn = np.sqrt((c * c).sum(dtype=dtype))
    t = one / cn if cn > 0 else one
    return s[_rows(inst)] * v, c * t, b * s, s, dtype(t)


def _perturbed(inst, seed):
    """The instance with row i multiplied by r_i in [1/4, 4] (log-uniform) and the objective by 3, in fp64; and r."""
    r = np.exp2(np.random.default_rng(seed).uniform(-2.0, 2.0, inst.m))
    return dataclasses.replace(inst, values=inst.values * r[_rows(inst)], rhs=inst.rhs * r, coefs=inst.coefs * 3.0), r


@pytest.fixture(scope="module")
def pack():
    insts = load_packed()
    assert len(insts) == 97
    return insts


@pytest.fixture(scope="module")
def fixtures(pack):
    by = {i.name: i for i in pack}
    return {"subset5": [by[n] for n in SUBSET5], "d6cube": [by["d6cube.mps"]]}


# ---------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------
def test_knife_edge_census(pack, fixtures):
    for name, insts in fixtures.items():
        assert sum(int(_knife_edge(i).sum()) for i in insts) == 0, f"{name} has knife-edge rows"
    counts = {i.name: int(_knife_edge(i).sum()) for i in pack}
    total_rows = sum(i.m for i in pack)
    print("knife-edge rows:", {k: v for k, v in counts.items() if v}, "of", total_rows)
    assert total_rows == 102466
    assert sum(counts.values()) <= 1e-3 * total_rows        # full Netlib: at most 0.1 % of the rows are masked
    assert max(np.diff(fixtures["d6cube"][0].indptr)) == 6184


def test_the_pack_is_a_fixed_point(pack, fixtures):
    """Every row is of one of three classes, every objective has unit norm; the fp64 stage leaves the chosen fixtures alone."""
    unit = capped = empty = 0
    for inst in pack:
        nrm = np.sqrt(_row_sq(inst))
        n_e = np.diff(inst.indptr) == 0
        n_u = ~n_e & (np.abs(nrm - 1.0) <= 2.5e-14)
        n_c = ~n_e & ~n_u & (inst.rhs == CAP) & (nrm < 1.0)
        assert (n_e | n_u | n_c).all(), inst.name
        assert np.abs(inst.rhs).max(initial=0.0) <= CAP
        unit, capped, empty = unit + int(n_u.sum()), capped + int(n_c.sum()), empty + int(n_e.sum())
        assert abs(np.linalg.norm(inst.coefs) - 1.0) <= 1.9e-15 or not inst.coefs.any(), inst.name
    assert (unit, capped, empty) == (86926, 14844, 696)
    for insts in fixtures.values():
        for inst in insts:
            v, c, b, s, t = _normalize_host(inst, np.float64)
            assert np.abs(v - inst.values).max() <= 1e-13 and np.abs(b - inst.rhs).max() <= 1e-13
            assert np.abs(c - inst.coefs).max() <= 1e-14 and np.abs(s - 1.0).max() <= 1e-13 and abs(t - 1.0) <= 1e-14


def test_fp32_yardstick_is_a_quarter_of_the_gate(pack):
    """The stage restated in fp32 numpy on the perturbed pack (rows x r_i in [1/4, 4], objective x 3) misses the pack by less
    than a quarter of the gate outside the knife-edge mask: what is left of the gate is the room for the summation order."""
    worst = {"values": 0.0, "rhs": 0.0, "coefs": 0.0}
    for k, inst in enumerate(pack):
        p, _ = _perturbed(inst, 100 + k)
        p32 = dataclasses.replace(p, values=p.values.astype(np.float32), rhs=p.rhs.astype(np.float32),
                                  coefs=p.coefs.astype(np.float32))
        v, c, b, _, _ = _normalize_host(p32, np.float32)
        keep = ~_knife_edge(inst)
        worst["values"] = max(worst["values"], np.abs(v - inst.values)[keep[_rows(inst)]].max(initial=0.0))
        worst["rhs"] = max(worst["rhs"], np.abs(b - inst.rhs)[keep].max(initial=0.0))
        worst["coefs"] = max(worst["coefs"], np.abs(c - inst.coefs).max(initial=0.0))
    print("fp32 restatement against the pack, worst absolute deviation:", worst)
    # the gates of the pack: values and objective coefficients reach 1, |b| reaches 5
    assert worst["values"] < 0.25 * BAR * 1.0
    assert worst["coefs"] < 0.25 * BAR * 1.0
    assert worst["rhs"] < 0.25 * BAR * CAP


def test_null_arguments_are_refused_with_a_message():
    L = _lib.lib()
    L.mllp_graph_dims(None, (ctypes.c_int64 * 12)())              # (some other message first)
    assert L.mllp_graph_normalize(None, None, None, 5.0, 0, None, None, None) == EINVAL
    assert b"null" in L.mllp_last_error()
    assert L.mllp_normalize_row_tier(3, None) == EINVAL
    tiers = []
    for n in (0, 64, 65, 1024, 1025, 1 << 40):
        t = ctypes.c_int(-1)
        assert L.mllp_normalize_row_tier(n, ctypes.byref(t)) == 0
        tiers.append(t.value)
    assert tiers == [0, 0, 1, 1, 2, 2]


# ---------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def LPBatch():
    _lib.lib()
    assert torch.cuda.is_available()
    from mllp_amd.graph import LPBatch as cls
    return cls


def _cat(insts, field):
    return np.concatenate([getattr(i, field) for i in insts])


def _close(got, want, what, worst=None):
    """|got - want| <= BAR * max|want|, elementwise; prints the worst deviation as a fraction of the gate first."""
    if isinstance(got, torch.Tensor):
        got = got.cpu().numpy()
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    gate = BAR * np.abs(want).max(initial=0.0)
    dev = np.abs(got - want).max(initial=0.0)
    print(f"{what}: worst deviation {dev:.3e}, gate {gate:.3e}, fraction {dev / gate if gate else 0.0:.4f}")
    if worst is not None:
        worst.append(dev / gate if gate else 0.0)
    assert np.isfinite(got).all() and dev <= gate, f"{what}: {dev:.3e} above the gate {gate:.3e}"


def _same(a, b, what):
    if isinstance(a, torch.Tensor):
        a, b = a.cpu().numpy(), b.cpu().numpy()
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{what}: bytes differ"


def _params(seed=5):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(_lib.NUM_PARAMS, generator=g) * 0.2).to("cuda")


def _dev(v):
    return torch.tensor(np.asarray(v), dtype=torch.float32, device="cuda")


def _perturbed_list(insts, seed=1):
    out = [_perturbed(i, seed + k) for k, i in enumerate(insts)]
    return [p for p, _ in out], np.concatenate([r for _, r in out])


CASES = [("subset5", [k]) for k in range(5)] + [("subset5", list(range(5))), ("d6cube", [0])]


@gpu
@pytest.mark.parametrize("fixture,which", CASES, ids=[f"{f}-{'all' if len(w) > 1 else w[0]}" for f, w in CASES])
def test_against_the_pack(LPBatch, fixtures, fixture, which):
    """1. Un-normalize in fp64 on the host, normalize on the device: values, x1, x2 are the pack's at 1e-5 of each tensor's
    maximum.  The scales: the pack is a fixed point (its own row scale is 1 for a unit row and 5 / 5 for a capped one), so
    the applied s_i times r_i must be 1 on every row that has nonzeros -- and s_i itself must be the fp64 rule's on every
    row, the empty ones included (whose b = 0 stays, s = 1) --, and 3 t_k must be 1.
    Measured on MI355X, worst over the cases (the full Netlib batch of the next test included): values 1.7e-7 (0.017 of the
    gate), x1 1.2e-7 (0.012), x2 8.8e-7 (0.018), row scales 4.6e-7 (0.012), row scale x r_i 1.6e-7 (0.016)."""
    insts = [fixtures[fixture][k] for k in which]
    assert not any(_knife_edge(i).any() for i in insts)
    pert, r = _perturbed_list(insts)
    b = LPBatch.from_instances(pert)
    row_scale, obj_scale = b.normalize()
    torch.cuda.synchronize()
    _close(b.export(2), _cat(insts, "values"), "values against the pack")
    _close(b.x1, _cat(insts, "coefs"), "x1 against the pack")
    _close(b.x2, _cat(insts, "rhs"), "x2 against the pack")
    s64 = np.concatenate([_normalize_host(p, np.float64)[3] for p in pert])
    _close(row_scale, s64, "row scales against the fp64 rule")
    has = np.concatenate([np.diff(i.indptr) > 0 for i in insts])
    _close((row_scale.cpu().numpy().astype(np.float64) * r)[has], np.ones(int(has.sum())), "row scale x r_i against the pack's 1")
    _close(obj_scale.cpu().numpy().astype(np.float64) * 3.0, np.ones(len(insts)), "objective scale x 3")


@gpu
def test_against_the_pack_full_netlib(LPBatch, pack):
    """1b. All 97 instances as one batch (every tier, 102 466 rows), the 61 knife-edge rows masked."""
    pert, r = _perturbed_list(pack, 300)
    edge = np.concatenate([_knife_edge(i) for i in pack])
    assert edge.sum() <= 1e-3 * edge.size
    b = LPBatch.from_instances(pert)
    b.normalize()
    torch.cuda.synchronize()
    row_off = np.cumsum([0] + [i.m for i in pack[:-1]])
    keep_e = ~edge[np.concatenate([_rows(i) + off for i, off in zip(pack, row_off)])]
    _close(b.export(2)[keep_e], _cat(pack, "values")[keep_e], "values against the pack")
    _close(b.x1, _cat(pack, "coefs"), "x1 against the pack")
    _close(b.x2.cpu().numpy()[~edge], _cat(pack, "rhs")[~edge], "x2 against the pack")


# lengths of test 2 with the tier each must reach: both sides of the thresholds 64 | 65 and 1024 | 1025, of one, two and
# several terms per lane in each tier (16, 64 and 256 lanes), the longest row of Netlib's class and one beyond 6144
TAILS = {0: 0, 1: 0, 15: 0, 16: 0, 17: 0, 31: 0, 32: 0, 33: 0, 63: 0, 64: 0,
         65: 1, 127: 1, 128: 1, 129: 1, 255: 1, 256: 1, 257: 1, 1023: 1, 1024: 1,
         1025: 2, 1279: 2, 1280: 2, 1281: 2, 6145: 2}


def _tails_instance(seed=7, n=6400):
    """One instance: every length of TAILS twice, at shuffled positions, the second copy of a length with the values (and
    columns) of the first -- equal rows at different places in different workgroups.  Values of a row are N(0, 1) / sqrt(len),
    so every norm is of order 1 and the gate (of the largest scale) means the same for every row."""
    rng = np.random.default_rng(seed)
    lens = np.array(list(TAILS) * 2)
    order = rng.permutation(lens.size)
    rows = {}
    for L in TAILS:
        cols = np.sort(rng.choice(n, size=L, replace=False)).astype(np.int32)
        rows[L] = (cols, rng.standard_normal(L) * rng.uniform(0.5, 2.0) / np.sqrt(max(L, 1)))
    lens = lens[order]
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    indices = np.concatenate([rows[L][0] for L in lens]).astype(np.int32)
    values = np.concatenate([rows[L][1] for L in lens])
    coefs = rng.standard_normal(n)
    return LPInstance("tails", indptr, indices, values, coefs, rng.uniform(-3.0, 3.0, lens.size), np.zeros(n, np.int32)), lens


@gpu
def test_reduction_tails(LPBatch):
    """2. Compute only, cap disabled: s_i = 1 / ||row_i|| against fp64 for every length of TAILS, the tier of each length
    asserted; equal rows at different positions get equal bits; nothing but the scales is written.
    Measured on MI355X: row scales 6.7e-8 from fp64 (0.003 of the gate of 2.3e-5), the objective scale 1.4e-10 (0.001)."""
    inst, lens = _tails_instance()
    for L, tier in TAILS.items():
        assert LPBatch.normalize_row_tier(L) == tier, f"length {L}"
    assert {0, 1, 2} == set(TAILS.values()) and lens.size > 2 * 16        # more than two workgroups of 16 rows
    b = LPBatch.from_instances([inst])
    v0, x1, x2 = b.export(2), b.x1.clone(), b.x2.clone()
    row_scale, obj_scale = b.normalize(rhs_cap=0.0, compute_only=True)
    torch.cuda.synchronize()
    v32 = inst.values.astype(np.float32).astype(np.float64)              # what the batch holds
    q = _row_sq(inst, v32)
    want = np.where(q > 0, 1.0 / np.sqrt(np.where(q > 0, q, 1.0)), 1.0)
    _close(row_scale, want, "row scales of the tail lengths against fp64")
    c32 = inst.coefs.astype(np.float32).astype(np.float64)
    _close(obj_scale, [1.0 / np.linalg.norm(c32)], "objective scale against fp64")
    got = row_scale.cpu().numpy()
    assert got[lens == 0].tolist() == [1.0, 1.0]
    for L in TAILS:
        i, j = np.flatnonzero(lens == L)
        assert got[i].tobytes() == got[j].tobytes(), f"equal rows of length {L} at positions {i} and {j} differ"
    _same(b.export(2), v0, "values after compute only")
    _same(b.x1, x1, "x1 after compute only")
    _same(b.x2, x2, "x2 after compute only")


def _cap_instance():
    indptr = np.array([0, 2, 4, 4, 4, 6], np.int64)
    indices = np.array([0, 2, 0, 2, 0, 1], np.int32)
    values = np.array([3.0, 4.0, 3.0, 4.0, 1.2, 1.6])
    rhs = np.array([100.0, -100.0, 0.0, -7.0, 2.0])
    return LPInstance("cap", indptr, indices, values, np.array([3.0, 0.0, 4.0]), rhs, np.zeros(3, np.int32))


@gpu
def test_cap_semantics(LPBatch):
    """3. Known answers: a positive and a negative row beyond the cap, an empty row with b = 0 and with b = -7, a row below."""
    b = LPBatch.from_instances([_cap_instance()])
    s, t = b.normalize()
    torch.cuda.synchronize()
    _close(s, [0.05, -0.05, 1.0, -5.0 / 7.0, 0.5], "row scales")
    _close(t, [0.2], "objective scale")
    _close(b.export(2), [0.15, 0.2, -0.15, -0.2, 0.6, 0.8], "values")
    _close(b.x2, [5.0, 5.0, 0.0, 5.0, 1.0], "right-hand sides")
    _close(b.x1, [0.6, 0.0, 0.8], "objective")
    assert s.cpu().numpy()[2] == 1.0 and b.x2.cpu().numpy()[2] == 0.0 and (s.cpu().numpy()[[1, 3]] < 0).all()
    for cap in (0.0, float("inf"), -1.0, float("nan")):
        b = LPBatch.from_instances([_cap_instance()])
        s, t = b.normalize(rhs_cap=cap)
        torch.cuda.synchronize()
        _close(s, [0.2, 0.2, 1.0, 1.0, 0.5], f"row scales, cap {cap}")
        _close(b.export(2), [0.6, 0.8, 0.6, 0.8, 0.6, 0.8], f"values, cap {cap}")
        _close(b.x2, [20.0, -20.0, 0.0, -7.0, 1.0], f"right-hand sides, cap {cap}")
    b = LPBatch.from_instances([_cap_instance()])
    s, _ = b.normalize(rhs_cap=30.0)                                     # another cap: only row 1 (|b s| = 20) is below it
    _close(s, [0.2, 0.2, 1.0, 1.0, 0.5], "row scales, cap 30")


def _fresh_like(LPBatch, b, insts):
    """A new batch built from b's exported values, with b's x1 / x2 (bit for bit)."""
    from test_set_values import _with_values
    fresh = LPBatch.from_instances(_with_values(insts, b.export(2)))
    fresh.x1.copy_(b.x1)
    fresh.x2.copy_(b.x2)
    return fresh


@gpu
def test_both_paths_match_a_fresh_build(LPBatch, fixtures):
    """4a. Forward logits on path 1 and on path 2 are bitwise those of a fresh batch built from the normalized values, with
    the inputs bound before the call; a backward without a new forward is refused."""
    pert, _ = _perturbed_list(fixtures["subset5"], 11)
    params = _params()
    for path in (1, 2):
        b = LPBatch.from_instances(pert)
        b.set_path(path)
        stale = b.forward(params).clone()                   # binds x1 / x2 (the fused path's gathered copies)
        b.normalize()
        dl = torch.randn(b.N, generator=torch.Generator().manual_seed(3)).to("cuda")
        with pytest.raises(_lib.MllpError, match="forward"):
            b.backward(params, dl)
        fresh = _fresh_like(LPBatch, b, pert)
        fresh.set_path(path)
        got = b.forward(params)
        assert not torch.equal(got, stale)
        _same(got, fresh.forward(params), f"logits on path {path}")
        _same(b.backward(params, dl), fresh.backward(params, dl), f"gradients on path {path}")
        for k in range(7):
            _same(b.export(k), fresh.export(k), f"export({k})")


@gpu
def test_every_copy_kind_is_refreshed(LPBatch, fixtures):
    """4b. With the streamed copies (geometries 0-4) and the library-built LDS-tiled copies attached: the copies are byte for
    byte those built from the normalized values, and the sweeps on them give the same bits."""
    from test_set_values import _attach_all, _copies, _same_lists, _sweeps
    pert, _ = _perturbed_list(fixtures["subset5"], 12)
    params = _params()
    b = LPBatch.from_instances(pert)
    tiled = _attach_all(b)
    assert tiled, "no LDS-tiled copy could be attached"
    before = b.set_values_bytes()
    b.normalize()
    assert b.set_values_bytes() == before + 4 * (b.nnz + b.M + b.n_inst)   # the scaled values and the scales' scratch
    fresh = _fresh_like(LPBatch, b, pert)
    assert _attach_all(fresh) == tiled
    _same_lists(_copies(b, tiled), _copies(fresh, tiled), "copies after normalize against copies built from its values")
    _same_lists(_sweeps(b, params), _sweeps(fresh, params), "sweeps on the refreshed copies")


@gpu
def test_alone_equals_batched_bitwise(LPBatch, fixtures):
    """5. An instance normalizes to the same bits alone and inside a batch: scales, values, x1, x2."""
    pert, _ = _perturbed_list(fixtures["subset5"] + fixtures["d6cube"], 13)
    batch = LPBatch.from_instances(pert)
    s, t = batch.normalize()
    v, off_m, off_e = batch.export(2), 0, 0
    for k, p in enumerate(pert):
        one = LPBatch.from_instances([p])
        s1, t1 = one.normalize()
        _same(s1, s[off_m:off_m + p.m], f"row scales of {p.name}")
        _same(t1, t[k:k + 1], f"objective scale of {p.name}")
        _same(one.export(2), v[off_e:off_e + p.nnz], f"values of {p.name}")
        _same(one.x2, batch.x2[off_m:off_m + p.m], f"x2 of {p.name}")
        off_m, off_e = off_m + p.m, off_e + p.nnz


@gpu
def test_idempotence(LPBatch, fixtures):
    """6. A second call moves nothing beyond the gate, and its scales are 1 (5 / 5 on the capped rows)."""
    insts = fixtures["subset5"]
    pert, _ = _perturbed_list(insts, 14)
    b = LPBatch.from_instances(pert)
    b.normalize()
    v, x1, x2 = b.export(2), b.x1.clone(), b.x2.clone()
    capped = x2.cpu().numpy() == np.float32(CAP)
    s, t = b.normalize()
    torch.cuda.synchronize()
    _close(b.export(2), v, "values after the second call")
    _close(b.x1, x1.cpu().numpy(), "x1 after the second call")
    _close(b.x2, x2.cpu().numpy(), "x2 after the second call")
    _close(s, np.ones(b.M), "second row scales")
    _close(t, np.ones(b.n_inst), "second objective scales")
    assert (np.abs(_cat(insts, "rhs")) == CAP).sum() > 0 and capped.sum() > 0     # (the case has capped rows)


def _load(b, pert):
    """The batch's values, x1 and x2 set (again) to the perturbed instances'."""
    b.set_values(_dev(_cat(pert, "values")))
    b.x1.copy_(_dev(_cat(pert, "coefs")))
    b.x2.copy_(_dev(_cat(pert, "rhs")))


def _state(b, scales):
    torch.cuda.synchronize()
    return [b.export(2), b.x1.clone(), b.x2.clone(), scales[0].clone(), scales[1].clone()]


@gpu
def test_repeat_and_capture(LPBatch, fixtures):
    """7. Two eager calls on equal inputs give equal bits; a captured call replayed on other values equals the eager call on
    those values.  ONE capture, ONE replay."""
    from test_set_values import _same_lists
    insts = fixtures["subset5"]
    pert1, _ = _perturbed_list(insts, 15)
    pert2, _ = _perturbed_list(insts, 16)
    b = LPBatch.from_instances(pert1)
    first = _state(b, b.normalize())                         # eager: allocates
    _load(b, pert1)
    _same_lists(_state(b, b.normalize()), first, "a second eager call on equal inputs")
    other = LPBatch.from_instances(pert2)
    want = _state(other, other.normalize())
    _load(b, pert1)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scales = b.normalize()
    _load(b, pert2)
    graph.replay()
    got = _state(b, scales)
    assert not np.array_equal(want[0], first[0])
    _same_lists(got, want, "the replay against the eager call")
    b.invalidate_inputs()
    _same(b.forward(_params()), other.forward(_params()), "logits after the replay")


@gpu
def test_refusals_write_nothing(LPBatch, fixtures):
    """8. A caller-owned tiled copy, compute only with a null output, unknown flags: MLLP_EINVAL and not a byte moved.
    Compute only leaves values, x1 and x2 alone and a pending backward valid."""
    L = _lib.lib()
    pert, _ = _perturbed_list(fixtures["subset5"], 17)
    params = _params()
    b = LPBatch.from_instances(pert)
    b.set_path(1)
    before = [b.export(2), b.x1.clone(), b.x2.clone()]

    def unchanged(what):
        torch.cuda.synchronize()
        for x, y in zip([b.export(2), b.x1, b.x2], before):
            _same(x, y, what)

    assert b.enable_tiled(False, variant=1, builder="torch") is not None
    with pytest.raises(_lib.MllpError, match="mllp_graph_build_tiled"):
        b.normalize()
    unchanged("after the refusal of a caller-owned tiled copy")
    b.disable_tiled(False, 1)
    rs, os_ = torch.full((b.M,), 7.0, device="cuda"), torch.full((b.n_inst,), 7.0, device="cuda")
    args = (b._h, _lib.ptr(b.x1), _lib.ptr(b.x2), 5.0)
    for flags, r, o, word in ((1, None, os_, "null output"), (1, rs, None, "null output"), (2, rs, os_, "flag"),
                              (-1, rs, os_, "flag")):
        assert L.mllp_graph_normalize(*args, flags, _lib.ptr(r), _lib.ptr(o), _lib.current_stream()) == EINVAL
        assert word.encode() in L.mllp_last_error()
    assert L.mllp_graph_normalize(b._h, None, _lib.ptr(b.x2), 5.0, 0, None, None, None) == EINVAL
    assert L.mllp_graph_normalize(b._h, _lib.ptr(b.x1), None, 5.0, 0, None, None, None) == EINVAL
    unchanged("after the refused calls")
    assert float(rs.min()) == 7.0 and float(os_.min()) == 7.0
    dl = torch.randn(b.N, generator=torch.Generator().manual_seed(3)).to("cuda")
    b.forward(params)
    want = b.backward(params, dl).clone()
    s, t = b.normalize(compute_only=True)
    unchanged("after compute only")
    _same(b.backward(params, dl), want, "the pending backward after compute only")
    ref = LPBatch.from_instances(pert)
    s2, t2 = ref.normalize()
    _same(s, s2, "compute-only row scales against the applied ones")
    _same(t, t2, "compute-only objective scales against the applied ones")
    assert L.mllp_graph_normalize(*args, 0, None, None, _lib.current_stream()) == 0      # null outputs: library scratch
    for x, y, what in ((b.export(2), ref.export(2), "values"), (b.x1, ref.x1, "x1"), (b.x2, ref.x2, "x2")):
        _same(x, y, what + " after a call without output arrays")
    assert not torch.equal(b.x2, before[2])
