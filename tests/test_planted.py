"""Planted-basis LPs (mllp_graph_plant_basis, mllp_lp_certificate; mllp_amd/planted.py).

CPU: the symbols, the refusals that need no GPU, the torch pattern generator, the oracle judged by a dense fp64 solve,
the matching on real patterns.  GPU: one ragged batch (tests/planted_oracle.py::ragged_case) through rule parity, the dense
fp64 solve, the certificate, normalization with a signed cap, the refresh of every copy, determinism, refusals, the memory
contract, the driver and a short training run.  Every tolerance is planted_oracle.row_bound: (L + 3) 2^-24 sum|terms|.
"""
import ctypes
import json
import math

import numpy as np
import pytest
import torch

import planted_oracle as po
from mllp_amd import _lib
from mllp_amd.data import SUBSET5, LPInstance, load_packed

gpu = pytest.mark.gpu
EINVAL = -1


# ---------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------
def test_symbols_are_exported():
    L = _lib.lib()
    for name in ("mllp_graph_plant_basis", "mllp_lp_certificate", "mllp_lp_certificate_scratch_bytes"):
        assert hasattr(L, name) and name in _lib._PROTOTYPES
    from mllp_amd.graph import LPBatch
    assert callable(LPBatch.plant_basis) and callable(LPBatch.certificate)


def test_bad_arguments_are_refused_without_a_gpu():
    """Null arguments, dominance <= 1, floor <= 0 and non-finite ones: MLLP_EINVAL with a message before any HIP call (the
    graph is a block of zeros that is never a graph: the checks come first)."""
    L = _lib.lib()
    fake = ctypes.create_string_buffer(1 << 16)
    g = ctypes.cast(fake, ctypes.c_void_p)
    buf = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    ok = [g, buf, buf, buf, buf, 1.25, 0.25, buf, buf, buf, None]
    L.mllp_graph_dims(None, (ctypes.c_int64 * 12)())              # (some other message first)
    for k in (0, 1, 2, 3, 4, 7, 8, 9):
        args = list(ok)
        args[k] = None
        assert L.mllp_graph_plant_basis(*args) == EINVAL
        assert b"mllp_graph_plant_basis" in L.mllp_last_error() and b"null" in L.mllp_last_error()
    for dom in (1.0, 0.5, -2.0, math.inf, math.nan):
        assert L.mllp_graph_plant_basis(*ok[:5], dom, 0.25, *ok[7:]) == EINVAL
        assert b"dominance" in L.mllp_last_error()
    for fl in (0.0, -0.25, math.inf, math.nan):
        assert L.mllp_graph_plant_basis(*ok[:5], 1.25, fl, *ok[7:]) == EINVAL
        assert b"floor" in L.mllp_last_error()
    cert = [g, buf, buf, buf, buf, buf, buf, buf, None]
    for k in range(8):
        args = list(cert)
        args[k] = None
        assert L.mllp_lp_certificate(*args) == EINVAL
        assert b"null" in L.mllp_last_error()
    assert L.mllp_lp_certificate_scratch_bytes(None, None) == EINVAL
    assert L.mllp_lp_certificate_scratch_bytes(g, None) == EINVAL


def _check_pattern(inst_m, inst_n, ptr, idx, pivot):
    ptr, idx, pivot = ptr.numpy().astype(np.int64), idx.numpy().astype(np.int64), pivot.numpy().astype(np.int64)
    assert ptr[0] == 0 and ptr[-1] == len(idx) and len(ptr) == sum(inst_m) + 1 and (np.diff(ptr) >= 1).all()
    rows = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    same_row = rows[1:] == rows[:-1]
    assert (np.diff(idx)[same_row] > 0).all(), "a row is not strictly ascending"
    hit = np.bincount(rows[idx == pivot[rows]], minlength=len(pivot))
    assert (hit == 1).all(), "a pivot is not an entry of its row"
    assert len(np.unique(pivot)) == len(pivot), "pivots are not injective"
    lo = np.repeat(np.concatenate([[0], np.cumsum(inst_n)])[:-1], inst_m)
    assert ((pivot >= lo) & (pivot < lo + np.repeat(inst_n, inst_m))).all(), "a pivot outside its instance's columns"
    assert ((idx >= lo[rows]) & (idx < (lo + np.repeat(inst_n, inst_m))[rows])).all()


def test_planted_pattern_on_cpu():
    from mllp_amd.planted import planted_pattern
    for n_inst, m, n, mean in ((4, 7, 19, 3.0), (2, 30, 30, 5.0), (3, 1, 1, 1.0), (1, 40, 100, 12.0)):
        inst_m, inst_n, ptr, idx, pivot = planted_pattern(n_inst, m, n, mean, 11, "cpu")
        assert inst_m == [m] * n_inst and inst_n == [n] * n_inst and ptr.dtype == idx.dtype == pivot.dtype == torch.int32
        _check_pattern(inst_m, inst_n, ptr, idx, pivot)
        for i in range(n_inst):                         # instance i alone (seed + i) is instance i of the batch
            _, _, p1, i1, v1 = planted_pattern(1, m, n, mean, 11 + i, "cpu")
            lo, hi = int(ptr[i * m]), int(ptr[(i + 1) * m])
            assert torch.equal(ptr[i * m:(i + 1) * m + 1] - lo, p1)
            assert torch.equal(idx[lo:hi] - i * n, i1) and torch.equal(pivot[i * m:(i + 1) * m] - i * n, v1)
    with pytest.raises(ValueError, match="n >= m"):
        planted_pattern(1, 5, 4, 2.0, 0, "cpu")


@pytest.fixture(scope="module")
def case():
    return po.ragged_case()


def _slices(c, k):
    r = slice(c["ptr_m"][k], c["ptr_m"][k + 1])
    s = slice(c["ptr_n"][k], c["ptr_n"][k + 1])
    e = slice(c["nnz_off"][k], c["nnz_off"][k + 1])
    return r, s, e


def _dense_of(c, k, values):
    r, s, e = _slices(c, k)
    ptr = c["ptr"][r.start:r.stop + 1].astype(np.int64)
    return po.dense(ptr - ptr[0], c["idx"][e] - s.start, values[e], r.stop - r.start, s.stop - s.start)


def test_the_case_has_every_tier():
    c = po.ragged_case()
    r, s, e = _slices(c, 4)
    rows, cols = np.diff(c["ptr"].astype(np.int64))[r], np.bincount(c["idx"], minlength=c["N"])[s]
    for length in po.LONG:
        assert (rows == length).any() and (cols == length).any()
    assert c["inst_m"] == [1, 3, 5, 40, 1200] and c["inst_n"] == [1, 3, 12, 100, 2400]
    basic = np.zeros(c["N"], bool)
    basic[c["pivot"]] = True
    assert basic[c["ptr_n"][1]:c["ptr_n"][2]].all()                                     # 3 x 3: all basic
    long_row = int(np.flatnonzero(rows == 1100)[0]) + r.start
    assert basic[c["idx"][c["ptr"][long_row]:c["ptr"][long_row + 1]]].mean() > 0.7      # ... most of them basic
    L = _lib.lib()
    tiers = set()
    for length in list(rows) + list(cols):
        t = ctypes.c_int(-1)
        assert L.mllp_normalize_row_tier(int(length), ctypes.byref(t)) == 0
        tiers.add(t.value)
    assert tiers == {0, 1, 2}


def test_the_oracle_certifies_itself(case):
    """The fp64 rule on the GPU tests' shapes, judged by a dense fp64 solve of what it stores: min x_B > 0.25 and min
    reduced cost > 0.25 (xstar and slack are in U(0.5, 1.5)); the oracle's own certificate agrees."""
    c = case
    o = po.plant(c["ptr"], c["idx"], c["val"], c["pivot"], c["xstar"], c["ystar"], c["slack"], c["N"])
    changed = np.flatnonzero(o["values"] != c["val"].astype(np.float64))
    assert set(changed) <= set(o["pivot_pos"])
    assert (np.abs(o["values"][o["pivot_pos"]]) - o["off"] >= po.FLOOR - 1e-9).all()    # strict row dominance
    for k in range(len(c["inst_m"])):
        r, s, e = _slices(c, k)
        x_b, red, cond = po.dense_solve(_dense_of(c, k, o["values"]), o["b"][r], o["c"][s], o["labels"][s])
        print(f"instance {k}: min x_B {x_b.min():.4f}, min reduced cost {red.min(initial=np.inf):.4f}, cond {cond:.1f}")
        assert x_b.min() > 0.25 and red.min(initial=np.inf) > 0.25
    cert, _ = po.certificate(c["ptr"], c["idx"], o["values"], o["c"], o["b"], c["xstar"] * o["labels"], c["ystar"],
                             o["labels"], c["ptr_m"], c["ptr_n"])
    assert (cert[:, 0] < 1e-9).all() and (cert[:, 1] >= 0.5).all() and (cert[:, 2] == 0).all()
    assert (cert[:, 3] >= 0.5 - 1e-9).all() and (cert[:, 4] < 1e-9).all() and list(cert[:, 5]) == c["inst_m"]


def test_pivots_by_matching_on_the_golden_instances():
    from mllp_amd.planted import pivots_by_matching
    for inst in load_packed(SUBSET5):
        piv = pivots_by_matching(inst)
        assert piv.dtype == np.int32 and piv.shape == (inst.m,) and len(np.unique(piv)) == inst.m
        for r in range(inst.m):
            assert piv[r] in inst.indices[inst.indptr[r]:inst.indptr[r + 1]]
    holed = LPInstance("holed", np.array([0, 2, 2, 3]), np.array([0, 1, 2], np.int32), np.ones(3), np.zeros(3), np.zeros(3),
                       np.zeros(3, np.int32))
    with pytest.raises(ValueError, match="holed"):
        pivots_by_matching(holed)


# ---------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def LPBatch():
    _lib.lib()
    assert torch.cuda.is_available()
    from mllp_amd.graph import LPBatch as cls
    return cls


def _dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda")


def _poison(n):
    return torch.full((n,), float("nan"), device="cuda")


def _build(LPBatch, c, values=None, x1=None, x2=None, labels=None):
    return LPBatch.from_device_csr(c["inst_m"], c["inst_n"], _dev(c["ptr"], torch.int32), _dev(c["idx"], torch.int32),
                                   _dev(c["val"] if values is None else values),
                                   _poison(c["N"]) if x1 is None else x1, _poison(c["M"]) if x2 is None else x2,
                                   _poison(c["N"]) if labels is None else labels)


def _plant(b, c, xstar=None):
    b.plant_basis(_dev(c["pivot"], torch.int32), _dev(c["xstar"] if xstar is None else xstar), _dev(c["ystar"]), _dev(c["slack"]),
                  po.DOMINANCE, po.FLOOR)
    torch.cuda.synchronize()
    return b


def _state(b):
    torch.cuda.synchronize()
    return dict(values=b.export(2), csc=b.export(5), x1=b.x1.cpu().numpy(), x2=b.x2.cpu().numpy(), labels=b.labels.cpu().numpy())


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{what}: bytes differ"


def _within(got, want, bound, what):
    got, want, bound = (np.asarray(a, np.float64) for a in (got, want, bound))
    dev = np.abs(got - want)
    worst = int(np.argmax(dev - bound)) if dev.size else 0
    if dev.size:
        print(f"{what}: worst |error| / bound {np.max(dev / np.maximum(bound, 1e-300)):.4f} over {dev.size}")
    assert np.isfinite(got).all() and (dev <= bound).all(), (f"{what}: element {worst} is off by {dev.flat[worst]:.3e}, "
                                                              f"bound {bound.flat[worst]:.3e}")


def _certifies(b, x, y, what):
    """(x, y, b.labels) certify the batch as it is stored, judged on its exported data: the device's six figures are within
    the oracle's bounds of the oracle's, and the residuals (fields 0 and 4) are at most 10 / 3 of those bounds.  Why 10 / 3:
    the stored LP is the planted one, scaled by `normalize` or not, with at most one rounding per stored number (a' = fl(s a),
    b' = fl(s b), c' = fl(t c); y' = fl(fl(t y) / s) has two), on top of the (L + 3) u sum|terms| of planting b and c: its
    TRUE residuals are within (L + 7) u sum|terms'|.  The device evaluation adds (L + 3) u sum|terms'|, and
    (2 L + 10) / (L + 3) <= 10 / 3.  Returns the figures."""
    torch.cuda.synchronize()
    ptr, idx, val = b.export(0), b.export(1), b.export(2)
    ptr_m, ptr_n = np.concatenate([[0], np.cumsum(b.inst_m)]), np.concatenate([[0], np.cumsum(b.inst_n)])
    labels = b.labels.cpu().numpy()
    got = b.certificate(x, y).cpu().numpy()
    want, bound = po.certificate(ptr, idx, val, b.x1.cpu().numpy(), b.x2.cpu().numpy(), x.cpu().numpy(), y.cpu().numpy(), labels,
                                 ptr_m, ptr_n)
    fin = np.isfinite(want)
    assert np.array_equal(np.isinf(got), ~fin) and (got[~fin] > 0).all(), what            # empty sets: +inf
    _within(got[fin], want[fin], bound[fin], what)
    print(what, "worst residuals", got[:, 0].max(), got[:, 4].max(), "smallest x_B, reduced cost", got[:, 1].min(), got[:, 3].min())
    assert (got[:, 0] <= bound[:, 0] * 10.0 / 3.0).all() and (got[:, 4] <= bound[:, 4] * 10.0 / 3.0).all(), what
    assert (got[:, 1] > 0).all() and (got[:, 2] == 0).all() and (got[:, 3] > 0).all() and list(got[:, 5]) == list(b.inst_m), what
    return got


@pytest.fixture(scope="module")
def planted(LPBatch, case):
    """the ragged batch planted ONCE (outputs NaN-poisoned before), with its exported state"""
    b = _build(LPBatch, case)
    _plant(b, case)
    return b, _state(b)


@gpu
def test_rule_parity(planted, case):
    """Labels exact, every non-pivot value bit-identical, pivot values / x2 / x1 against the fp64 rule, each stage fed the
    device's own fp32 output of the stage before."""
    c = case
    _, st = planted
    o = po.plant(c["ptr"], c["idx"], c["val"], c["pivot"], c["xstar"], c["ystar"], c["slack"], c["N"])
    _same(st["labels"], o["labels"].astype(np.float32), "labels")
    keep = np.ones(len(c["val"]), bool)
    keep[o["pivot_pos"]] = False
    _same(st["values"][keep], c["val"][keep], "non-pivot values")
    _within(st["values"][o["pivot_pos"]], o["values"][o["pivot_pos"]], po.row_bound(o["row_len"], o["pivot_abs"]), "pivot values")
    staged = po.rhs_and_costs(c["ptr"], c["idx"], st["values"], c["pivot"], c["xstar"], c["ystar"], c["slack"], c["N"])
    _within(st["x2"], staged["b"], po.row_bound(o["row_len"], staged["b_abs"]), "x2 = b")
    _within(st["x1"], staged["c"], po.row_bound(o["col_len"], staged["c_abs"]), "x1 = c")
    rows = np.repeat(np.arange(c["M"]), np.diff(c["ptr"].astype(np.int64)))
    order = np.lexsort((rows, c["idx"]))                     # CSR(A^T): by column, rows ascending
    _same(st["csc"], st["values"][order], "the transposed orientation's values")


@gpu
def test_optimality_by_dense_solve(planted, case):
    """A dense fp64 solve of the exported data: |x_B - xstar|_inf <= (max row bound) / min_i(|d_i| - off_i), hence
    x_B > 0, and every reduced cost is positive."""
    c = case
    _, st = planted
    staged = po.rhs_and_costs(c["ptr"], c["idx"], st["values"], c["pivot"], c["xstar"], c["ystar"], c["slack"], c["N"])
    row_len = np.diff(c["ptr"].astype(np.int64))
    o = po.plant(c["ptr"], c["idx"], st["values"], c["pivot"], c["xstar"], c["ystar"], c["slack"], c["N"])   # (off of the stored rows)
    margin = np.abs(st["values"][o["pivot_pos"]].astype(np.float64)) - o["off"]
    for k in range(len(c["inst_m"])):
        r, s, e = _slices(c, k)
        x_b, red, cond = po.dense_solve(_dense_of(c, k, st["values"]), st["x2"][r], st["x1"][s], st["labels"][s])
        on = st["labels"][s] != 0
        assert margin[r].min() > 0.0
        bound = po.row_bound(row_len[r], staged["b_abs"][r]).max() / margin[r].min()
        err = np.abs(x_b - c["xstar"][s][on].astype(np.float64)).max()
        print(f"instance {k}: |x_B - xstar| {err:.3e}, bound {bound:.3e}, min x_B {x_b.min():.4f}, "
              f"min reduced cost {red.min(initial=np.inf):.4f}, cond {cond:.1f}")
        assert err <= bound and x_b.min() > 0.0 and red.min(initial=np.inf) > 0.0


@gpu
def test_certificate_matches_the_oracle(planted, case):
    c = case
    b, st = planted
    x = _dev(c["xstar"] * st["labels"])
    got = b.certificate(x, _dev(c["ystar"])).cpu().numpy()
    want, bound = po.certificate(c["ptr"], c["idx"], st["values"], st["x1"], st["x2"], c["xstar"] * st["labels"], c["ystar"],
                                 st["labels"], c["ptr_m"], c["ptr_n"])
    assert got.shape == (5, 6) and got.dtype == np.float32
    fin = np.isfinite(want)
    assert np.array_equal(np.isinf(got), ~fin) and (got[~fin] > 0).all()          # empty sets: +inf
    # a max / min of figures each within its bound moves by at most the largest bound (want is finite where compared)
    _within(got[fin], want[fin], bound[fin], "certificate")
    assert list(got[:, 5]) == c["inst_m"] and (got[:, 2] == 0).all()
    assert (got[:, 1] >= 0.5).all() and (got[2:, 3] > 0.25).all()
    # one basic column out, one nonbasic column in: the basis is no longer optimal for (x, y)
    for k in (2, 3, 4):
        s = slice(c["ptr_n"][k], c["ptr_n"][k + 1])
        mask = st["labels"].copy()
        out_j = s.start + int(np.flatnonzero(mask[s] != 0)[0])
        in_j = s.start + int(np.flatnonzero(mask[s] == 0)[0])
        mask[out_j], mask[in_j] = 0.0, 1.0
        sw = b.certificate(x, _dev(c["ystar"]), _dev(mask)).cpu().numpy()
        assert sw[k, 3] < 0.0 or sw[k, 4] > 0.0, f"instance {k}: the swapped basis still certifies"
        assert sw[k, 5] == c["inst_m"][k]
        _same(np.delete(sw, k, 0), np.delete(got, k, 0), "the other instances' certificates")


@gpu
def test_signed_cap_after_normalize(LPBatch, case):
    """xstar x 8 puts rows beyond the cap of 5, rows with negative b_i among them (their rows flip), and leaves others
    below it.  After normalize(): labels unchanged, and (xstar, t_k ystar_i / s_i) certify the stored batch (_certifies)."""
    from mllp_amd.planted import _transform_duals
    c = case
    xs = c["xstar"] * np.float32(8.0)
    b = _plant(_build(LPBatch, c), c, xs)
    labels, b_before = b.labels.clone(), b.x2.cpu().numpy()
    s, t = b.normalize(5.0)
    torch.cuda.synchronize()
    sc, x2 = s.cpu().numpy(), b.x2.cpu().numpy()
    capped = np.abs(x2 - 5.0) < 1e-5
    print(f"{capped.sum()} of {c['M']} rows capped, {(capped & (b_before < 0)).sum()} of them flipped")
    assert capped.sum() > 10 and (capped & (b_before < 0)).sum() > 0 and (sc[capped & (b_before < 0)] < 0).all()
    assert (~capped).sum() > 10 and (x2 < 5.0 + 1e-5).all()
    _same(b.labels.cpu().numpy(), labels.cpu().numpy(), "labels after normalize")
    _certifies(b, _dev(xs) * b.labels, _transform_duals(b, _dev(c["ystar"]), s, t), "certificate of the normalized batch")


def _params(seed=5):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(_lib.NUM_PARAMS, generator=g) * 0.2).to("cuda")


@gpu
@pytest.mark.parametrize("path", [1, 2])
def test_every_copy_is_refreshed(LPBatch, case, path):
    """loss_step after planting (inputs bound and copies made BEFORE it) is bit for bit that of a fresh batch built from the
    exported values, x1, x2 and labels."""
    c = case
    params = _params()
    b = _build(LPBatch, c, x1=torch.zeros(c["N"], device="cuda"), x2=torch.zeros(c["M"], device="cuda"),
               labels=torch.zeros(c["N"], device="cuda"))
    b.set_path(path)
    stale = [t.clone() for t in b.loss_step(params)]
    _plant(b, c)
    got = [t.clone() for t in b.loss_step(params)]
    st = _state(b)
    fresh = _build(LPBatch, c, values=st["values"], x1=b.x1.clone(), x2=b.x2.clone(), labels=b.labels.clone())
    fresh.set_path(path)
    want = fresh.loss_step(params)
    assert not torch.equal(got[1], stale[1])
    for a, w, what in zip(got, want, ("loss", "logits", "gradients")):
        assert torch.isfinite(a).all()
        _same(a.cpu().numpy(), w.cpu().numpy(), f"{what} on path {path}")
    for k in range(7):
        _same(b.export(k), fresh.export(k), f"export({k})")


@gpu
def test_determinism_and_batch_independence(LPBatch, planted, case):
    """Two runs are bitwise equal; the big instance alone equals itself inside the batch (values, x1, x2, labels and its
    certificate)."""
    c = case
    b, st = planted
    again = _state(_plant(_build(LPBatch, c), c))
    for k in st:
        _same(again[k], st[k], f"{k} of a second run")
    one = po.ragged_case(which=[4])
    r, s, e = _slices(c, 4)
    for k, sl in (("val", e), ("xstar", s), ("ystar", r), ("slack", s)):
        _same(one[k], c[k][sl], f"the case's {k}")
    b1 = _plant(_build(LPBatch, one), one)
    alone = _state(b1)
    for k, sl in (("values", e), ("x1", s), ("x2", r), ("labels", s)):
        _same(alone[k], st[k][sl], f"{k} of the big instance alone")
    cert = b.certificate(_dev(c["xstar"] * st["labels"]), _dev(c["ystar"])).cpu().numpy()
    cert1 = b1.certificate(_dev(one["xstar"] * alone["labels"]), _dev(one["ystar"])).cpu().numpy()
    _same(cert1[0], cert[4], "certificate of the big instance alone")
    _same(b.certificate(_dev(c["xstar"] * st["labels"]), _dev(c["ystar"])).cpu().numpy(), cert, "a second certificate")


@gpu
def test_bad_pivots_are_refused_and_nothing_is_written(LPBatch, case):
    c = case
    b = _build(LPBatch, c)
    before = _state(b)
    r4 = int(c["ptr_m"][4])
    dup = c["pivot"].copy()
    dup[r4 + 1] = dup[r4]                                # (also absent from row r4 + 1, or present: either way claimed twice)
    row = c["idx"][c["ptr"][r4]:c["ptr"][r4 + 1]]
    absent = c["pivot"].copy()
    taken = set(c["pivot"].tolist()) | set(row.tolist())
    absent[r4] = next(j for j in range(int(c["ptr_n"][4]), int(c["ptr_n"][5])) if j not in taken)
    outside = c["pivot"].copy()
    outside[0] = c["N"] + 7
    for piv, word in ((dup, "two rows"), (absent, "absent"), (outside, "outside")):
        with pytest.raises(_lib.MllpError, match=word):
            b.plant_basis(_dev(piv, torch.int32), _dev(c["xstar"]), _dev(c["ystar"]), _dev(c["slack"]))
        after = _state(b)
        for k in before:
            _same(after[k], before[k], f"{k} after the refusal ({word})")
    assert np.isnan(before["x1"]).all() and np.isnan(before["x2"]).all() and np.isnan(before["labels"]).all()
    with pytest.raises(_lib.MllpError, match="dominance"):
        b.plant_basis(_dev(c["pivot"], torch.int32), _dev(c["xstar"]), _dev(c["ystar"]), _dev(c["slack"]), dominance=1.0)
    assert b.enable_tiled(False, variant=1, builder="torch") is not None
    with pytest.raises(_lib.MllpError, match="mllp_graph_build_tiled"):
        _plant(b, c)
    b.disable_tiled(False, 1)
    after = _state(b)
    for k in before:
        _same(after[k], before[k], f"{k} after the refusal of a caller-owned tiled copy")
    _plant(b, c)                                         # ... and the same batch still plants
    assert np.isfinite(b.x1.cpu().numpy()).all()


@gpu
def test_memory_contract(LPBatch, planted, case):
    """Guard bands around every caller buffer stay intact, inputs are not written, and outputs / scratch poisoned with
    zeros, NaN or the largest float give the same bits -- both calls, through the C ABI."""
    from guarded import PATTERNS, Guarded, same_bits
    L = _lib.lib()
    c = case
    _, st = planted
    stream = _lib.current_stream()
    runs = {}
    for name, fill in PATTERNS.items():
        b = _build(LPBatch, c)
        ins = [Guarded(c["M"], torch.int32, "cuda", data=c["pivot"], name="pivot", shift=4),
               Guarded(c["N"], device="cuda", data=c["xstar"], name="xstar", shift=4),
               Guarded(c["M"], device="cuda", data=c["ystar"], name="ystar", shift=8),
               Guarded(c["N"], device="cuda", data=c["slack"], name="slack", shift=12)]
        outs = [Guarded(n, device="cuda", fill=fill, name=what, shift=4) for n, what in
                ((c["N"], "x1"), (c["M"], "x2"), (c["N"], "labels"))]
        _lib.check(L.mllp_graph_plant_basis(b._h, *[g.ptr for g in ins], po.DOMINANCE, po.FLOOR, *[g.ptr for g in outs], stream))
        torch.cuda.synchronize()
        for g in ins + outs:
            g.check()
        n = ctypes.c_int64()
        _lib.check(L.mllp_lp_certificate_scratch_bytes(b._h, ctypes.byref(n)))
        assert n.value == 4 * (c["M"] + c["N"])
        cin = [Guarded(c["N"], device="cuda", data=outs[0].view, name="c", shift=4),
               Guarded(c["M"], device="cuda", data=outs[1].view, name="b", shift=4),
               Guarded(c["N"], device="cuda", data=c["xstar"] * st["labels"], name="x", shift=4),
               Guarded(c["M"], device="cuda", data=c["ystar"], name="y", shift=4),
               Guarded(c["N"], device="cuda", data=outs[2].view, name="basis", shift=4)]
        cert = Guarded(5 * 6, device="cuda", fill=fill, name="cert", shift=4)
        scratch = Guarded(n.value // 4, device="cuda", fill=fill, name="scratch", shift=4)
        _lib.check(L.mllp_lp_certificate(b._h, *[g.ptr for g in cin], cert.ptr, scratch.ptr, stream))
        torch.cuda.synchronize()
        for g in cin + [cert, scratch]:
            g.check()
        runs[name] = dict(x1=outs[0].bits(), x2=outs[1].bits(), labels=outs[2].bits(), cert=cert.bits(),
                          values=b.export(2).view(np.int32), csc=b.export(5).view(np.int32))
    for name in runs:
        same_bits(runs[name], runs["zero"], f"outputs under {name} poison against zero poison")
    _same(runs["nan"]["x1"].view(np.float32), st["x1"], "x1 against the shared planted batch")
    _same(runs["nan"]["values"].view(np.float32), st["values"], "values against the shared planted batch")


@gpu
def test_planted_batch_generator_certifies(LPBatch):
    """mllp_amd.planted.planted_batch on the device, plain and normalized: labels are m per instance, the returned points
    certify, instance i is the same alone and inside the batch."""
    from mllp_amd.planted import planted_batch
    for normalize in (False, True):
        b, xstar, ystar = planted_batch(6, 20, 50, 4.0, 3, normalize=normalize)
        cert = _certifies(b, xstar * b.labels, ystar, f"planted_batch(normalize={normalize})")
        assert list(cert[:, 5]) == [20] * 6 and (cert[:, 1] >= 0.5).all()
    b, _, _ = planted_batch(6, 20, 50, 4.0, 3)
    one, _, _ = planted_batch(1, 20, 50, 4.0, 3 + 4)
    e0, e1 = int(b.export(0)[4 * 20]), int(b.export(0)[5 * 20])
    _same(one.export(2), b.export(2)[e0:e1], "values of instance 4 alone")
    _same(one.x1.cpu().numpy(), b.x1[200:250].cpu().numpy(), "x1 of instance 4 alone")
    _same(one.x2.cpu().numpy(), b.x2[80:100].cpu().numpy(), "x2 of instance 4 alone")


@gpu
def test_planted_from_real_patterns(LPBatch):
    from mllp_amd.planted import planted_from_instances
    insts = load_packed(SUBSET5)
    b, xstar, ystar = planted_from_instances(insts, seed=2)
    cert = _certifies(b, xstar * b.labels, ystar, "planted on the golden patterns")
    assert list(cert[:, 5]) == [i.m for i in insts] and (cert[:, 1] >= 0.5).all()
    holed = LPInstance("holed", np.array([0, 2, 2, 3]), np.array([0, 1, 2], np.int32), np.ones(3), np.zeros(3), np.zeros(3),
                       np.zeros(3, np.int32))
    with pytest.raises(ValueError, match="holed"):
        planted_from_instances(insts[:1] + [holed])
    b2, _, _ = planted_from_instances(insts[:1] + [holed], on_deficient="skip")
    assert b2.names == [insts[0].name]


@gpu
def test_driver_with_planted_data(tmp_path, monkeypatch):
    from mllp_amd import experiment
    cfg = ("train_data_type: 'planted'\ntrain_lr: 1.e-3\ntrain_iter: 2\nmethods:\n  - 'gs-topk'\nbatch_size: 3\nholdout: 0.25\n"
           "planted: {instances: 8, m: 20, n: 50, row_nnz: 4, seed: 5}\n")
    (tmp_path / "cfg.yaml").write_text(cfg)
    monkeypatch.chdir(tmp_path)
    assert experiment.main(["--cfg", str(tmp_path / "cfg.yaml")]) == 0
    assert (tmp_path / "linear_program_planted_gs-topk.pt").exists()
    log = json.load(open(tmp_path / "train_log.json"))
    assert set(log) == {"obj", "val_obj"} | {f"planted{5 + i}" for i in range(8)}
    assert len(log["val_obj"]) == 2 and all(math.isfinite(v) and v > 0.0 for v in log["val_obj"] + log["obj"])
    (tmp_path / "angle.yaml").write_text(cfg.replace("gs-topk", "angleNet"))
    with pytest.raises(ValueError, match="planted"):
        experiment.main(["--cfg", str(tmp_path / "angle.yaml")])


@gpu
def test_a_planted_batch_can_be_learned(LPBatch):
    """30 full-batch Adam steps on 16 planted instances: the loss ends below the first step's."""
    from mllp_amd.model import GNNModel, set_seed
    from mllp_amd.planted import planted_batch
    from mllp_amd.trainer import LPTrainer
    set_seed()
    b, _, _ = planted_batch(16, 20, 50, 4.0, 9, normalize=True)
    tr = LPTrainer(GNNModel().to("cuda").flat_parameters().detach(), lr=1e-2, use_hip_graph=False)
    losses = [float(tr.step(b)[0][0]) for _ in range(30)]
    print("losses:", losses[0], losses[-1])
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0]
