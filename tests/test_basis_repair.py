"""Repair and solve a predicted basis on the device (mllp_basis_repair; LPBatch.ranking / repair_basis / solve_basis / solved;
DESIGN.md 4.13) against the fp64 oracle of tests/basis_oracle.py.  GPU tests.

THE GAP CONDITION.  Every test first asserts, from the oracle alone, that every fp64 ratio r / amax met on the oracle's walk
lies outside [tol / 64, 64 tol]: the device's fp32 ratios then fall on the same side of tol, so accepted sets compare exactly.

THE ERROR BAR of x and y.  u = m 2^-24 cond_inf(B) ||.||_inf (cond and the norm from the oracle's dense fp64 solve).  The
largest error measured over the planted cases of this file (the ragged batch and both sides of the LDS threshold) is
MEASURED_UNITS; the bar is 4 x that (X_BAR), the margin for other seeds.  The figures are in DESIGN.md 4.13.

THE RESIDUAL BOUNDS of the certificate of a repaired solution follow from that bar: |Ax - b|_i <= ||A||_inf X_BAR u_x +
the evaluation's own bound (planted_oracle.row_bound), |c - A'y|_j <= ||A||_1 X_BAR u_y + that bound.
"""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import basis_oracle as bo
import planted_oracle as po
from guarded import PATTERNS, Guarded, same_bits
from mllp_amd import _lib

pytestmark = pytest.mark.gpu
EINVAL = -1
TOL = 2.0 ** -12
MEASURED_UNITS = 0.1841     # instance 2 (5 x 12) of the ragged batch, y
X_BAR = 4 * MEASURED_UNITS
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LDS_MAX = int(re.search(r"BASIS_LDS_MAX_M\s*=\s*(\d+)", open(os.path.join(ROOT, "mllp_amd", "csrc", "internal.h")).read()).group(1))


# ---------------------------------------------------------------------------------------------------
# cases (numpy; no GPU)
# ---------------------------------------------------------------------------------------------------
def planted_shapes(shapes, seed):
    """planted_oracle.ragged_case for other shapes (no long rows): the same dict"""
    parts, numbers = [], []
    for k, (m, n) in enumerate(shapes):
        parts.append(po._instance(m, n, 4.0, seed + k))
        rng = np.random.default_rng(1000 + seed + k)
        numbers.append(((rng.random(n) + 0.5).astype(np.float32), (rng.random(m) * 2 - 1).astype(np.float32),
                        (rng.random(n) + 0.5).astype(np.float32)))
    inst_m, inst_n = [s[0] for s in shapes], [s[1] for s in shapes]
    ptr_m, ptr_n = np.concatenate([[0], np.cumsum(inst_m)]), np.concatenate([[0], np.cumsum(inst_n)])
    nnz_off = np.concatenate([[0], np.cumsum([len(p[1]) for p in parts])])
    ptr = np.concatenate([[0]] + [p[0][1:] + nnz_off[i] for i, p in enumerate(parts)]).astype(np.int32)
    idx = np.concatenate([p[1] + ptr_n[i] for i, p in enumerate(parts)]).astype(np.int32)
    val = np.concatenate([p[2] for p in parts])
    pivot = np.concatenate([p[3] + ptr_n[i] for i, p in enumerate(parts)]).astype(np.int32)
    xstar, ystar, slack = (np.concatenate([t[j] for t in numbers]) for j in range(3))
    return dict(inst_m=inst_m, inst_n=inst_n, ptr_m=ptr_m, ptr_n=ptr_n, nnz_off=nnz_off, ptr=ptr, idx=idx, val=val, pivot=pivot,
                xstar=xstar, ystar=ystar, slack=slack, M=int(ptr_m[-1]), N=int(ptr_n[-1]))


def dense_case(mats, seed=0):
    """a batch from dense matrices (zeros are absent entries): CSR in global ids, integer-valued c and b"""
    rng = np.random.default_rng(seed)
    inst_m, inst_n = [a.shape[0] for a in mats], [a.shape[1] for a in mats]
    ptr_m, ptr_n = np.concatenate([[0], np.cumsum(inst_m)]), np.concatenate([[0], np.cumsum(inst_n)])
    ptr, idx, val = [0], [], []
    for k, a in enumerate(mats):
        for r in range(a.shape[0]):
            cols = np.flatnonzero(a[r])
            idx += list(cols + ptr_n[k])
            val += list(a[r, cols])
            ptr.append(len(idx))
    M, N = int(ptr_m[-1]), int(ptr_n[-1])
    return dict(inst_m=inst_m, inst_n=inst_n, ptr_m=ptr_m, ptr_n=ptr_n, ptr=np.array(ptr, np.int32), idx=np.array(idx, np.int32),
                val=np.array(val, np.float32), M=M, N=N, mats=[np.asarray(a, np.float64) for a in mats],
                c=rng.integers(-4, 5, N).astype(np.float32), b=rng.integers(-4, 5, M).astype(np.float32))


def int_matrix(m, n, density, seed):
    """small integers, about `density` of them nonzero, the last m columns the identity (full row rank)"""
    rng = np.random.default_rng(seed)
    a = rng.integers(-3, 4, (m, n)) * (rng.random((m, n)) < density)
    a[:, n - m:] = np.eye(m, dtype=a.dtype)
    return a.astype(np.float64)


def inject(a):
    """columns 0, 1, 2 of `a` become: zeros, a copy of column 3, 2 x column 3 - column 4 (exact in fp32: small integers).
    Ranked first, the zero column is rejected, the copy and the combination are accepted, and columns 3 and 4 -- the
    originals -- are then dependent on them."""
    a = a.copy()
    a[:, 3] = np.where(a[:, 3] == 0, 1, a[:, 3])        # (dense: never a zero column, and not a multiple of column 4)
    a[0, 4], a[1, 4] = 1, -2
    a[:, 0] = 0
    a[:, 1] = a[:, 3]
    a[:, 2] = 2 * a[:, 3] - a[:, 4]
    return a


def repair_mats():
    return [inject(int_matrix(5, 12, 0.6, 3)), inject(int_matrix(40, 100, 0.15, 5))]


def deficient_mats():
    twin = int_matrix(4, 8, 0.7, 11)
    twin[:, 4:] = np.diag([1, 2, 3, 4])
    twin[3] = twin[1]                                   # two identical rows: rank 3
    return [int_matrix(3, 6, 0.7, 12), twin, np.zeros((3, 5)), np.zeros((0, 4)), int_matrix(6, 10, 0.6, 13),
            int_matrix(3, 7, 0.7, 14), int_matrix(4, 9, 0.7, 15), int_matrix(2, 5, 0.8, 16)]


def natural_order(c, lists=None):
    """[N] int32: per instance the given local list (padded with -1), default 0 .. n - 1"""
    out = np.full(c["N"], -1, np.int32)
    for k, n in enumerate(c["inst_n"]):
        lst = list(range(n)) if lists is None or lists[k] is None else list(lists[k])
        out[c["ptr_n"][k]:c["ptr_n"][k] + len(lst)] = lst
    return out


def local_lists(c, order):
    return [order[c["ptr_n"][k]:c["ptr_n"][k + 1]] for k in range(len(c["inst_n"]))]


def oracle_walks(mats, c, order, tol=TOL, check_gap=True):
    walks = [bo.walk(a, lst, tol) for a, lst in zip(mats, local_lists(c, order))]
    if check_gap:
        for k, w in enumerate(walks):
            assert bo.gap_ok(w["ratios"], tol), f"instance {k}: a ratio of the oracle's walk is inside [tol / 64, 64 tol]: {w['ratios']}"
    return walks


# ---------------------------------------------------------------------------------------------------
# device helpers
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def LPBatch():
    _lib.lib()
    assert torch.cuda.is_available()
    from mllp_amd.graph import LPBatch as cls
    assert hasattr(cls, "repair_basis")
    return cls


def _dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda")


def _poison(n):
    return torch.full((n,), float("nan"), device="cuda")


def _build(LPBatch, c, x1=None, x2=None, labels=None):
    return LPBatch.from_device_csr(c["inst_m"], c["inst_n"], _dev(c["ptr"], torch.int32), _dev(c["idx"], torch.int32), _dev(c["val"]),
                                   _poison(c["N"]) if x1 is None else x1, _poison(c["M"]) if x2 is None else x2,
                                   _poison(c["N"]) if labels is None else labels)


def _planted(LPBatch, c):
    """the case planted on the device; returns (batch, per-instance dense fp64 matrices of what it stores, state)"""
    b = _build(LPBatch, c)
    b.plant_basis(_dev(c["pivot"], torch.int32), _dev(c["xstar"]), _dev(c["ystar"]), _dev(c["slack"]), po.DOMINANCE, po.FLOOR)
    torch.cuda.synchronize()
    st = dict(values=b.export(2), x1=b.x1.cpu().numpy(), x2=b.x2.cpu().numpy(), labels=b.labels.cpu().numpy())
    mats = []
    for k in range(len(c["inst_m"])):
        r0, r1 = c["ptr_m"][k], c["ptr_m"][k + 1]
        e = slice(c["nnz_off"][k], c["nnz_off"][k + 1])
        ptr = c["ptr"][r0:r1 + 1].astype(np.int64)
        mats.append(po.dense(ptr - ptr[0], c["idx"][e] - c["ptr_n"][k], st["values"][e], r1 - r0, c["inst_n"][k]))
    return b, mats, st


def _labels_first(c, labels):
    out = np.zeros(c["N"], np.int32)
    for k in range(len(c["inst_n"])):
        s = slice(c["ptr_n"][k], c["ptr_n"][k + 1])
        out[s] = np.concatenate([np.flatnonzero(labels[s] != 0), np.flatnonzero(labels[s] == 0)])
    return out


def _host(rep):
    torch.cuda.synchronize()
    return {k: None if getattr(rep, k) is None else getattr(rep, k).cpu().numpy()
            for k in ("basis", "col_of_row", "x", "y", "status", "quality")}


def _bits(h):
    return {k: np.ascontiguousarray(v).view(np.int32).reshape(-1).copy() for k, v in h.items() if v is not None}


def _inst(c, h, k):
    """instance k's part of every output"""
    s, r = slice(c["ptr_n"][k], c["ptr_n"][k + 1]), slice(c["ptr_m"][k], c["ptr_m"][k + 1])
    part = dict(basis=s, x=s, col_of_row=r, y=r, status=slice(k, k + 1), quality=slice(k, k + 1))
    return {name: h[name][sl] for name, sl in part.items() if h[name] is not None}


def _check_planted(b, c, mats, st, h, walks, what):
    """the assertions of a planted batch repaired with the labels first; returns the largest x / y error in units of u"""
    worst = 0.0
    feas, opt = [], []
    for k, (m, n) in enumerate(zip(c["inst_m"], c["inst_n"])):
        s, r = slice(c["ptr_n"][k], c["ptr_n"][k + 1]), slice(c["ptr_m"][k], c["ptr_m"][k + 1])
        assert walks[k]["status"] == [m, m, 0, 0]
        assert list(h["status"][k]) == [m, m, 0, 0], f"{what}: instance {k} status {h['status'][k]}"
        assert np.array_equal(h["basis"][s], st["labels"][s]) and np.array_equal(walks[k]["basis"], st["labels"][s])
        assert sorted(h["col_of_row"][r]) == sorted(np.flatnonzero(st["labels"][s]))
        assert h["quality"][k, 0] > 64 * TOL and h["quality"][k, 1] == 0.0
        xo, yo, cond = bo.basic_solution(mats[k], st["x2"][r], st["x1"][s], walks[k]["col_of_row"])
        ux, uy = bo.error_units(h["x"][s], xo, m, cond), bo.error_units(h["y"][r], yo, m, cond)
        print(f"{what}: instance {k} ({m} x {n}): cond_inf {cond:.1f}, x error {ux:.4f} u, y error {uy:.4f} u")
        worst = max(worst, ux, uy)
        assert ux <= X_BAR and uy <= X_BAR, f"{what}: instance {k}: {ux:.4f} / {uy:.4f} units against the bar {X_BAR}"
        unit = max(m, 1) * bo.U * cond
        feas.append(np.abs(mats[k]).sum(1).max(initial=0.0) * X_BAR * unit * np.abs(xo).max(initial=0.0))
        opt.append(np.abs(mats[k]).sum(0).max(initial=0.0) * X_BAR * unit * np.abs(yo).max(initial=0.0))
    # the certificate: the device's figures against the oracle's on the same (x, y, basis), and the residual bounds
    rep_x, rep_y, rep_basis = _dev(h["x"]), _dev(h["y"]), _dev(h["basis"])
    got = b.certificate(rep_x, rep_y, rep_basis).cpu().numpy()
    want, bound = po.certificate(c["ptr"], c["idx"], st["values"], st["x1"], st["x2"], h["x"], h["y"], h["basis"], c["ptr_m"], c["ptr_n"])
    fin = np.isfinite(want)
    assert np.array_equal(np.isinf(got), ~fin)
    assert (np.abs(got[fin].astype(np.float64) - want[fin]) <= bound[fin]).all(), f"{what}: certificate against the oracle's"
    assert (got[:, 0] <= np.array(feas) + bound[:, 0]).all() and (got[:, 4] <= np.array(opt) + bound[:, 4]).all(), what
    assert (got[:, 1] > 0).all() and (got[:, 2] == 0).all() and (got[:, 3] > 0).all() and list(got[:, 5]) == list(c["inst_m"]), what
    return worst, float((np.array(feas) + bound[:, 0]).max()), float((np.array(opt) + bound[:, 4]).max())


# ---------------------------------------------------------------------------------------------------
# planted batches: the ragged case, both sides of the LDS threshold
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ragged(LPBatch):
    c = po.ragged_case()
    b, mats, st = _planted(LPBatch, c)
    order = _labels_first(c, st["labels"])
    return dict(c=c, b=b, mats=mats, st=st, order=order, walks=oracle_walks(mats, c, order))


@pytest.fixture(scope="module")
def threshold(LPBatch):
    c = planted_shapes([(5, 12), (LDS_MAX, 2 * LDS_MAX + 16), (LDS_MAX + 1, 2 * LDS_MAX + 16)], 40)
    b, mats, st = _planted(LPBatch, c)
    order = _labels_first(c, st["labels"])
    return dict(c=c, b=b, mats=mats, st=st, order=order, walks=oracle_walks(mats, c, order))


def test_ragged_planted_batch(ragged):
    """1 x 1, 3 x 3 all basic, 5 x 12, 40 x 100 and 1200 x 2400, labels first: rank m, basis == labels, nothing rejected;
    x and y within the bar of the dense fp64 solve; the certificate holds; `solved` reports every instance optimal."""
    g = ragged
    rep = g["b"].repair_basis(order=_dev(g["order"], torch.int32), tol=TOL)
    h = _host(rep)
    worst, feas_tol, opt_tol = _check_planted(g["b"], g["c"], g["mats"], g["st"], h, g["walks"], "ragged")
    print(f"ragged: largest error {worst:.4f} units of u (bar {X_BAR})")
    got = g["b"].solved(rep, feas_tol, opt_tol)
    for key in ("usable", "primal_feasible", "optimal"):
        assert got[key].dtype == torch.bool and bool(got[key].all()), key
    assert not bool(got["skipped"].any())


def test_both_sides_of_the_lds_threshold(LPBatch, threshold):
    """m = threshold (T in LDS) and threshold + 1 (T in scratch) with the same assertions; the threshold-sized instance alone
    gives the bits it gives inside the batch."""
    g = threshold
    c = g["c"]
    assert c["inst_m"][1] == LDS_MAX and c["inst_m"][2] == LDS_MAX + 1
    n = ctypes.c_int64(-1)
    _lib.check(_lib.lib().mllp_basis_repair_scratch_bytes(g["b"]._h, 1 << 40, ctypes.byref(n)))
    assert n.value == 4 * (LDS_MAX + 1) ** 2        # m^2 words, only for the instance above the threshold
    h = _host(g["b"].repair_basis(order=_dev(g["order"], torch.int32), tol=TOL))
    worst, _, _ = _check_planted(g["b"], c, g["mats"], g["st"], h, g["walks"], "threshold")
    print(f"threshold: largest error {worst:.4f} units of u (bar {X_BAR})")
    one = planted_shapes([(LDS_MAX, 2 * LDS_MAX + 16)], 41)               # (seed + 1: instance 1 of the batch)
    b1, _, st1 = _planted(LPBatch, one)
    s = slice(c["ptr_n"][1], c["ptr_n"][2])
    assert np.array_equal(st1["values"], g["st"]["values"][c["nnz_off"][1]:c["nnz_off"][2]]) and np.array_equal(st1["x1"], g["st"]["x1"][s])
    h1 = _host(b1.repair_basis(order=_dev(g["order"][s], torch.int32), tol=TOL))
    same_bits(_bits(h1), _bits(_inst(c, h, 1)), "the threshold-sized instance alone against inside the batch")


# ---------------------------------------------------------------------------------------------------
# repair
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def repair(LPBatch):
    c = dense_case(repair_mats(), 1)
    order = natural_order(c)                    # the injected columns 0, 1, 2 first
    walks = oracle_walks(c["mats"], c, order)
    return dict(c=c, b=_build(LPBatch, c, _dev(c["c"]), _dev(c["b"])), order=order, walks=walks)


def _check_against_walks(c, h, walks, what, x1=None, x2=None):
    for k, w in enumerate(walks):
        s, r = slice(c["ptr_n"][k], c["ptr_n"][k + 1]), slice(c["ptr_m"][k], c["ptr_m"][k + 1])
        m = c["inst_m"][k]
        assert list(h["status"][k]) == w["status"], f"{what}: instance {k}: status {h['status'][k]}, the oracle's {w['status']}"
        assert np.array_equal(h["basis"][s], w["basis"]), f"{what}: instance {k}: another accepted set"
        got_cols = sorted(j for j in h["col_of_row"][r] if j >= 0)
        assert got_cols == sorted(w["accepted"]) and (h["col_of_row"][r] >= 0).sum() == w["status"][0]
        q = h["quality"][k]
        assert (q[0] > TOL if w["accepted_flags"].any() else q[0] == np.inf), f"{what}: instance {k}: quality {q}"
        assert (0 <= q[1] < TOL) if (~w["accepted_flags"]).any() else q[1] == 0.0, f"{what}: instance {k}: quality {q}"
        if w["status"][3] == 0 and m:
            xo, yo, cond = bo.basic_solution(c["mats"][k], (c["b"] if x2 is None else x2)[r], (c["c"] if x1 is None else x1)[s],
                                             w["col_of_row"])
            ux, uy = bo.error_units(h["x"][s], xo, m, cond), bo.error_units(h["y"][r], yo, m, cond)
            print(f"{what}: instance {k}: cond_inf {cond:.1f}, x error {ux:.4f} u, y error {uy:.4f} u")
            assert ux <= X_BAR and uy <= X_BAR
        else:
            assert not h["x"][s].any() and not h["y"][r].any(), f"{what}: instance {k}: x and y are not zeros"


def test_repair_of_injected_columns(repair):
    """A zero column, an exact copy of a column and a small-integer combination of two, ranked first: the accepted set is the
    oracle's (on 5 x 12 also the brute force's), `rejected` counts them, `quality` lies on the right sides of tol."""
    g = repair
    c = g["c"]
    for k, w in enumerate(g["walks"]):
        assert w["status"][0] == c["inst_m"][k] and w["status"][3] == 0
        assert w["accepted"][:2] == [1, 2] and not {0, 3, 4} & set(w["accepted"]) and w["status"][2] == 3
    best = bo.brute_force(c["mats"][0], local_lists(c, g["order"])[0])
    assert sorted(best) == sorted(g["walks"][0]["accepted"])
    h = _host(g["b"].repair_basis(order=_dev(g["order"], torch.int32), tol=TOL))
    _check_against_walks(c, h, g["walks"], "repair")
    assert sorted(np.flatnonzero(h["basis"][:12])) == sorted(best)


def test_solve_basis(ragged, repair):
    """solve_basis(labels) is repair_basis(labels first), bit for bit; a basis with a dependent column swapped in: code 1."""
    g = ragged
    a = _host(g["b"].solve_basis(g["b"].labels, tol=TOL))
    b = _host(g["b"].repair_basis(order=_dev(g["order"], torch.int32), tol=TOL))
    same_bits(_bits(a), _bits(b), "solve_basis(labels) against repair_basis(labels first)")
    c = repair["c"]
    mask = np.concatenate([w["basis"] for w in repair["walks"]]).astype(np.float32)
    lists = []
    for k, w in enumerate(repair["walks"]):             # column 2 (= 2 x column 3 - column 4) out, its source 3 in: dependent on column 1
        assert mask[c["ptr_n"][k] + 2] == 1 and mask[c["ptr_n"][k] + 3] == 0
        mask[c["ptr_n"][k] + 2], mask[c["ptr_n"][k] + 3] = 0, 1
        lists.append(list(np.flatnonzero(mask[c["ptr_n"][k]:c["ptr_n"][k + 1]])))
    walks = oracle_walks(c["mats"], c, natural_order(c, lists))
    h = _host(repair["b"].solve_basis(_dev(mask), tol=TOL))
    for k, w in enumerate(walks):
        m = c["inst_m"][k]
        assert w["status"] == [m - 1, m, 1, 1] and list(h["status"][k]) == w["status"]
    _check_against_walks(c, h, walks, "swapped basis")


# ---------------------------------------------------------------------------------------------------
# agreement with predict_basis
# ---------------------------------------------------------------------------------------------------
def _key(z):
    u = np.asarray(z, np.float32).view(np.uint32).astype(np.int64)
    return np.where(u & 0x80000000, (~u) & 0xFFFFFFFF, u | 0x80000000)


def test_agreement_with_predict_basis(threshold):
    """Logits whose top-m set is the planted (nonsingular) basis, in random order, with tied logits inside the set, a tie
    across the selection's edge and +-0.0 outside: `ranking` is the order of the select kernels, and the repaired basis is
    `predict_basis`' mask."""
    g = threshold
    c, b = g["c"], g["b"]
    rng = np.random.default_rng(7)
    z = np.empty(c["N"], np.float32)
    for k in range(len(c["inst_n"])):
        s = slice(c["ptr_n"][k], c["ptr_n"][k + 1])
        lab = g["st"]["labels"][s] != 0
        on, off = np.flatnonzero(lab), np.flatnonzero(~lab)
        zk = np.where(lab, 2.0 + rng.random(lab.size), -1.0 - rng.random(lab.size)).astype(np.float32)
        zk[on[1]] = zk[on[2]] = 2.5                     # a tie inside the selection
        assert on[0] < off[-1]
        zk[on[0]] = zk[off[-1]] = 1.0                   # a tie across its edge: the lower index wins
        zk[off[0]], zk[off[1]], zk[off[2]] = -0.0, 0.0, -0.0
        zk[off[3]] = zk[off[4]] = -1.5
        z[s] = zk
    order = b.ranking(_dev(z)).cpu().numpy()
    assert order.dtype == np.int32
    for k in range(len(c["inst_n"])):
        s = slice(c["ptr_n"][k], c["ptr_n"][k + 1])
        want = np.lexsort((np.arange(s.stop - s.start), -_key(z[s])))
        assert np.array_equal(order[s], want), f"ranking of instance {k}"
        off = np.flatnonzero(g["st"]["labels"][s] == 0)
        pos = {j: p for p, j in enumerate(order[s])}
        assert pos[off[1]] < pos[off[0]] < pos[off[2]]  # +0.0 before both -0.0, those by index
    walks = oracle_walks(g["mats"], c, order)
    for k, w in enumerate(walks):
        assert w["status"] == [c["inst_m"][k], c["inst_m"][k], 0, 0]
    pred = b.predict_basis(_dev(z), want="mask").mask.cpu().numpy()
    h = _host(b.repair_basis(logits=_dev(z), tol=TOL))
    assert np.array_equal(h["basis"], pred.astype(np.float32)) and np.array_equal(pred, g["st"]["labels"].astype(np.uint8))
    assert [list(r) for r in h["status"]] == [w["status"] for w in walks]


# ---------------------------------------------------------------------------------------------------
# rank deficiency, empty instances, skipped instances, bad ids, short lists
# ---------------------------------------------------------------------------------------------------
def test_rank_deficiency_and_edge_instances(LPBatch):
    mats = deficient_mats()
    c = dense_case(mats, 2)
    lists = [None, None, None, None, None, [1, 0, 7, 2, 3, 4, 5], [3, 1, -1, 0, 2, 4, 5, 6, 7], None]
    order = natural_order(c, lists)
    order[c["ptr_n"][6] + 3:c["ptr_n"][7]] = [0, 2, 4, 5, 6, 7]         # (entries behind the first -1 are never read)
    walks = oracle_walks(mats, c, order)
    m_of = c["inst_m"]
    assert walks[1]["status"] == [3, 8, 1, 1]                            # two identical rows: rank m - 1
    assert walks[2]["status"] == [0, 5, 3, 1] and walks[3]["status"] == [0, 0, 0, 0]
    assert walks[5]["status"][3] == 3 and walks[5]["status"][1] == 2     # the id 7 >= n = 7 ends the instance
    assert walks[6]["status"] == [2, 2, 0, 1]                            # the list is cut short by -1
    assert all(walks[k]["status"][3] == 0 for k in (0, 4, 7))
    b = _build(LPBatch, c, _dev(c["c"]), _dev(c["b"]))
    dev_order = _dev(order, torch.int32)
    h = _host(b.repair_basis(order=dev_order, tol=TOL))
    _check_against_walks(c, h, walks, "edge instances")
    assert list(h["status"][5]) == walks[5]["status"]
    # m > max_m: instance 4 (6 rows) is skipped, outputs defaulted; every other instance keeps its bits
    h5 = _host(b.repair_basis(order=dev_order, tol=TOL, max_m=5))
    k = 4
    part = _inst(c, h5, k)
    assert list(part["status"][0]) == [0, 0, 0, 2] and not part["basis"].any() and not part["x"].any() and not part["y"].any()
    assert (part["col_of_row"] == -1).all() and part["quality"][0, 0] == np.inf and part["quality"][0, 1] == 0.0
    for j in range(len(m_of)):
        if j != k:
            same_bits(_bits(_inst(c, h5, j)), _bits(_inst(c, h, j)), f"instance {j} beside a skipped one")
    n = ctypes.c_int64(-1)
    _lib.check(_lib.lib().mllp_basis_repair_scratch_bytes(b._h, 5, ctypes.byref(n)))
    assert n.value == 0
    got = b.solved(b.repair_basis(order=dev_order, tol=TOL, max_m=5), 1e-3, 1e-3)
    assert got["skipped"].cpu().tolist() == [j == k for j in range(len(m_of))]
    assert got["usable"].cpu().tolist() == [w["status"][3] == 0 and j != k for j, w in enumerate(walks)]


# ---------------------------------------------------------------------------------------------------
# optional outputs, reproducibility, graph capture
# ---------------------------------------------------------------------------------------------------
def _abi_call(b, c, order, bufs, tol=TOL, max_m=None, scratch=None, x1=None, x2=None, g_override=False):
    """mllp_basis_repair through the C ABI; bufs: dict name -> c_void_p / tensor / None"""
    p = lambda v: v if isinstance(v, ctypes.c_void_p) else _lib.ptr(v)      # noqa: E731
    L = _lib.lib()
    return L.mllp_basis_repair(None if g_override else b._h, p(b.x1 if x1 is None else x1), p(b.x2 if x2 is None else x2), p(order),
                               tol, max(c["inst_m"]) if max_m is None else max_m,
                               *[p(bufs.get(k)) for k in ("basis", "col_of_row", "x", "y", "status", "quality")], p(scratch),
                               _lib.current_stream())


def test_optional_outputs_and_reproducibility(threshold):
    """Each optional output alone gives the bits of the full call; two runs are bitwise equal; a replay of a captured graph
    equals the eager call."""
    g = threshold
    c, b = g["c"], g["b"]
    order = _dev(g["order"], torch.int32)
    oracle_walks(g["mats"], c, g["order"])
    full = _bits(_host(b.repair_basis(order=order, tol=TOL)))
    same_bits(_bits(_host(b.repair_basis(order=order, tol=TOL))), full, "a second run")
    for want in (("basis",), ("col_of_row",), ("quality",), ("x", "y"), ()):
        got = _bits(_host(b.repair_basis(order=order, tol=TOL, want=want)))
        assert set(got) == set(want) | {"status"}
        same_bits(got, {k: full[k] for k in got}, f"want={want}")
    with pytest.raises(ValueError):
        b.repair_basis(order=order, tol=TOL, want=("x",))
    # graph capture: preallocated buffers, the batch's scratch (made by the calls above)
    bufs = dict(basis=_poison(c["N"]), col_of_row=_poison(c["M"]).view(torch.int32), x=_poison(c["N"]), y=_poison(c["M"]),
                status=_poison(4 * 3).view(torch.int32), quality=_poison(2 * 3))
    scratch = b._repair_scratch[1]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc = _abi_call(b, c, order, bufs, scratch=scratch)
    assert rc == 0
    for _ in range(2):
        for t in bufs.values():
            t.view(torch.int32).fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        same_bits({k: v.cpu().numpy().view(np.int32).reshape(-1) for k, v in bufs.items()}, full, "a replay of the captured call")


# ---------------------------------------------------------------------------------------------------
# memory contract
# ---------------------------------------------------------------------------------------------------
def test_memory_contract(threshold):
    """Guard bands around every caller buffer stay intact, inputs are not written, outputs and scratch poisoned with zeros,
    NaN or the largest float give the same bits (T in LDS and in scratch); refused calls leave the poison untouched."""
    g = threshold
    c, b = g["c"], g["b"]
    oracle_walks(g["mats"], c, g["order"])
    n = ctypes.c_int64()
    max_m = max(c["inst_m"])
    _lib.check(_lib.lib().mllp_basis_repair_scratch_bytes(b._h, max_m, ctypes.byref(n)))
    assert n.value > 0
    ni = len(c["inst_m"])
    runs = {}
    for name, fill in PATTERNS.items():
        ins = dict(x1=Guarded(c["N"], device="cuda", data=g["st"]["x1"], name="x1", shift=4),
                   x2=Guarded(c["M"], device="cuda", data=g["st"]["x2"], name="x2", shift=8),
                   order=Guarded(c["N"], torch.int32, "cuda", data=g["order"], name="order", shift=12))
        outs = dict(basis=Guarded(c["N"], device="cuda", fill=fill, name="basis", shift=4),
                    col_of_row=Guarded(c["M"], torch.int32, "cuda", fill=fill, name="col_of_row", shift=4),
                    x=Guarded(c["N"], device="cuda", fill=fill, name="x", shift=4), y=Guarded(c["M"], device="cuda", fill=fill, name="y", shift=8),
                    status=Guarded(4 * ni, torch.int32, "cuda", fill=fill, name="status", shift=4),
                    quality=Guarded(2 * ni, device="cuda", fill=fill, name="quality", shift=4))
        scratch = Guarded(n.value // 4, device="cuda", fill=fill, name="scratch", shift=4)
        ptrs = {k: v.ptr for k, v in outs.items()}
        # refusals first: the poison stays
        before = {k: v.bits() for k, v in outs.items()}
        before["scratch"] = scratch.bits()
        bad = [dict(g_override=True), dict(order=ctypes.c_void_p(0)), dict(bufs={**ptrs, "status": ctypes.c_void_p(0)}),
               dict(bufs={**ptrs, "x": ctypes.c_void_p(0)}), dict(bufs={**ptrs, "y": ctypes.c_void_p(0)}),
               dict(x1=ctypes.c_void_p(0)), dict(x2=ctypes.c_void_p(0)), dict(scratch=ctypes.c_void_p(0)),
               dict(tol=float("nan")), dict(tol=float("inf")), dict(tol=-1.0), dict(max_m=-1)]
        for kw in bad:
            args = dict(order=ins["order"].ptr, bufs=ptrs, scratch=scratch.ptr, x1=ins["x1"].ptr, x2=ins["x2"].ptr, max_m=max_m)
            args.update(kw)
            assert _abi_call(b, c, args.pop("order"), args.pop("bufs"), **args) == EINVAL, kw
            assert b"mllp_basis_repair" in _lib.lib().mllp_last_error()
        torch.cuda.synchronize()
        after = {k: v.bits() for k, v in outs.items()}
        after["scratch"] = scratch.bits()
        same_bits(after, before, f"buffers after the refused calls ({name} poison)")
        assert _abi_call(b, c, ins["order"].ptr, ptrs, scratch=scratch.ptr, x1=ins["x1"].ptr, x2=ins["x2"].ptr, max_m=max_m) == 0
        torch.cuda.synchronize()
        for v in list(ins.values()) + list(outs.values()) + [scratch]:
            v.check()
        runs[name] = {k: v.bits() for k, v in outs.items()}
    for name in runs:
        same_bits(runs[name], runs["zero"], f"outputs under {name} poison against zero poison")
    same_bits(runs["nan"], _bits(_host(b.repair_basis(order=_dev(g["order"], torch.int32), tol=TOL))), "the C ABI against repair_basis")


# ---------------------------------------------------------------------------------------------------
# driver
# ---------------------------------------------------------------------------------------------------
def test_driver_reports_solved(tmp_path, monkeypatch):
    """8 planted instances, a quarter held out, `report_solved`: the log gains the four counts per epoch.  The ranking
    holds every column and a planted LP has full row rank, so every held-out instance is usable or skipped: those two counts
    sum to the held-out count, and optimal <= feasible <= usable."""
    from mllp_amd import experiment
    cfg = ("train_data_type: 'planted'\ntrain_lr: 1.e-3\ntrain_iter: 2\nmethods:\n  - 'gs-topk'\nbatch_size: 3\nholdout: 0.25\n"
           "planted: {instances: 8, m: 20, n: 50, row_nnz: 4, seed: 5}\n")
    for block, skipped in (("report_solved: {feas_tol: 1.e-3, opt_tol: 1.e-3, max_m: 20}\n", 0),
                           ("report_solved: {feas_tol: 1.e-3, opt_tol: 1.e-3, max_m: 19}\n", 2)):
        (tmp_path / "cfg.yaml").write_text(cfg + block)
        monkeypatch.chdir(tmp_path)
        assert experiment.main(["--cfg", str(tmp_path / "cfg.yaml")]) == 0
        log = json.load(open(tmp_path / "train_log.json"))
        assert set(log) == {"obj", "val_obj", "usable", "feasible", "optimal", "skipped"} | {f"planted{5 + i}" for i in range(8)}
        for e in range(2):
            usable, feasible, optimal, skip = (log[k][e] for k in ("usable", "feasible", "optimal", "skipped"))
            assert skip == skipped and usable + skip == 2 and 0 <= optimal <= feasible <= usable
        assert all(len(log[k]) == 2 for k in ("usable", "feasible", "optimal", "skipped"))
        assert all(math.isfinite(v) for v in log["obj"] + log["val_obj"])
