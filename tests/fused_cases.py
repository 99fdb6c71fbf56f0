"""Inputs and census of tests/test_fused_oracle.py (test infrastructure, no GPU needed).

1. `constants()`: the tier thresholds, the workgroup size and the grid cap of the fused latency-regime path, PARSED from
   host_graph.h / fused_kernels.hip / internal.h, so a moved tier fails the census instead of silently changing what the
   inputs reach.
2. `census()`: a pure-Python restatement of what host_graph.cpp does with a single-instance batch (everything in one
   partition): rows per tier, items and block rows per partition, the pigeonhole bound ceil(items / wavefronts) on the
   longest wavefront list and -- `exact=True` -- the list length of every wavefront from a restatement of the host's
   longest-processing-time assignment (host_build_wave_lists).
3. The instances: a two-sided block diagonal diag(B, C^T) has the row degrees of B among its rows and the row degrees of
   C among its columns, so one constructor controls both orientations.
4. `model_dt()`: the decomposition of oracle/spmm_form.py in a chosen floating-point type (spmm_form computes in fp64
   whatever it is given); the fp32 run against the fp64 run is the yardstick of the tolerances.
5. Inputs that several test modules share: ragged random instances and the ragged batch of the copy compositions, the
   inputs of the one-launch small step, the batches of degree grids with their per-tensor caps.
"""
import math
import os
import re

import numpy as np
import scipy.sparse as sp

from mllp_amd.data import SUBSET5, LPInstance
from oracle import spmm_form as o2
from oracle.pyg_restatement import CONV_CIN, state_dict_spec

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "mllp_amd", "csrc")


# ---------------------------------------------------------------------------------------------------------------------
# 1. constants of the code under test
# ---------------------------------------------------------------------------------------------------------------------
def _src(name, csrc=None):
    with open(os.path.join(csrc or CSRC, name)) as f:
        return f.read()


def _ints(text, pattern, what):
    m = re.search(pattern, text)
    assert m, f"cannot find {what}"
    return [int(v) for v in m.groups()]


def constants(csrc=None):
    h, k, i = _src("host_graph.h", csrc), _src("fused_kernels.hip", csrc), _src("internal.h", csrc)
    three = r"\[3\]\s*=\s*\{\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*\}"
    c = dict(T16=_ints(h, r"constexpr\s+int\s+FUSED_T16" + three, "FUSED_T16"),
             T1=_ints(h, r"constexpr\s+int\s+FUSED_T1" + three, "FUSED_T1"),
             PARTS=_ints(h, r"constexpr\s+int\s+FUSED_PARTS\s*=\s*(\d+)", "FUSED_PARTS")[0],
             FT=_ints(k, r"constexpr\s+int\s+FT\s*=\s*(\d+)", "FT")[0],
             STAT_BLOCKS_MAX=_ints(i, r"constexpr\s+int\s+STAT_BLOCKS_MAX\s*=\s*(\d+)", "STAT_BLOCKS_MAX")[0])
    c["COST_ITEM"], c["COST_STEP"], c["COST_BLOCK_ROW"] = _ints(
        h, r"FUSED_COST_ITEM\s*=\s*(\d+)\s*,\s*FUSED_COST_STEP\s*=\s*(\d+)\s*,\s*FUSED_COST_BLOCK_ROW\s*=\s*(\d+)", "FUSED_COST_*")
    assert c["FT"] % 64 == 0
    c["FW"] = c["FT"] // 64                      # wavefronts per workgroup
    return c


# The three kinds of wavefront lists (fused_graph_build): name -> (1-channel geometry, nonzeros of a base-tier unit per
# step, workgroups per CU).  Units per wavefront: 16 quads / 64 lanes; a group row takes 4 units, a wave row all of them,
# a block row all units of the workgroup.
KINDS = {"16": (False, 4, 1), "src16": (False, 2, 2), "1": (True, 8, 1)}


def step_widths(kind, c=None):
    """nonzeros per step of a row in the base / group / wave / block tier of the kernels that walk lists of `kind`"""
    c = c or constants()
    scalar, e, _ = KINDS[kind]
    units = 64 if scalar else 16
    return dict(base=e, group=4 * e, wave=units * e, block=c["FW"] * units * e)


def grid_per_partition(cus, c=None):
    c = c or constants()
    return max(min(int(cus), c["STAT_BLOCKS_MAX"]) // c["PARTS"], 1)        # fused_grid() / NP


def reduce_loops(csrc=None):
    """The loops of fused_reduce_body over the per-workgroup partials, PARSED from fused_kernels.hip:
    (slices, [(lookahead, stride), ...]) for `b = slice; for (; b + lookahead < nblk; b += stride)` in source order, where
    `slices` is the number of distinct starting values of b (RT >> the shift of `slice = tid >> ..`)."""
    k = _src("fused_kernels.hip", csrc)
    m = re.search(r"void\s+fused_reduce_body\s*\(.*?\n\}\n", k, re.S)
    assert m, "cannot find fused_reduce_body"
    body = m.group(0)
    body = body[body.index("float* sh4"):]                  # behind the fc partials' own branch
    rt = _ints(k, r"constexpr\s+int\s+RT\s*=\s*(\d+)", "RT")[0]
    shift = _ints(body, r"slice\s*=\s*tid\s*>>\s*(\d+)", "slice = tid >> ..")[0]
    assert re.search(r"int\s+b\s*=\s*slice\s*;", body), "cannot find b = slice"
    loops = [(int(la or 0), int(st)) for la, st in
             re.findall(r"for\s*\(\s*;\s*b(?:\s*\+\s*(\d+))?\s*<\s*A\.nblk\s*;\s*b\s*\+=\s*(\d+)\s*\)", body)]
    assert len(loops) == 3, f"fused_reduce_body: expected three loops over the partials, found {loops}"
    return rt >> shift, loops


def reduce_trips(nblk, slices, loops):
    """Trips of every loop of reduce_loops() for nblk partials, per thread: [{trips of the threads} per loop], and the
    partials each starting value visits (they must tile 0 .. nblk - 1)."""
    trips = [set() for _ in loops]
    seen = []
    for b in range(slices):
        for i, (la, st) in enumerate(loops):
            n = 0
            while b + la < nblk:
                seen += list(range(b, b + st, slices))
                b += st
                n += 1
            trips[i].add(n)
    return trips, sorted(seen)


# ---------------------------------------------------------------------------------------------------------------------
# 2. census
# ---------------------------------------------------------------------------------------------------------------------
def degrees(inst):
    """(row degrees, column degrees) of an instance"""
    return np.diff(inst.indptr).astype(np.int64), np.bincount(inst.indices, minlength=inst.n).astype(np.int64)


def tier_counts(deg, T):
    deg = np.asarray(deg)
    return dict(block=int((deg > T[2]).sum()), wave=int(((deg > T[1]) & (deg <= T[2])).sum()),
                group=int(((deg > T[0]) & (deg <= T[1])).sum()), base=int((deg <= T[0]).sum()))


def lpt_lengths(deg, kind, gp, c=None):
    """Items of every wavefront of a partition that holds exactly the rows `deg`: host_build_wave_lists restated (costs
    from the first row of an item, heaviest item first to the wavefront that would finish it first, ties to the lower
    wavefront id, wavefronts charged their workgroup's block rows first)."""
    c = c or constants()
    scalar, e_base, mult = KINDS[kind]
    T = c["T1"] if scalar else c["T16"]
    U = 64 if scalar else 16
    RG = U // 4
    wpg, gpk = c["FW"], gp * mult
    nw = gpk * wpg
    d = np.sort(np.asarray(deg, np.int64))[::-1]
    t = tier_counts(d, T)
    w0, g0, b0 = t["block"], t["block"] + t["wave"], t["block"] + t["wave"] + t["group"]
    first = np.concatenate([d[w0:g0], d[g0:b0:RG], d[b0::U]])
    width = np.concatenate([np.full(t["wave"], U * e_base), np.full(len(d[g0:b0:RG]), 4 * e_base),
                            np.full(len(d[b0::U]), e_base)])
    cost = c["COST_ITEM"] + c["COST_STEP"] * np.maximum(-(-first // width), 1)
    order = np.argsort(-cost, kind="stable")
    w = np.arange(nw)
    slow = 1000 + 95 * ((w % wpg) // 4)
    bi = w // wpg
    n_rows = np.where(t["block"] > bi, (t["block"] - bi + gpk - 1) // gpk, 0)
    load = c["COST_BLOCK_ROW"] * n_rows * slow // 1000
    counts = np.zeros(nw, np.int64)
    add = {}
    for cst in cost[order].tolist():
        a = add.get(cst)
        if a is None:
            a = add[cst] = cst * slow // 1000
        tw = load + a
        k = int(np.argmin(tw))          # the first minimum: ties to the lower wavefront id
        load[k] = tw[k]
        counts[k] += 1
    assert counts.sum() == len(first)
    return counts


def census(inst, cus=256, exact=False, c=None):
    """{orientation: {kind: dict(tiers, items, block_rows, waves, bound, laps[, lengths])}} of the single-instance batch
    [inst]: one partition holds everything, the other seven are empty."""
    c = c or constants()
    gp = grid_per_partition(cus, c)
    out = {}
    for orient, deg in zip(("A", "At"), degrees(inst)):
        out[orient] = {}
        for kind, (scalar, _, mult) in KINDS.items():
            T = c["T1"] if scalar else c["T16"]
            U = 64 if scalar else 16
            t = tier_counts(deg, T)
            items = t["wave"] + -(-t["group"] // (U // 4)) + -(-t["base"] // U)
            waves = gp * mult * c["FW"]
            e = dict(tiers=t, items=items, block_rows=t["block"], waves=waves, bound=-(-items // waves),
                     laps=-(-t["block"] // (gp * mult)))
            if exact:
                e["lengths"] = lpt_lengths(deg, kind, gp, c)
            out[orient][kind] = e
    return out


def census_lines(name, cen):
    lines = []
    for orient, kinds in cen.items():
        for kind, e in kinds.items():
            t = e["tiers"]
            s = (f"[census {name}] {orient:2s} {kind:5s} block {t['block']:5d} wave {t['wave']:6d} group {t['group']:6d} "
                 f"base {t['base']:7d} | items {e['items']:6d} / {e['waves']} wavefronts: longest list >= {e['bound']}")
            if "lengths" in e:
                s += f", exactly {int(e['lengths'].min())}..{int(e['lengths'].max())}"
            lines.append(s + f" | block rows per partition {e['block_rows']} ({e['laps']} laps)")
    return lines


# ---------------------------------------------------------------------------------------------------------------------
# 3. instances
# ---------------------------------------------------------------------------------------------------------------------
def block_of(degs, width, rng, values="normal", amp=1.0):
    """CSR block with the given row degrees: row i holds `degs[i]` consecutive columns (cyclic) from a random start, so
    the column degrees stay near sum(degs) / width.  values: "normal", "up" (ascending along every row) or "updown"
    (even rows ascending, odd rows descending)."""
    assert max(degs, default=0) <= width
    indptr = np.concatenate([[0], np.cumsum(degs)]).astype(np.int64)
    idx, val = [], []
    for i, d in enumerate(degs):
        cols = np.sort((int(rng.integers(width)) + np.arange(d)) % width)
        idx.append(cols)
        if values == "normal":
            v = rng.standard_normal(d)
            v[v == 0] = 1.0
        else:
            v = np.linspace(-amp, amp, d) if d > 1 else np.ones(d)
            if values == "updown" and i % 2:
                v = v[::-1]
        val.append(v)
    idx = np.concatenate(idx) if idx else np.zeros(0, np.int64)
    val = np.concatenate(val) if val else np.zeros(0)
    return sp.csr_matrix((val, idx, indptr), shape=(len(degs), width))


def two_sided(B, C, rng, name):
    """diag(B, C^T): its rows carry the row degrees of B (and the column degrees of C), its columns those of C (and the
    column degrees of B)."""
    A = sp.block_diag([B, C.T.tocsr()], format="csr")
    A.sort_indices()
    m, n = A.shape
    return LPInstance(name, A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data.astype(np.float64),
                      rng.standard_normal(n), rng.standard_normal(m), (rng.random(n) < 0.4).astype(np.int32))


# 0 .. 25: the base tier up to its last row (16), its steps of 2 / 4 / 8 nonzeros, and the first group rows.
# 31 .. 33, 47 .. 49, 63 .. 65: the group tier's steps of 16 / 32 nonzeros and its last row (64).
# 127 .. 129, 511 .. 513, 767 .. 769: wave-tier steps of 64 (forward / backward 16), 128 (source-major) and 512 (1 channel).
# 1023 .. 1025 and 4095 .. 4097: the last wave row and the first block row of the two geometries; a row of 1025 .. 4096 is a
# block row of the 16-channel sweeps and a wave row of layer 1.
# 1535 .. 1537, 3071 .. 3073, 6143 .. 6145: block-tier steps of 768, 1536 (source-major) and 6144 (1 channel).
GRID_DEGREES = (list(range(26)) + [31, 32, 33, 47, 48, 49, 63, 64, 65, 127, 128, 129, 511, 512, 513, 767, 768, 769,
                                   1023, 1024, 1025, 1535, 1536, 1537, 3071, 3072, 3073, 4095, 4096, 4097,
                                   6143, 6144, 6145])


def degree_grid(variant, seed=0, c=None):
    """One LP whose rows AND columns carry GRID_DEGREES.  variant 0: every tier population is a whole number of items in
    both geometries (group rows a multiple of 16, base rows a multiple of 64); variant 1: one more than that, so the last
    item of every tier holds a single row.  The pattern depends on the variant only, the values on the seed."""
    c = c or constants()
    T = c["T16"]
    assert T[:2] == c["T1"][:2]
    pat = np.random.default_rng(1000 + variant)
    width = max(GRID_DEGREES) + 55
    B = block_of(GRID_DEGREES, width, pat)
    deg = np.concatenate([np.diff(B.indptr), np.bincount(B.indices, minlength=width)])
    group = int(((deg > T[0]) & (deg <= T[1])).sum())
    k = (variant - group) % 16                       # filler group rows of T[0] + 1 nonzeros, each in columns of its own
    fill = T[0] + 1
    base = int((deg <= T[0]).sum()) + k * fill
    z = (variant - base) % 64                        # filler rows without nonzeros
    rows = len(GRID_DEGREES) + k + z
    cols = width + k * fill
    indptr = np.concatenate([B.indptr, B.indptr[-1] + fill * np.arange(1, k + 1), np.full(z, B.indptr[-1] + fill * k)])
    indices = np.concatenate([B.indices, width + np.arange(k * fill)])
    B = sp.csr_matrix((np.ones(len(indices)), indices, indptr), shape=(rows, cols))
    rng = np.random.default_rng(seed)
    B.data = rng.standard_normal(B.nnz)
    inst = two_sided(B, B, rng, f"grid{variant}s{seed}")
    # distinct values in the two halves (the pattern of the second half is the transpose of the first)
    inst.values[:] = rng.standard_normal(inst.nnz)
    return inst


def chunk_base(seed=3):
    """Base LP of the list-chunk cases: 36 rows of 65 .. 100 nonzeros (one item each in every list kind) over 192 columns,
    whose own degrees (about 15) mix base and group rows in; both orientations through diag(B, B^T)."""
    rng = np.random.default_rng(seed)
    B = block_of(list(range(65, 101)), 192, rng)
    return two_sided(B, B, rng, "chunkbase")


def chunk_base_small(seed=3):
    """A base LP of three items per side (wave rows of 65 and 66 nonzeros, a group row of 17) over 70 columns of about two:
    replicas of it move the list lengths of a SMALL grid in steps fine enough to land on 63 / 64 and 65 / 66 items, which
    chunk_base()'s 72 wave rows per replica step over at 8 workgroups (12 wavefronts)."""
    rng = np.random.default_rng(seed)
    B = block_of([65, 66, 17], 70, rng)
    return two_sided(B, B, rng, "chunksmall")


def block_laps_instance(cus=256, seed=4, c=None):
    """2 * gp + 1 rows and columns above T1[2] nonzeros and as many in T16[2] + 1 .. T1[2]: the block-tier loop of both
    geometries runs a second and a third lap."""
    c = c or constants()
    n = 2 * grid_per_partition(cus, c) + 1
    rng = np.random.default_rng(seed)
    degs = ([c["T1"][2] + 1 + 3 * i for i in range(n)] +
            [c["T16"][2] + 1 + (i * (c["T1"][2] - c["T16"][2] - 1)) // (n - 1) for i in range(n)])
    B = block_of(degs, 2 * c["T1"][2], rng)
    return two_sided(B, B, rng, "blocklaps")


SHARP_AMP = 1.0
# group, wave, block (16) / wave (1), block of both: one 1-channel step, and three (a 1-channel block step is 6144 nonzeros)
SHARP_DEGREES = [40, 40, 700, 700, 2000, 2000, 5000, 5000, 12400, 12400]
SHARP_WIDTH = 12600


def sharp_instance(seed=6, amp=SHARP_AMP):
    """Rows and columns of the group, wave and both block tiers whose coefficients ascend (even rows) or descend (odd
    rows) along the row: whatever the sign of the edge term's factor t_i, one row of each pair has logits that increase
    along the row, so its running maximum moves in every step."""
    rng = np.random.default_rng(seed)
    B = block_of(SHARP_DEGREES, SHARP_WIDTH, rng, values="updown", amp=amp)
    C = block_of(SHARP_DEGREES, SHARP_WIDTH, rng, values="updown", amp=amp)
    inst = two_sided(B, C, rng, "sharp")
    inst.coefs[:] = rng.uniform(-0.2, 0.2, inst.n)          # small source features: the edge term a_ij t_i leads
    inst.rhs[:] = rng.uniform(-0.2, 0.2, inst.m)
    return inst


def sharp_rows(inst):
    """{orientation: ids of the sharp rows} of sharp_instance(): the first rows of A (block B) and the last columns
    (block C^T)"""
    k = len(SHARP_DEGREES)
    return {"A": np.arange(k), "At": inst.n - k + np.arange(k)}


def sharp_state(factor, seed=9):
    import torch
    from oracle import pyg_restatement as o1
    sd = o1.init_state(seed, torch.float64)
    for key in sd:
        if "lin_query" in key or "lin_edge" in key:
            sd[key] = sd[key] * factor
    return sd


def replicate(base, R, name=None, basis_seed=None):
    """ONE instance that is the block diagonal of R copies of `base`.  basis_seed: labels drawn anew for every copy
    (they do not enter the logits), so the BCE gradient differs from copy to copy."""
    m, n, e = base.m, base.n, base.nnz
    indptr = np.concatenate([[0], (base.indptr[1:][None, :] + e * np.arange(R)[:, None]).reshape(-1)]).astype(np.int64)
    indices = (base.indices.astype(np.int64)[None, :] + n * np.arange(R)[:, None]).reshape(-1).astype(np.int32)
    basis = np.tile(base.basis, R)
    if basis_seed is not None:
        basis = (np.random.default_rng(basis_seed).random(n * R) < 0.4).astype(np.int32)
    return LPInstance(name or f"{base.name}x{R}", indptr, indices, np.tile(base.values, R), np.tile(base.coefs, R),
                      np.tile(base.rhs, R), basis)


def empty_instance(m, n, seed=0):
    rng = np.random.default_rng(seed)
    return LPInstance(f"nonz{m}x{n}", np.zeros(m + 1, np.int64), np.zeros(0, np.int32), np.zeros(0),
                      rng.standard_normal(n), rng.standard_normal(m), (rng.random(n) < 0.4).astype(np.int32))


def single_row_instance(deg, seed=0):
    rng = np.random.default_rng(seed)
    return LPInstance(f"row{deg}", np.array([0, deg], np.int64), np.arange(deg, dtype=np.int32), rng.standard_normal(deg),
                      rng.standard_normal(deg), rng.standard_normal(1), (rng.random(deg) < 0.4).astype(np.int32))


def one_hop(inst, orient, row, k=4):
    """up to k variables within one hop of row `row` of an orientation: the variables of a constraint row; a variable
    itself and variables that share its first constraint"""
    if orient == "A":
        v = inst.indices[inst.indptr[row]:inst.indptr[row + 1]]
        return np.unique(v[np.linspace(0, len(v) - 1, min(k, len(v))).astype(int)]) if len(v) else np.zeros(0, int)
    out = [row]
    rows = np.repeat(np.arange(inst.m), np.diff(inst.indptr))[inst.indices == row]
    if len(rows):
        r = rows[0]
        out += [int(x) for x in inst.indices[inst.indptr[r]:inst.indptr[r + 1]][:k - 1]]
    return np.unique(out)


def spot_tiers(c=None):
    """The distinct degree ranges of the two geometries: name -> (lowest, highest degree, what it is in the 16-channel /
    1-channel sweeps).  A row of T16[2] + 1 .. T1[2] nonzeros is a block row of the former and a wave row of the latter."""
    c = c or constants()
    T16, T1 = c["T16"], c["T1"]
    assert T16[:2] == T1[:2] and T16[2] < T1[2]
    return {"base": (1, T16[0], "base / base"), "group": (T16[0] + 1, T16[1], "group / group"),
            "wave": (T16[1] + 1, T16[2], "wave / wave"), "block16_wave1": (T16[2] + 1, T1[2], "block / wave"),
            "block": (T1[2] + 1, 1 << 30, "block / block")}


def tier_rows(inst, c=None):
    """{(orientation, range of spot_tiers()): id of the longest row of that range, or None}"""
    out = {}
    for orient, deg in zip(("A", "At"), degrees(inst)):
        for name, (lo, hi, _) in spot_tiers(c).items():
            ids = np.flatnonzero((deg >= lo) & (deg <= hi))
            out[(orient, name)] = int(ids[np.argmax(deg[ids])]) if len(ids) else None
    return out


# The tier cases of the fused layer-3 launch (tests/test_fused_l3_pair.py; tools/fused_dump.py runs them too):
# name -> (variable-side degrees that C's rows bring, width of C, the tier of the 16-channel lists they must reach)
L3_TIER_CASES = {
    "base": ([0, 1, 4, 5, 16] * 7 + [2, 3], 40, "base"),             # 37 rows: the last base item holds 5 + |B's columns| % 16
    "group": ([17, 64, 33, 18, 17, 64, 0, 5], 80, "group"),           # six group rows: one full item of four and a partial one
    "wave": ([65, 1024, 640, 0, 1, 16], 1100, "wave"),
    "block": ([1025, 6145, 3, 0, 17, 65], 6200, "block"),
}
L3_B_DEGREES, L3_B_WIDTH = [2, 3, 1, 0, 2], 9                         # the constraint block: base-tier degrees on both sides


def l3_tier_instance(name):
    degs, width, _ = L3_TIER_CASES[name]
    rng = np.random.default_rng(100 + sorted(L3_TIER_CASES).index(name))
    return two_sided(block_of(L3_B_DEGREES, L3_B_WIDTH, rng), block_of(degs, width, rng), rng, f"l3{name}")


# ---------------------------------------------------------------------------------------------------------------------
# 4. the oracle's decomposition in a chosen floating-point type
# ---------------------------------------------------------------------------------------------------------------------
def _seg(ptr, dt):
    n_rows, nnz = len(ptr) - 1, int(ptr[-1])
    rows = np.repeat(np.arange(n_rows), np.diff(ptr))
    return sp.csr_matrix((np.ones(nnz, dt), (rows, np.arange(nnz))), shape=(n_rows, nnz)), rows


def _fwd_dt(p, ptr, idx, val, X_src, x_dst, dt):
    f = dt(4.0)
    Pq, pq0, Pt, pt0 = p["Wk"].T @ p["Wq"] / f, p["Wk"].T @ p["bq"] / f, p["Wq"].T @ p["we"] / f, (p["bq"] @ p["we"]) / f
    S_mat, rows = _seg(ptr, dt)
    qp = x_dst @ Pq.T + pq0
    t = x_dst @ Pt + pt0
    Xe = X_src[idx]
    l = np.einsum("ec,ec->e", qp[rows], Xe) + val * t[rows]
    mx = np.full(len(ptr) - 1, -np.inf, dt)
    np.maximum.at(mx, rows, l)
    mx = np.where(np.diff(ptr) > 0, mx, dt(0.0)).astype(dt)
    pe = np.exp(l - mx[rows])
    L = S_mat @ pe
    rinv = dt(1.0) / (L + dt(1e-16))
    Z = (S_mat @ (pe[:, None] * Xe)) * rinv[:, None]
    u = (S_mat @ (pe * val)) * rinv
    S = L * rinv
    o = Z @ p["Wv"].T + S[:, None] * p["bv"] + u[:, None] * p["we"] + x_dst @ p["Ws"].T + p["bs"]
    h = np.maximum(o, dt(0.0))
    assert h.dtype == dt and l.dtype == dt
    return h, dict(qp=qp, t=t, mx=mx, rinv=rinv, Z=Z, u=u, S=S, h=h, l=l)


def _bwd_dt(p, ptr, idx, val, X_src, x_dst, sv, dh, dt, need_input_grads=True):
    f = dt(4.0)
    Pq, Pt, Pb = p["Wk"].T @ p["Wq"] / f, p["Wq"].T @ p["we"] / f, p["Wq"].T @ p["bk"] / f
    S_mat, rows = _seg(ptr, dt)
    g = dh * (sv["h"] > 0)
    gv, ge, gb = g @ p["Wv"], g @ p["we"], g @ p["bv"]
    D = np.einsum("nc,nc->n", gv, sv["Z"]) + gb * sv["S"] + ge * sv["u"]
    cc = gb - D
    Xe = X_src[idx]
    alpha = np.exp(sv["l"] - sv["mx"][rows]) * sv["rinv"][rows]
    dl = alpha * (np.einsum("ec,ec->e", gv[rows], Xe) + val * ge[rows] + cc[rows])
    dqp, ds, dtt = S_mat @ (dl[:, None] * Xe), S_mat @ dl, S_mat @ (dl * val)
    dx_dst = dX_src = None
    if need_input_grads:
        dx_dst = g @ p["Ws"] + dqp @ Pq + ds[:, None] * Pb + dtt[:, None] * Pt
        contrib = alpha[:, None] * gv[rows] + dl[:, None] * sv["qp"][rows]
        dX_src = np.zeros_like(X_src)
        np.add.at(dX_src, idx, contrib)
    A_dx, s_dqp = dqp.T @ x_dst, dqp.sum(0)
    v_ds, v_dt, s_ds, s_dt = ds @ x_dst, dtt @ x_dst, ds.sum(), dtt.sum()
    grads = {
        "lin_skip.weight": g.T @ x_dst, "lin_skip.bias": g.sum(0),
        "lin_value.weight": g.T @ sv["Z"], "lin_value.bias": (g * sv["S"][:, None]).sum(0),
        "lin_key.weight": (p["Wq"] @ A_dx.T + np.outer(p["bq"], s_dqp)) / f,
        "lin_key.bias": (p["Wq"] @ v_ds + p["bq"] * s_ds) / f,
        "lin_edge.weight": ((g * sv["u"][:, None]).sum(0) + (p["Wq"] @ v_dt + p["bq"] * s_dt) / f)[:, None],
        "lin_query.weight": (p["Wk"] @ A_dx + np.outer(p["bk"], v_ds) + np.outer(p["we"], v_dt)) / f,
        "lin_query.bias": (p["Wk"] @ s_dqp + p["bk"] * s_ds + p["we"] * s_dt) / f,
    }
    return grads, dx_dst, dX_src


def model_dt(sd, batch, dt, dlogits=None):
    """oracle/spmm_form.py::gnn_forward_backward with every array and every operation in the type `dt` (np.float32 or
    np.float64); the fp64 run equals spmm_form (tests/test_fused_oracle.py checks it).  Returns dict(logits, loss, grads)."""
    a = lambda x: np.asarray(x, dtype=dt)
    P = {}
    for name in CONV_CIN:
        p = o2.conv_params(sd, name)
        P[name] = {k: a(v) for k, v in p.items()}
    x1, x2 = a(batch.x1)[:, None], a(batch.x2)[:, None]
    ov = (batch.cp, batch.ri, a(batch.cv))
    oc = (batch.rp, batch.ci, a(batch.va))
    h1v, s1v = _fwd_dt(P["gconv1_w2s"], *ov, x2, x1, dt)
    h1c, s1c = _fwd_dt(P["gconv1_s2w"], *oc, x1, x2, dt)
    h2v, s2v = _fwd_dt(P["gconv2_w2s"], *ov, h1c, h1v, dt)
    h2c, s2c = _fwd_dt(P["gconv2_s2w"], *oc, h1v, h1c, dt)
    h3v, s3v = _fwd_dt(P["gconv3_w2s"], *ov, h2c, h2v, dt)
    wfc, bfc = a(sd["fc.weight"])[0], a(sd["fc.bias"])[0]
    z = h3v @ wfc + bfc
    y, wn = a(batch.basis), a(batch.wnode)
    bce = np.maximum(z, dt(0)) - z * y + np.log1p(np.exp(-np.abs(z)))
    loss = (wn * bce).sum()
    dz = wn * (dt(1.0) / (dt(1.0) + np.exp(-z)) - y) if dlogits is None else a(dlogits)
    assert z.dtype == dt and dz.dtype == dt
    G = {"fc.weight": (dz @ h3v)[None, :], "fc.bias": np.array([dz.sum()])}
    dh3v = dz[:, None] * wfc[None, :]
    g3, d_h2v, d_h2c = _bwd_dt(P["gconv3_w2s"], *ov, h2c, h2v, s3v, dh3v, dt)
    g2v, d_h1v_a, d_h1c_a = _bwd_dt(P["gconv2_w2s"], *ov, h1c, h1v, s2v, d_h2v, dt)
    g2c, d_h1c_b, d_h1v_b = _bwd_dt(P["gconv2_s2w"], *oc, h1v, h1c, s2c, d_h2c, dt)
    g1v, _, _ = _bwd_dt(P["gconv1_w2s"], *ov, x2, x1, s1v, d_h1v_a + d_h1v_b, dt, need_input_grads=False)
    g1c, _, _ = _bwd_dt(P["gconv1_s2w"], *oc, x1, x2, s1c, d_h1c_a + d_h1c_b, dt, need_input_grads=False)
    for name, gd in (("gconv3_w2s", g3), ("gconv2_w2s", g2v), ("gconv2_s2w", g2c), ("gconv1_w2s", g1v), ("gconv1_s2w", g1c)):
        for k, v in gd.items():
            assert v.dtype == dt, (name, k, v.dtype)
            G[f"{name}.{k}"] = v
    flat = [np.asarray(G.get(key, np.zeros(shape)), dtype=np.float64).reshape(-1) for key, shape in state_dict_spec()]
    return dict(logits=z.astype(np.float64), loss=float(loss), grads=np.concatenate(flat))


def rel_err(got, want):
    """the figure `close` of tests/test_hip_parity.py bounds: max |got - want| / max |want|"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max()) / max(float(np.abs(want).max()), 1e-30)


def running_max_moves(l_row, width):
    """True if the maximum over the first k steps of `width` entries grows with every step k"""
    n = len(l_row)
    mx = [l_row[s:s + width].max() for s in range(0, n, width)]
    return all(b > a for a, b in zip(mx, mx[1:]))


# layers whose destinations are the rows of an orientation: (saved-state key, source activations, list kind)
SHARP_LAYERS = {"A": (("s1c", "x1", "1"), ("s2c", "h1v", "16")),
                "At": (("s1v", "x2", "1"), ("s2v", "h1c", "16"), ("s3v", "h2c", "16"))}


def sharp_report(r, batch, rows, c=None):
    """For every sharp row and every layer it is a destination of, on the fp64 oracle result `r`: (orientation, layer,
    row, degree, tier, steps, whether the running maximum moves in every step of that tier's kernel, largest attention
    weight of the row)."""
    c = c or constants()
    out = []
    for orient, layers in SHARP_LAYERS.items():
        ptr, idx, val, _, _ = batch.orient(orient == "At")
        for key, src, kind in layers:
            sv = r["saved"][key]
            X = {"x1": batch.x1[:, None], "x2": batch.x2[:, None]}.get(src)
            X = r[src] if X is None else X
            T = c["T1"] if kind == "1" else c["T16"]
            for row in rows[orient]:
                e = slice(int(ptr[row]), int(ptr[row + 1]))
                deg = e.stop - e.start
                l = X[idx[e]] @ sv["qp"][row] + val[e] * sv["t"][row]
                tier = "block" if deg > T[2] else "wave" if deg > T[1] else "group" if deg > T[0] else "base"
                w = step_widths(kind, c)[tier]
                a = np.exp(l - l.max())
                out.append((orient, key, int(row), deg, tier, -(-deg // w), running_max_moves(l, w), float(a.max() / a.sum())))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# 5. ragged instances and the inputs of the one-launch small step (shared by several test modules)
# ---------------------------------------------------------------------------------------------------------------------
def holes_instance(seed, m, n):
    """Random LP with empty rows, empty columns and a few dense rows (ragged input for the tiled copies)."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(m):
        u = rng.random()
        k = 0 if u < 0.3 else (int(rng.integers(1, 4)) if u < 0.6 else (n // 2 if u > 0.98 else int(rng.poisson(12)) + 1))
        cols = np.sort(rng.choice(n - n // 10, size=min(k, n - n // 10), replace=False)).astype(np.int32)   # last 10 % of the columns stay empty
        rows.append(cols)
    indptr = np.zeros(m + 1, np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    indices = np.concatenate(rows).astype(np.int32) if indptr[-1] else np.zeros(0, np.int32)
    values = rng.standard_normal(indptr[-1])
    return LPInstance(f"holes{seed}", indptr, indices, values, rng.standard_normal(n), rng.random(m) * 5,
                      (rng.random(n) < 0.37).astype(np.int32))


def ragged_instance(seed, m, n, dense_rows=(), mean=14):
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(m):
        u = rng.random()
        k = 0 if u < 0.2 else (int(rng.integers(1, 4)) if u < 0.45 else int(rng.poisson(mean)) + 1)
        if i in dense_rows:
            k = dense_rows[i]
        hi = max(1, n - n // 10)                               # the last 10 % of the columns stay empty
        rows.append(np.sort(rng.choice(hi, size=min(k, hi), replace=False)).astype(np.int32))
    indptr = np.zeros(m + 1, np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    indices = np.concatenate(rows).astype(np.int32) if indptr[-1] else np.zeros(0, np.int32)
    values = rng.standard_normal(indptr[-1])
    return LPInstance(f"ragged{seed}", indptr, indices, values, rng.standard_normal(n), rng.random(m) * 5,
                      (rng.random(n) < 0.37).astype(np.int32))


def ragged_batch():
    """Empty rows, a dense row block, an instance without nonzeros, a 3 x 5 instance, and instances of exactly 480 / 481
    and 512 / 513 rows (tile boundaries of the copies)."""
    empty = LPInstance("empty", np.zeros(6, np.int64), np.zeros(0, np.int32), np.zeros(0), np.zeros(4), np.zeros(5),
                       np.zeros(4, np.int32))
    return [ragged_instance(21, 400, 700, {i: 30 + 7 * i for i in range(0, 60, 3)}), holes_instance(1, 700, 900), empty,
            ragged_instance(50, 480, 721), ragged_instance(51, 481, 1100), holes_instance(2, 3, 5),
            ragged_instance(52, 512, 800), ragged_instance(53, 513, 640, mean=40)]


def golden_state(golden):
    import torch
    from oracle import pyg_restatement as o1
    return {k: v.numpy() for k, v in o1.unflatten_state(torch.tensor(golden["weights_flat"])).items()}


def small_inst(A, name, seed):
    A = sp.csr_matrix(A)
    A.sort_indices()
    rng = np.random.default_rng(seed)
    m, n = A.shape
    return LPInstance(name, A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data.astype(np.float64),
                      rng.standard_normal(n), rng.standard_normal(m), (rng.random(n) < 0.4).astype(np.int32))


def small_grid(seed):
    """rows AND columns of 0 .. 25 nonzeros (fused_cases.block_of / two_sided)"""
    rng = np.random.default_rng(seed)
    B = block_of(list(range(26)), 40, rng)
    return two_sided(B, B, rng, f"grid25s{seed}")


def small_long(as_column):
    """one entry of 6 145 nonzeros (above every step of the other paths' tiers; this kernel gives each of its 64 groups a
    chunk of 97 entries, the last one 34) beside rows of 0 .. 5"""
    rng = np.random.default_rng(11)
    B = block_of([6145] + [i % 6 for i in range(30)], 6200, rng)
    return small_inst(B.T if as_column else B, "longcol" if as_column else "longrow", 12)


def small_sharp():
    """fused_cases' sharp case at this kernel's size: coefficients ascending (even rows) / descending (odd rows) along rows
    on both sides of SM_LONG = 128 entries, in both orientations; the scores are doubled by the caller's weights"""
    rng = np.random.default_rng(6)
    degs = [40, 40, 128, 128, 129, 129, 700, 700, 1500, 1500]
    B = block_of(degs, 1600, rng, values="updown")
    C = block_of(degs, 1600, rng, values="updown")
    inst = two_sided(B, C, rng, "sharp_small")
    inst.coefs[:] = rng.uniform(-0.2, 0.2, inst.n)
    inst.rhs[:] = rng.uniform(-0.2, 0.2, inst.m)
    return inst


def small_step_cases(golden, subset5):
    sd = golden_state(golden)
    cases = [(i.name, sd, [i]) for i in subset5]
    by = {i.name: i for i in subset5}
    cases += [("ragged3", sd, [by["afiro.mps"], empty_instance(3, 5), by["sc50a.mps"]]),
              ("1x1", sd, [small_inst(np.array([[1.5]]), "one", 1)]),
              ("nonz", sd, [empty_instance(7, 9), empty_instance(2, 1, seed=1)]),
              ("grid25", sd, [small_grid(0)]),
              ("grid25x2", sd, [small_grid(0), small_grid(1)]),
              ("longrow", sd, [small_long(False)]),
              ("longcol", sd, [small_long(True)]),
              ("sharp", {k: v.numpy() for k, v in sharp_state(2.0).items()}, [small_sharp()])]
    return cases


SMALL_CASE_NAMES = SUBSET5 + ["ragged3", "1x1", "nonz", "grid25", "grid25x2", "longrow", "longcol", "sharp"]
# Tensors that the fp32 reference itself cannot pin on their own scale (tests/grad_scales.py; counted by
# tests/test_grad_scales.py on the CPU): gconv1_w2s.lin_query.weight, a cancellation, on three inputs.  The 1 x 1 instance is
# no per-tensor input: with one nonzero per row every attention gradient is a cancellation to zero (three tensors exempt).
SMALL_PER_TENSOR_CAPS = dict({n: 0 for n in SMALL_CASE_NAMES if n != "1x1"}, **{"kb2.mps": 1, "sc50a.mps": 1, "ragged3": 1})


# test_fused_oracle.py's batches of n degree grids of different values, (variant, n) -> tensors that the fp32 restatement
# alone exempts from the per-tensor check of tests/grad_scales.py on the loss step (always two large bias tensors of one
# conv, lin_skip.bias and lin_value.bias at 1.3e-5 .. 1.8e-5: the restatement sums up to 10^6 terms one after the other);
# None: more than two, no per-tensor input (grid1 x 8: four).  Asserted on the CPU by tests/test_grad_scales.py.
GRID_BATCH_CAPS = {(0, 1): 0, (0, 2): 0, (0, 7): 2, (0, 8): 0, (0, 9): 2, (1, 1): 0, (1, 2): 0, (1, 7): 0, (1, 8): None, (1, 9): 2}
GRID_BATCH_EXEMPT_STATED = {(1, 8): 4}


def grid_batch(variant, n_inst):
    return [degree_grid(variant, seed=s) for s in range(n_inst)]
