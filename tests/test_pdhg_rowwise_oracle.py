"""CPU: the conditions that tests/test_pdhg_rowwise.py rests on, asserted from tests/pdhg_rowwise.py alone (no GPU, no library).

1. A correct fp32 execution stays inside the bound: the lane-order restatement against the fp64 reference, in every row, column
   and scalar of `tiers`, `mixed` and `many`, every run of RUNS and every K:  |fp32 - fp64| / bound <= 1.
   RECORDED: the largest ratio is 0.471 (`tiers`, mllp_lp_pdhg_scaled at its defaults, K = 1, x).
2. Every mutation of the rule's restatement (`mut` of pdhg_rowwise.lane32) leaves the bound by at least 4 x on every row it
   affects -- and on d_kkt where that row is the instance's worst, which in `tiers` it always is -- and moves nothing else
   beyond its bound.  A mutation of ONE row states its rows by name; RECORDED: the smallest ratio of such a row is 65.7
   (`tiers`, the 1 x 4097 row without its terms from 4096 on, y after one Halpern iteration).  A mutation of the rule for EVERY
   row (w1 and w2 swapped, reflect ignored, clip omitted, tc_j taken as dc_j, the evaluation from the iterate) states its rows by
   the fp64 rule run with the mutation: affected where that differs from the rule by 5 bounds and 1 of its own, unaffected where
   it is equal.  RECORDED: affected are 98.6 to 99.99 % of the entries of x and y in `tiers` and `mixed` and 67.6 to 73.8 % in
   `many` (26 to 32 % are equal: empty instances, columns clipped either way), 10.8 % of `many`'s x for the omitted clip; at
   most 1.41 % of a vector lie between; the smallest ratio of an affected entry is 5.54; every instance with rows and columns
   shows the evaluation from the iterate in d_kkt.
3. The clip is exercised without hiding a designated column (every column of `tiers`, the columns of `mixed` above 64 terms):
   none comes within 8 bounds of zero; at most a quarter of all columns clip, and some of `many` do in every run.  `many` alone
   is held to a half, not a quarter: its instances must have a solution (or mllp_lp_pdhg_rays would stop on an exact ray), a
   vertex of such an LP has n - m columns at zero, the iteration heads there, and the 0 x 2 instances -- 10.8 % of its columns,
   c > 0 and nothing else -- clip within two steps whatever the seed.
4. What mllp_lp_pdhg_spectral's estimate shows of a dropped term, after one round and after two.
5. The layout is what DESIGN.md 4.29 says.
"""
import numpy as np
import pytest

import pdhg_rowwise as rw
import test_basis_repair as tb

LOCAL_RUNS = [("pdhg", {}), ("pdhg_halpern", dict(reflect=True))]


@pytest.fixture(scope="module")
def cases():
    return dict(tiers=rw.tiers(tb.dense_case), mixed=rw.mixed(tb.dense_case), many=rw.many(tb.dense_case))


def _all_ratios(got, ref):
    rs = rw.ratios(got, ref)
    rs["rp"], rs["rd"] = rw.ratio(got["rp"], ref["rp"]), rw.ratio(got["rd"], ref["rd"])
    return rs


def test_a_correct_fp32_execution_stays_inside_the_bound(cases):
    top = (0.0, ())
    for name, case in cases.items():
        for call, kw, Ks in rw.RUNS:
            for K in Ks:
                rs = _all_ratios(rw.lane32(case, call, K, **kw), rw.reference(case, call, K, **kw))
                for field, v in rs.items():
                    assert np.isfinite(v).all() and v.max(initial=0.0) <= 1.0, (name, call, kw, K, field, v.max())
                    top = max(top, (float(v.max(initial=0.0)), (name, call, str(kw), K, field)), key=lambda p: p[0])
    print(f"largest ratio of the lane-order fp32 restatement: {top[0]:.3f} at {top[1]}")
    assert top[0] > 0.01        # (the bound is not vacuous: fp32 comes within two orders of it)


# ---------------------------------------------------------------------------------------------------
# mutations
# ---------------------------------------------------------------------------------------------------
def _local_mutations(cases):
    """(batch, mutation, rows that may move: {field: ids}, rows that must leave the bound: [(field, id, the K's)])"""
    out = []
    t, mx = cases["tiers"], cases["mixed"]
    n0 = rw.MIXED_SHAPE[1]

    def row_mut(name, case, kind, r, K0=0):
        inst = int(case.ri[r])
        cols = case.ecol[case.rows.ptr[r]:case.rows.ptr[r + 1]]      # their dual residuals read y_r at the evaluation
        must = [("rp", r, (0, 1)), ("y", r, (1,))] if K0 == 0 else [("y", r, (1,))]
        if name == "tiers" and K0 == 0:
            must.append(("kkt", (inst, 0), (0, 1)))
        out.append((name, dict(kind=kind, orient="row", r=r), dict(y=[r], rp=[r], rd=cols, kkt=[inst]), must))

    def col_mut(name, case, kind, j):
        inst = int(case.ci[j])
        rows_ = case.at_idx[case.cols.ptr[j]:case.cols.ptr[j + 1]]     # they gather xbar_j in the same iteration
        must = [("x", j, (1,))] + ([("rd", j, (0,))] if kind != "neighbour_rhs" else [])      # (after a step max(., 0) may hide the residual)
        if name == "tiers" and kind != "neighbour_rhs":
            must.append(("kkt", (inst, 1), (0,)))
        out.append((name, dict(kind=kind, orient="col", r=j), dict(x=[j], rd=[j], y=rows_, rp=rows_, kkt=[inst]), must))

    for tier in (0, 1, 2):                                           # 1. the last term of a row, per tier, both orientations
        row_mut("tiers", t, "drop_last", rw.first_row(t, tier))
        col_mut("tiers", t, "drop_last", rw.first_col(t, tier))
    for r in (2, 8, 30):
        row_mut("mixed", mx, "drop_last", r)
        col_mut("mixed", mx, "drop_last", n0 + r)
    for r in (47, 128, 192):                                         # 2. the tail past 1024 floor((L - 1) / 1024)
        row_mut("mixed", mx, "drop_tail", r)
        col_mut("mixed", mx, "drop_tail", n0 + r)
    last = int(np.flatnonzero(rw.row_tier(t.rows.len) == 2)[-1])
    row_mut("tiers", t, "drop_tail", last)
    row_mut("mixed", mx, "unwritten", 192, K0=1)                     # 3. the ragged last chunk's one row
    row_mut("mixed", mx, "neighbour_rhs", 13, K0=1)                  # 4. a wave-tier row with the b (c) of the row before
    col_mut("mixed", mx, "neighbour_rhs", n0 + 13)
    return out


def test_every_local_mutation_leaves_the_bound_where_it_acts_and_nowhere_else(cases):
    smallest = (np.inf, ())
    for name, mut, may, must in _local_mutations(cases):
        case = cases[name]
        for call, kw in LOCAL_RUNS:
            for K in (0, 1):
                rs = _all_ratios(rw.lane32(case, call, K, mut=mut, **kw), rw.reference(case, call, K, **kw))
                for field, idx, Ks in must:
                    if K in Ks:
                        got = float(rs[field][idx])
                        assert got >= 4.0, (name, mut, call, K, field, idx, got)
                        smallest = min(smallest, (got, (name, mut["kind"], mut["orient"], mut["r"], call, K, field)), key=lambda p: p[0])
                column = mut["orient"] == "col"
                for field, v in rs.items():
                    if K and column and field in ("rp", "rd"):       # (x_j moves the rows that gather it, and y every residual)
                        continue
                    v = v.copy()
                    if field == "kkt":       # primal, dual, gap: downstream of a moved row after a step; before, its own error only
                        v[may["kkt"][0], :3 if K else 0] = 0.0
                        if not K:
                            v[may["kkt"][0], 1 if column else 0] = 0.0
                    elif field in may:
                        v[np.asarray(may[field], np.int64)] = 0.0
                    assert v.max(initial=0.0) <= 1.0, (name, mut, call, K, field, int(v.argmax()), v.max())
    print(f"smallest ratio of a row that a local mutation affects: {smallest[0]:.3g} at {smallest[1]}")


GLOBAL = (("swap_w", "pdhg_halpern", dict(reflect=True), 3, ("x", "y")),
          ("no_reflect", "pdhg_halpern", dict(reflect=True), 2, ("x", "y")),
          ("tc_is_dc", "pdhg_scaled", {}, 1, ("x", "y")),
          ("no_clip", "pdhg", {}, 1, ("x", "y")),
          ("eval_iterate", "pdhg_halpern", dict(reflect=True), 2, ("kkt",)))


def test_every_global_mutation_leaves_the_bound_on_every_row_it_affects(cases):
    """5. w1 and w2 swapped (equal at k = 0: the third output is the first to tell);  6. reflect ignored;  7. clip omitted;
    8. tc_j taken as dc_j;  9. the evaluation from the iterate (which IS the step's output after one iteration: K = 2).
    THE AFFECTED SET of such a mutation is stated by the rule itself: the fp64 reference runs WITH the mutation, and an entry
    is affected where that run differs from the rule's by at least 5 bounds of the rule plus 1 of its own, unaffected where the
    two are equal (an empty instance, a column clipped under both, dc_j = 1, a column that does not clip).  The fp32 mutant is
    then beyond 4 bounds on EVERY affected entry and inside 1 on every unaffected one; the entries between the two -- the
    mutation moves them by less than 6 bounds -- are counted, and are at most 2 % of a vector"""
    least, between_most = np.inf, 0.0
    for name, case in cases.items():
        for kind, call, kw, K, fields in GLOBAL:
            ref, refm = rw.reference(case, call, K, **kw), rw.reference(case, call, K, mut=dict(kind=kind), **kw)
            rs = rw.ratios(rw.lane32(case, call, K, mut=dict(kind=kind), **kw), ref)
            for f in fields:
                if f == "kkt":
                    a, b = (np.stack([q.v for q in r["kkt"][:3]], 1) for r in (ref, refm))
                    ea, eb = (np.stack([q.e for q in r["kkt"][:3]], 1) for r in (ref, refm))
                    # an instance's three errors count as one entry: the mutation shows in d_kkt where it shows in one of them
                    full = (case.inst_m > 0) & (case.inst_n > 0)
                    hit = np.abs(a - b) >= 10.0 * ea + 2.0 * eb
                    assert hit[full].any(1).all(), (name, kind, np.flatnonzero(full & ~hit.any(1))[:8])
                    assert (np.where(hit, rs["kkt"][:, :3], np.inf)[full].min(1) >= 4.0).all(), (name, kind)
                    print(f"{name:6s} {kind:13s} kkt: every instance with rows and columns is affected in one of its three errors")
                    continue
                else:
                    a, b, ea, eb, v = ref[f].v, refm[f].v, ref[f].e, refm[f].e, rs[f]
                delta = np.abs(a - b)
                affected, same = delta >= 10.0 * ea + 2.0 * eb, delta == 0
                assert affected.any() or (kind == "no_clip" and name != "many"), (name, kind, f)     # (no column of `tiers` clips)
                if not affected.any():
                    continue
                assert (v[affected] >= 4.0).all(), (name, kind, f, float(v[affected].min()))
                assert (v[same] <= 1.0).all(), (name, kind, f, float(v[same].max()))
                between = 1.0 - (affected | same).mean()
                least, between_most = min(least, float(v[affected].min())), max(between_most, between)
                print(f"{name:6s} {kind:13s} {f:3s}: affected {affected.mean():.4f} (smallest ratio {v[affected].min():.3g}), unaffected "
                      f"{same.mean():.4f}, between {between:.4f}")
                assert between <= 0.02, (name, kind, f, between)
            if kind == "tc_is_dc":
                assert (np.abs(ref["x"].v - refm["x"].v)[ref["dc"].v == 1.0] == 0).all()
            if kind == "no_clip":
                assert (np.abs(ref["x"].v - refm["x"].v)[ref["xun"].v > 0] == 0).all()
    print(f"global mutations: smallest ratio of an affected entry {least:.3g}; at most {between_most:.4f} of a vector between")


def test_what_the_power_iteration_catches(cases):
    """mllp_lp_pdhg_spectral's estimate against its propagated bound when a walk of a power round drops the last term of ONE
    row (column).  After ONE round every such drop in `tiers` is beyond 4 bounds: the gathered vector is the hash start, the
    terms of a 1 x L row cancel, and one term stands out.  After TWO rounds the vector is the row itself, the terms are
    squares, a term is 1 / L of the sum, and the bound -- which adds the errors of w and of its norm where the normalisation
    cancels them -- no longer sees a term of a 1 x L row from L = 1023 on; tests/test_pdhg_rowwise.py therefore runs both"""
    t, mx = cases["tiers"], cases["mixed"]
    n0, m0 = rw.MIXED_SHAPE[1], rw.MIXED_SHAPE[0]
    for P in (1, 2):
        ref = rw.power(rw.Ref(), t, P)
        assert rw.ratio(rw.power(rw.Lane(), t, P), ref).max() <= 1.0
        got = {}
        for k in range(t.K):
            wide, L = k % 2 == 0, rw.TIER_LENGTHS[k // 2]
            if L > 1:
                mut = dict(kind="drop_last", orient="row" if wide else "col", r=int(t.dict["ptr_m" if wide else "ptr_n"][k]), phases=("power",))
                got[L, wide] = float(rw.ratio(rw.power(rw.Lane(mut), t, P), ref)[k])
        print(f"tiers, {P} round(s): smallest ratio of a dropped last term {min(got.values()):.3g}; below 4: {sorted(k for k, v in got.items() if v < 4.0)}")
        if P == 1:
            assert min(got.values()) >= 4.0, got
        else:
            assert all(v >= 4.0 for (L, wide), v in got.items() if not wide or L < 1023), got
        ref = rw.power(rw.Ref(), mx, P)
        assert rw.ratio(rw.power(rw.Lane(), mx, P), ref).max() <= 1.0
        for orient, r, inst in (("row", 2, 0), ("row", 8, 0), ("row", 30, 0), ("row", 47, 0), ("row", 192, 0), ("col", n0 + 30, 1), ("col", n0 + 192, 1),
                                ("row", m0 + 5, 1), ("col", 5, 0)):
            mut = dict(kind="drop_last", orient=orient, r=r, phases=("power",))
            print(f"mixed, {P} round(s): {orient} {r} without its last term: ratio {float(rw.ratio(rw.power(rw.Lane(mut), mx, P), ref)[inst]):.3g}")


# ---------------------------------------------------------------------------------------------------
# the inputs
# ---------------------------------------------------------------------------------------------------
def test_the_clip_is_exercised_and_hides_no_designated_column(cases):
    for name, case in cases.items():
        if case.designated.any():
            margin = rw.clip_margin(case)
            print(f"{name}: the closest a designated column comes to the clip is {margin:.1f} bounds")
            assert margin > 8.0, (name, margin)
    for call, kw, Ks in rw.RUNS:
        for K in Ks[1:]:
            clipped = {name: rw.reference(case, call, K, **kw)["xun"].v <= 0 for name, case in cases.items()}
            share = np.concatenate(list(clipped.values())).mean()
            print(f"{call} {kw} K = {K}: clipped " + ", ".join(f"{n} {v.mean():.3f}" for n, v in clipped.items()) + f", of all columns {share:.3f}")
            assert share <= 0.25 and clipped["many"].any() and clipped["many"].mean() <= 0.5, (call, kw, K, share)


def test_the_layout_is_what_the_design_says(cases):
    t, mx, mn = cases["tiers"], cases["mixed"], cases["many"]
    # tiers: 38 instances, one row (column) of every length
    assert t.K == 2 * len(rw.TIER_LENGTHS) and t.A.nnz == 2 * sum(rw.TIER_LENGTHS)
    assert [(int(m), int(n)) for m, n in zip(t.inst_m[0::2], t.inst_n[0::2])] == [(1, L) for L in rw.TIER_LENGTHS]
    assert [(int(m), int(n)) for m, n in zip(t.inst_m[1::2], t.inst_n[1::2])] == [(L, 1) for L in rw.TIER_LENGTHS]
    for L, want in ((64, 0), (65, 1), (1024, 1), (1025, 2)):
        assert int(rw.row_tier(L)) == want
    assert sorted(set(-(-np.array(rw.TIER_LENGTHS) // 64))) [-1] == 65       # an L x 1 column sweep: up to 65 items of 64 rows
    # mixed: instance 0 is 193 x 2100 with MIXED_ROWS, instance 1 its transpose
    m, n = rw.MIXED_SHAPE
    assert list(mx.inst_m) == [m, n] and list(mx.inst_n) == [n, m] and m % 64 == 1
    lens = mx.rows.len[:m]
    assert all(lens[r] == L for r, L in rw.MIXED_ROWS.items())
    other = np.delete(lens, list(rw.MIXED_ROWS))
    assert other.min() >= 2 and other.max() <= 6
    tier = rw.row_tier(lens)
    wave0 = [r for r in range(64) if tier[r] == 1]
    assert {r % 4 for r in wave0} == {0, 1, 2, 3} and len({r // 4 for r in wave0}) >= 3      # every position g, three wavefronts
    assert sorted(lens[wave0]) == [65, 65, 128, 1023, 1024, 1024]
    assert [r for r in range(64) if tier[r] == 2] == [30, 47] and not (tier[64:128] == 2).any()
    assert {0, 1, 16, 17, 64} <= set(lens[:64][tier[:64] == 0])
    assert tier[127] == 1 and tier[128] == 2 and tier[192] == 2 and lens[192] == 2048           # the 128-row boundary, the ragged chunk
    assert np.array_equal(mx.cols.len[n:], lens) and np.array_equal(mx.rows.len[m:], mx.cols.len[:n])       # the transpose
    # many: items behind instance 1024 in both orientations, empty instances in between
    assert mn.K == rw.MANY_COUNT == 1100 and rw.MANY_BIG > 1024
    assert (int(mn.inst_m[rw.MANY_BIG]), int(mn.inst_n[rw.MANY_BIG])) == (70, 130) and -(-70 // 64) == 2 and -(-130 // 64) == 3
    assert (mn.inst_m[1024:rw.MANY_BIG] == 0).any() and (mn.inst_n[1024:rw.MANY_BIG] == 0).any()
    shapes = {(int(a), int(b)) for a, b in zip(mn.inst_m, mn.inst_n)}
    assert shapes == set(rw.MANY_SHAPES) | {rw.MANY_BIG_SHAPE}


def test_the_depths_and_the_sum_bound_at_the_longest_row():
    assert [int(rw.depth(L)) for L in (1, 16, 17, 64, 65, 1024, 1025, 2048, 2049, 4097)] == [5, 5, 6, 8, 8, 22, 12, 12, 13, 15]
    assert int(rw.depth_inst(1)) == 11 and int(rw.depth_inst(4097)) == 15
    # 4097 terms of at most 1.5 * 1.5 * (a few): the sum's own part of the bound stays far below a dropped term of 0.25
    assert 2 * (int(rw.depth(4097)) + 2) * rw.U * 4097 * 2.25 < 0.019
