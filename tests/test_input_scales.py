"""Input gradients against the fp64 oracle unit by unit, each ON ITS OWN SCALE (tests/input_scales.py): every element of
dx1 and dx2, every edge of dvalues, dvalues per constraint row and per column, every array per instance; for one conv,
dx_src and dx_dst per node row.

The gap this closes, as tests (the census and the mutations below): `close` of tests/test_input_grads.py holds an array to
5e-5 of ITS MAXIMUM.  On the degree grid half of dx2 and a third of the edges of dvalues lie below that bound altogether, on a
mixed-size batch under BCE the large instances do (1 / n_k), and so does a seventh of the source rows of a conv's dx_src on
the grid: zeros written there, or a large instance 2 % off, pass.  Those are the rows in the last item of a tier list, the
tail chunks of split rows and the instances the partitioner places last.

Bar: RTOL_GRAD = 5e-5, per unit.  Yardstick: the float32 oracle under K_ORDERS = 8 summation orders (the edge list and the
hidden channels permuted); a unit is checked where the yardstick is below RTOL_GRAD / 8 of its own scale, exempt (global
bound only) where it is not; the exempt share is capped per unit kind before a result is looked at.
test_fresh_fp32_orders_pass_the_rule is the arbiter of K_ORDERS and MARGIN: six further fp32 orders, taken as the "kernel",
pass on every input of the GPU part with nothing failing (worst unit of twelve: 3.9e-5 of itself, dvalues of grid1x2, BCE).

Inputs (all small): the degree grid alone (`grid_batch(0, 1)`), two grids of variant 1 (`grid_batch(1, 2)`), the five golden
instances, and MIX, a mixed-size Netlib batch: the five golden instances with woodw, fit2p, 80bau3b, pds-06 and ken-11
(225 k nonzeros; under BCE the per-instance scales of dvalues span 590 x).  d6cube is not in MIX: under BCE the fp32 oracle
itself misses 97 % of its columns (one row holds all 6 184 of them), so a batch with it breaks the cap on exempt columns;
its long row is what the grids' rows of 6 145 stand for.

Every GPU test prints, per unit kind, the worst own-scale deviation of the kernels over the checked units next to the
yardstick's ("[figure] ...").  Measured on an MI355X, worst over the four inputs and both functionals (bar 5.0e-05):

  whole model         dx1      dx2  dvalues   dv/row   dv/col dx1/inst dx2/inst  dv/inst
  fused            1.2e-05  2.2e-05  2.2e-05  1.1e-05  1.4e-05  6.9e-07  3.1e-07  4.1e-07
  generic          1.5e-05  1.8e-05  1.9e-05  1.2e-05  1.1e-05  6.1e-07  3.3e-07  4.5e-07
  generic (4, 16)  1.6e-05  1.7e-05  1.8e-05  1.3e-05  1.2e-05  5.8e-07  2.7e-07  4.5e-07
  generic (64,256) 1.5e-05  1.8e-05  1.9e-05  1.2e-05  1.1e-05  6.1e-07  3.3e-07  4.5e-07    (the default tiers below 32 M nonzeros)
  streamed         2.4e-05  1.6e-05  3.0e-05  8.2e-06  1.4e-05  6.7e-07  2.6e-06  6.3e-07
  tiled            2.2e-05  1.9e-05  2.4e-05  1.1e-05  1.2e-05  8.5e-07  2.2e-06  7.7e-07
  yardstick        6.2e-06  6.2e-06  6.2e-06  6.2e-06  6.2e-06  1.6e-06  2.1e-06  1.7e-06

  one conv         dx_src/row  dx_dst/row       (grid0 and MIX, gconv2_w2s and gconv2_s2w)
  generic             5.9e-07     6.4e-07       the same at (4, 16)
  streamed 1 / 2 / 3  3.7e-06 / 3.3e-06 / 5.9e-07     9.1e-07 / 6.4e-07 / 8.6e-07
  tiled 1 / 2 / 4     2.3e-06 / 3.3e-06 / 5.9e-07     6.9e-07 / 6.4e-07 / 9.2e-07
  yardstick           5.1e-06     2.1e-06

The per-element figures of the kernels are two to five times the yardstick's worst checked unit (which is the threshold,
RTOL_GRAD / 8, by construction) and at most 0.6 of the bar; per row, per column and per instance there is a factor of four
and more.  No kernel was found wrong.  With the edge list alone permuted (no channels) one checked edge of MIX failed on
the LDS-tiled configuration at 5.3e-05: tests/input_scales.py says why that was the yardstick's fault.
"""
import numpy as np
import pytest
import torch

import fused_cases as fc
import input_scales as isc
from input_scales import RTOL_GRAD, close
from mllp_amd import _lib
from mllp_amd.data import SUBSET5, load_packed
from oracle import pyg_restatement as o1
from test_input_grads import oracle_input_grads

gpu = pytest.mark.gpu

MIX = list(SUBSET5) + ["woodw.mps", "fit2p.mps", "80bau3b.mps", "pds-06.mps", "ken-11.mps"]
INPUTS = ["grid0", "grid1x2", "subset5", "mix"]
LINEAR_SEED = {"grid0": 30, "grid1x2": 31, "subset5": 21, "mix": 9}       # the seeds of tests/test_input_grads_fused.py
FUNCTIONALS = ["linear", "bce"]
FRESH_SEEDS = range(900, 906)                                              # disjoint from the yardstick's (isc.YARD_SEED + k)
CONVS = [("gconv2_w2s", True, 7), ("gconv2_s2w", False, 8)]                # name, dst_is_var, seed of the features
CONV_INPUTS = ["grid0", "mix"]


class Case:
    """one input under one functional: reference, units, scales, yardstick -- shared, never modified"""

    def __init__(self, flat, insts, fn):
        self.flat, self.insts, self.fn = flat, insts, fn
        self.lay = isc.Layout(insts)
        self.want = isc.model_reference(flat, insts, fn)
        self.scales = isc.unit_scales(self.want, self.lay)
        self.yard = isc.model_yardstick(flat, insts, fn, self.want, self.lay)

    def fp32(self, seed):
        return isc.model_grads_f32(self.flat, self.insts, self.fn, seed)

    def top(self, array):
        return float(np.abs(self.want[array]).max())


class Refs:
    def __init__(self, golden, subset5):
        self.flat = golden["weights_flat"]
        self.build = {"grid0": lambda: fc.grid_batch(0, 1), "grid1x2": lambda: fc.grid_batch(1, 2),
                      "subset5": lambda: list(subset5), "mix": lambda: load_packed(MIX)}
        self.insts, self.cases, self.convs = {}, {}, {}

    def input(self, name):
        if name not in self.insts:
            self.insts[name] = self.build[name]()
        return self.insts[name]

    def layout(self, name):
        if ("lay", name) not in self.insts:
            self.insts[("lay", name)] = isc.Layout(self.input(name))
        return self.insts[("lay", name)]

    def __call__(self, name, functional):
        if (name, functional) not in self.cases:
            insts = self.input(name)
            fn = isc.BCE(insts) if functional == "bce" else isc.Linear(sum(i.n for i in insts), LINEAR_SEED[name])
            self.cases[(name, functional)] = Case(self.flat, insts, fn)
        return self.cases[(name, functional)]

    def conv(self, name, conv):
        if (name, conv) not in self.convs:
            if "sd9" not in self.convs:
                self.convs["sd9"] = {k: v.numpy() for k, v in o1.init_state(9, torch.float64).items()}
            dst_is_var, seed = {c[0]: c[1:] for c in CONVS}[conv]
            self.convs[(name, conv)] = isc.ConvCase(self.input(name), self.convs["sd9"], conv, dst_is_var, seed)
        return self.convs[(name, conv)]


@pytest.fixture(scope="module")
def refs(golden, subset5):
    return Refs(golden, subset5)


def _report(what, table):
    print("\n" + "\n".join(isc.table_lines(what, table)))
    for kind, t in table.items():
        print(f"[figure] {what} | {kind}: deviation {t['dev']:.1e}, yardstick {t['yard']:.1e}")


def _share(mask):
    return float(np.mean(mask))


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the census of what today's check cannot see
# ---------------------------------------------------------------------------------------------------------------------
def test_blindness_census(refs):
    """The inputs are sharp cases: the shares of units below RTOL_GRAD of their array's maximum (invisible to `close`) and
    below 1e-2 of it, on the fp64 oracle alone.  An input that stops being one fails here."""
    below = lambda s, top, f: _share(s[s > 0] < f * top)
    g = refs("grid0", "linear")
    s2, sv = g.scales["dx2"], g.scales["dvalues"]
    assert below(s2, g.top(1), RTOL_GRAD) >= 0.25 and below(s2, g.top(1), 1e-2) >= 0.9
    assert below(sv, g.top(2), RTOL_GRAD) >= 0.2 and below(sv, g.top(2), 1e-2) >= 0.7
    rows = g.scales["dvalues per row"]
    assert below(rows, g.top(2), RTOL_GRAD) >= 0.01 and below(rows, g.top(2), 1e-2) >= 0.9
    gb = refs("grid0", "bce")
    assert below(gb.scales["dx2"], gb.top(1), RTOL_GRAD) >= 0.8
    m = refs("mix", "bce")
    si = m.scales["dvalues per instance"]
    assert si.max() / si.min() >= 100, "the per-instance scales of dvalues must span 100 x under BCE"
    assert (si < 1e-2 * si.max()).sum() >= 3
    c = refs.conv("grid0", "gconv2_w2s")
    ss = isc.unit_scales(c.want, c.lay)["dx_src per node row"]
    assert below(ss, ss.max(), RTOL_GRAD) >= 0.1 and below(ss, ss.max(), 1e-2) >= 0.9
    c = refs.conv("mix", "gconv2_s2w")
    ss = isc.unit_scales(c.want, c.lay)["dx_src per node row"]
    assert below(ss, ss.max(), 1e-2) >= 0.1


def test_blindness_census_of_the_full_netlib_batch(refs):
    """Netlib-97 under BCE with inv_batch 1 / 97, the input of the full-batch tests: a tenth of dx2 and a thirtieth of the
    edges are below the bound, and whole instances sit below 1e-2 of the maximum"""
    insts = load_packed()
    assert len(insts) == 97
    _, dx1, dx2, dv, _ = oracle_input_grads(refs.flat, insts, isc.BCE(insts))
    lay = isc.Layout(insts)
    s2, sv = np.abs(dx2), np.abs(dv)
    assert _share(s2[s2 > 0] < RTOL_GRAD * s2.max()) >= 0.10
    assert _share(sv[sv > 0] < RTOL_GRAD * sv.max()) >= 0.03 and _share(sv[sv > 0] < 1e-2 * sv.max()) >= 0.9
    si = isc.unit_scales([dx1, dx2, dv], lay)["dvalues per instance"]
    small = [lay.names[k] for k in np.flatnonzero(si < 1e-2 * si.max())]
    assert len(small) >= 10 and {"pds-06.mps", "ken-11.mps", "fit2p.mps"} <= set(small), small


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the rule is sturdy (fresh fp32 orders pass it) and the caps hold
# ---------------------------------------------------------------------------------------------------------------------
def test_an_order_is_the_same_function(refs, subset5):
    """an order of the yardstick (edge list and hidden channels permuted) computes the oracle's gradients exactly: in fp64
    it differs from the natural order by rounding alone, and in fp32 it does differ (it is another sample)"""
    fn = isc.BCE(subset5)
    want = isc.model_reference(refs.flat, subset5, fn)
    for seed in (isc.YARD_SEED + 1, FRESH_SEEDS[0]):
        got = isc.model_grads(refs.flat, subset5, fn, torch.float64, seed)
        for g, w in zip(got, want):
            close(g, w, 1e-13, f"order {seed} in fp64")
    a, b = isc.model_grads_f32(refs.flat, subset5, fn), isc.model_grads_f32(refs.flat, subset5, fn, isc.YARD_SEED + 1)
    short = np.flatnonzero((isc.Layout(subset5).row_deg <= 2))
    assert len(short) and (a[1][short] != b[1][short]).any(), "rows of one or two entries must see another order too"



@pytest.mark.parametrize("functional", FUNCTIONALS)
@pytest.mark.parametrize("name", INPUTS)
def test_fresh_fp32_orders_pass_the_rule(refs, name, functional):
    """The float32 oracle under six orders of summation that the yardstick has not seen, as the "kernel": nothing fails, on
    every input of the GPU part.  The arbiter of K_ORDERS and MARGIN."""
    c = refs(name, functional)
    isc.assert_caps(c.scales, c.yard, c.lay, f"{name} {functional}")
    worst = {}
    for seed in FRESH_SEEDS:
        t = isc.close_per_unit(c.fp32(seed), c.want, c.yard, c.lay, f"{name} {functional}, fp32 order {seed}")
        worst = {k: dict(t[k], dev=max(t[k]["dev"], worst.get(k, t[k])["dev"])) for k in t}
    _report(f"fresh fp32 orders, {name} {functional}", worst)
    assert all(t["checked"] > 0 for t in worst.values())


@pytest.mark.parametrize("conv", [c[0] for c in CONVS])
@pytest.mark.parametrize("name", CONV_INPUTS)
def test_fresh_fp32_orders_pass_the_rule_on_one_conv(refs, name, conv):
    c = refs.conv(name, conv)
    isc.assert_caps(isc.unit_scales(c.want, c.lay), c.yard, c.lay, f"{name} {conv}")
    worst = {}
    for seed in FRESH_SEEDS:
        t = isc.close_per_unit(c.f32(seed), c.want, c.yard, c.lay, f"{name} {conv}, fp32 order {seed}")
        worst = {k: dict(t[k], dev=max(t[k]["dev"], worst.get(k, t[k])["dev"])) for k in t}
    _report(f"fresh fp32 orders, {name} {conv}", worst)
    assert all(t["checked"] > 0 for t in worst.values())


# ---------------------------------------------------------------------------------------------------------------------
# CPU: mutations that today's check accepts and the rule rejects
# ---------------------------------------------------------------------------------------------------------------------
def _gap(c, got, kinds, what):
    """`got` passes the old check and breaks the rule in (at least) the unit kinds `kinds`"""
    assert isc.old_check_accepts(got, c.want), f"{what}: the old check must accept this mutation (the gap on record)"
    bad = isc.failures(got, c.want, c.yard, c.lay)
    assert bad, f"{what}: the rule must reject this mutation"
    hit = {b.split(":")[0] for b in bad}
    assert set(kinds) <= hit, f"{what}: rejected in {sorted(hit)}, expected {kinds}"
    with pytest.raises(AssertionError, match="own scale|exactly zero"):
        isc.close_per_unit(got, c.want, c.yard, c.lay, what)
    print(f"\n{what}: " + " | ".join(bad)[:1500])


def _kernel_like(c):
    """an unmutated result: the fp32 oracle in a fresh order, which passes both checks"""
    got = c.fp32(FRESH_SEEDS[0])
    assert isc.old_check_accepts(got, c.want) and not isc.failures(got, c.want, c.yard, c.lay)
    return got


def test_mutation_zeros_in_the_small_half_of_dx2(refs):
    c = refs("grid0", "linear")
    got = _kernel_like(c)
    small = np.abs(c.want[1]) < RTOL_GRAD * c.top(1)
    assert small.mean() >= 0.25
    got[1][small] = 0.0
    _gap(c, got, ["dx2"], "zeros in every dx2 element below 5e-5 of the max")


def test_mutation_zeros_in_the_tail_chunk_of_a_block_row(refs):
    """the last 768 entries (one block-tier step of the 16-channel sweeps) of the longest row of A^T, a variable of 6 145
    nonzeros: three quarters of them are below the global bar.  (The constraint rows of that length are not blind: their
    edges reach 0.2 of the maximum, and all but a handful are above the bar.)"""
    c = refs("grid0", "linear")
    got = _kernel_like(c)
    lay = c.lay
    T = fc.constants()["T1"][2]
    col = int(np.argmax(lay.col_deg))
    assert lay.col_deg[col] > T
    edges = np.flatnonzero(lay.var == col)[-768:]                  # ascending constraint ids: the order of the row of A^T
    assert len(edges) == 768
    hit = edges[np.abs(c.want[2][edges]) < RTOL_GRAD * c.top(2)]
    assert len(hit) >= 384
    got[2][hit] = 0.0
    _gap(c, got, ["dvalues"], f"zeros in {len(hit)} of the last 768 entries of column {col} ({lay.col_deg[col]} nonzeros)")


def test_mutation_a_large_instance_two_percent_off(refs):
    """pds-06 (63 220 nonzeros, the largest of MIX) under BCE: its dx1 and its dvalues are at 2e-3 of their arrays' maxima,
    so 2 % of them is below the old bar; the rule rejects both.  Its dx2 is at 1.4e-2 of the maximum (in no Netlib batch is a
    large instance's dx2 below 2.5e-3 of the largest: dx2 does not carry the factor 1 / degree), so there the old check
    sees 2 % too -- stated here as a fact, and the rule sees it as well."""
    c = refs("mix", "bce")
    got = _kernel_like(c)
    lay = c.lay
    k = lay.names.index("pds-06.mps")
    rel = [float(c.scales[f"{a} per instance"][k]) / c.top(w) for w, a in enumerate(isc.ARRAYS)]
    assert rel[0] < 0.9 * RTOL_GRAD / 0.02 and rel[2] < 0.9 * RTOL_GRAD / 0.02 and rel[1] < 2e-2, rel
    owners = (lay.inst_of_var, lay.inst_of_con, lay.inst_of_edge)
    for w in (0, 2):
        got[w][owners[w] == k] *= 1.02
    _gap(c, got, ["dx1", "dvalues", "dx1 per instance", "dvalues per instance", "dvalues per row", "dvalues per column"],
         f"dx1 and dvalues of pds-06 (at {rel[0]:.1e} and {rel[2]:.1e} of the maxima) scaled by 1.02")
    got[1][owners[1] == k] *= 1.02
    assert not isc.old_check_accepts(got, c.want)
    assert {"dx2", "dx2 per instance"} <= {b.split(":")[0] for b in isc.failures(got, c.want, c.yard, c.lay)}


def last_item_rows(deg, T):
    """Rows that sit alone in the last item of a tier list, where a tier's population is one more than a whole number of
    items (degree_grid(1)): the fused path sorts an instance's rows by degree, longest first and stably, so the last row
    of the group tier (items of 4 rows) and of the base tier (items of 16 / 64 rows) is the highest id of the tier's lowest
    degree.  Rows without nonzeros have no edges and are left out."""
    deg = np.asarray(deg)
    out = []
    for lo, hi, per_item in ((T[2], 1 << 30, 1), (T[1], T[2], 1), (T[0], T[1], 4), (-1, T[0], 16)):
        ids = np.flatnonzero((deg > lo) & (deg <= hi))
        assert per_item == 1 or len(ids) % per_item == 1, (lo, hi, len(ids))
        last = ids[deg[ids] == deg[ids].min()][-1]
        if deg[last] > 0:
            out.append(int(last))
    return out


def test_mutation_zeros_in_the_rows_alone_in_the_last_item_of_a_tier_list(refs):
    """degree_grid(1): the group and the base tier hold one row more than a whole number of items, in both orientations, and
    a wave or block row is an item of its own; the last item of each of the four lists holds one row.  These rows are NOT
    blind as wholes: their largest edges are at 5e-3 .. 0.2 of the array's maximum, so zeros in all their edges fail the old
    check too (asserted, as a fact about the input).  What the old check cannot see of them is every edge below the bar of
    the array: zeros there pass it, and the rule rejects them."""
    c = refs("grid1x2", "linear")
    lay, T = c.lay, fc.constants()["T16"]
    edges, m0, n0 = [], 0, 0
    for inst in c.insts:                                      # two instances, two partitions: every instance has its lists
        rdeg, cdeg = fc.degrees(inst)
        rows, cols = last_item_rows(rdeg, T), last_item_rows(cdeg, T)
        assert len(rows) >= 3 and len(cols) >= 3
        edges += [np.flatnonzero(lay.con == m0 + r) for r in rows] + [np.flatnonzero(lay.var == n0 + v) for v in cols]
        m0, n0 = m0 + inst.m, n0 + inst.n
    edges = np.unique(np.concatenate(edges))
    got = _kernel_like(c)
    got[2][edges] = 0.0
    assert not isc.old_check_accepts(got, c.want)
    assert {"dvalues", "dvalues per row", "dvalues per column"} <= {b.split(":")[0] for b in isc.failures(got, c.want, c.yard, c.lay)}
    got = _kernel_like(c)
    hit = edges[np.abs(c.want[2][edges]) < RTOL_GRAD * c.top(2)]
    assert len(hit) >= 100
    got[2][hit] = 0.0
    _gap(c, got, ["dvalues"], f"zeros in the {len(hit)} edges below the bar of the {len(edges)} edges of the rows and columns "
                              f"that are alone in a last item")


def test_mutation_zeros_in_the_small_source_rows_of_a_conv(refs):
    c = refs.conv("grid0", "gconv2_w2s")
    got = c.f32(FRESH_SEEDS[0])
    assert isc.old_check_accepts(got, c.want) and not isc.failures(got, c.want, c.yard, c.lay)
    s = np.abs(c.want[0]).max(axis=1)
    small = s < RTOL_GRAD * s.max()
    assert small.mean() >= 0.1
    got[0][small] = 0.0
    _gap(c, got, ["dx_src per node row"], f"zeros in {int(small.sum())} source rows below 5e-5 of the top")


def test_the_limit_of_the_rule_is_the_exempt_unit(refs):
    """2 x RTOL_GRAD of ITS OWN scale added to one unit: a checked unit fails the rule (and passes the old check); an exempt
    unit passes both, and only an error of the array's scale is caught there -- by the global bound, as before."""
    c = refs("grid0", "bce")
    chk, _, ex = isc.classify(c.scales, c.yard)["dvalues"]
    s, top = c.scales["dvalues"], c.top(2)
    small = s < 1e-3 * top
    u = int(np.flatnonzero(chk & small)[0])
    got = [a.copy() for a in c.want]
    got[2][u] += 2 * RTOL_GRAD * s[u]
    _gap(c, got, ["dvalues"], "a checked edge off by 2 x RTOL_GRAD of itself")
    v = int(np.flatnonzero(ex & small & (s > 0))[0])
    got = [a.copy() for a in c.want]
    got[2][v] += 2 * RTOL_GRAD * s[v]
    assert isc.old_check_accepts(got, c.want) and not isc.failures(got, c.want, c.yard, c.lay)
    isc.close_per_unit(got, c.want, c.yard, c.lay, "an exempt edge off by 2 x RTOL_GRAD of itself")
    got[2][v] = c.want[2][v] + 2 * RTOL_GRAD * top
    assert not any(b.startswith("dvalues:") for b in isc.failures(got, c.want, c.yard, c.lay))     # not as an edge
    assert not isc.old_check_accepts(got, c.want)                  # an error of that size: the global bound, as before
    with pytest.raises(AssertionError):
        isc.close_per_unit(got, c.want, c.yard, c.lay, "an exempt edge off by 2 x RTOL_GRAD of the maximum")


def test_zero_units_demand_zeros(refs):
    """80bau3b's columns without nonzeros: dvalues per column has no edges there (zero in every order), and a dx2 of an empty
    row of the grid is a zero unit or an exempt one by the fp32 orders alone"""
    c = refs("mix", "linear")
    _, zero, _ = isc.classify(c.scales, c.yard)["dvalues per column"]
    assert zero.sum() >= 127
    g = refs("grid0", "linear")
    chk, zero, ex = isc.classify(g.scales, g.yard)["dx2"]
    assert zero.sum() > 0 and (g.lay.row_deg[zero] == 0).all()
    got = [a.copy() for a in g.want]
    got[1][np.flatnonzero(zero)[0]] = 1e-30
    bad = isc.failures(got, g.want, g.yard, g.lay)
    assert len(bad) == 1 and "exactly zero" in bad[0]


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the whole model
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def LPBatch():
    _lib.lib()                      # fail loudly: no fallback
    assert torch.cuda.is_available()
    from mllp_amd.graph import LPBatch as cls
    return cls


@pytest.fixture(scope="module")
def flat_gpu(golden):
    return torch.tensor(golden["weights_flat"], dtype=torch.float32, device="cuda")


MODEL_CONFIGS = ["fused", "generic", "generic-4-16", "generic-64-256", "streamed", "tiled"]


def empty_tail_chunks(deg, tier_block):
    """host_build_tiers restated: a row above 4 * tier_block nonzeros is split into nck chunks of equal shares rounded up to
    whole passes of 256 nonzeros, so its last chunks can be empty.  Returns (split rows, empty chunks)."""
    chunk = 4 * tier_block
    rows = empty = 0
    for d in np.asarray(deg)[np.asarray(deg) > chunk].tolist():
        nck = -(-d // chunk)
        per = (-(-d // nck) + 255) & ~255
        rows += 1
        empty += sum(c * per >= d for c in range(nck))
    return rows, empty


def _forced_tiers(LPBatch, insts, lay, tw, tb, demand_split):
    """a batch under forced row tiers; dims() must report the split rows of the restatement, in both orientations"""
    b = LPBatch.from_instances(insts, tier_wave=tw, tier_block=tb)
    d = b.dims()
    for o, deg in (("A", lay.row_deg), ("At", lay.col_deg)):
        rows, empty = empty_tail_chunks(deg, tb)
        assert d[f"{o}_split"] == rows, (o, d, rows)
        assert not demand_split or (rows > 0 and empty > 0 and d[f"{o}_block"] > 0 and d[f"{o}_wave"] > 0), (o, d, rows, empty)
    return b


def _model_batch(LPBatch, insts, lay, config):
    if config.startswith("generic-"):
        tw, tb = (int(v) for v in config.split("-")[1:])
        # at (4, 16) rows above 64 nonzeros are split and rows of 65 .. 256 end in an empty chunk; the golden five have none
        b = _forced_tiers(LPBatch, insts, lay, tw, tb, demand_split=(tb == 16 and max(lay.row_deg.max(), lay.col_deg.max()) > 64))
    else:
        b = LPBatch.from_instances(insts)
    if config == "streamed":
        info = b.enable_stream_step(max_slots_per_nnz=1e9)
        assert not any(v.get("dropped") for v in info.values()) and all(v["n_tiles"] > 0 for v in info.values())
    if config == "tiled":
        info = b.enable_tiled_step()
        assert all(v is not None for v in info.values()), info
    b.set_path(2 if config == "fused" else 1)
    return b


@gpu
@pytest.mark.parametrize("name", INPUTS)
@pytest.mark.parametrize("config", MODEL_CONFIGS)
def test_model_input_grads_unit_by_unit(LPBatch, refs, flat_gpu, config, name):
    """One batch; the linear functional through forward + input_grads (fused) or backward_inputs (generic), and BCE through
    loss_step_inputs -- each held to the oracle unit by unit."""
    lin, bce = refs(name, "linear"), refs(name, "bce")
    for c in (lin, bce):
        isc.assert_caps(c.scales, c.yard, c.lay, f"{name}")           # before any result is looked at
    b = _model_batch(LPBatch, lin.insts, lin.lay, config)
    r = lin.fn.r.float().cuda()
    b.forward(flat_gpu)
    out = b.input_grads(flat_gpu, r) if config == "fused" else b.backward_inputs(flat_gpu, r)
    got_lin = [t.cpu().numpy() for t in out[1:]]
    got_bce = [t.cpu().numpy() for t in b.loss_step_inputs(flat_gpu)[3:]]
    for fname, c, got in (("linear", lin, got_lin), ("bce", bce, got_bce)):
        what = f"{config} {name} {fname}"
        _report(what, isc.table_of(isc._f64(got), c.want, c.yard, c.lay))           # every figure, before anything is asserted
        isc.close_per_unit(got, c.want, c.yard, c.lay, what)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: one conv
# ---------------------------------------------------------------------------------------------------------------------
CONV_CONFIGS = ["generic", "generic-4-16", "streamed-1", "streamed-2", "streamed-3", "tiled-1", "tiled-2", "tiled-4"]


def _conv_batch(LPBatch, insts, lay, config, dst_is_var):
    """The copy a configuration attaches, on the orientation the sweep that uses it walks: the forward (streamed 1, tiled 1)
    and the destination-major backward (streamed 3, tiled 4) walk the conv's own orientation, the source-major backward
    (streamed 2, tiled 2) the other one."""
    kind, _, arg = config.partition("-")
    if kind == "generic" and arg:
        tw, tb = (int(v) for v in arg.split("-"))
        b = _forced_tiers(LPBatch, insts, lay, tw, tb, demand_split=True)
    else:
        b = LPBatch.from_instances(insts)
    b.set_path(1)
    tr = bool(dst_is_var) if arg != "2" else not dst_is_var
    if kind == "streamed":
        info = b.build_stream_copy(tr, int(arg))
        assert info["n_tiles"] > 0 and info["entry_slots"] >= b.nnz, info
    if kind == "tiled":
        assert b.enable_tiled(tr, variant=int(arg)) is not None
    return b


@gpu
@pytest.mark.parametrize("conv,dst_is_var", [c[:2] for c in CONVS])
@pytest.mark.parametrize("name", CONV_INPUTS)
@pytest.mark.parametrize("config", CONV_CONFIGS)
def test_conv_input_grads_row_by_row(LPBatch, refs, config, name, conv, dst_is_var):
    """mllp_tconv_fwd / mllp_tconv_bwd of one 16-channel conv: dx_src per source node row and dx_dst per destination node
    row, on the degree grid (which no per-layer test ran) and on the mixed Netlib batch"""
    c = refs.conv(name, conv)
    isc.assert_caps(isc.unit_scales(c.want, c.lay), c.yard, c.lay, f"{name} {conv}")
    b = _conv_batch(LPBatch, refs.input(name), refs.layout(name), config, dst_is_var)
    sd = {k: torch.tensor(v) for k, v in refs.convs["sd9"].items()}
    cp = o1.flatten_state(sd).float().cuda()[_lib.conv_param_slice(conv)].contiguous()
    dev = lambda a: torch.tensor(a, dtype=torch.float32, device="cuda")
    xs, xd, dh = dev(c.xs), dev(c.xd), dev(c.dh)
    ws = b.tconv_workspace(dst_is_var, 16)
    h = b.tconv_fwd(dst_is_var, 16, cp, xs, xd, ws)
    close(h.cpu().numpy(), c.h, 1e-5, f"{config} {name} {conv} h")
    _, dxd, dxs, _ = b.tconv_bwd(dst_is_var, 16, cp, xs, xd, h, ws, dh)
    got = [dxs.cpu().numpy(), dxd.cpu().numpy()]
    what = f"{config} {name} {conv}"
    _report(what, isc.table_of(isc._f64(got), c.want, c.yard, c.lay))
    isc.close_per_unit(got, c.want, c.yard, c.lay, what)


@gpu
@pytest.mark.parametrize("conv,dst_is_var", [("gconv1_w2s", True), ("gconv1_s2w", False)])
def test_one_channel_conv_on_the_grid_never_writes_dx(LPBatch, refs, conv, dst_is_var):
    """the layer-1 convs have no dx of their own (include/mllp_hip.h: with cin = 1 the dx pointers are never written; the
    model's input gradients are mllp_gnn_backward_inputs): on the degree grid the buffers handed over keep their bits"""
    insts = refs.input("grid0")
    b = LPBatch.from_instances(insts)
    b.set_path(1)
    nd, ns = (b.N, b.M) if dst_is_var else (b.M, b.N)
    rng = np.random.default_rng(3)
    dev = lambda a: torch.tensor(a, dtype=torch.float32, device="cuda")
    flat = o1.flatten_state(o1.init_state(9, torch.float64)).float().cuda()
    cp = flat[_lib.conv_param_slice(conv)].contiguous()
    xs, xd, dh = dev(rng.standard_normal((ns, 1))), dev(rng.standard_normal((nd, 1))), dev(rng.standard_normal((nd, 16)))
    ws = b.tconv_workspace(dst_is_var, 1)
    h = b.tconv_fwd(dst_is_var, 1, cp, xs, xd, ws)
    SENT = -12345.0
    dxd, dxs = torch.full((nd,), SENT, device="cuda"), torch.full((ns,), SENT, device="cuda")
    pg = torch.full((cp.numel(),), float("nan"), device="cuda")
    p = _lib.ptr
    for acc in (0, 3):
        dh_k = dh.clone()                      # the call overwrites it with the masked gradient
        _lib.check(_lib.lib().mllp_tconv_bwd(b._h, int(dst_is_var), 1, p(cp), p(xs), p(xd), p(h), p(ws), p(dh_k), p(dxd),
                                             p(dxs), acc, p(pg), _lib.current_stream()))
        torch.cuda.synchronize()
        assert (dxd == SENT).all() and (dxs == SENT).all(), f"accumulate = {acc}"
        assert torch.isfinite(pg).all()
