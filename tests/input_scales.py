"""Input gradients compared unit by unit, each on its own scale (test infrastructure, no GPU needed).

`close` of tests/test_input_grads.py divides one maximum error by one maximum reference value per output array.  An edge's
gradient scales with its attention weight (about 1 / degree) and a BCE dz with 1 / n_k, so the rows that sit alone in the
last item of a tier list, the tail chunk of a split row and the large instances of a mixed batch are orders of magnitude
below the array's maximum: a bound of RTOL_GRAD * max|g| is more than all of them.  tests/grad_scales.py removed this for
the 56 parameter tensors; here the same rule holds the per-node and per-edge outputs, in UNITS:

  whole model   every element of dx1 [N], of dx2 [M], every edge of dvalues [nnz]; dvalues per constraint row and per column
                (scale = max|want| over the unit, error = max|got - want| over the unit); each array per instance
  one conv      dx_src per source node row, dx_dst per destination node row (max over the 16 channels)

Yardstick: what fp32 can deliver.  The same oracle computation in float32 under K_ORDERS summation orders; a unit's
yardstick is its worst deviation from the fp64 result over the orders.  Whole model: autograd through
oracle.pyg_restatement.gnn_forward on float32 tensors, order 0 the natural edge order, the others seeded random
permutations of the edge list (tests/test_oracle.py::test_edge_permutation_invariance vouches for the invariance) AND of
the 16 hidden channels of every layer (`permuted_channels`; exact in fp64, tests/test_input_scales.py checks it).  One
conv: fused_cases._fwd_dt / _bwd_dt in np.float32 with the entries permuted inside their rows.

Why the channels too.  Permuting the edge list reorders the sums over a node's edges, and a row of one or two entries has
nothing to reorder: all eight edge orders gave such a unit the same fp32 value, one sample instead of eight, and whether
it came out checked or exempt was the luck of that sample.  Found on the MI355X: an edge of pds-06 (row and column of two
entries, 8e-4 of the array's maximum) sat at 2.6e-6 of itself in all eight orders on one host and at 1.7e-5 in all eight on
another (the hosts' fp32 matrix products differ), and the kernels were 5.3e-5 off it, against 2.9e-5 .. 3.9e-5 for their
worst unit otherwise.  With the channels permuted the orders disagree on such units, they are exempt, and the kernels'
worst checked unit is at 3.0e-5.

A unit is CHECKED where its yardstick is below RTOL_GRAD / MARGIN of its own scale, and must then be within RTOL_GRAD of its
own scale.  Otherwise it is EXEMPT (ill-conditioned on this input: the fp32 reference misses it too) and stays under the
array's global bound.  A unit whose reference is exactly zero (an empty row) has no scale: where every fp32 order gives an
exact zero the kernel must write zero, otherwise the unit is exempt.  Exemption comes from the yardstick alone, never from
the result under test, and `assert_caps` bounds the exempt share of every unit kind before a result is looked at.

No tolerance is introduced: the bar is RTOL_GRAD of tests/test_input_grads.py.  K_ORDERS = 8 and MARGIN = 8 were measured:
with one order and a margin of 4 (the rule of grad_scales) a second fp32 order broke the bar on up to 185 checked units of
Netlib-97; with 8 and 8 the worst of six further orders stays below the bar on every input
(tests/test_input_scales.py::test_fresh_fp32_orders_pass_the_rule is the arbiter).
"""
import numpy as np
import torch

import fused_cases as fc
from oracle import pyg_restatement as o1
from oracle import spmm_form as o2
from test_input_grads import RTOL_GRAD, close, oracle_input_grads

K_ORDERS = 8
MARGIN = 8
YARD_SEED = 100                   # orders 1 .. K_ORDERS - 1 are the permutations of seeds YARD_SEED + k; fresh orders: other seeds
CAP_ELEMENT, CAP_ROW, CAP_INSTANCES, CAP_NODE_ROW = 0.20, 0.05, 2, 0.05
ARRAYS = ("dx1", "dx2", "dvalues")


# ---------------------------------------------------------------------------------------------------------------------
# functionals of the logits, usable in either floating-point type
# ---------------------------------------------------------------------------------------------------------------------
class Linear:
    """L = sum_i r_i z_i with the r of tests/test_input_grads_fused.py (a seeded standard normal vector)"""

    def __init__(self, n, seed):
        self.r = torch.randn(n, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)

    def __call__(self, z):
        return (z.reshape(-1) * self.r.to(z.dtype)).sum()


class BCE:
    """L = inv_batch * sum_k mean_i BCE(z_i, y_i) over the instances k: what mllp_gnn_loss_step_inputs differentiates"""

    def __init__(self, insts, inv_batch=None):
        self.off = np.concatenate([[0], np.cumsum([i.n for i in insts])])
        self.y = [torch.tensor(np.asarray(i.basis), dtype=torch.float64) for i in insts]
        self.inv_batch = 1.0 / len(insts) if inv_batch is None else inv_batch

    def __call__(self, z):
        z = z.reshape(-1)
        return self.inv_batch * sum(torch.nn.functional.binary_cross_entropy_with_logits(
            z[self.off[k]:self.off[k + 1]], y.to(z.dtype)) for k, y in enumerate(self.y))


# ---------------------------------------------------------------------------------------------------------------------
# units of a block-diagonal batch
# ---------------------------------------------------------------------------------------------------------------------
class Layout:
    """Who owns what in the batch of `insts`: constraint row, column and instance of every edge (CSR order of A), instance
    of every node, the degrees."""

    def __init__(self, insts):
        self.names = [i.name for i in insts]
        self.inst_m, self.inst_n = np.array([i.m for i in insts]), np.array([i.n for i in insts])
        self.M, self.N, self.nnz = int(self.inst_m.sum()), int(self.inst_n.sum()), int(sum(i.nnz for i in insts))
        k = np.arange(len(insts))
        self.inst_of_var, self.inst_of_con = np.repeat(k, self.inst_n), np.repeat(k, self.inst_m)
        n_off = np.concatenate([[0], np.cumsum(self.inst_n)])
        self.row_deg = np.concatenate([np.diff(i.indptr) for i in insts]).astype(np.int64)
        self.con = np.repeat(np.arange(self.M), self.row_deg)
        self.var = (np.concatenate([i.indices.astype(np.int64) + n_off[j] for j, i in enumerate(insts)])
                    if self.nnz else np.zeros(0, np.int64))
        self.col_deg = np.bincount(self.var, minlength=self.N).astype(np.int64)
        self.inst_of_edge = self.inst_of_con[self.con]
        # kind -> (array, group key of every element or None, number of units, cap class)
        self.kinds = {"dx1": (0, None, self.N, "element"), "dx2": (1, None, self.M, "element"),
                      "dvalues": (2, None, self.nnz, "element"),
                      "dvalues per row": (2, self.con, self.M, "row"), "dvalues per column": (2, self.var, self.N, "row"),
                      "dx1 per instance": (0, self.inst_of_var, len(insts), "instance"),
                      "dx2 per instance": (1, self.inst_of_con, len(insts), "instance"),
                      "dvalues per instance": (2, self.inst_of_edge, len(insts), "instance")}

    def describe(self, kind, u):
        """where a unit sits: its instance and the degree of its row"""
        u = int(u)
        if kind == "dx1" or kind == "dvalues per column":
            return f"column {u} of {self.names[self.inst_of_var[u]]}, degree {self.col_deg[u]}"
        if kind == "dx2" or kind == "dvalues per row":
            return f"row {u} of {self.names[self.inst_of_con[u]]}, degree {self.row_deg[u]}"
        if kind == "dvalues":
            r, c = int(self.con[u]), int(self.var[u])
            first = int(np.searchsorted(self.con, r))
            return (f"edge {u} (row {r}, degree {self.row_deg[r]}, entry {u - first}; column {c}, degree {self.col_deg[c]}) "
                    f"of {self.names[self.inst_of_edge[u]]}")
        return f"instance {u} ({self.names[u]}, {self.inst_m[u]} x {self.inst_n[u]})"


class NodeRows:
    """Units of one conv's outputs: the node rows of dx_src [n_src, 16] and dx_dst [n_dst, 16]"""

    def __init__(self, n_src, n_dst, src_deg, dst_deg):
        self.src_deg, self.dst_deg = np.asarray(src_deg), np.asarray(dst_deg)
        self.kinds = {"dx_src per node row": (0, None, n_src, "node row"), "dx_dst per node row": (1, None, n_dst, "node row")}

    def describe(self, kind, u):
        deg = self.src_deg if kind.startswith("dx_src") else self.dst_deg
        return f"node row {int(u)}, degree {deg[int(u)]}"


def _groupmax(a, key, n):
    if a.ndim == 2:                    # a node row of a conv output: the max over its 16 channels
        a = a.max(axis=1)
    if key is None:
        return a
    out = np.zeros(n)
    np.maximum.at(out, key, a)
    return out


def unit_scales(want, lay):
    """{kind: max|want| over every unit}"""
    return {k: _groupmax(np.abs(want[w]), key, n) for k, (w, key, n, _) in lay.kinds.items()}


def unit_errors(got, want, lay):
    """{kind: max|got - want| over every unit}"""
    return {k: _groupmax(np.abs(got[w] - want[w]), key, n) for k, (w, key, n, _) in lay.kinds.items()}


def _f64(arrays):
    return [np.asarray(a, np.float64) for a in arrays]


# ---------------------------------------------------------------------------------------------------------------------
# the fp32 oracle under an order of summation
# ---------------------------------------------------------------------------------------------------------------------
# what feeds a conv's source side (lin_key, lin_value) and its destination side (lin_query, lin_skip): o1.gnn_forward
_CONV_INPUTS = {"gconv1_w2s": (None, None), "gconv1_s2w": (None, None), "gconv2_w2s": ("gconv1_s2w", "gconv1_w2s"),
                "gconv2_s2w": ("gconv1_w2s", "gconv1_s2w"), "gconv3_w2s": ("gconv2_s2w", "gconv2_w2s")}


def permuted_channels(sd, seed):
    """The same function of the inputs with the 16 hidden channels of every layer renumbered (one seeded permutation per
    conv): every sum over channels -- the query-key products, the next layer's projections, fc -- adds its terms in another
    order.  Permuting the edge list reorders the sums over a node's EDGES only, which for a row of one or two entries is
    no reordering at all; this reorders what such a row is made of."""
    g = torch.Generator().manual_seed(seed)
    pi = {c: torch.randperm(o1.FEAT, generator=g) for c in _CONV_INPUTS}
    out = dict(sd)
    for c, (src, dst) in _CONV_INPUTS.items():
        for lin, side in (("lin_key", src), ("lin_value", src), ("lin_query", dst), ("lin_skip", dst), ("lin_edge", None)):
            w = sd[f"{c}.{lin}.weight"][pi[c]]
            out[f"{c}.{lin}.weight"] = w if side is None else w[:, pi[side]]
            if lin != "lin_edge":
                out[f"{c}.{lin}.bias"] = sd[f"{c}.{lin}.bias"][pi[c]]
    out["fc.weight"] = sd["fc.weight"][:, pi["gconv3_w2s"]]
    return out


def model_grads(flat, insts, loss_fn, dt, seed=None):
    """(dx1, dx2, dvalues in CSR order) of autograd through o1.gnn_forward in the type dt; seed: the edge list permuted by
    torch.randperm of that seed and the hidden channels by permuted_channels (None: everything in its natural order)"""
    sd = {k: v.detach().to(dt) for k, v in o1.unflatten_state(torch.tensor(flat)).items()}
    ei, x1, x2, ea = o1.batch_graphs([o1.instance_graph(i, torch.float32) for i in insts])
    x1, x2, ea = (t.to(dt).requires_grad_(True) for t in (x1, x2, ea))
    if seed is None:
        z = o1.gnn_forward(sd, ei, x1, x2, ea)
    else:
        perm = torch.randperm(ei.shape[1], generator=torch.Generator().manual_seed(seed))
        z = o1.gnn_forward(permuted_channels(sd, seed), ei[:, perm], x1, x2, ea[perm])
    g = torch.autograd.grad(loss_fn(z), [x1, x2, ea])
    return [t.reshape(-1).double().numpy() for t in g]


def model_grads_f32(flat, insts, loss_fn, seed=None):
    return model_grads(flat, insts, loss_fn, torch.float32, seed)


def model_reference(flat, insts, loss_fn):
    """the fp64 oracle of tests/test_input_grads.py: [dx1, dx2, dvalues], read-only"""
    want = _f64(oracle_input_grads(flat, insts, loss_fn)[1:4])
    for a in want:
        a.setflags(write=False)
    return want


def model_yardstick(flat, insts, loss_fn, want, lay, orders=K_ORDERS):
    """{kind: every unit's worst absolute deviation of the fp32 oracle from `want` over the orders}"""
    yard = None
    for k in range(orders):
        e = unit_errors(model_grads_f32(flat, insts, loss_fn, YARD_SEED + k if k else None), want, lay)
        yard = e if yard is None else {u: np.maximum(yard[u], e[u]) for u in e}
    for a in yard.values():
        a.setflags(write=False)
    return yard


def _row_order(ptr, rng):
    """a permutation of the entries that keeps every entry in its row"""
    rows = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    return np.lexsort((rng.random(len(rows)), rows))


def conv_f32(p, ptr, idx, val, xs, xd, dh, seed=None):
    """(dx_src, dx_dst) of fused_cases._fwd_dt / _bwd_dt in np.float32; seed: entries permuted inside their rows"""
    dt = np.float32
    if seed is not None:
        o = _row_order(ptr, np.random.default_rng(seed))
        idx, val = idx[o], val[o]
    p32 = {k: np.asarray(v, dt) for k, v in p.items()}
    a = lambda x: np.asarray(x, dt)
    h, sv = fc._fwd_dt(p32, ptr, idx, a(val), a(xs), a(xd), dt)
    _, dxd, dxs = fc._bwd_dt(p32, ptr, idx, a(val), a(xs), a(xd), sv, a(dh), dt)
    assert dxd.dtype == dt and dxs.dtype == dt
    return dxs.astype(np.float64), dxd.astype(np.float64)


class ConvCase:
    """One 16-channel TransformerConv on a batch, as tests/test_stream_attn.py::_layer_case draws it: the inputs, the fp64
    oracle (o2.conv_fwd / conv_bwd), the node-row units and their fp32 yardstick."""

    def __init__(self, insts, sd, name, dst_is_var, seed, orders=K_ORDERS):
        ob = o2.BatchCSR(insts)
        rng = np.random.default_rng(seed)
        self.name, self.dst_is_var = name, dst_is_var
        self.p = o2.conv_params(sd, name)
        self.ptr, self.idx, val, nd, ns = ob.orient(dst_is_var)
        r32 = lambda a: a.astype(np.float32).astype(np.float64)
        self.val = r32(val)
        self.xs, self.xd, self.dh = (r32(rng.standard_normal((n, 16))) for n in (ns, nd, nd))
        self.h, saved = o2.conv_fwd(self.p, self.ptr, self.idx, self.val, self.xs, self.xd)
        _, dxd, dxs, _ = o2.conv_bwd(self.p, self.ptr, self.idx, self.val, self.xs, self.xd, saved, self.dh)
        self.lay = NodeRows(ns, nd, np.bincount(self.idx, minlength=ns), np.diff(self.ptr))
        self.want = [dxs, dxd]
        for a in self.want:
            a.setflags(write=False)
        self.yard = None
        for k in range(orders):
            e = unit_errors(self.f32(YARD_SEED + k if k else None), self.want, self.lay)
            self.yard = e if self.yard is None else {u: np.maximum(self.yard[u], e[u]) for u in e}

    def f32(self, seed):
        return conv_f32(self.p, self.ptr, self.idx, self.val, self.xs, self.xd, self.dh, seed)


# ---------------------------------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------------------------------
def classify(scales, yard):
    """{kind: (checked, zero, exempt)} boolean arrays over the units, from the reference and the yardstick alone.
    checked: a scale of its own and a yardstick below RTOL_GRAD / MARGIN of it; zero: reference and every fp32 order exactly
    zero (zeros are demanded); exempt: the rest."""
    out = {}
    for k, s in scales.items():
        y = yard[k]
        live = s > 0
        checked = live & (y < (RTOL_GRAD / MARGIN) * s)
        zero = ~live & (y == 0)
        out[k] = (checked, zero, ~checked & ~zero)
    return out


def exempt_shares(scales, yard, lay):
    """{kind: (exempt units, units, cap class)}"""
    return {k: (int(ex.sum()), len(ex), lay.kinds[k][3]) for k, (_, _, ex) in classify(scales, yard).items()}


def assert_caps(scales, yard, lay, what=""):
    """the caps on the exempt share: conditions on the input, asserted before a result is looked at"""
    bad = []
    for k, (n_ex, n, cls) in exempt_shares(scales, yard, lay).items():
        if cls == "instance":
            ok, cap = n_ex <= CAP_INSTANCES, f"{CAP_INSTANCES} instances"
        else:
            share = {"element": CAP_ELEMENT, "row": CAP_ROW, "node row": CAP_NODE_ROW}[cls]
            ok, cap = n_ex <= share * n, f"{share:.0%}"
        if not ok:
            bad.append(f"{k}: {n_ex} of {n} units exempt, cap {cap}")
    assert not bad, f"{what}: the fp32 yardstick exempts too much of this input: " + "; ".join(bad)


def _top(want, w):
    a = np.abs(want[w])
    return max(float(a.max()), 1e-30) if a.size else 1e-30


def table_of(got, want, yard, lay):
    """{kind: dict(units, checked, zero, exempt, blind (scale below RTOL_GRAD of the array's max), yard, dev)}: yard and dev
    are the worst own-scale figures of the yardstick and of `got` over the CHECKED units"""
    scales, errs = unit_scales(want, lay), unit_errors(got, want, lay)
    out = {}
    for k, (chk, zero, ex) in classify(scales, yard).items():
        s, top = scales[k], _top(want, lay.kinds[k][0])
        rel = lambda e: float((e[chk] / s[chk]).max()) if chk.any() else 0.0
        out[k] = dict(units=len(s), checked=int(chk.sum()), zero=int(zero.sum()), exempt=int(ex.sum()),
                      blind=int(((s > 0) & (s < RTOL_GRAD * top)).sum()), yard=rel(yard[k]), dev=rel(errs[k]))
    return out


def table_lines(what, table):
    lines = [f"[per unit] {what}: kind, units, checked, zero, exempt, below {RTOL_GRAD:.0e} of the array's max, "
             f"worst yardstick, worst deviation (own scale, checked units)"]
    for k, t in table.items():
        lines.append(f"  {k:22s} {t['units']:8d} {t['checked']:8d} {t['zero']:6d} {t['exempt']:7d} {t['blind']:8d} "
                     f"{t['yard']:9.2e} {t['dev']:9.2e}")
    return lines


def failures(got, want, yard, lay, worst=4):
    """messages of the unit kinds that break the rule: checked units at or above RTOL_GRAD of their own scale, zero units
    that are not zero"""
    scales, errs = unit_scales(want, lay), unit_errors(got, want, lay)
    bad = []
    for k, (chk, zero, _) in classify(scales, yard).items():
        s, e, top = scales[k], errs[k], _top(want, lay.kinds[k][0])
        rel = np.where(chk, e / np.where(s > 0, s, 1.0), 0.0)
        off = np.flatnonzero(chk & ~(rel < RTOL_GRAD))
        if len(off):
            show = off[np.argsort(-rel[off])[:worst]]
            units = "; ".join(f"{lay.describe(k, u)}: deviation {rel[u]:.2e} of its own scale, which is {s[u] / top:.1e} of "
                              f"the array's max, yardstick {yard[k][u] / s[u]:.1e}" for u in show)
            bad.append(f"{k}: {len(off)} of {int(chk.sum())} checked units at or above {RTOL_GRAD} of their own scale, worst: {units}")
        nz = np.flatnonzero(zero & (e != 0))
        if len(nz):
            bad.append(f"{k}: {len(nz)} units must be exactly zero (the reference and every fp32 order are), first: "
                       + "; ".join(lay.describe(k, u) for u in nz[:worst]))
    return bad


def close_per_unit(got, want, yard, lay, what=""):
    """The rule on a result.  got, want: the arrays of lay.kinds in order.  Returns table_of(); raises AssertionError that
    names every offending unit kind and its worst units."""
    got = _f64(got)
    for g, w in zip(got, want):
        assert g.shape == w.shape, what
        assert np.isfinite(g).all(), what
    scales = unit_scales(want, lay)
    assert_caps(scales, yard, lay, what)
    bad = failures(got, want, yard, lay)
    assert not bad, f"{what}: " + " | ".join(bad)
    for g, w, name in zip(got, want, ARRAYS if len(got) == 3 else ("dx_src", "dx_dst")):      # the exempt units too
        close(g, w, RTOL_GRAD, f"{what}: {name} on the scale of its maximum")
    return table_of(got, want, yard, lay)


def old_check_accepts(got, want):
    """what the suite asked before: every array within RTOL_GRAD of ITS maximum"""
    try:
        for g, w in zip(got, want):
            close(g, w, RTOL_GRAD)
    except AssertionError:
        return False
    return True
