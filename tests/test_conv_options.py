"""The options of mllp_tconv_bwd (include/mllp_hip.h): the two `accumulate` bits and the optional d_dx_dst / d_dx_src, on the
three implementations of the backward sweeps -- the generic sweeps over the plain CSR, the LDS-tiled copies and the
streamed copies -- and in both orientations.  Every other caller passes accumulate = 0 and both pointers or neither; the
whole-model backward passes 0 or 3 (3 for gconv2_s2w only, so the whole-model tests do see an accumulating kernel that
stops accumulating, but not which bit belongs to which buffer, nor a bit alone, nor one gradient without the other).
Here one TransformerConv's backward runs with accumulate in {0, 1, 2, 3} x {both, dst only, src only, neither} through
the C ABI.

The cell (accumulate = 0, both) is the ANCHOR: it is held to the fp64 oracle at the bars of
tests/test_hip_parity.py::test_single_layer_forward_backward (imported, not restated), and every other cell is compared
with it BIT FOR BIT: an accumulating call is one fp32 add of the buffer's prior content and the finished sum, so
`prior + anchor`, formed in numpy float32, is the expected content exactly.  No tolerance is introduced here.

The dx buffers start from a PRIOR without zeros and subnormals (so neither the sign of a zero nor a flushed subnormal can
excuse a difference), d_param_grads from NaN, d_dh from a saved copy; the workspace is the forward's and is never
refreshed between the calls.  With cin = 1 the dx pointers are "never computed here and never written": buffers given
anyway must keep the prior's bits.

Before anything is compared each test asserts that its batch reaches the kernels it is about (row tiers and split rows of
the generic sweeps in both orientations, tiles with several column blocks on the copies, no other copy in the way) and
prints what it found (-s shows it)."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import fused_cases as fc
from mllp_amd import _lib
from mllp_amd._lib import conv_param_slice
from mllp_amd.data import LPInstance
from oracle import pyg_restatement as o1
from oracle import spmm_form as o2
from test_hip_parity import RTOL_ACT, RTOL_GRAD, close

gpu = pytest.mark.gpu

TIER_WAVE, TIER_BLOCK = 4, 16            # the generic batch: rows of <= 4 entries per lane group, <= 16 per wavefront,
CHUNK = 4 * TIER_BLOCK                   # <= 64 one workgroup chunk, longer ones split over workgroups (host_graph.cpp)
IMPLS = ("generic", "tiled", "streamed")
CONVS16 = (("gconv2_w2s", 1), ("gconv2_s2w", 0))
CONVS1 = (("gconv1_w2s", 1), ("gconv1_s2w", 0))
KEYS = ("lin_key.weight", "lin_key.bias", "lin_query.weight", "lin_query.bias", "lin_value.weight", "lin_value.bias",
        "lin_edge.weight", "lin_skip.weight", "lin_skip.bias")
WANTS = {"both": (True, True), "dst": (True, False), "src": (False, True), "none": (False, False)}
CELLS = [(acc, want) for acc in (0, 1, 2, 3) for want in WANTS]
# the copies a conv's backward runs on: (transpose of the orientation, id) of the destination-major and of the source-major
# sweep -- destination = variables walks A^T (transpose 1) destination-major and A source-major
TILED_BDST, TILED_BSRC, TILED_SCALAR = 4, 2, 3
GEOM_BDST, GEOM_BSRC, GEOM_LANE1 = 3, 2, 4


def cell_name(acc, want):
    return f"acc{acc}-{want}"


# ---------------------------------------------------------------------------------------------------------------------
# the batch, its tiers restated on the host, the prior
# ---------------------------------------------------------------------------------------------------------------------
_DENSE21 = {i: 30 + 7 * i for i in range(0, 60, 3)}
_MEMO = {}


def column_heavy_instance():
    """The transposed pattern of ragged_instance(21, 400, 700, dense rows of 30 .. 429 entries): COLUMNS of that length."""
    src = fc.ragged_instance(21, 400, 700, _DENSE21)
    A = sp.csr_matrix((src.values, src.indices, src.indptr), shape=(src.m, src.n)).T.tocsr()
    A.sort_indices()
    rng = np.random.default_rng(77)
    return LPInstance("ragged21T", A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data.astype(np.float64),
                      rng.standard_normal(src.m), rng.random(src.n) * 5, (rng.random(src.m) < 0.37).astype(np.int32))


def instances():
    if "insts" not in _MEMO:
        _MEMO["insts"] = fc.ragged_batch() + [column_heavy_instance()]
    return _MEMO["insts"]


def oracle_batch():
    if "ob" not in _MEMO:
        _MEMO["ob"] = o2.BatchCSR(instances())
    return _MEMO["ob"]


def tier_census(ptr):
    """What mllp_graph_dims reports for one orientation at TIER_WAVE / TIER_BLOCK (host_graph.cpp::host_build_tiers)."""
    deg = np.diff(ptr)
    split = deg > CHUNK
    one_chunk = (deg > TIER_BLOCK) & ~split
    return dict(group=int((deg <= TIER_WAVE).sum()), wave=int(((deg > TIER_WAVE) & (deg <= TIER_BLOCK)).sum()),
                one_chunk=int(one_chunk.sum()), split=int(split.sum()),
                block=int(one_chunk.sum() + (-(-deg[split] // CHUNK)).sum()), empty=int((deg == 0).sum()))


def prior(n, seed):
    """standard_normal in fp32 with every element below 2^-8 in magnitude replaced by 1: no zero, no subnormal, and no sum
    of it with another float is subnormal (a nonzero fp32 sum with |p| >= 2^-8 is a multiple of 2^-32 at the least)."""
    p = np.random.default_rng(seed).standard_normal(n).astype(np.float32)
    p[np.abs(p) < 2.0 ** -8] = 1.0
    return p


def test_batch_has_every_tier_split_rows_and_holes_in_both_orientations():
    insts, ob = instances(), oracle_batch()
    assert {480, 481, 512, 513} <= {i.m for i in insts} and (3, 5) in {(i.m, i.n) for i in insts}
    assert any(i.nnz == 0 for i in insts)
    heavy = insts[-1]
    cols = np.bincount(heavy.indices, minlength=heavy.n)
    assert ((cols >= 70) & (cols <= 500)).sum() >= 3, "the added instance must have a few columns of 70 to 500 entries"
    for name, ptr in (("A", ob.rp), ("At", ob.cp)):
        c = tier_census(ptr)
        assert c["group"] > 0 and c["wave"] > 0 and c["one_chunk"] > 0 and c["split"] > 0 and c["empty"] > 0, (name, c)


def test_prior_has_no_zero_and_no_subnormal_and_the_cells_are_sixteen():
    p = prior(100000, 5)
    assert p.dtype == np.float32 and np.isfinite(p).all() and (np.abs(p) >= 2.0 ** -8).all() and (p == 1.0).any()
    assert len(CELLS) == 16 and len({cell_name(*c) for c in CELLS}) == 16 and CELLS[0] == (0, "both")


# ---------------------------------------------------------------------------------------------------------------------
# the three implementations, with their reach assertions
# ---------------------------------------------------------------------------------------------------------------------
def _tiled_info(b, transpose, variant):
    d = (ctypes.c_int64 * 5)()
    _lib.check(_lib.lib().mllp_graph_tiled_info(b._h, int(transpose), int(variant), d))
    return dict(n_tiles=int(d[0]), n_tb=int(d[1]), max_blocks=int(d[2]), owned=int(d[3]), max_run=int(d[4]))


def _no_copies(b, tiled=True, streamed=True):
    for tr in (0, 1):
        for v in (TILED_BSRC, TILED_SCALAR, TILED_BDST):
            assert not tiled or _tiled_info(b, tr, v)["n_tiles"] == 0
        for g in (GEOM_BSRC, GEOM_BDST, GEOM_LANE1):
            assert not streamed or b.stream_copy_info(bool(tr), g)["n_tiles"] == 0


def batch_of(impl):
    """One batch per implementation, built once: (batch, {what the reach assertions found})."""
    if impl in _MEMO:
        return _MEMO[impl]
    from mllp_amd.graph import LPBatch
    _lib.lib()                      # fail loudly: no fallback
    assert torch.cuda.is_available()
    saved, LPBatch.default_path = LPBatch.default_path, 1
    try:
        insts, reach = instances(), {}
        if impl == "generic":
            b = LPBatch.from_instances(insts, tier_wave=TIER_WAVE, tier_block=TIER_BLOCK)
            d, ob = b.dims(), oracle_batch()
            for name, ptr in (("A", ob.rp), ("At", ob.cp)):
                c = tier_census(ptr)
                got = {k: d[f"{name}_{k}"] for k in ("group", "wave", "block", "split")}
                assert got == {k: c[k] for k in got}, (name, got, c)
                assert min(got.values()) > 0 and c["one_chunk"] > 0 and c["empty"] > 0, (name, c)
                reach[name] = dict(c)
            assert d["A_split"] > 0 and d["At_split"] > 0
            _no_copies(b)
        elif impl == "tiled":
            b = LPBatch.from_instances(insts)
            for tr in (0, 1):
                for v in (TILED_BSRC, TILED_BDST, TILED_SCALAR):
                    assert b.enable_tiled(bool(tr), variant=v) is not None, (tr, v)      # mllp_graph_build_tiled
                    i = _tiled_info(b, tr, v)
                    assert i["n_tiles"] > 0 and i["owned"] == 1 and i["n_tb"] > i["n_tiles"] and i["max_blocks"] > 1, (tr, v, i)
                    reach[("At" if tr else "A", v)] = i
            _no_copies(b, tiled=False)
        else:
            b = LPBatch.from_instances(insts)
            for tr in (0, 1):
                for g in (GEOM_BSRC, GEOM_BDST, GEOM_LANE1):
                    i = b.build_stream_copy(bool(tr), g)
                    assert i["n_tiles"] > 0 and i["entry_slots"] >= b.nnz, (tr, g, i)
                    # (geometry 4 cuts a tile's columns into blocks of 20 000: one block per tile on any small batch)
                    assert g == GEOM_LANE1 or i["n_tb"] > i["n_tiles"], (tr, g, i)
                    reach[("At" if tr else "A", g)] = {k: i[k] for k in ("n_tiles", "n_tb", "entry_slots")}
            _no_copies(b, streamed=False)
        assert b.path == 1
    finally:
        LPBatch.default_path = saved
    print(f"\nreach[{impl}]: M {b.M} N {b.N} nnz {b.nnz}: {reach}")
    _MEMO[impl] = (b, reach)
    return _MEMO[impl]


def assert_reach(impl, reach, dst_is_var, cin):
    """the copies (or tiers) THIS conv's sweeps run on are there: the destination-major sweep walks A^T when the destinations
    are the variables, the source-major one the other orientation"""
    o_dst, o_src = ("At", "A") if dst_is_var else ("A", "At")
    if impl == "generic":
        used = [o_dst] + ([o_src] if cin == 16 else [])
        assert all(reach[o]["split"] > 0 and reach[o]["empty"] > 0 for o in used)
    elif impl == "tiled":
        used = [(o_dst, TILED_BDST), (o_src, TILED_BSRC)] if cin == 16 else [(o_dst, TILED_SCALAR)]
        assert all(reach[u]["n_tiles"] > 0 and reach[u]["max_blocks"] > 1 for u in used)
    else:
        used = [(o_dst, GEOM_BDST), (o_src, GEOM_BSRC)] if cin == 16 else [(o_dst, GEOM_LANE1)]
        assert all(reach[u]["n_tiles"] > 0 for u in used)
        assert cin == 1 or all(reach[u]["n_tb"] > reach[u]["n_tiles"] for u in used)
    return used


# ---------------------------------------------------------------------------------------------------------------------
# inputs, the fp64 oracle (once per conv), one conv on one batch
# ---------------------------------------------------------------------------------------------------------------------
def _sd9():
    if "sd9" not in _MEMO:
        sd = o1.init_state(9, torch.float64)
        _MEMO["sd9"] = ({k: v.numpy() for k, v in sd.items()}, o1.flatten_state(sd).float().numpy())
    return _MEMO["sd9"]


def inputs(name, dst_is_var, cin):
    """fp32 inputs of one conv and the fp64 oracle on them: computed on first use, shared, never modified"""
    if ("in", name) in _MEMO:
        return _MEMO[("in", name)]
    sd, flat = _sd9()
    ob = oracle_batch()
    ptr, idx, val, nd, ns = ob.orient(dst_is_var)
    rng = np.random.default_rng(300 + conv_param_slice(name).start)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)       # noqa: E731
    f64 = lambda a: a.astype(np.float64)                            # noqa: E731
    xs, xd, dh = f32(rng.standard_normal((ns, cin))), f32(rng.standard_normal((nd, cin))), f32(rng.standard_normal((nd, 16)))
    p = o2.conv_params(sd, name)
    val = f64(f32(val))                                             # the graph holds fp32 coefficients
    h_ref, saved = o2.conv_fwd(p, ptr, idx, val, f64(xs), f64(xd))
    grads, dxd, dxs, inter = o2.conv_bwd(p, ptr, idx, val, f64(xs), f64(xd), saved, f64(dh), need_input_grads=(cin == 16))
    r = dict(nd=nd, ns=ns, xs=xs, xd=xd, dh=dh, cp=f32(flat[conv_param_slice(name)]), h_ref=h_ref, g_ref=inter["g"],
             grads=grads, dxd_ref=dxd, dxs_ref=dxs, prior_d=prior(nd * cin, 11), prior_s=prior(ns * cin, 12))
    _MEMO[("in", name)] = r
    return r


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1).view(np.uint32)


def differ(got, want):
    """'' when two fp32 arrays hold the same bits, else how many words differ and the first of them"""
    g, w = bits(got), bits(want)
    bad = np.flatnonzero(g != w)
    if bad.size == 0:
        return ""
    k = int(bad[0])
    return f"{bad.size} of {g.size} words differ, first at {k}: {g[k]:#010x} != {w[k]:#010x}"


class Conv:
    """one conv on one batch: device inputs, the forward's workspace, and mllp_tconv_bwd with any options"""

    def __init__(self, b, name, dst_is_var, cin):
        self.b, self.dst_is_var, self.cin, self.I = b, int(dst_is_var), cin, inputs(name, dst_is_var, cin)
        I, dev = self.I, (lambda a: torch.tensor(a, dtype=torch.float32, device="cuda"))
        self.cp, self.xs, self.xd, self.dh0 = dev(I["cp"]), dev(I["xs"]), dev(I["xd"]), dev(I["dh"])
        self.prior_d, self.prior_s = dev(I["prior_d"]), dev(I["prior_s"])
        self.dxd, self.dxs = torch.empty_like(self.prior_d), torch.empty_like(self.prior_s)
        self.dh, self.pg = torch.empty_like(self.dh0), torch.empty_like(self.cp)
        self.h = torch.empty(I["nd"], 16, device="cuda", dtype=torch.float32)
        self.ws = b.tconv_workspace(dst_is_var, cin)
        p = _lib.ptr
        _lib.check(_lib.lib().mllp_tconv_fwd(b._h, self.dst_is_var, cin, p(self.cp), p(self.xs), p(self.xd), p(self.h),
                                             p(self.ws), _lib.current_stream()))
        torch.cuda.synchronize()
        self.h_bits = self.h.cpu().numpy()

    def bwd(self, acc, dst, src, refill=True):
        """d_dh restored, d_param_grads NaN, the dx buffers refilled with the prior (unless refill=False); the workspace is
        left as the previous call left it.  Returns host copies of every buffer."""
        self.dh.copy_(self.dh0)
        self.pg.fill_(float("nan"))
        if refill:
            self.dxd.copy_(self.prior_d)
            self.dxs.copy_(self.prior_s)
        p = _lib.ptr
        _lib.check(_lib.lib().mllp_tconv_bwd(self.b._h, self.dst_is_var, self.cin, p(self.cp), p(self.xs), p(self.xd),
                                             p(self.h), p(self.ws), p(self.dh), p(self.dxd) if dst else None,
                                             p(self.dxs) if src else None, int(acc), p(self.pg), _lib.current_stream()))
        torch.cuda.synchronize()
        return {k: getattr(self, k).cpu().numpy() for k in ("dh", "pg", "dxd", "dxs")}

    def check_oracle(self, out):
        """the bars of tests/test_hip_parity.py::test_single_layer_forward_backward"""
        I, nd, ns, cin = self.I, self.I["nd"], self.I["ns"], self.cin
        close(self.h_bits, I["h_ref"], RTOL_ACT, "h")
        close(out["dh"].reshape(nd, 16), I["g_ref"], 1e-7, "masked dh")
        if cin == 16:
            close(out["dxd"].reshape(nd, 16), I["dxd_ref"], RTOL_GRAD, "dx_dst")
            close(out["dxs"].reshape(ns, 16), I["dxs_ref"], RTOL_GRAD, "dx_src")
        pg, o3 = out["pg"], 0
        for key in KEYS:
            ref = np.asarray(I["grads"][key]).reshape(-1)
            if key == "lin_key.bias":
                assert np.abs(pg[o3:o3 + ref.size]).max() < 1e-5        # ~0 (noise)
            else:
                close(pg[o3:o3 + ref.size], ref, RTOL_GRAD, key)
            o3 += ref.size
        assert o3 == pg.size
        assert differ(self.h.cpu().numpy(), self.h_bits) == "", "d_h_out is an input of the backward"


# ---------------------------------------------------------------------------------------------------------------------
# cin = 16: the sixteen cells
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name,dst_is_var", CONVS16)
@pytest.mark.parametrize("impl", IMPLS)
def test_accumulate_bits_and_optional_outputs(impl, name, dst_is_var):
    b, reach = batch_of(impl)
    used = assert_reach(impl, reach, dst_is_var, 16)
    print(f"\n{impl} {name} (dst_is_var = {dst_is_var}): destination-major sweep on {used[0]}, source-major sweep on {used[1]}")
    c = Conv(b, name, dst_is_var, 16)
    I = c.I
    out = {cell: c.bwd(cell[0], *WANTS[cell[1]]) for cell in CELLS}
    anchor = out[(0, "both")]
    c.check_oracle(anchor)                                                      # a. the anchor against the oracle
    want_acc = {"dxd": I["prior_d"] + anchor["dxd"], "dxs": I["prior_s"] + anchor["dxs"]}    # numpy float32: one fp32 add
    assert want_acc["dxd"].dtype == np.float32 and want_acc["dxs"].dtype == np.float32
    fails = []
    for (acc, want), o in out.items():
        cell = cell_name(acc, want)
        for k, bit, given, pri in (("dxd", acc & 1, WANTS[want][0], I["prior_d"]), ("dxs", (acc >> 1) & 1, WANTS[want][1], I["prior_s"])):
            if given:                                                           # b. every requested dx buffer
                d = differ(o[k], want_acc[k] if bit else anchor[k])
                if d:
                    fails.append(f"{cell}: {k} != {'prior + anchor' if bit else 'anchor'} ({d})")
            elif differ(o[k], pri):                                             # (a buffer that was not handed over)
                fails.append(f"{cell}: {k} was not given to the call and changed")
        for k in ("dh", "pg"):                                                  # c. everything else ignores the options
            d = differ(o[k], anchor[k])
            if d:
                fails.append(f"{cell}: {k} differs from the anchor's ({d})")
    for k in ("dh", "pg"):                                                      # d. a set bit with a NULL pointer is ignored
        d = differ(out[(3, "none")][k], out[(0, "none")][k])
        if d:
            fails.append(f"acc3-none vs acc0-none: {k} ({d})")
    # e. accumulation twice: the second call adds into what the first left
    c.bwd(3, True, True)
    twice = c.bwd(3, True, True, refill=False)
    for k in ("dxd", "dxs"):
        d = differ(twice[k], want_acc[k] + anchor[k])
        if d:
            fails.append(f"acc3-both twice: {k} != (prior + anchor) + anchor ({d})")
    # the workspace was never refreshed: the first cell again gives the first cell's bits
    again = c.bwd(0, True, True)
    for k in ("dh", "pg", "dxd", "dxs"):
        d = differ(again[k], anchor[k])
        if d:
            fails.append(f"acc0-both run again at the end: {k} ({d})")
    assert not fails, f"{impl} {name}: {len(fails)} findings\n  " + "\n  ".join(fails)


# ---------------------------------------------------------------------------------------------------------------------
# cin = 1: the dx pointers are never written
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name,dst_is_var", CONVS1)
@pytest.mark.parametrize("impl", IMPLS)
def test_one_channel_conv_never_writes_dx(impl, name, dst_is_var):
    b, reach = batch_of(impl)
    used = assert_reach(impl, reach, dst_is_var, 1)
    print(f"\n{impl} {name} (dst_is_var = {dst_is_var}): destination-major sweep on {used[0]}")
    c = Conv(b, name, dst_is_var, 1)
    I = c.I
    null = c.bwd(0, False, False)
    c.check_oracle(null)
    fails = []
    for acc in (0, 3):
        o = c.bwd(acc, True, True)
        for k, pri in (("dxd", I["prior_d"]), ("dxs", I["prior_s"])):
            d = differ(o[k], pri)
            if d:
                fails.append(f"acc{acc}-both: {k} was written ({d})")
        for k in ("dh", "pg"):
            d = differ(o[k], null[k])
            if d:
                fails.append(f"acc{acc}-both: {k} differs from the call with NULL pointers ({d})")
    assert not fails, f"{impl} {name}: {len(fails)} findings\n  " + "\n  ".join(fails)
