"""The fused latency-regime path at grids other than the device's.

fused_grid() gives the sweeps one workgroup per CU, 256 on the devices that run this suite, and a lot hangs on that one
number: the wavefront lists (their length, the 64-item chunks a wavefront walks, the laps of the block tier), the
workgroup coordinates of every sweep, the rows of `stats` and `head_partials` that are written at all, and the trip counts
of the three loops of fused_reduce_body, of which a grid of 256 runs the first one only.  mllp_set_fused_grid_limit
(mllp_amd.graph.fused_grid_limit) lowers the grid of the batches created under it; this file runs the cases of
tests/test_fused_oracle.py there, through that file's helpers and at its bars (RTOL_ACT, RTOL_GRAD, the per-tensor check of
tests/grad_scales.py with the caps of fused_cases.GRID_BATCH_CAPS): no tolerance is new.

  FULL  = (8, 40, 168)   every loop of the reduce runs (test_reduce_trip_counts has the counts); 8 is one workgroup per partition
  MODES = (32, 64, 128)  the CU counts of the MI355X's partition modes (CPX, QPX, DPX); two trips of the 32-stride loop

Every GPU test creates its batches under the limit, forces set_path(2), asserts the grid the batch reports, and fills the
workspace and every output with NaN before a whole-model call (memory contract, rule 1): at a small grid the rows of
`stats` and `head_partials` behind the grid are never written and stay NaN, so a reduce that reads them gives NaN
gradients.  The exception is the workspace before a train step with flags bit 0, which carries the folded weights (the
header forbids poisoning it).  A grid above the device's CU count is skipped: the limit can only lower the grid.

What the limit does not reproduce is the residency of a partitioned device: all CUs are still there.
"""
import numpy as np
import pytest
import torch

import fused_cases as fc
import grad_scales as gs
from mllp_amd import _lib
from oracle import spmm_form as o2
from test_abi import _declared
from test_fused_oracle import (_check_block_laps, _check_replicas, _check_step, _nan, _oracle, _params, _poison, _sd,
                               assert_chunk_reach, assert_grid_reach, assert_laps_reach)
from test_hip_parity import RTOL_ACT, RTOL_GRAD, close, close_elementwise, grad_mask

gpu = pytest.mark.gpu
FULL = (8, 40, 168)
MODES = (32, 64, 128)
GRIDS = tuple(sorted(FULL + MODES))

# Replica counts R of a base LP (fc.replicate(base, R, basis_seed=R)) at which, at a grid of g workgroups, some wavefront's
# 16-channel list has exactly 63 and 64 items / exactly 65 and 66 items, in both orientations; found by a scan with
# census(..., exact=True), asserted again by the CPU test below and by the GPU test (as R_LISTS of test_fused_oracle.py
# for 256).  base "chunk": fc.chunk_base(), 72 wave rows per replica; with 12 wavefronts (grid 8) its list lengths step
# over both pairs, and at grid 40 over 63 / 64 (scanned to R = 2000), so those three entries use fc.chunk_base_small().
# No pair is left out at any grid.  "chunks": every list kind above 64 items and the 16-channel lists above 128 (three
# chunks) by pigeonhole, 25 replicas of chunk_base() per workgroup of a partition and one more.
R_TABLE = {
    8: {"lists63_64": ("small", 105, (63, 64)), "lists65_66": ("small", 109, (65, 66)), "chunks": ("chunk", 26, ())},
    32: {"lists63_64": ("chunk", 53, (63, 64)), "lists65_66": ("chunk", 46, (65, 66)), "chunks": ("chunk", 101, ())},
    40: {"lists63_64": ("small", 526, (63, 64)), "lists65_66": ("chunk", 63, (65, 66)), "chunks": ("chunk", 126, ())},
    64: {"lists63_64": ("chunk", 89, (63, 64)), "lists65_66": ("chunk", 92, (65, 66)), "chunks": ("chunk", 201, ())},
    128: {"lists63_64": ("chunk", 178, (63, 64)), "lists65_66": ("chunk", 184, (65, 66)), "chunks": ("chunk", 401, ())},
    168: {"lists63_64": ("chunk", 233, (63, 64)), "lists65_66": ("chunk", 241, (65, 66)), "chunks": ("chunk", 526, ())},
}
CHUNK_CASES = ("lists63_64", "lists65_66", "chunks")
BASES = {"chunk": fc.chunk_base, "small": fc.chunk_base_small}
DIRECT_NNZ = 400_000          # below it the list cases also run the oracle on the whole replicated instance

# trips per thread of the three loops of fused_reduce_body (128-stride, 32-stride, remainder), derived from its conditions
TRIPS = {8: (0, 0, 2), 32: (0, 1, 0), 40: (0, 1, 2), 64: (0, 2, 0), 128: (1, 0, 0), 168: (1, 1, 2), 256: (2, 0, 0)}


def _set_limit(n, prev=True):
    import ctypes
    p = ctypes.c_int64(-7)
    rc = _lib.lib().mllp_set_fused_grid_limit(n, ctypes.byref(p) if prev else None)
    return rc, int(p.value)


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_grid_limit_setter_without_gpu():
    from mllp_amd.graph import fused_grid_limit, set_fused_grid_limit
    L = _lib.lib()
    start = set_fused_grid_limit(0)
    try:
        assert _set_limit(0) == (0, 0)                               # 0 round-trips
        assert _set_limit(40) == (0, 0) and _set_limit(8) == (0, 40)     # the previous value comes back
        rc, prev = _set_limit(-1)
        assert rc == -1 and prev == -7                               # refused: nothing written, nothing changed
        msg = L.mllp_last_error()
        assert b"mllp_set_fused_grid_limit" in msg and b"limit" in msg
        assert _set_limit(1 << 40, prev=False)[0] == 0               # previous may be NULL; any non-negative value is taken
        assert _set_limit(0) == (0, 1 << 40)
        with fused_grid_limit(168):
            with fused_grid_limit(8):
                assert set_fused_grid_limit(8) == 8
            assert set_fused_grid_limit(168) == 168
            with pytest.raises(_lib.MllpError, match="mllp_set_fused_grid_limit"):
                with fused_grid_limit(-3):
                    pass
            assert set_fused_grid_limit(168) == 168
            with pytest.raises(ZeroDivisionError):
                with fused_grid_limit(32):
                    1 / 0
            assert set_fused_grid_limit(168) == 168                  # restored when the body raises
        assert set_fused_grid_limit(0) == 0
        assert L.mllp_graph_fused_grid(None, None) == -1
        assert b"mllp_graph_fused_grid" in L.mllp_last_error() and b"null" in L.mllp_last_error()
    finally:
        set_fused_grid_limit(start)


def test_header_exports_and_ctypes_table_agree():
    import ctypes
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("mllp_set_fused_grid_limit", "mllp_graph_fused_grid"):
        assert name in _declared() and name in _lib._PROTOTYPES and hasattr(L, name), name
    assert sorted(_lib._PROTOTYPES) == _declared()


def test_grid_rule():
    """G = max(min(CUs, STAT_BLOCKS_MAX, limit) / 8, 1) * 8, workgroups per partition G / 8"""
    c = fc.constants()
    assert (c["STAT_BLOCKS_MAX"], c["PARTS"]) == (256, 8)
    want = {1: 8, 7: 8, 8: 8, 9: 8, 40: 40, 255: 248, 256: 256, 304: 256}
    for cus, G in want.items():
        assert G == max(min(cus, 256) // 8, 1) * 8
        assert fc.grid_per_partition(cus) * c["PARTS"] == G, cus
    for g in GRIDS:
        assert fc.grid_per_partition(g) * c["PARTS"] == g           # the test grids are grids: the limit is not rounded


@pytest.mark.parametrize("g", GRIDS)
def test_cases_reach_at_every_grid(g):
    assert_grid_reach(0, g)
    assert_grid_reach(1, g)
    assert_laps_reach(g)


def _chunk_case(g, case):
    base, R, exact = R_TABLE[g][case]
    return BASES[base](), R, exact


@pytest.mark.parametrize("g", GRIDS)
def test_list_chunk_table_reaches_the_chunk_boundary(g):
    assert sorted(R_TABLE) == list(GRIDS) and all(sorted(R_TABLE[k]) == sorted(CHUNK_CASES) for k in R_TABLE)
    for case in CHUNK_CASES:
        base, R, exact = _chunk_case(g, case)
        assert exact == {"lists63_64": (63, 64), "lists65_66": (65, 66), "chunks": ()}[case]
        assert_chunk_reach(R, g, exact=exact, base=base)


def test_reduce_trip_counts():
    """The three loops of fused_reduce_body, restated from their parsed conditions: FULL gives each of them a grid with no
    trip and one with one trip, the 32-stride and the remainder loop one with two; 256 runs the first loop alone (the
    reason for this file).  Every partial is read once at every grid."""
    slices, loops = fc.reduce_loops()
    assert slices == 4 and loops == [(124, 128), (28, 32), (0, 4)]
    for (la, st) in loops:
        assert st % slices == 0 and la == st - slices               # a trip is taken when its last partial exists
    got = {}
    for n in sorted(TRIPS):
        trips, seen = fc.reduce_trips(n, slices, loops)
        assert seen == list(range(n)), n
        assert all(len(t) == 1 for t in trips), (n, trips)          # the same count in every thread
        got[n] = tuple(t.pop() for t in trips)
    assert got == TRIPS
    # A grid is a multiple of 8, so the remainder loop (4 partials per trip of the 4 slices) makes an even number of
    # trips: one trip cannot happen.  FULL runs every loop (the first with 0 and 1 trips, the second with 0 and 1, the
    # third with 2); the second loop's two trips and the third's none come with MODES.
    for loop, (full, both) in enumerate((({0, 1}, {0, 1}), ({0, 1}, {0, 1, 2}), ({2}, {0, 2}))):
        assert {got[g][loop] for g in FULL} == full, (loop, full)
        assert {got[g][loop] for g in GRIDS} == both, (loop, both)
    assert got[256] == (2, 0, 0)


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    _lib.lib()                      # fail loudly: no fallback
    assert torch.cuda.is_available()
    from mllp_amd.graph import LPBatch, set_fused_grid_limit
    assert LPBatch.default_path == 0
    assert set_fused_grid_limit(0) == 0, "a grid limit was left behind by an earlier test"
    return LPBatch, torch.cuda.get_device_properties(0).multi_processor_count


def _dev_grid(cus):
    return fc.grid_per_partition(cus) * fc.constants()["PARTS"]


def _need(g, cus):
    if g > cus:
        pytest.skip(f"a grid of {g} workgroups needs {g} CUs, the device has {cus}: the limit only lowers the grid")


def _maker(g):
    """batches created under a limit of g workgroups, on the fused path, that report that grid"""
    from mllp_amd.graph import fused_grid_limit

    def make(LPBatch, insts):
        with fused_grid_limit(g):
            b = LPBatch.from_instances(insts).set_path(2)
        info = b.fused_grid_info()
        assert info[0] == g and info[1] == 8 and info[3] == g, info
        return b
    return make


_CACHE = {}


def _grid_reference(golden, variant, n_inst):
    """(state dict, instances, fp64 oracle result, fp32 yardstick) of a batch of degree grids: once for all grids"""
    key = ("grid", variant, n_inst)
    if key not in _CACHE:
        sd = _sd(golden)
        insts = fc.grid_batch(variant, n_inst)
        _CACHE[key] = (sd, insts, _oracle(sd, insts, f"grid{variant} x {n_inst}"), gs.yardstick(sd, o2.BatchCSR(insts)))
    return _CACHE[key]


def _subset5_reference(golden, subset5):
    if "subset5" not in _CACHE:
        sd = _sd(golden)
        _CACHE["subset5"] = (sd, _oracle(sd, list(subset5), "subset5"))
    return _CACHE["subset5"]


@gpu
def test_limit_takes_effect_and_grids_alternate(dev, golden):
    """1, 2. A batch reports the grid of the limit it was created under, and keeps it; batches created outside report the
    device's grid again; a limit above the CU count changes nothing.  Nothing grid-dependent is cached per process: a
    grid-8 batch and a full-grid batch give their own bits, each within the bars, when their calls alternate."""
    from mllp_amd.graph import fused_grid_limit, set_fused_grid_limit
    LPBatch, cus = dev
    G = _dev_grid(cus)
    sd, insts, r, _ = _grid_reference(golden, 1, 1)
    with fused_grid_limit(8):
        b8 = LPBatch.from_instances(insts)
        assert b8.fused_grid_info() == (8, 8, cus, 8)
    assert set_fused_grid_limit(0) == 0
    assert b8.set_path(2).fused_grid_info() == (8, 8, cus, 8)        # the limit of its creation, also for a later set_path
    bf = LPBatch.from_instances(insts).set_path(2)
    assert bf.fused_grid_info() == (G, 8, cus, 0)
    with fused_grid_limit(cus + 100):
        assert LPBatch.from_instances(insts).fused_grid_info() == (G, 8, cus, cus + 100)
    with fused_grid_limit(G):
        assert LPBatch.from_instances(insts).fused_grid_info() == (G, 8, cus, G)
    p = _params(sd)
    keep = grad_mask()
    first = {}
    for k in range(3):
        for name, b in (("grid 8", b8), ("device grid", bf)):
            got = [t.clone() for t in b.loss_step(p, **_poison(b, "logits", "loss", "grads"))]
            if name not in first:
                first[name] = got
                close_elementwise(got[1].cpu().numpy(), r["logits"], RTOL_ACT, f"{name}: logits, element-wise")
                close(got[0].cpu().numpy(), [r["loss"]], RTOL_ACT, f"{name}: loss")
                close(got[2].cpu().numpy()[keep], r["grads"][keep], RTOL_GRAD, f"{name}: gradients")
            for a, w, what in zip(got, first[name], ("loss", "logits", "grads")):
                assert torch.equal(a, w), f"{name}, round {k}: {what} changed after a call at the other grid"


DEGREE_CASES = ([(g, v, 1) for g in FULL for v in (0, 1)] + [(40, 1, 9)] + [(g, 1, 1) for g in MODES])


@gpu
@pytest.mark.parametrize("g,variant,n_inst", DEGREE_CASES, ids=[f"grid{g}-variant{v}-x{n}" for g, v, n in DEGREE_CASES])
def test_degree_grid_against_oracle(dev, golden, g, variant, n_inst):
    """3. test_fused_oracle.py's F at a grid of g workgroups: both sides of every tier threshold and the last partial step
    of every tier in every kernel family; with nine instances over eight partitions one partition holds two."""
    LPBatch, cus = dev
    _need(g, cus)
    assert_grid_reach(variant, g)
    sd, insts, r, yard = _grid_reference(golden, variant, n_inst)
    _check_step(LPBatch, insts, sd, r, f"grid {g}: grid{variant} x {n_inst}", max_exempt=fc.GRID_BATCH_CAPS[(variant, n_inst)],
                make=_maker(g), poison=True, yard=yard)


@gpu
@pytest.mark.parametrize("g", FULL)
def test_block_laps_against_oracle(dev, golden, g):
    """4. more than 2 * gp block rows in one partition, with a spotlight on a row of the third lap"""
    LPBatch, cus = dev
    _need(g, cus)
    b = _check_block_laps(LPBatch, golden, g, make=_maker(g), poison=True)
    assert b.fused_grid_info()[0] == g


@gpu
@pytest.mark.parametrize("case", CHUNK_CASES)
@pytest.mark.parametrize("g", FULL + (32, ))
def test_list_chunks_against_oracle(dev, golden, g, case):
    """5. wavefront lists of exactly 63 .. 66 items and of three chunks at a grid of g workgroups"""
    LPBatch, cus = dev
    _need(g, cus)
    base, R, exact = _chunk_case(g, case)
    inst, _ = assert_chunk_reach(R, g, exact=exact, base=base)
    _check_replicas(LPBatch, golden, inst, R, f"grid {g}: {base.name} x {R}", direct=bool(exact) and inst.nnz < DIRECT_NNZ,
                    base=base, make=_maker(g), poison=True)


@gpu
@pytest.mark.parametrize("g", GRIDS)
def test_train_step_tail_equals_loss_step_plus_adam(dev, golden, subset5, g):
    """6. fused_tail_kernel sums the partials with nblk = G: three one-launch steps (flags bit 0 from the second on) give
    the bits of three rounds of loss_step + mllp_adam_step on a second batch of the same grid, and the first step's
    gradients are the oracle's."""
    from mllp_amd.graph import adam_step
    LPBatch, cus = dev
    _need(g, cus)
    sd, r = _subset5_reference(golden, subset5)
    make = _maker(g)
    flat = _params(sd)

    def fresh():
        p = flat.clone()
        return p, torch.zeros_like(p), torch.zeros_like(p), torch.tensor([0.0, 1e-3, 0.9, 0.999], device="cuda")

    names = ("loss", "logits", "grads", "params", "exp_avg", "exp_avg_sq", "state")
    b0 = make(LPBatch, list(subset5))
    p0, m0, v0, s0 = fresh()
    ref = []
    for k in range(3):
        loss, logits, grads = b0.loss_step(p0, **_poison(b0, "logits", "loss", "grads"))
        adam_step(p0, grads, m0, v0, s0, 1e-8)
        ref.append([t.clone() for t in (loss, logits, grads, p0, m0, v0, s0)])
    b1 = make(LPBatch, list(subset5))
    p1, m1, v1, s1 = fresh()
    b1.workspace().fill_(float("nan"))          # before the first step only: from the second on it holds the folded weights
    for k in range(3):
        loss, logits, grads = b1.train_step(p1, m1, v1, s1, 1e-8, logits=_nan(b1.N), loss=_nan(1), grads=_nan(4721), param_gen=k)
        assert b1._folded is not None
        for got, want, what in zip((loss, logits, grads, p1, m1, v1, s1), ref[k], names):
            assert torch.equal(got, want), f"grid {g}, step {k}: {what} differs from loss_step + adam_step"
    assert float(s1[0]) == 3.0
    keep = grad_mask()
    close_elementwise(ref[0][1].cpu().numpy(), r["logits"], RTOL_ACT, f"grid {g}: logits of the first step")
    close(ref[0][0].cpu().numpy(), [r["loss"]], RTOL_ACT, f"grid {g}: loss of the first step")
    close(ref[0][2].cpu().numpy()[keep], r["grads"][keep], RTOL_GRAD, f"grid {g}: gradients of the first step")


@pytest.fixture(scope="module")
def inputs_oracle(golden, subset5):
    from test_input_grads import oracle_input_grads
    from test_input_grads_fused import _bce_loss, _oracle_logits
    flat = golden["weights_flat"]
    return oracle_input_grads(flat, subset5, _bce_loss(subset5, 1.0 / len(subset5))), _oracle_logits(flat, subset5)


@gpu
@pytest.mark.parametrize("g", (8, 168))
def test_loss_step_inputs(dev, golden, subset5, inputs_oracle, g):
    """7. dx1, dx2 and dvalues of the loss step at the bars of tests/test_input_grads_fused.py; loss, logits and parameter
    gradients bit for bit those of loss_step at the same grid."""
    from test_input_grads_fused import RTOL_OUT, _check_four, _same
    LPBatch, cus = dev
    _need(g, cus)
    (oloss, ox1, ox2, odv, opg), ologits = inputs_oracle
    make = _maker(g)
    p = torch.tensor(golden["weights_flat"], dtype=torch.float32, device="cuda")
    b = make(LPBatch, list(subset5))
    b.loss_step_inputs(p)                       # (the first call that asks for dvalues allocates the position map)
    outs = _poison(b, "logits", "loss", "grads")
    dx1, dx2, dv = _nan(b.N), _nan(b.M), _nan(b.nnz)
    b._check_inputs()
    _lib.check(_lib.lib().mllp_gnn_loss_step_inputs(
        b._h, _lib.ptr(p), _lib.ptr(b.x1), _lib.ptr(b.x2), _lib.ptr(b.labels), 1.0 / b.n_inst, _lib.ptr(b.workspace()),
        _lib.ptr(outs["logits"]), _lib.ptr(outs["loss"]), _lib.ptr(outs["grads"]), _lib.ptr(dx1), _lib.ptr(dx2), _lib.ptr(dv),
        _lib.current_stream()))
    loss, logits, grads = outs["loss"], outs["logits"], outs["grads"]
    assert abs(float(loss) - oloss) < RTOL_OUT * abs(oloss), (float(loss), oloss)
    close(logits.cpu().numpy(), ologits, RTOL_OUT, f"grid {g}: logits")
    _check_four((grads, dx1, dx2, dv), (ox1, ox2, odv, opg), f"grid {g}: loss step")
    b2 = make(LPBatch, list(subset5))
    _same((loss, logits, grads), b2.loss_step(p, **_poison(b2, "logits", "loss", "grads")), f"grid {g}: loss_step_inputs against loss_step")


@gpu
def test_across_grids(dev, golden):
    """8. One degree grid at 8, 40, 168 and the device's grid.  The forward has no sum across workgroups and a row's order of
    summation is fixed by its item (item_request: the tier and the position in it), whichever wavefront of whichever
    workgroup walks the item; a block row is summed by one whole workgroup whatever the grid: the logits are the same BITS at
    every grid.  The loss and the gradients are sums of per-workgroup partials and differ in rounding (printed); each grid
    is held to the oracle by the tests above."""
    LPBatch, cus = dev
    sd, insts, r, _ = _grid_reference(golden, 1, 1)
    G = _dev_grid(cus)
    p = _params(sd)
    keep = grad_mask()
    got = {}
    for g in sorted({g for g in FULL if g <= cus} | {G}):
        b = _maker(g)(LPBatch, insts) if g != G else LPBatch.from_instances(insts).set_path(2)
        assert b.fused_grid_info()[0] == g
        got[g] = [t.clone() for t in b.loss_step(p, **_poison(b, "logits", "loss", "grads"))]
    ref = got[G]
    for g, (loss, logits, grads) in got.items():
        dz = fc.rel_err(logits.cpu().numpy(), ref[1].cpu().numpy())
        dg = fc.rel_err(grads.cpu().numpy()[keep], ref[2].cpu().numpy()[keep])
        dl = abs(float(loss) - float(ref[0])) / abs(float(ref[0]))
        print(f"[across grids] grid {g:3d} against grid {G}: logits {dz:.1e} (bit-equal: {torch.equal(logits, ref[1])}), "
              f"loss {dl:.1e}, gradients {dg:.1e}")
    for g, (loss, logits, grads) in got.items():
        assert torch.equal(logits, ref[1]), f"grid {g}: the logits are not those of grid {G} bit for bit"
