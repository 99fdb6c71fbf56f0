"""The fused latency-regime path (fused_kernels.hip + host_graph.cpp) against the fp64 oracle (oracle/spmm_form.py) on
inputs built around the kernels' own structure: the tier edges of both geometries, the last partial step and the last
partial item of every tier, empty tiers and empty partitions, wavefront lists of 63 .. 66 items and of several 64-item
chunks, a second and third lap of the block-tier loop, a sharpened softmax in every merged tier, batches without
nonzeros.  Every GPU test forces set_path(2) on a fresh batch and starts by asserting, through the census of
tests/fused_cases.py, that its input reaches what it claims; the CPU tests make the same assertions for 256 CUs and check
the identities that let one cheap oracle run stand for a 4.7 M-nonzero instance.  tests/test_fused_grids.py makes them for
grids of 8, 32, 40, 64, 128 and 168 workgroups and runs the same cases there, through the helpers of this file.

Tolerances are those of tests/test_hip_parity.py: 1e-5 for logits and losses, 5e-5 for gradients, lin_key.bias masked.
Yardstick: the same decomposition in fp32 on the CPU against fp64 (fused_cases.model_dt), as max|diff| / max|ref|; the
test asserts that it stays below a quarter of the bar for every case.  Worst figures (logits, loss, gradients):

  grid0        3.5e-07  3.4e-08  2.1e-07
  grid1        4.7e-07  2.8e-08  3.1e-07
  blocklaps    1.5e-06  4.3e-08  4.8e-07
  chunkbase    3.4e-07  7.8e-08  7.7e-08
  sharp        8.0e-07  1.7e-08  5.5e-06

The fp32 run sums a row's terms one after the other, so its error grows with the row length and with the spread of the
logits; that caps the sharpening: the scores of the sharp case are scaled by 2, not by 6 as in
test_hip_parity.py::test_online_softmax_rescale_is_exercised (at 6 the yardstick is 1.1e-05, above the bar itself).
What the sharp case therefore is: rows whose running maximum moves in EVERY step of every merged tier (rescale of the
running sums, merges of partial states with different maxima), with the largest attention weight 1.3 to 4 times the
uniform one.  It is not a wide logit range: a missing subtraction of the maximum or an exp-range problem would not
show here (the 700-long ramp of test_hip_parity.py, scores x 6, runs on the fused path too and is the test for that).
"""
import time

import numpy as np
import pytest
import torch

import fused_cases as fc
import grad_scales as gs
from oracle import pyg_restatement as o1
from oracle import spmm_form as o2
from test_hip_parity import RTOL_ACT, RTOL_GRAD, close, close_elementwise, grad_mask

gpu = pytest.mark.gpu
SHARP_FACTOR = 2.0
GRID_BATCHES = (1, 2, 7, 8, 9)
R_LISTS = (388, 402)          # wavefronts with exactly 63 and 64 / 65 and 66 items in the 16-channel lists (256 CUs)
R_CHUNKS = 800                # every list kind above 64 items by pigeonhole; the 16-channel lists hold three chunks


def _sd(golden):
    return {k: v.numpy() for k, v in o1.unflatten_state(torch.tensor(golden["weights_flat"])).items()}


def _oracle(sd, insts, what, **kw):
    t0 = time.perf_counter()
    r = o2.gnn_forward_backward(sd, o2.BatchCSR(insts), **kw)
    print(f"[oracle] {what}: {time.perf_counter() - t0:.2f} s")
    return r


def _show(name, cen):
    print("\n" + "\n".join(fc.census_lines(name, cen)))


# ---------------------------------------------------------------------------------------------------------------------
# what every case claims to reach (asserted on the CPU for 256 CUs, and again by the GPU tests for the device's CUs; for
# the other grids in tests/test_fused_grids.py)
# ---------------------------------------------------------------------------------------------------------------------
def assert_grid_reach(variant, cus):
    c = fc.constants()
    inst = fc.degree_grid(variant)
    cen = fc.census(inst, cus)
    _show(inst.name, cen)
    rows, cols = fc.degrees(inst)
    for deg in (rows, cols):
        have = set(deg.tolist())
        assert set(fc.GRID_DEGREES) <= have
        # both sides of every threshold, and the last partial step of every tier of every kernel family
        for T in (c["T16"], c["T1"]):
            for t in T:
                assert {t, t + 1} <= have, t
        for kind in fc.KINDS:
            w = fc.step_widths(kind, c)
            T = c["T1"] if fc.KINDS[kind][0] else c["T16"]
            for tier, lo, hi in (("base", 0, T[0]), ("group", T[0], T[1]), ("wave", T[1], T[2]), ("block", T[2], 1 << 30)):
                mine = [d for d in have if lo < d <= hi]
                assert any(d % w[tier] for d in mine) and any(d % w[tier] == 0 for d in mine), (kind, tier)
    for orient in ("A", "At"):
        for kind, e in cen[orient].items():
            t = e["tiers"]
            assert min(t.values()) > 0, (orient, kind, t)
            U = 64 if fc.KINDS[kind][0] else 16
            assert t["group"] % (U // 4) == variant and t["base"] % U == variant, (orient, kind, t)
    return inst, cen


def assert_chunk_reach(R, cus, exact=(), base=None):
    inst = fc.replicate(base or fc.chunk_base(), R, basis_seed=R)
    cen = fc.census(inst, cus, exact=bool(exact))
    _show(inst.name, cen)
    for orient in ("A", "At"):
        if exact:
            L = cen[orient]["16"]["lengths"]
            for n in exact:
                assert (L == n).any(), f"{orient}: no wavefront with exactly {n} items: {sorted(set(L.tolist()))}"
        else:
            for kind, e in cen[orient].items():
                assert e["bound"] >= 65, (orient, kind, e["bound"])
            assert cen[orient]["16"]["bound"] > 128              # three chunks
        t = cen[orient]["16"]["tiers"]
        assert t["wave"] and t["group"] and t["base"]
    return inst, cen


def assert_laps_reach(cus):
    c = fc.constants()
    inst = fc.block_laps_instance(cus)
    cen = fc.census(inst, cus)
    _show(inst.name, cen)
    gp = fc.grid_per_partition(cus, c)
    for deg in fc.degrees(inst):
        assert (deg > c["T1"][2]).sum() >= 2 * gp + 1
        assert ((deg > c["T16"][2]) & (deg <= c["T1"][2])).sum() >= 2 * gp + 1
    for orient in ("A", "At"):
        for kind, e in cen[orient].items():
            assert e["laps"] >= 3, (orient, kind, e)
    return inst, cen


def assert_sharp_reach(cus=256):
    inst = fc.sharp_instance()
    _show(inst.name, fc.census(inst, cus))
    sd = {k: v.numpy() for k, v in fc.sharp_state(SHARP_FACTOR).items()}
    b = o2.BatchCSR([inst])
    r = o2.gnn_forward_backward(sd, b)
    rep = fc.sharp_report(r, b, fc.sharp_rows(inst))
    seen = {}
    for orient, key, row, deg, tier, steps, moves, amax in rep:
        kind = "1" if key.startswith("s1") else "16"
        if steps >= 2:
            seen.setdefault((orient, kind, tier), []).append((moves, amax * deg))
    print("\n[sharp] (orientation, geometry, tier): rows whose running maximum moves in every step / rows, largest share of "
          "one nonzero in units of the uniform share")
    for k, v in sorted(seen.items()):
        print(f"  {k}: {sum(m for m, _ in v)} / {len(v)}, {max(a for m, a in v if m) if any(m for m, _ in v) else 0:.2f}")
    # the merged tiers of both geometries, both orientations (the 1-channel block rows with more than one step are the two
    # of 12400 nonzeros: three steps of 6144)
    want = [(o, g, t) for o in ("A", "At") for g in ("16", "1") for t in ("group", "wave", "block")]
    for k in want:
        assert k in seen and any(m for m, _ in seen[k]), f"{k}: no row whose running maximum moves in every step"
        # stated share: where the maximum climbs, the largest attention weight is at least 1.3 x the uniform one
        assert max(a for m, a in seen[k] if m) >= 1.3, k
    return inst, sd, r


# ---------------------------------------------------------------------------------------------------------------------
# CPU: A census, B degree grid, C identities, D sharp cases, E tolerances
# ---------------------------------------------------------------------------------------------------------------------
def test_constants_are_parsed_and_consistent():
    c = fc.constants()
    assert c["T16"][0] < c["T16"][1] < c["T16"][2] <= c["T1"][2] and c["T16"][:2] == c["T1"][:2]
    assert c["FT"] == 64 * c["FW"] and c["PARTS"] == 8
    # a row between the two block thresholds is a block row of the 16-channel sweeps and a wave row of layer 1
    assert any(c["T16"][2] < d <= c["T1"][2] for d in fc.GRID_DEGREES)
    assert fc.step_widths("16", c) == dict(base=4, group=16, wave=64, block=c["FT"])
    assert fc.step_widths("src16", c) == dict(base=2, group=8, wave=32, block=c["FT"] // 2)
    assert fc.step_widths("1", c) == dict(base=8, group=32, wave=512, block=8 * c["FT"])


@pytest.mark.parametrize("variant", [0, 1])
def test_degree_grid_reaches_every_tier_edge(variant):
    assert_grid_reach(variant, 256)


def test_census_pigeonhole_and_exact_lists_agree():
    inst = fc.replicate(fc.chunk_base(), 40)
    cen = fc.census(inst, 256, exact=True)
    for orient in cen:
        for kind, e in cen[orient].items():
            L = e["lengths"]
            assert L.sum() == e["items"] and L.max() >= e["bound"] and len(L) == e["waves"]


def test_list_chunk_cases_reach_the_chunk_boundary():
    assert_chunk_reach(R_LISTS[0], 256, exact=(63, 64))
    assert_chunk_reach(R_LISTS[1], 256, exact=(65, 66))
    assert_chunk_reach(R_CHUNKS, 256)


def test_block_laps_case_reaches_the_third_lap():
    assert_laps_reach(256)


def test_replica_identities(golden):
    """C. R block-diagonal copies of a base LP as one instance: the base logits in every copy, and the backward from a
    dlogits equals the base LP's backward from the sum of its R slices."""
    sd = _sd(golden)
    base, R = fc.chunk_base(), 5
    inst = fc.replicate(base, R, basis_seed=1)
    rb = o2.gnn_forward_backward(sd, o2.BatchCSR([base]), want_grads=False)
    dz = np.random.default_rng(2).standard_normal(inst.n) / inst.n
    rr = o2.gnn_forward_backward(sd, o2.BatchCSR([inst]), dlogits=dz)
    np.testing.assert_allclose(rr["logits"].reshape(R, base.n), np.broadcast_to(rb["logits"], (R, base.n)), rtol=1e-12, atol=1e-14)
    want = o2.gnn_forward_backward(sd, o2.BatchCSR([base]), dlogits=dz.reshape(R, base.n).sum(0))["grads"]
    np.testing.assert_allclose(rr["grads"], want, rtol=1e-9, atol=1e-12 * np.abs(want).max())
    # the loss step of the replicated instance is the backward from its own BCE gradient
    full = o2.gnn_forward_backward(sd, o2.BatchCSR([inst]))
    y = inst.basis.astype(np.float64)
    dzl = (1.0 / (1.0 + np.exp(-full["logits"])) - y) / inst.n
    want = o2.gnn_forward_backward(sd, o2.BatchCSR([base]), dlogits=dzl.reshape(R, base.n).sum(0))["grads"]
    np.testing.assert_allclose(full["grads"], want, rtol=1e-9, atol=1e-12 * np.abs(want).max())


def test_sharp_cases_are_sharp_on_the_oracle():
    assert_sharp_reach()


def _yardstick_cases(golden):
    sd = _sd(golden)
    return [("grid0", sd, fc.degree_grid(0)), ("grid1", sd, fc.degree_grid(1)), ("blocklaps", sd, fc.block_laps_instance()),
            ("chunkbase", sd, fc.chunk_base()),
            ("sharp", {k: v.numpy() for k, v in fc.sharp_state(SHARP_FACTOR).items()}, fc.sharp_instance())]


def test_fp32_yardstick_is_a_quarter_of_the_bar(golden):
    """E. model_dt in fp64 is spmm_form; in fp32 it misses fp64 by less than a quarter of every tolerance used below."""
    keep = grad_mask()
    for name, sd, inst in _yardstick_cases(golden):
        b = o2.BatchCSR([inst])
        r = o2.gnn_forward_backward(sd, b)
        r64, r32 = fc.model_dt(sd, b, np.float64), fc.model_dt(sd, b, np.float32)
        assert np.array_equal(r64["logits"], r["logits"]) and np.array_equal(r64["grads"], r["grads"]) and r64["loss"] == r["loss"]
        e = (fc.rel_err(r32["logits"], r["logits"]), abs(r32["loss"] - r["loss"]) / abs(r["loss"]),
             fc.rel_err(r32["grads"][keep], r["grads"][keep]))
        print(f"[yardstick] {name:10s} logits {e[0]:.1e}  loss {e[1]:.1e}  gradients {e[2]:.1e}")
        assert e[0] < RTOL_ACT / 4 and e[1] < RTOL_ACT / 4 and e[2] < RTOL_GRAD / 4, (name, e)


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    from mllp_amd import _lib
    _lib.lib()                      # fail loudly: no fallback
    assert torch.cuda.is_available()
    from mllp_amd.graph import LPBatch
    assert LPBatch.default_path == 0
    return LPBatch, torch.cuda.get_device_properties(0).multi_processor_count


def _fused(LPBatch, insts):
    return LPBatch.from_instances(insts).set_path(2)


def _params(sd):
    flat = o1.flatten_state({k: torch.as_tensor(v) for k, v in sd.items()}).numpy()
    return torch.tensor(flat, dtype=torch.float32, device="cuda")


def _nan(n):
    return torch.full((n,), float("nan"), device="cuda")


def _poison(b, *names):
    """The workspace and the named outputs of the next whole-model call filled with NaN (memory contract, rule 1: the bits
    may not depend on what they held).  Returns the outputs as keyword arguments of the call."""
    b.workspace().fill_(float("nan"))
    n = dict(logits=b.N, loss=1, grads=4721)
    return {k: _nan(n[k]) for k in names}


def _check_step(LPBatch, insts, sd, r, what, max_exempt=None, make=None, poison=False, yard=None):
    """logits (max norm and element-wise), loss, gradients (max_exempt given: every tensor on its own scale too, at most
    that many exempted by the fp32 yardstick: tests/grad_scales.py), a bitwise-equal second run, forward-only logits.
    make: how the batches are created (tests/test_fused_grids.py: under a grid limit); poison: NaN in the workspace and
    in every output before every call; yard: the yardstick of this input, where the caller has it already."""
    make = make or _fused
    p = _params(sd)
    b = make(LPBatch, insts)
    out = lambda bb, *names: _poison(bb, *names) if poison else {}
    loss, logits, grads = [t.clone() for t in b.loss_step(p, **out(b, "logits", "loss", "grads"))]
    keep = grad_mask()
    close(logits.cpu().numpy(), r["logits"], RTOL_ACT, f"{what}: logits")
    close_elementwise(logits.cpu().numpy(), r["logits"], RTOL_ACT, f"{what}: logits, element-wise")
    close(loss.cpu().numpy(), [r["loss"]], RTOL_ACT, f"{what}: loss")
    close(grads.cpu().numpy()[keep], r["grads"][keep], RTOL_GRAD, f"{what}: gradients")
    if max_exempt is not None:
        gs.close_per_tensor(grads.cpu().numpy(), r["grads"], yard or gs.yardstick(sd, o2.BatchCSR(insts)),
                            f"{what}: gradients", max_exempt=max_exempt)
    l2, z2, g2 = b.loss_step(p, **out(b, "logits", "loss", "grads"))
    assert torch.equal(l2, loss) and torch.equal(z2, logits) and torch.equal(g2, grads), f"{what}: not run-to-run exact"
    b2 = make(LPBatch, insts)
    fwd = b2.forward(p, **out(b2, "logits")).cpu().numpy()
    close(fwd, r["logits"], RTOL_ACT, f"{what}: forward-only logits")
    close_elementwise(fwd, r["logits"], RTOL_ACT, f"{what}: forward-only logits, element-wise")
    return b, p


@gpu
@pytest.mark.parametrize("n_inst", GRID_BATCHES)
@pytest.mark.parametrize("variant", [0, 1])
def test_degree_grid_against_oracle(dev, golden, variant, n_inst):
    """F. 1, 2, 7, 8 and 9 instances over 8 partitions: at least 8 - n partitions are empty, with 9 one holds two.  Every
    tensor's gradient is checked on its own scale as well (fused_cases.GRID_BATCH_CAPS: what the fp32 yardstick exempts, at
    most two large bias tensors; never a key, query or edge tensor), except on grid1 x 8, where the yardstick exempts four."""
    LPBatch, cus = dev
    assert_grid_reach(variant, cus)
    sd = _sd(golden)
    insts = fc.grid_batch(variant, n_inst)
    r = _oracle(sd, insts, f"grid{variant} x {n_inst}")
    _check_step(LPBatch, insts, sd, r, f"grid{variant} x {n_inst}", max_exempt=fc.GRID_BATCH_CAPS[(variant, n_inst)])


# the distinct degree ranges of the two geometries (fused_cases.spot_tiers): base, group and wave rows of both, rows that are
# block rows of the 16-channel sweeps and wave rows of layer 1, block rows of both
SPOTS = [(o, t) for o in ("A", "At") for t in ("base", "group", "wave", "block16_wave1", "block")]


@gpu
@pytest.mark.parametrize("orient,tier", SPOTS, ids=["-".join(s) for s in SPOTS])
def test_spotlight_backward(dev, golden, orient, tier):
    """G. dlogits nonzero only within one hop of one row of a tier: an error in that row is at full scale in the
    parameter gradients instead of one term among 10^4.  Every sweep family (forward and backward of both geometries, the
    source-major sweep) walks that row or its neighbours in the tier named."""
    LPBatch, cus = dev
    inst, _ = assert_grid_reach(1, cus)
    assert sorted(fc.spot_tiers()) == sorted({t for _, t in SPOTS})
    row = fc.tier_rows(inst)[(orient, tier)]
    assert row is not None
    geo = fc.spot_tiers()[tier][2]
    hot = fc.one_hop(inst, orient, row)
    assert 1 <= len(hot) <= 4
    dz = np.zeros(inst.n)
    dz[hot] = np.random.default_rng(row).choice([-1.0, 1.0], len(hot)) * (1.0 + np.arange(len(hot)))
    sd = _sd(golden)
    r = _oracle(sd, [inst], f"spotlight {orient} {geo} {tier} (row {row}, {len(hot)} variables)", dlogits=dz)
    p = _params(sd)
    b = _fused(LPBatch, [inst])
    z = b.forward(p)
    close_elementwise(z.cpu().numpy(), r["logits"], RTOL_ACT, "logits, element-wise")
    g = b.backward(p, torch.tensor(dz, dtype=torch.float32, device="cuda")).cpu().numpy()
    keep = grad_mask()
    close(g[keep], r["grads"][keep], RTOL_GRAD, f"spotlight {orient} {geo} {tier}: gradients")


def _check_replicas(LPBatch, golden, inst, R, what, direct, base=None, make=None, poison=False):
    make = make or _fused
    out = lambda bb, *names: _poison(bb, *names) if poison else {}
    sd = _sd(golden)
    base = base or fc.chunk_base()
    rb = _oracle(sd, [base], f"{what}: base LP", want_grads=False)
    p = _params(sd)
    b = make(LPBatch, [inst])
    z = b.forward(p, **out(b, "logits")).cpu().numpy().astype(np.float64).reshape(R, base.n)
    want = np.broadcast_to(rb["logits"], z.shape)
    close(z, want, RTOL_ACT, f"{what}: logits of the {R} replicas")
    close_elementwise(z, want, RTOL_ACT, f"{what}: logits of the {R} replicas, element-wise")
    # a dlogits that differs from replica to replica == the base LP's backward from the sum of the slices
    dz = (np.random.default_rng(R).standard_normal(inst.n) / np.sqrt(inst.n)).astype(np.float32)
    g = b.backward(p, torch.tensor(dz, device="cuda"), **({"grads": _nan(4721)} if poison else {})).cpu().numpy()
    rg = _oracle(sd, [base], f"{what}: base LP, summed dlogits", dlogits=dz.astype(np.float64).reshape(R, base.n).sum(0))
    keep = grad_mask()
    close(g[keep], rg["grads"][keep], RTOL_GRAD, f"{what}: gradients of a per-replica dlogits")
    # the loss step: labels differ per replica; its gradient is the backward from (sigmoid(z) - y) / N
    b = make(LPBatch, [inst])
    loss, logits, grads = b.loss_step(p, **out(b, "logits", "loss", "grads"))
    zr = np.tile(rb["logits"], R)
    y = inst.basis.astype(np.float64)
    want_loss = float((np.maximum(zr, 0) - zr * y + np.log1p(np.exp(-np.abs(zr)))).mean())
    close(loss.cpu().numpy(), [want_loss], RTOL_ACT, f"{what}: loss")
    dzl = (1.0 / (1.0 + np.exp(-zr)) - y) / inst.n
    rl = _oracle(sd, [base], f"{what}: base LP, summed BCE gradient", dlogits=dzl.reshape(R, base.n).sum(0))
    close(grads.cpu().numpy()[keep], rl["grads"][keep], RTOL_GRAD, f"{what}: gradients of the loss step")
    if direct:
        rd = _oracle(sd, [inst], f"{what}: the whole instance, directly")
        close(loss.cpu().numpy(), [rd["loss"]], RTOL_ACT, f"{what}: loss, direct")
        close_elementwise(logits.cpu().numpy(), rd["logits"], RTOL_ACT, f"{what}: logits, direct")
        close(grads.cpu().numpy()[keep], rd["grads"][keep], RTOL_GRAD, f"{what}: gradients, direct")


@gpu
@pytest.mark.parametrize("R,exact", [(R_LISTS[0], (63, 64)), (R_LISTS[1], (65, 66)), (R_CHUNKS, ())],
                         ids=["lists63_64", "lists65_66", "chunks"])
def test_list_chunks_against_oracle(dev, golden, R, exact):
    """H. wavefront lists of exactly 63 .. 66 items (the two-deep item pipeline drains at 64) and of several chunks."""
    LPBatch, cus = dev
    inst, _ = assert_chunk_reach(R, cus, exact=exact)
    _check_replicas(LPBatch, golden, inst, R, f"chunkbase x {R}", direct=R == min(R_LISTS))


@gpu
def test_block_laps_against_oracle(dev, golden):
    """I. more than 2 * gp block rows in one partition, in both geometries and both orientations."""
    LPBatch, cus = dev
    _check_block_laps(LPBatch, golden, cus)


def _check_block_laps(LPBatch, golden, cus, make=None, poison=False):
    """the laps instance of a grid of `cus` workgroups: the whole step, then a spotlight on a row of the third lap"""
    inst, _ = assert_laps_reach(cus)
    sd = _sd(golden)
    r = _oracle(sd, [inst], "blocklaps")
    b, p = _check_step(LPBatch, [inst], sd, r, "blocklaps", make=make, poison=poison)
    dz = np.zeros(inst.n)
    last = int(np.argsort(-fc.degrees(inst)[0], kind="stable")[2 * fc.grid_per_partition(cus)])     # a row of the third lap
    hot = fc.one_hop(inst, "A", last)
    dz[hot] = 1.0
    rs = _oracle(sd, [inst], "blocklaps, spotlight on a row of the third lap", dlogits=dz)
    b.forward(p, **(_poison(b, "logits") if poison else {}))
    g = b.backward(p, torch.tensor(dz, dtype=torch.float32, device="cuda"), **({"grads": _nan(4721)} if poison else {}))
    g = g.cpu().numpy()
    close(g[grad_mask()], rs["grads"][grad_mask()], RTOL_GRAD, "blocklaps: spotlight gradients")
    return b


@gpu
def test_sharp_cases_against_oracle(dev):
    """J. ascending and descending coefficients along rows of the group, wave and block tiers, scores scaled."""
    LPBatch, cus = dev
    inst, sd, r = assert_sharp_reach(cus)
    _check_step(LPBatch, [inst], sd, r, "sharp")


DEGENERATE = {
    "no_nonzeros": lambda: [fc.empty_instance(5, 7, 1), fc.empty_instance(1, 1, 2), fc.empty_instance(70, 3, 3)],
    "one_by_one": lambda: [fc.single_row_instance(1, 4)],
    "one_block_row": lambda: [fc.single_row_instance(6145, 5)],
}


@gpu
@pytest.mark.parametrize("case", list(DEGENERATE))
def test_degenerate_batches_against_oracle(dev, golden, case):
    """K. nnz == 0 (the sweeps' unconditional loads read entry 0 of arrays that fused_graph_build allocates with room for
    one entry), a 1 x 1 instance, one row of 6145 nonzeros and nothing else."""
    LPBatch, cus = dev
    insts = DEGENERATE[case]()
    if case == "no_nonzeros":
        assert sum(i.nnz for i in insts) == 0
    if case == "one_block_row":
        assert insts[0].nnz > fc.constants()["T1"][2] + fc.step_widths("1")["block"] // 3
    for inst in insts:
        _show(inst.name, fc.census(inst, cus))
    sd = _sd(golden)
    r = _oracle(sd, insts, case)
    _check_step(LPBatch, insts, sd, r, case)
