"""Every parameter tensor's gradient against the fp64 oracle ON ITS OWN SCALE (tests/grad_scales.py), on the whole-model
paths that have no per-layer entry point: the fused latency-regime path, the generic sweeps under forced tiers, the
one-launch small step, the streamed and LDS-tiled copies.

The gap this closes, as a test (test_old_check_accepts_zeroed_attention_tensors): on Netlib-97 the gradients of
gconv1_s2w.lin_key.weight and gconv1_s2w.lin_query.weight are 9.3e-6 and 3.1e-5 of the largest gradient, so the
whole-model check `close(grads[keep], ref[keep], 5e-5)` accepts ZEROS written into either; 12 of the 42 live tensors are
below 1e-3 of the largest.  The key, query and edge gradients are what the tier-specific backward sweeps produce (dqp, ds,
dt summed over rows), so a block-tier or merge bug that touches a few rows changes them and nothing else.

Bar: RTOL_GRAD = 5e-5 of tests/test_hip_parity.py, per tensor.  Yardstick: fused_cases.model_dt in fp32 against fp64, per
tensor; a tensor is checked on its own scale where the yardstick is below a quarter of the bar, and exempt (global bound
only) where it is not.  CAPS states how many tensors the reference alone exempts on each input, measured on the CPU for the
loss step and for the seed-5 dlogits; the only exemptions among the GPU inputs are gconv1_w2s.lin_query.weight on kb2
(1.8e-8 of the largest gradient, fp32 reference off by 6e-4), on sc50a (2.9e-8, 3.6e-4) and on the small step's ragged3,
which holds sc50a (7.8e-5, 1.3e-5): pure cancellation.  The 1 x 1 input of tests/test_small_step.py is no per-tensor
input (NOT_PER_TENSOR): with one nonzero per row every attention gradient is a cancellation to zero.  The batches of 7, 8
and 9 degree grids of different values of tests/test_fused_oracle.py are counted here too (GRID_BATCH_CAPS, loss step).

The degree grids run alone and as a batch of nine replicas with labels of their own (nine instances over the eight
partitions of the fused path); a batch of replicas computes the LP's own backward from the summed dL/dz
(test_replica_batch_identity), so its reference and yardstick cost one run of the LP.  The replicas are not shuffled:
they differ in their labels only, which are drawn at random for every one, so any order of them is the same kind of batch.

Worst own-scale deviation of the kernels over all checked tensors, per group, measured on an MI355X (loss step, seed-5
dlogits; the worst fp32 yardstick of the same inputs is 8.2e-06, 9.1e-06):

  fused        1.7e-05  1.2e-05    gconv1_s2w.lin_query.weight: sc50a (2.3e-6 of the largest gradient), blend (3.6e-5)
  generic      3.1e-06  3.5e-06
  small step   1.5e-05  -          gconv1_s2w.lin_query.weight on sc50a; the call has no backward entry
  copies       5.9e-07  1.3e-06    none / streamed / tiled: 5.2e-07 1.2e-06 / 5.9e-07 1.3e-06 / 5.8e-07 7.7e-07

Every figure is below the bar of 5e-05; without sc50a and blend no fused or small-step figure is above 5.3e-06.
"""
import numpy as np
import pytest
import torch

import fused_cases as fc
import grad_scales as gs
from mllp_amd.data import SUBSET5, load_packed
from oracle import pyg_restatement as o1
from oracle import spmm_form as o2
from test_hip_parity import RTOL_GRAD, close, grad_mask
from fused_cases import SMALL_CASE_NAMES, small_step_cases
from fused_cases import SMALL_PER_TENSOR_CAPS as SMALL_STEP_CAPS
from fused_cases import ragged_batch as _ragged_batch

gpu = pytest.mark.gpu

SINGLES = [n[:-4] for n in SUBSET5]                               # adlittle, afiro, blend, kb2, sc50a
N_REPLICAS = 9                                                    # over the 8 partitions of the fused path: one holds two
# exempt tensors that the fp32 reference alone needs, loss step and seed-5 dlogits alike (test_yardsticks_are_within_the_caps)
CAPS = {"subset5": 0, "afiro": 0, "adlittle": 0, "blend": 0, "ragged": 0, "grid0": 0, "grid1": 0, "chunkbase": 0,
        "kb2": 1, "sc50a": 1, "grid0x9": 0, "grid1x9": 0,
        }
# batches of grids of different values (tests/test_fused_oracle.py), loss step only: the caps live beside the inputs
GRID_BATCH_NAMES = {f"grid{v}+{n}": (v, n) for (v, n) in fc.GRID_BATCH_CAPS if n > 1}
CAPS.update({name: fc.GRID_BATCH_CAPS[key] for name, key in GRID_BATCH_NAMES.items()})
CAPS.update({"small:" + n: cap for n, cap in SMALL_STEP_CAPS.items() if n not in SUBSET5})
assert all(SMALL_STEP_CAPS[n + ".mps"] == CAPS[n] for n in SINGLES)
NOT_PER_TENSOR = {"1x1": 3}               # input of test_small_step.py -> exempt tensors of its loss step
Q1 = "gconv1_w2s.lin_query.weight"
EXEMPT_NAMED = {"kb2": {Q1}, "sc50a": {Q1}, "small:ragged3": {Q1}}


def _sd(golden):
    return {k: v.numpy() for k, v in o1.unflatten_state(torch.tensor(golden["weights_flat"])).items()}


def _replicas(base, R=N_REPLICAS):
    """R replicas of an LP as one batch, every replica with labels of its own (fused_cases.replicate draws them anew)"""
    return [fc.replicate(base, 1, name=f"{base.name}r{k}", basis_seed=100 + k) for k in range(R)]


def _summed_dlogits(sd, base, insts, dz):
    """A batch of replicas of one LP computes that LP's backward from the sum of the replicas' dL/dz (exact: the replicas
    share every activation; test_replica_batch_identity); for the loss step dL/dz is the BCE gradient of every replica's
    own labels, (sigmoid(z) - y_k) / (n R)."""
    R = len(insts)
    if dz is not None:
        return dz.astype(np.float64).reshape(R, base.n).sum(0)
    z = o2.gnn_forward_backward(sd, o2.BatchCSR([base]), want_grads=False)["logits"]
    return sum((1.0 / (1.0 + np.exp(-z)) - i.basis) / (base.n * R) for i in insts)


class Refs:
    """name -> instances, weights, and per mode ("loss", "dz"): dlogits, fp64 oracle gradients, fp32 yardstick.  Computed
    once per session, shared, never modified."""

    def __init__(self, golden, subset5):
        sd = _sd(golden)
        by = {i.name[:-4]: i for i in subset5}
        self.build = {"subset5": lambda: (sd, list(subset5)), "ragged": lambda: (sd, _ragged_batch()),
                      "grid0": lambda: (sd, [fc.degree_grid(0)]), "grid1": lambda: (sd, [fc.degree_grid(1)]),
                      "grid0x9": lambda: (sd, _replicas(fc.degree_grid(0))), "grid1x9": lambda: (sd, _replicas(fc.degree_grid(1))),
                      "chunkbase": lambda: (sd, [fc.chunk_base()])}
        for n in SINGLES:
            self.build[n] = lambda n=n: (sd, [by[n]])
        for n, key in GRID_BATCH_NAMES.items():
            self.build[n] = lambda key=key: (sd, fc.grid_batch(*key))
        for n, sd_n, insts in small_step_cases(golden, subset5):
            self.build["small:" + n] = lambda sd_n=sd_n, insts=insts: (sd_n, insts)
        self.inputs, self.refs = {}, {}

    def input(self, name):
        if name not in self.inputs:
            sd, insts = self.build[name]()
            # the reference of a batch of replicas is computed on the LP itself (_summed_dlogits)
            self.inputs[name] = (sd, insts, None if name.endswith("x9") else o2.BatchCSR(insts))
        return self.inputs[name]

    def __call__(self, name, mode):
        if (name, mode) not in self.refs:
            sd, insts, ob = self.input(name)
            N = sum(i.n for i in insts)
            dz = (np.random.default_rng(5).standard_normal(N) / max(N, 1)).astype(np.float32) if mode == "dz" else None
            dz64 = None if dz is None else dz.astype(np.float64)
            if ob is None:
                base = self.input(name[:-2])[1][0]
                ob, dz64 = o2.BatchCSR([base]), _summed_dlogits(sd, base, insts, dz)
            want = o2.gnn_forward_backward(sd, ob, dlogits=dz64)["grads"]
            want.setflags(write=False)
            self.refs[(name, mode)] = (dz, want, gs.yardstick(sd, ob, dz64))
        return self.refs[(name, mode)]


@pytest.fixture(scope="session")
def refs(golden, subset5):
    return Refs(golden, subset5)


FUSED_INPUTS = ["subset5"] + SINGLES + ["grid0", "grid1", "grid0x9", "grid1x9", "chunkbase"]
GENERIC_CASES = [("subset5", (1024, 4096)), ("subset5", (64, 256)), ("subset5", (8, 64)), ("grid0", (0, 0))]
SMALL_INPUTS = SINGLES + ["small:" + n for n in SMALL_CASE_NAMES if n not in SUBSET5 and n not in NOT_PER_TENSOR]
assert set(SMALL_CASE_NAMES) - set(SMALL_STEP_CAPS) == set(NOT_PER_TENSOR)
COPY_CONFIGS = ["none", "streamed_all", "tiled"]
GROUPS = {"fused": (FUSED_INPUTS, ("loss", "dz")), "generic": (sorted({n for n, _ in GENERIC_CASES}), ("loss", "dz")),
          "small step": (SMALL_INPUTS, ("loss",)), "copies": (["ragged"], ("loss", "dz"))}


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the helper against the old check, the yardsticks of every input, coverage
# ---------------------------------------------------------------------------------------------------------------------
def test_tensor_slices_partition_the_state_dict():
    live, key_bias, unused = gs.tensor_slices()
    seen = np.zeros(4721, int)
    for s in list(live.values()) + list(key_bias.values()) + list(unused.values()):
        seen[s] += 1
    assert (seen == 1).all()
    keep = grad_mask()
    for s in key_bias.values():
        assert not keep[s].any()
    assert all(n.startswith("gconv3_s2w.") for n in unused) and "fc.weight" in live and "fc.bias" in live


def _mutations(want, s):
    zeros, scaled = want.copy(), want.copy()
    zeros[s] = 0.0
    scaled[s] = want[s] * (1 + 1e-3)
    return (("zeros", zeros), ("times 1 + 1e-3", scaled))


def test_every_mutation_of_a_checked_tensor_fails_subset5(refs):
    """fp64 oracle gradients of subset5 with one live tensor replaced by zeros, or scaled by 1 + 1e-3: close_per_tensor
    fails for every one; the unmutated gradients pass; a nonzero in gconv3_s2w fails."""
    _, want, yard = refs("subset5", "loss")
    assert not gs.exempt_tensors(yard)
    table, checked = gs.close_per_tensor(want, want, yard, "subset5, unmutated", max_exempt=0)
    assert len(checked) == 42 and all(dev == 0.0 for _, _, dev in table.values())
    live, _, unused = gs.tensor_slices()
    for name, s in live.items():
        for how, got in _mutations(want, s):
            with pytest.raises(AssertionError, match=name.replace(".", r"\.")):
                gs.close_per_tensor(got, want, yard, f"{name} {how}", max_exempt=0)
    got = want.copy()
    got[next(iter(unused.values()))][3] = 1e-30
    with pytest.raises(AssertionError, match="not exactly zero"):
        gs.close_per_tensor(got, want, yard, "gconv3_s2w", max_exempt=0)
    # an exempt tensor is not checked on its own scale, and more exempt tensors than the cap is an error of its own
    name = "gconv2_w2s.lin_query.weight"
    loose = dict(yard, **{name: (yard[name][0], RTOL_GRAD / 4)})
    with pytest.raises(AssertionError, match="cap 0"):
        gs.close_per_tensor(want, want, loose, "one exempt, cap 0", max_exempt=0)
    _, checked = gs.close_per_tensor(_mutations(want, live[name])[1][1], want, loose, "one exempt, cap 1", max_exempt=1)
    assert checked == set(live) - {name}


@pytest.fixture(scope="module")
def netlib_grads(golden):
    r = o2.gnn_forward_backward(_sd(golden), o2.BatchCSR(load_packed()))
    return r["grads"]


def test_every_mutation_of_a_live_tensor_fails_netlib97(netlib_grads):
    """The same on Netlib-97, sizes only: the fp32 restatement sums 8 M terms one after the other there (own-scale error
    up to 1.7e-4), so the full batch has no per-tensor yardstick and every tensor counts as checked."""
    want = netlib_grads
    sizes = gs.own_scale_errors(want, want)
    yard = {name: (size, 0.0) for name, (size, _) in sizes.items()}
    gs.close_per_tensor(want, want, yard, "Netlib-97, unmutated", max_exempt=0)
    for name, s in gs.tensor_slices()[0].items():
        for how, got in _mutations(want, s):
            with pytest.raises(AssertionError, match=name.replace(".", r"\.")):
                gs.close_per_tensor(got, want, yard, f"{name} {how}", max_exempt=0)


def test_old_check_accepts_zeroed_attention_tensors(netlib_grads):
    """THE GAP: the whole-model check of the suite passes with zeros in place of two tensors of Netlib-97.  If these asserts
    stop holding, the weights or the data changed: update the figures in the module docstring."""
    want = netlib_grads
    keep = grad_mask()
    sizes = gs.own_scale_errors(want, want)
    live = gs.tensor_slices()[0]
    for name in ("gconv1_s2w.lin_key.weight", "gconv1_s2w.lin_query.weight"):
        zeros = _mutations(want, live[name])[0][1]
        assert sizes[name][0] < RTOL_GRAD
        close(zeros[keep], want[keep], RTOL_GRAD, name)                   # passes: that is the gap
    small = sorted(n for n, (size, _) in sizes.items() if size < 1e-3)
    print(f"\nNetlib-97: {len(small)} of {len(sizes)} live tensors below 1e-3 of the largest gradient")
    assert len(small) == 12


ALL_INPUTS = sorted({n for names, _ in GROUPS.values() for n in names} | set(GRID_BATCH_NAMES))


@pytest.mark.parametrize("name", ALL_INPUTS)
def test_yardsticks_are_within_the_caps(refs, name):
    """What the reference alone needs: the number of tensors whose fp32 yardstick is not below a quarter of the bar, for
    the loss step and for the seed-5 dlogits."""
    for mode in ("loss",) if name in GRID_BATCH_NAMES else ("loss", "dz"):
        _, want, yard = refs(name, mode)
        ex = gs.exempt_tensors(yard)
        if CAPS[name] is None:                              # stated as no per-tensor input, with its count
            assert len(ex) == fc.GRID_BATCH_EXEMPT_STATED[GRID_BATCH_NAMES[name]] > 2, (name, ex)
            continue
        worst = max(yard[n][1] for n in gs.checked_tensors(yard))
        print(f"\n[yardstick] {name} ({mode}): worst own-scale error of the {len(gs.checked_tensors(yard))} checked tensors "
              f"{worst:.1e}; exempt: " + (", ".join(f"{n} (size {yard[n][0]:.1e}, fp32 off by {yard[n][1]:.1e})" for n in ex) or "none"))
        assert len(ex) <= CAPS[name] <= 2, (name, mode, ex)
        if name in GRID_BATCH_NAMES:        # large bias tensors summed over 10^5 .. 10^6 rows; never a key, query or edge tensor
            assert all(n.endswith(("lin_skip.bias", "lin_value.bias")) for n in ex), (name, ex)
        else:
            assert set(ex) <= EXEMPT_NAMED.get(name, set()), (name, mode, ex)


def test_replica_batch_identity(golden):
    """what lets one oracle run of an LP stand for a batch of its replicas: the batch's gradients, computed directly"""
    sd, base = _sd(golden), fc.chunk_base()
    insts = _replicas(base, 3)
    assert len({i.basis.tobytes() for i in insts}) == 3
    dz = (np.random.default_rng(5).standard_normal(3 * base.n) / (3 * base.n)).astype(np.float32)
    for d in (None, dz):
        direct = o2.gnn_forward_backward(sd, o2.BatchCSR(insts), dlogits=None if d is None else d.astype(np.float64))["grads"]
        via = o2.gnn_forward_backward(sd, o2.BatchCSR([base]), dlogits=_summed_dlogits(sd, base, insts, d))["grads"]
        np.testing.assert_allclose(via, direct, rtol=1e-9, atol=1e-12 * np.abs(direct).max())


def test_small_step_inputs_left_out_are_no_per_tensor_inputs(refs):
    for name, stated in NOT_PER_TENSOR.items():
        n_ex = len(gs.exempt_tensors(refs("small:" + name, "loss")[2]))
        assert n_ex > 2 and n_ex == stated, (name, n_ex)


@pytest.mark.parametrize("group", list(GROUPS))
def test_every_live_tensor_is_checked_in_every_group(refs, group):
    names, modes = GROUPS[group]
    checked = set()
    for name in names:
        for mode in modes:
            yard = refs(name, mode)[2]
            checked |= gs.checked_tensors(yard)
    assert len(checked) == 42


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
    return LPBatch


def _params(sd):
    flat = o1.flatten_state({k: torch.as_tensor(v) for k, v in sd.items()}).numpy()
    return torch.tensor(flat, dtype=torch.float32, device="cuda")


def _check(refs, name, mode, got, what, group):
    _, want, yard = refs(name, mode)
    got = got.cpu().numpy()
    errs = gs.own_scale_errors(got, want)
    print("\n" + "\n".join(gs.table_lines(what, {n: (errs[n][0], yard[n][1], errs[n][1]) for n in yard})))
    on = gs.checked_tensors(yard)
    print(f"[worst] {group} | {what} | deviation {max(errs[n][1] for n in on):.2e} | yardstick {max(yard[n][1] for n in on):.2e}")
    return gs.close_per_tensor(got, want, yard, what, max_exempt=CAPS[name])


def _loss_and_backward(refs, b, p, name, what, group):
    """the loss step, then a backward from the seed-5 dlogits after a forward"""
    _check(refs, name, "loss", b.loss_step(p)[2], f"{what}: loss step", group)
    dz = refs(name, "dz")[0]
    b.forward(p)
    _check(refs, name, "dz", b.backward(p, torch.tensor(dz, device="cuda")), f"{what}: backward of the seed-5 dlogits", group)


@gpu
@pytest.mark.parametrize("name", FUSED_INPUTS)
def test_fused_path_per_tensor(dev, refs, name):
    sd, insts, _ = refs.input(name)
    b = dev.from_instances(insts).set_path(2)
    _loss_and_backward(refs, b, _params(sd), name, f"fused, {name}", "fused")


@gpu
@pytest.mark.parametrize("name,tiers", GENERIC_CASES, ids=[f"{n}-{t[0]}-{t[1]}" for n, t in GENERIC_CASES])
def test_generic_path_per_tensor(dev, refs, name, tiers):
    sd, insts, _ = refs.input(name)
    b = dev.from_instances(insts, tier_wave=tiers[0], tier_block=tiers[1]).set_path(1)
    _loss_and_backward(refs, b, _params(sd), name, f"generic, {name}, tiers {tiers}", "generic")


@gpu
@pytest.mark.parametrize("name", SMALL_INPUTS)
def test_small_step_per_tensor(dev, refs, name):
    sd, insts, _ = refs.input(name)
    b = dev.from_instances(insts)
    assert b.small_step_fits(), name
    _check(refs, name, "loss", b.train_step_small(_params(sd))[2], f"small step, {name}: loss step", "small step")


@gpu
@pytest.mark.parametrize("config", COPY_CONFIGS)
def test_copies_per_tensor(dev, refs, config):
    sd, insts, _ = refs.input("ragged")
    b = dev.from_instances(insts).set_path(1)
    if config == "streamed_all":
        infos = b.enable_stream_step(max_slots_per_nnz=float("inf"))
        assert sorted(infos) == [(tr, g) for tr in (False, True) for g in (1, 2, 3, 4)]
        assert not any(i.get("dropped") for i in infos.values())
    if config == "tiled":
        for k, i in b.enable_tiled_step().items():
            assert i is not None, k
    _loss_and_backward(refs, b, _params(sd), "ragged", f"copies {config}, ragged", "copies")
