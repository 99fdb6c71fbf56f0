"""The fused layer-3 launch of a loss step (fused_kernels.hip::fused_l3_kernel): layer 3's forward sweep, fc, BCE and the
destination-major backward sweep of the same rows run per item in one kernel, and Z / aux of gconv3_w2s, h3v and d3v are
no longer written.  `loss_step` and `train_step` on the fused path (set_path(2)) go through it; everything else keeps the
two kernels it replaces.

1. Tier cases: single-instance batches diag(B, C^T) (fused_cases.two_sided) whose VARIABLE-side degrees -- the rows of the
   launch -- are those of C's rows: degree 0, 1, 4, 5, 16 (base tier, one and several steps, a last item that is partial),
   17 and 64 (group), 65 and 1024 (wave), 1025 and 6145 = 2 * 768 * 4 + 1 (block tier, two and nine workgroup steps).
   Logits, loss and every parameter tensor's gradient against the fp64 oracle at the suite's bars, two runs bit for bit,
   and train_step == loss_step + adam_step bit for bit.
2. The same bitwise checks on the five golden instances, and `input_grads` after a `loss_step` on the same workspace.

Yardstick of the bars (fused_cases.model_dt in fp32 against fp64 on the CPU, max|diff| / max|ref|; logits, loss, all
gradients, worst tensor on its own scale) -- asserted below, by a test that needs no GPU, to stay under a quarter of
RTOL_ACT / RTOL_GRAD:

  base     3.1e-07  3.2e-08  9.2e-08  1.9e-06
  group    4.6e-07  1.0e-07  7.2e-08  9.3e-07
  wave     6.6e-07  9.0e-08  1.2e-07  3.2e-06
  block    1.8e-07  1.2e-08  1.4e-07  1.8e-06

The yardstick exempts no tensor on any of the four inputs (max_exempt = 0).

No comparison with `forward` + `backward(dlogits)` bit for bit: the BCE gradient the library used is not readable without
a new export (d3v is no longer stored, and a dlogits recomputed in torch differs from the kernel's expf by an ulp).  The
equality with the two launches this one replaces rests on the code: every half of a row (forward projection, sweep,
merges, epilogue; destination-major projection, sweep, merge, tail, statistics) is one function that fwd16_row, bwd16_row
and l3_row all call, and fused_l3_kernel uses fused_fwd16_kernel's item walk.  The by-hand comparisons against the parent
builds are recorded in profiles/fused_l3_pair.md (bench.py --dump-outputs: loss, logits and parameters identical after 25
steps) and profiles/fused_shared_rows.md (the same, and every output of tools/fused_dump.py).
"""
import numpy as np
import pytest
import torch

import fused_cases as fc
import grad_scales as gs
from oracle import pyg_restatement as o1
from oracle import spmm_form as o2
from test_hip_parity import RTOL_ACT, RTOL_GRAD, close, close_elementwise, grad_mask
from test_input_grads import oracle_input_grads

gpu = pytest.mark.gpu

CASES = fc.L3_TIER_CASES
_instance = fc.l3_tier_instance


def _assert_reach(name, inst, cus):
    degs, _, tier = CASES[name]
    c = fc.constants()
    T = c["T16"]
    cols = fc.degrees(inst)[1]
    assert set(degs) <= set(cols.tolist())
    t = fc.census(inst, cus)["At"]["16"]["tiers"]
    print("\n" + "\n".join(fc.census_lines(inst.name, fc.census(inst, cus))))
    assert t[tier] > 0, (name, t)
    if name == "base":
        assert t["group"] == t["wave"] == t["block"] == 0 and t["base"] % 16 != 0, t
        assert {0, 1, 4, 5, T[0]} <= set(cols.tolist())
    if name == "group":
        assert {T[0] + 1, T[1]} <= set(cols.tolist()) and t["group"] % 4 != 0 and t["wave"] == t["block"] == 0, t
    if name == "wave":
        assert {T[1] + 1, T[2]} <= set(cols.tolist()) and t["block"] == 0, t
    if name == "block":
        w = fc.step_widths("16", c)["block"]
        assert T[2] + 1 in cols and (cols > 2 * w * 4).any() and t["block"] == 2, t
        assert -(-(T[2] + 1) // w) == 2 and -(-int(cols.max()) // w) > 2


@pytest.fixture(scope="module")
def dev():
    from mllp_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available()
    from mllp_amd.graph import LPBatch
    return LPBatch, torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def sd(golden):
    return {k: v.numpy() for k, v in o1.unflatten_state(torch.tensor(golden["weights_flat"])).items()}


def _params(sd):
    flat = o1.flatten_state({k: torch.as_tensor(v) for k, v in sd.items()}).numpy()
    return torch.tensor(flat, dtype=torch.float32, device="cuda")


def _fused(LPBatch, insts):
    return LPBatch.from_instances(insts).set_path(2)


def _adam_state(p):
    return torch.zeros_like(p), torch.zeros_like(p), torch.tensor([0.0, 1e-3, 0.9, 0.999], device="cuda")


def _train_equals_loss_plus_adam(LPBatch, insts, p, what, steps=3):
    """train_step against loss_step + adam_step on a second batch: loss, logits, gradients, parameters, both moments and
    the step counter bit for bit, over `steps` steps (the second and third reuse the weights the tail folded)"""
    from mllp_amd.graph import adam_step
    b0, b1 = _fused(LPBatch, insts), _fused(LPBatch, insts)
    p0, p1 = p.clone(), p.clone()
    (m0, v0, s0), (m1, v1, s1) = _adam_state(p0), _adam_state(p1)
    for k in range(steps):
        loss, logits, grads = b0.loss_step(p0)
        adam_step(p0, grads, m0, v0, s0, 1e-8)
        got = b1.train_step(p1, m1, v1, s1, 1e-8, param_gen=k)
        for a, w, n in zip((*got, p1, m1, v1, s1), (loss, logits, grads, p0, m0, v0, s0),
                           ("loss", "logits", "grads", "params", "exp_avg", "exp_avg_sq", "state")):
            assert torch.equal(a, w), f"{what}: train_step differs from loss_step + adam_step in {n}, step {k}"


def _yardstick(sd, inst):
    """(fp64 oracle result, per-tensor yardstick, worst fp32-against-fp64 figures: logits, loss, gradients, worst tensor)"""
    ob = o2.BatchCSR([inst])
    r = o2.gnn_forward_backward(sd, ob)
    r32 = fc.model_dt(sd, ob, np.float32)
    keep = grad_mask()
    yard = gs.yardstick(sd, ob)
    e = (fc.rel_err(r32["logits"], r["logits"]), abs(r32["loss"] - r["loss"]) / abs(r["loss"]),
         fc.rel_err(r32["grads"][keep], r["grads"][keep]), max(err for _, err in yard.values()))
    return r, yard, e


@pytest.mark.parametrize("name", list(CASES))
def test_cases_reach_their_tier_and_the_fp32_reference_keeps_the_bars(sd, name):
    """No GPU: at 256 CUs every case reaches the tier it is meant for, and the reference alone (model_dt in fp32 against
    fp64) stays under a quarter of every bar, with no tensor exempt from the per-tensor check."""
    inst = _instance(name)
    _assert_reach(name, inst, 256)
    _, yard, e = _yardstick(sd, inst)
    print(f"[yardstick] {name:6s} logits {e[0]:.1e}  loss {e[1]:.1e}  gradients {e[2]:.1e}  worst tensor {e[3]:.1e}")
    assert e[0] < RTOL_ACT / 4 and e[1] < RTOL_ACT / 4 and e[2] < RTOL_GRAD / 4, (name, e)
    assert gs.exempt_tensors(yard) == [], name


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_tier_cases_against_oracle(dev, sd, name):
    LPBatch, cus = dev
    inst = _instance(name)
    _assert_reach(name, inst, cus)
    r, yard, e = _yardstick(sd, inst)
    keep = grad_mask()
    assert e[0] < RTOL_ACT / 4 and e[1] < RTOL_ACT / 4 and e[2] < RTOL_GRAD / 4, (name, e)
    p = _params(sd)
    b = _fused(LPBatch, [inst])
    loss, logits, grads = [t.clone() for t in b.loss_step(p)]
    print(f"[deviation] {name:6s} logits {fc.rel_err(logits.cpu().numpy(), r['logits']):.1e}  "
          f"loss {abs(float(loss) - r['loss']) / abs(r['loss']):.1e}  "
          f"gradients {fc.rel_err(grads.cpu().numpy()[keep], r['grads'][keep]):.1e}")
    close(logits.cpu().numpy(), r["logits"], RTOL_ACT, f"{name}: logits")
    close_elementwise(logits.cpu().numpy(), r["logits"], RTOL_ACT, f"{name}: logits, element-wise")
    close(loss.cpu().numpy(), [r["loss"]], RTOL_ACT, f"{name}: loss")
    close(grads.cpu().numpy()[keep], r["grads"][keep], RTOL_GRAD, f"{name}: gradients")
    table, _ = gs.close_per_tensor(grads.cpu().numpy(), r["grads"], yard, f"{name}: gradients", max_exempt=0)
    print("\n".join(gs.table_lines(name, table)))
    l2, z2, g2 = b.loss_step(p)
    assert torch.equal(l2, loss) and torch.equal(z2, logits) and torch.equal(g2, grads), f"{name}: not run-to-run exact"
    _train_equals_loss_plus_adam(LPBatch, [inst], p, name)


@gpu
def test_subset5_run_to_run_and_train_step(dev, subset5, golden):
    LPBatch, _ = dev
    p = torch.tensor(golden["weights_flat"], dtype=torch.float32, device="cuda")
    b = _fused(LPBatch, subset5)
    first = [t.clone() for t in b.loss_step(p)]
    for a, w in zip(b.loss_step(p), first):
        assert torch.equal(a, w)
    for a, w in zip(_fused(LPBatch, subset5).loss_step(p), first):       # another workspace, never written by a forward
        assert torch.equal(a, w)
    _train_equals_loss_plus_adam(LPBatch, subset5, p, "subset5")


@gpu
def test_input_grads_after_a_loss_step_on_the_same_workspace(dev, subset5, golden):
    """Two checks.  forward, loss_step, then input_grads from a given dlogits on the same workspace: that backward
    rewrites every record itself, so this half shows only that the loss step in between did not damage what it reads
    (h3v, Z and aux left by the forward).  The check of the records that the fused layer-3 launch writes is the second
    half: loss_step_inputs reads rec of gconv3_w2s as that launch left it."""
    LPBatch, _ = dev
    flat = golden["weights_flat"]
    p = torch.tensor(flat, dtype=torch.float32, device="cuda")
    rr = torch.randn(sum(i.n for i in subset5), generator=torch.Generator().manual_seed(21), dtype=torch.float64)
    _, ox1, ox2, odv, opg = oracle_input_grads(flat, subset5, lambda z: (z * rr).sum())
    b = _fused(LPBatch, subset5)
    b.forward(p)
    b.loss_step(p)
    grads, dx1, dx2, dv = b.input_grads(p, rr.float().cuda())
    keep = grad_mask()
    close(dx1.cpu().numpy(), ox1, RTOL_GRAD, "dx1")
    close(dx2.cpu().numpy(), ox2, RTOL_GRAD, "dx2")
    close(dv.cpu().numpy(), odv, RTOL_GRAD, "dvalues")
    close(grads.cpu().numpy()[keep], opg[keep], RTOL_GRAD, "parameter gradients")
    # the records of the fused launch: the input gradients of the loss itself
    ib = 1.0 / len(subset5)
    off = np.concatenate([[0], np.cumsum([i.n for i in subset5])])
    ys = [torch.tensor(np.asarray(i.basis), dtype=torch.float64) for i in subset5]

    def bce(z):
        z = z.reshape(-1)
        return ib * sum(torch.nn.functional.binary_cross_entropy_with_logits(z[off[k]:off[k + 1]], ys[k])
                        for k in range(len(subset5)))
    _, lx1, lx2, ldv, lpg = oracle_input_grads(flat, subset5, bce)
    _, _, g, dx1, dx2, dv = _fused(LPBatch, subset5).loss_step_inputs(p)
    close(dx1.cpu().numpy(), lx1, RTOL_GRAD, "loss step dx1")
    close(dx2.cpu().numpy(), lx2, RTOL_GRAD, "loss step dx2")
    close(dv.cpu().numpy(), ldv, RTOL_GRAD, "loss step dvalues")
    close(g.cpu().numpy()[keep], lpg[keep], RTOL_GRAD, "loss step parameter gradients")
