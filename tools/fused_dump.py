#!/usr/bin/env python3
"""Every output of a fixed list of calls on the fused latency-regime path (set_path(2)), written to one .npz: the
material for a bit-for-bit comparison of two builds of the library on the same card (the bits depend on the CU count, so
no committed file can pin them).  The library is chosen through MLLP_LIB as in tools/profile_step.py (a name under
mllp_amd/csrc or an absolute path).

Inputs: the four tier instances of tests/test_fused_l3_pair.py (fused_cases.L3_TIER_CASES), fused_cases.ragged_batch()
and the five golden instances (as ONE batch: each instance's rows still carry their own outputs).  Calls: forward; forward + backward from a seeded dlogits; loss_step; three train_steps
(parameters and both Adam moments after the third); forward + input_grads; loss_step_inputs; the weighted loss step of
tests/test_weighted_loss.py (seeded instance weights with one zero, pos_weight "balanced").

usage: python3 tools/fused_dump.py OUT.npz"""
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def dump(out_path):
    import torch
    if os.environ.get("MLLP_LIB"):
        from mllp_amd import _lib
        _lib.LIB_PATH = os.path.join(ROOT, "mllp_amd", "csrc", os.environ["MLLP_LIB"])
    import fused_cases as fc
    from mllp_amd.data import SUBSET5, load_packed
    from mllp_amd.graph import LPBatch

    gold = np.load(os.path.join(ROOT, "tests", "golden", "subset5.npz"), allow_pickle=False)
    p0 = torch.tensor(gold["weights_flat"], dtype=torch.float32, device="cuda")
    batches = {name: [fc.l3_tier_instance(name)] for name in fc.L3_TIER_CASES}
    batches["ragged"] = fc.ragged_batch()
    batches["subset5"] = load_packed(SUBSET5)
    out = {}

    def keep(key, tensors):
        for i, t in enumerate(tensors):
            if t is not None:
                out[f"{key}.{i}"] = t.detach().cpu().numpy().copy()

    for name, insts in batches.items():
        fused = lambda: LPBatch.from_instances(insts).set_path(2)      # noqa: E731  (a fresh workspace per call sequence)
        n_var = sum(i.n for i in insts)
        dz = torch.randn(n_var, generator=torch.Generator().manual_seed(7), dtype=torch.float32).cuda()
        b = fused()
        keep(f"{name}.forward", [b.forward(p0)])
        keep(f"{name}.backward", [b.backward(p0, dz)])
        keep(f"{name}.loss_step", fused().loss_step(p0))
        b = fused()
        p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
        state = torch.tensor([0.0, 1e-3, 0.9, 0.999], device="cuda")
        for k in range(3):
            keep(f"{name}.train_step{k}", b.train_step(p, m, v, state, 1e-8, param_gen=k))
        keep(f"{name}.adam", [p, m, v, state])
        b = fused()
        b.forward(p0)
        keep(f"{name}.input_grads", b.input_grads(p0, dz))
        keep(f"{name}.loss_step_inputs", fused().loss_step_inputs(p0))
        w = (np.random.default_rng(5).random(len(insts)) * 2.0).astype(np.float32)
        w[min(1, len(insts) - 1)] = 0.0 if len(insts) > 1 else w[0]
        keep(f"{name}.weighted", fused().loss_step_weighted(p0, torch.tensor(w, device="cuda"), "balanced"))
        torch.cuda.synchronize()
        print(f"[fused_dump] {name}: {len(out)} arrays so far", flush=True)
    np.savez(out_path, **out)
    print(f"[fused_dump] wrote {len(out)} arrays to {out_path}")
    return 0


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.exit(dump(sys.argv[1]))
