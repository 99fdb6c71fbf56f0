#!/usr/bin/env python3
"""Every output of the calls whose sums take the fixed order of csrc/ordered_sum.h (normalize, plant_basis, certificate,
balanced_pos_weight, weighted_loss), written to one .npz: the material for a bit-for-bit comparison of two builds of the
library.  None of these bits depend on the CU count or the batch, so two builds that differ anywhere differ by a defect.
The library is chosen through MLLP_LIB as in tools/fused_dump.py (a name under mllp_amd/csrc or an absolute path).

Inputs (every tier, both sides of 64 | 65 and 1024 | 1025, on rows and on columns): test_normalize._tails_instance(),
planted_oracle.ragged_case() whole and its big instance alone, the five golden instances as one batch.  The ragged cases
are planted with their own pivots and numbers first; the other calls then run on whatever the batch holds.

usage: python3 tools/ordered_dump.py OUT.npz"""
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
    import planted_oracle as po
    import test_normalize
    from mllp_amd.data import SUBSET5, load_packed
    from mllp_amd.graph import LPBatch

    def dev(a, dtype=torch.float32):
        return torch.tensor(np.asarray(a), dtype=dtype, device="cuda")

    def from_case(c):
        zeros = lambda n: torch.zeros(n, device="cuda")      # noqa: E731
        return LPBatch.from_device_csr(c["inst_m"], c["inst_n"], dev(c["ptr"], torch.int32), dev(c["idx"], torch.int32),
                                       dev(c["val"]), zeros(c["N"]), zeros(c["M"]), zeros(c["N"]))

    cases = {"ragged": po.ragged_case(), "big_alone": po.ragged_case(which=[4])}
    batches = {"tails": lambda: LPBatch.from_instances([test_normalize._tails_instance()[0]]),
               "ragged": lambda: from_case(cases["ragged"]), "big_alone": lambda: from_case(cases["big_alone"]),
               "subset5": lambda: LPBatch.from_instances(load_packed(SUBSET5))}
    out = {}

    def keep(key, tensors):
        for i, t in enumerate(tensors):
            out[f"{key}.{i}"] = t.detach().cpu().numpy().copy() if isinstance(t, torch.Tensor) else np.array(t)

    def state(b):
        torch.cuda.synchronize()
        return [b.export(2), b.export(5), b.x1, b.x2, b.labels]

    for name, make in batches.items():
        b = make()
        if name in cases:
            c = cases[name]
            b.plant_basis(dev(c["pivot"], torch.int32), dev(c["xstar"]), dev(c["ystar"]), dev(c["slack"]), po.DOMINANCE, po.FLOOR)
            keep(f"{name}.plant", state(b))
            keep(f"{name}.certificate", [b.certificate(dev(c["xstar"]) * b.labels, dev(c["ystar"]))])
        keep(f"{name}.scales_only", b.normalize(compute_only=True))
        keep(f"{name}.pos_weight", [b.balanced_pos_weight()])
        z = torch.randn(b.N, generator=torch.Generator().manual_seed(7), dtype=torch.float32).cuda()
        w = (np.random.default_rng(5).random(b.n_inst) * 2.0).astype(np.float32)
        w[min(1, b.n_inst - 1)] = 0.0
        got = b.weighted_loss(z, dev(w), "balanced")
        keep(f"{name}.weighted", [got["loss"], got["inst_loss"], got["dlogits"]])
        keep(f"{name}.weighted_serial", [b.weighted_loss(z, dev(w), "balanced", want="loss")["loss"]])
        scales = b.normalize()
        keep(f"{name}.normalize", state(b)[:4] + list(scales))
        print(f"[ordered_dump] {name}: {len(out)} arrays so far", flush=True)
    np.savez(out_path, **out)
    print(f"[ordered_dump] wrote {len(out)} arrays to {out_path}")
    return 0


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.exit(dump(sys.argv[1]))
