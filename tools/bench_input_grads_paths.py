"""Input gradients on the two whole-model paths, full Netlib batch, all in one process: the generic pair forward +
mllp_gnn_backward_inputs on path 1 (the only way before mllp_gnn_input_grads: the baseline) against forward +
mllp_gnn_input_grads and mllp_gnn_loss_step_inputs on the fused path 2, and mllp_gnn_loss_step on both paths for the
post-pass's share.  Method of tools/bench_input_grads.py (median of --iters host-timed iterations after a warm-up); the
configurations alternate over --rounds rounds, and the spread of a configuration is (max - min) / median of its rounds.
Prints one JSON line.

    python tools/bench_input_grads_paths.py [--iters 50] [--rounds 5]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_input_grads import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    from mllp_amd.data import load_packed
    from mllp_amd.graph import LPBatch
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "subset5.npz"))
    params = torch.tensor(gold["weights_flat"], dtype=torch.float32, device="cuda")
    inst = load_packed()
    b1 = LPBatch.from_instances(inst).set_path(1)
    b2 = LPBatch.from_instances(inst).set_path(2)
    dl = torch.randn(b1.N, device="cuda")
    for b in (b1, b2):                     # builds each graph's A^T -> A position map once
        b.loss_step_inputs(params)
    configs = {
        "p1_fwd_backward_inputs_ms": lambda: (b1.forward(params), b1.backward_inputs(params, dl)),      # baseline
        "p2_fwd_input_grads_ms": lambda: (b2.forward(params), b2.input_grads(params, dl)),
        "p2_fwd_backward_ms": lambda: (b2.forward(params), b2.backward(params, dl)),
        "p1_loss_step_inputs_ms": lambda: b1.loss_step_inputs(params),
        "p2_loss_step_inputs_ms": lambda: b2.loss_step_inputs(params),
        "p2_loss_step_inputs_values_only_ms": lambda: b2.loss_step_inputs(params, x1=False, x2=False),
        "p1_loss_step_ms": lambda: b1.loss_step(params),
        "p2_loss_step_ms": lambda: b2.loss_step(params),
    }
    rounds = {k: [] for k in configs}
    for _ in range(args.rounds):
        for k, fn in configs.items():
            rounds[k].append(timed(fn, args.iters))
    out = {"batch": "netlib97", "nnz": b1.nnz, "iters": args.iters, "rounds": args.rounds}
    for k, v in rounds.items():
        out[k] = float(np.median(v))
        out[k.replace("_ms", "_spread")] = float((max(v) - min(v)) / np.median(v))
    out["fused_pair_over_baseline"] = out["p2_fwd_input_grads_ms"] / out["p1_fwd_backward_inputs_ms"]
    out["fused_loss_step_inputs_over_generic"] = out["p2_loss_step_inputs_ms"] / out["p1_loss_step_inputs_ms"]
    out["p2_post_pass_ms"] = out["p2_loss_step_inputs_ms"] - out["p2_loss_step_ms"]
    out["p1_post_pass_ms"] = out["p1_loss_step_inputs_ms"] - out["p1_loss_step_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
