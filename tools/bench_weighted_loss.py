"""The weighted loss head on the full Netlib batch, both whole-model paths, all in one process: mllp_gnn_loss_step_weighted
(balanced pos_weight, inst_weight 1 / n_inst) against mllp_gnn_loss_step, the pair forward + backward that the weighted step
is built from, mllp_weighted_loss alone (all three outputs; per-instance losses only; the loss only, and the loss only through the
C ABI without a buffer for the per-instance losses) and LPBatch.evaluate.  Method of
tools/bench_input_grads_paths.py: device events around one call, median of --iters calls after a warm-up; the
configurations alternate over --rounds rounds, and the spread of a configuration is (max - min) / median of its rounds.
Prints one JSON line.

    python tools/bench_weighted_loss.py [--iters 50] [--rounds 5]
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
    w = 1.0 / b1.n_inst
    bufs = {}
    for b in (b1, b2):
        b.balanced_pos_weight()
        bufs[b.token] = b.loss_step_weighted(params, w, "balanced")      # (reused below: no allocation inside the timing)
    z = b2.forward(params).clone()
    dl = torch.randn(b1.N, device="cuda")

    def weighted(b):
        loss, logits, grads, inst_loss = bufs[b.token]
        return lambda: b.loss_step_weighted(params, w, "balanced", logits, loss, inst_loss, grads)

    def plain(b):
        loss, logits, grads, _ = bufs[b.token]
        return lambda: b.loss_step(params, w, logits, loss, grads)

    def pair(b):
        _, logits, grads, _ = bufs[b.token]
        return lambda: (b.forward(params, logits), b.backward(params, dl, grads))

    from mllp_amd import _lib
    wt, pw, lo = b2._per_instance(w, "bench", "w"), b2.balanced_pos_weight(), torch.zeros(1, device="cuda")

    def serial():
        _lib.check(_lib.lib().mllp_weighted_loss(b2._h, _lib.ptr(z), _lib.ptr(b2.labels), _lib.ptr(wt), _lib.ptr(pw), None, None,
                                                 _lib.ptr(lo), _lib.current_stream()))

    configs = {
        "p1_loss_step_ms": plain(b1), "p1_loss_step_weighted_ms": weighted(b1), "p1_fwd_backward_ms": pair(b1),
        "p2_loss_step_ms": plain(b2), "p2_loss_step_weighted_ms": weighted(b2), "p2_fwd_backward_ms": pair(b2),
        "weighted_loss_all_outputs_ms": lambda: b2.weighted_loss(z, w, "balanced"),
        "weighted_loss_inst_loss_only_ms": lambda: b2.weighted_loss(z, None, "balanced", want="inst_loss"),
        "weighted_loss_loss_only_ms": lambda: b2.weighted_loss(z, w, "balanced", want="loss"),
        "weighted_loss_c_abi_loss_without_inst_loss_ms": serial,       # one workgroup takes the instances in turn
        "p2_forward_ms": lambda: b2.forward(params, bufs[b2.token][1]),
        "p2_evaluate_ms": lambda: b2.evaluate(params, "balanced"),
    }
    rounds = {k: [] for k in configs}
    for _ in range(args.rounds):
        for k, fn in configs.items():
            rounds[k].append(timed(fn, args.iters))
    out = {"batch": "netlib97", "nnz": b1.nnz, "N": b1.N, "n_inst": b1.n_inst, "max_inst_n": max(b1.inst_n),
           "iters": args.iters, "rounds": args.rounds}
    for k, v in rounds.items():
        out[k] = float(np.median(v))
        out[k.replace("_ms", "_spread")] = float((max(v) - min(v)) / np.median(v))
    for p in ("p1", "p2"):
        out[f"{p}_weighted_over_plain"] = out[f"{p}_loss_step_weighted_ms"] / out[f"{p}_loss_step_ms"]
        out[f"{p}_weighted_minus_pair_ms"] = out[f"{p}_loss_step_weighted_ms"] - out[f"{p}_fwd_backward_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
