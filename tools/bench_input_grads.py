"""Cost of the input gradients: forward + mllp_gnn_backward against forward + mllp_gnn_backward_inputs (all three
inputs, and edge values only) on the full Netlib batch, generic sweeps (path 1).  Prints one JSON line.

    python tools/bench_input_grads.py [--iters 50]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for _ in range(iters):
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        ms.append(ev[0].elapsed_time(ev[1]))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    from mllp_amd.data import load_packed
    from mllp_amd.graph import LPBatch
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "subset5.npz"))
    params = torch.tensor(gold["weights_flat"], dtype=torch.float32, device="cuda")
    b = LPBatch.from_instances(load_packed())
    b.set_path(1)
    dl = torch.randn(b.N, device="cuda")
    b.forward(params)
    b.backward_inputs(params, dl)          # builds the graph's A^T -> A position map once
    out = {
        "batch": "netlib97", "nnz": b.nnz, "path": 1, "iters": args.iters,
        "fwd_ms": timed(lambda: b.forward(params), args.iters),
        "fwd_bwd_ms": timed(lambda: (b.forward(params), b.backward(params, dl)), args.iters),
        "fwd_bwd_inputs_ms": timed(lambda: (b.forward(params), b.backward_inputs(params, dl)), args.iters),
        "fwd_bwd_values_only_ms": timed(lambda: (b.forward(params), b.backward_inputs(params, dl, x1=False, x2=False)),
                                        args.iters),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
