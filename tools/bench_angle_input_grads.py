"""Cost of AngleModel's input gradients: mllp_angle_backward against mllp_angle_backward_inputs with dx only, dcos only
and both, on one Netlib instance (default 25fv47, N = 1 877) at feat_dim 256.  One forward fills the workspace (a
backward leaves what it reads unchanged), then the four calls are timed alternately, one call per event pair, after a
warm-up.  Prints one JSON line: median ms per call, the ratio to mllp_angle_backward, and the added HBM bytes.

    python tools/bench_angle_input_grads.py [--instance 25fv47] [--feat-dim 256] [--iters 20]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instance", default="25fv47")
    ap.add_argument("--feat-dim", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    from mllp_amd import _lib
    from mllp_amd.angle import AngleModel, build_graph_from_Q_sets, dense_instance_tensors
    from mllp_amd.data import load_packed
    from mllp_amd.model import set_seed
    inst = load_packed([args.instance])[0]
    Q, coefs, basis = dense_instance_tensors(inst)
    g = build_graph_from_Q_sets(Q, coefs, torch.device("cuda"), inst.name, basis)
    N, F = g.num_nodes, args.feat_dim
    set_seed(42)
    flat = AngleModel(feat_dim=F).to("cuda").flat_parameters().detach().contiguous()
    L, s = _lib.lib(), _lib.current_stream()
    ws = g.workspace(F)
    logits = torch.empty(N - 1, device="cuda")
    dl = torch.randn(N - 1, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)) / (N - 1)
    grads = torch.empty_like(flat)
    dx, dcos = torch.empty(N, 2, device="cuda"), torch.empty(N, N, device="cuda")
    base = (N, F, _lib.ptr(g.cos), _lib.ptr(g.x), _lib.ptr(flat), _lib.ptr(ws), _lib.ptr(dl), _lib.ptr(grads))
    _lib.check(L.mllp_angle_forward(N, F, _lib.ptr(g.cos), _lib.ptr(g.x), _lib.ptr(flat), _lib.ptr(ws), _lib.ptr(logits), s))
    calls = {
        "backward": lambda: L.mllp_angle_backward(*base, s),
        "inputs_dx": lambda: L.mllp_angle_backward_inputs(*base, _lib.ptr(dx), None, s),
        "inputs_dcos": lambda: L.mllp_angle_backward_inputs(*base, None, _lib.ptr(dcos), s),
        "inputs_both": lambda: L.mllp_angle_backward_inputs(*base, _lib.ptr(dx), _lib.ptr(dcos), s),
    }
    for _ in range(args.warmup):
        for fn in calls.values():
            _lib.check(fn())
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = {k: [] for k in calls}
    for _ in range(args.iters):                 # alternating: the four variants see the same machine state
        for k, fn in calls.items():
            ev[0].record()
            _lib.check(fn())
            ev[1].record()
            torch.cuda.synchronize()
            ms[k].append(ev[0].elapsed_time(ev[1]))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    nn = N * N * 4
    out = {
        "instance": inst.name, "N": N, "feat_dim": F, "iters": args.iters,
        "ms": {k: round(v, 4) for k, v in med.items()},
        "ratio_to_backward": {k: round(v / med["backward"], 4) for k, v in med.items()},
        # dcos: stored by the first layer application, loaded and stored by the other two; dx: the layer-1 dX GEMM reads
        # dO, dQ, dK, dV and writes [N, 2] (plus its split partial sums)
        "added_hbm_bytes": {"dcos": 5 * nn, "dx": 4 * N * F * 4 + N * 2 * 4},
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
