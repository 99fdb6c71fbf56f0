"""Cost of planting a basis in a resident batch (mllp_graph_plant_basis) and of certifying it (mllp_lp_certificate), beside
mllp_graph_normalize in the same run, on a planted batch of the synthetic batch's shape (256 instances of 10000 x 20000,
about 200 nonzeros per row).  Prints one JSON line (profiles/planted_bench.json).

    python tools/bench_planted.py [--instances 256] [--m 10000] [--n 20000] [--row-nnz 200] [--iters 10]

Every figure is the median of host-clock windows that start and end in a device synchronise.  normalize is the
like-for-like comparison: two sweeps (row scales, the scaled values) plus the refresh of every value-holding array, where
planting is validation, two sweeps (rows over CSR(A), columns over CSR(A^T)) plus the same refresh.

ALGORITHMIC BYTES per call, with nnz nonzeros, M rows, N columns (gathers counted once per nonzero at 4 bytes, row
pointers and per-row words once):
  refresh      (mllp_graph_set_values without re-blocked copies) copy nnz values: 8 nnz; A^T gather: position 4 + value 4 +
               store 4 = 12 nnz                                                                            -> 20 nnz
  plant        validate 4 N (owner cleared) + 12 M; rows: index 4 + value 4 + owner 4 + xstar 4 + new value 4 = 20 nnz,
               + 12 M; refresh 20 nnz; columns: index 4 + value 4 + ystar 4 = 12 nnz, + 16 N       -> 52 nnz + 24 M + 20 N
  certificate  rows: index 4 + value 4 + x 4 = 12 nnz, + 12 M; columns 12 nnz + 12 N; reduce 4 M + 12 N
                                                                                                    -> 24 nnz + 16 M + 24 N
  normalize    row scales: value 4 nnz + 12 M; objective 8 N; scaled values: value 4 + store 4 = 8 nnz (the row of a nonzero
               is found by bisection of the row pointers, cached); refresh 20 nnz                  -> 32 nnz + 12 M + 8 N
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def host_median(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    secs = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
    return float(np.median(secs)), float(np.min(secs)), float(np.max(secs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=256)
    ap.add_argument("--m", type=int, default=10000)
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--row-nnz", type=float, default=200.0)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    from mllp_amd.graph import LPBatch
    from mllp_amd.planted import _numbers, planted_pattern
    assert torch.cuda.is_available(), "bench_planted needs the GPU: there is no CPU path"
    dev = "cuda"
    t0 = time.perf_counter()
    inst_m, inst_n, ptr, idx, pivot = planted_pattern(args.instances, args.m, args.n, args.row_nnz, 1234, dev)
    nnz, M, N = int(idx.numel()), args.instances * args.m, args.instances * args.n
    g = torch.Generator(device=dev).manual_seed(99)
    val = torch.randn(nnz, device=dev, generator=g)
    _, xstar, ystar, slack = _numbers(7, 0, M, N, dev)
    b = LPBatch.from_device_csr(inst_m, inst_n, ptr, idx, val, torch.empty(N, device=dev), torch.empty(M, device=dev),
                                torch.empty(N, device=dev))
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    b.plant_basis(pivot, xstar, ystar, slack)                # first call: allocates, builds the maps
    x = xstar * b.labels
    cert = b.certificate(x, ystar)
    ok = bool((cert[:, 1] > 0).all() and (cert[:, 3] > 0).all() and (cert[:, 5] == args.m).all())
    worst = [float(cert[:, 0].max()), float(cert[:, 4].max())]
    plant = host_median(lambda: b.plant_basis(pivot, xstar, ystar, slack), args.iters)
    certt = host_median(lambda: b.certificate(x, ystar), args.iters)
    setv = host_median(lambda: b.set_values(val), args.iters)
    b.plant_basis(pivot, xstar, ystar, slack)
    b.normalize()
    norm = host_median(lambda: b.normalize(), args.iters)
    by = {"plant": 52 * nnz + 24 * M + 20 * N, "certificate": 24 * nnz + 16 * M + 24 * N, "normalize": 32 * nnz + 12 * M + 8 * N,
          "set_values": 20 * nnz}
    t = {"plant": plant, "certificate": certt, "normalize": norm, "set_values": setv}
    out = {"batch": f"planted {args.instances} x ({args.m} x {args.n})", "instances": args.instances, "rows": M, "cols": N,
           "nnz": nnz, "iters": args.iters, "build_s": round(build_s, 2), "certified": ok, "worst_residuals": worst}
    for k in t:
        out[k] = {"us": {a: round(v * 1e6, 1) for a, v in zip(("median", "min", "max"), t[k])}, "algorithmic_bytes": by[k],
                  "GBps": round(by[k] / t[k][0] / 1e9, 1)}
    out["plant_over_normalize"] = round(plant[0] / norm[0], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
