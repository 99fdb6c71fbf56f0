"""Cost of normalizing a resident batch on the device (mllp_graph_normalize) beside the floor it sits on and the host round
trip it replaces, on the full Netlib batch.  Prints one JSON line (profiles/normalize_bench.json).

    python tools/bench_normalize.py [--iters 50] [--round-trips 10] [--synthetic-inst 0]

Every figure is the median of host-clock windows that start and end in a device synchronise:
  normalize_us        LPBatch.normalize(): row scales, objective scales, x1 / x2, the scaled values, every copy refreshed
  set_values_us       LPBatch.set_values() alone: the refresh that normalize ends in
  round_trip_s        what a user did before: export(2) and x1 / x2 to the host, the stage in numpy (fp64), from_instances
--synthetic-inst N > 0 adds the scales alone (compute only: the row kernel reads every value once, the objective kernel is
one workgroup per instance) on the synthetic batch of N instances, with the bytes per second of the values read.
"""
import argparse
import dataclasses
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def host_median(fn, iters, warmup=3):
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


def numpy_normalize(inst, values, coefs, rhs, cap=5.0):
    """oracle/mps_norm.py's rule on one instance's arrays, fp64."""
    q = np.zeros(inst.m)
    nz = np.diff(inst.indptr) > 0
    if values.size:
        q[nz] = np.add.reduceat(values * values, inst.indptr[:-1][nz])
    nrm = np.sqrt(q)
    s = np.where(nrm > 0, 1.0 / np.where(nrm > 0, nrm, 1.0), 1.0)
    over = np.abs(rhs * s) > cap
    s = np.where(over, cap / np.where(over, rhs, 1.0), s)
    cn = np.linalg.norm(coefs)
    return dataclasses.replace(inst, values=values * np.repeat(s, np.diff(inst.indptr)), rhs=rhs * s,
                               coefs=coefs / (cn if cn > 0 else 1.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--round-trips", type=int, default=10)
    ap.add_argument("--synthetic-inst", type=int, default=0)
    args = ap.parse_args()
    from mllp_amd.data import load_packed
    from mllp_amd.graph import LPBatch, synthetic_batch
    assert torch.cuda.is_available(), "bench_normalize needs the GPU: there is no CPU path"
    insts = load_packed()
    b = LPBatch.from_instances(insts)
    values = torch.tensor(b.export(2), device="cuda")
    b.normalize()                                            # first call: allocates, builds the maps
    torch.cuda.synchronize()

    def round_trip():
        v = b.export(2).astype(np.float64)
        x1, x2 = b.x1.cpu().numpy().astype(np.float64), b.x2.cpu().numpy().astype(np.float64)
        out, e, n, m = [], 0, 0, 0
        for i in insts:
            out.append(numpy_normalize(i, v[e:e + i.nnz], x1[n:n + i.n], x2[m:m + i.m]))
            e, n, m = e + i.nnz, n + i.n, m + i.m
        return LPBatch.from_instances(out)

    nrm = host_median(lambda: b.normalize(), args.iters)
    setv = host_median(lambda: b.set_values(values), args.iters)
    only = host_median(lambda: b.normalize(compute_only=True), args.iters)
    trip = host_median(round_trip, args.round_trips, warmup=1)
    out = {"batch": "netlib97", "instances": b.n_inst, "rows": b.M, "nnz": b.nnz, "iters": args.iters,
           "normalize_us": {k: round(x * 1e6, 1) for k, x in zip(("median", "min", "max"), nrm)},
           "set_values_us": {k: round(x * 1e6, 1) for k, x in zip(("median", "min", "max"), setv)},
           "scales_only_us": {k: round(x * 1e6, 1) for k, x in zip(("median", "min", "max"), only)},
           "round_trip_s": {k: round(x, 4) for k, x in zip(("median", "min", "max"), trip)}, "round_trips": args.round_trips,
           "round_trip_over_normalize": round(trip[0] / nrm[0], 1), "synthetic": "not taken"}
    del b
    if args.synthetic_inst > 0:
        sb = synthetic_batch(n_inst=args.synthetic_inst)
        sb.normalize(compute_only=True)
        med, lo, hi = host_median(lambda: sb.normalize(compute_only=True), args.iters)
        out["synthetic"] = {"instances": sb.n_inst, "rows": sb.M, "nnz": sb.nnz,
                            "scales_only_us": {"median": round(med * 1e6, 1), "min": round(lo * 1e6, 1), "max": round(hi * 1e6, 1)},
                            "values_read_GBps": round(4.0 * sb.nnz / med / 1e9, 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
