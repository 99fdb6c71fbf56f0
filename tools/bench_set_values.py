"""Cost of refreshing a batch's coefficients in place (mllp_graph_set_values) beside the rebuild it replaces, timed in
the same process and alternating with it.  Two cases:
  netlib97       the 97 Netlib instances on the fused path, no re-blocked copies; rebuild = LPBatch.from_instances
  synthetic256   the device-generated synthetic batch at its default size with the training step's eight streamed
                 copies (enable_stream_step); rebuild = LPBatch.from_device_csr + enable_stream_step
For each: the steady-state call, the one-off first call that builds the position maps, the bytes of the maps, the rebuild.
Prints one JSON line (kept under profiles/).

    python tools/bench_set_values.py [--iters 30] [--calls 10] [--rebuilds 5] [--synthetic-inst 256]

set_values: device events around `calls` back-to-back launches, divided by `calls`; median over `iters` windows after a
warm-up.  The rebuild is host work that ends in a synchronise: host clock around it, one rebuild every
iters / rebuilds windows.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def stats(xs, digits):
    return {"median": round(float(np.median(xs)), digits), "min": round(float(np.min(xs)), digits),
            "max": round(float(np.max(xs)), digits), "n": len(xs)}


def host_seconds(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def measure(batch, rebuild, iters, calls, rebuilds):
    values = torch.tensor(batch.export(2), device="cuda")
    other = (values * 1.25).contiguous()
    first_s, _ = host_seconds(lambda: batch.set_values(other))          # builds the maps
    for _ in range(3 * calls):
        batch.set_values(values)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    every = max(iters // max(rebuilds, 1), 1)
    call_us, rebuild_s = [], []
    for it in range(iters):
        ev[0].record()
        for k in range(calls):
            batch.set_values(other if k & 1 else values)
        ev[1].record()
        torch.cuda.synchronize()
        call_us.append(ev[0].elapsed_time(ev[1]) * 1e3 / calls)
        if it % every == 0 and len(rebuild_s) < rebuilds:
            sec, fresh = host_seconds(rebuild)
            rebuild_s.append(sec)
            del fresh
    med_call, med_rebuild = float(np.median(call_us)), float(np.median(rebuild_s))
    return {"instances": batch.n_inst, "nnz": batch.nnz, "map_bytes": batch.set_values_bytes(),
            "set_values_us": stats(call_us, 1), "first_call_s": round(first_s, 4), "rebuild_s": stats(rebuild_s, 4),
            "rebuild_over_set_values": round(med_rebuild * 1e6 / med_call, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rebuilds", type=int, default=5)
    ap.add_argument("--synthetic-inst", type=int, default=256)
    args = ap.parse_args()
    from mllp_amd.data import load_packed
    from mllp_amd.graph import LPBatch, synthetic_batch
    assert torch.cuda.is_available(), "bench_set_values needs the GPU: there is no CPU path"
    out = {"iters": args.iters, "calls_per_window": args.calls}
    insts = load_packed()
    b = LPBatch.from_instances(insts)
    out["netlib97"] = measure(b, lambda: LPBatch.from_instances(insts), args.iters, args.calls, args.rebuilds)
    del b
    sb = synthetic_batch(n_inst=args.synthetic_inst)
    copies = sb.enable_stream_step()
    ptr, idx, val = sb._device_orientation(False)

    def rebuild():
        fresh = LPBatch.from_device_csr(sb.inst_m, sb.inst_n, ptr, idx, val, sb.x1, sb.x2, sb.labels)
        fresh.enable_stream_step()
        return fresh
    out["synthetic256"] = dict(measure(sb, rebuild, args.iters, args.calls, args.rebuilds),
                               copies=sum(1 for i in copies.values() if not i.get("dropped")))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
