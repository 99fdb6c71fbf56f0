"""Cost of the device top-m selection (mllp_topm_select) beside (a) mllp_topm_metrics on the same logits -- the same
radix select, one pass over the logits less, labels read instead of outputs written -- and (b) what a caller did before:
one torch.topk per instance, the 0/1 vector filled on the host, with its copy back.  Two batches: the 97 Netlib instances
(logits of the model with the golden weights) and the device-generated synthetic batch (256 instances of 10 000 x 20 000;
the selection depends on the segment sizes only, so the matrix is generated thin and the logits are random normal).
Prints one JSON line.

    python tools/bench_predict.py [--iters 30] [--calls 10] [--row-nnz 4]

Kernel times: device events around `calls` back-to-back launches, divided by `calls`; median over `iters` windows after
a warm-up (an event pair around one 50 us kernel would measure the events).  (b) is host time around the loop, which ends
in its own copies.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def device_us(fn, iters, calls):
    for _ in range(3 * calls):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    us = []
    for _ in range(iters):
        ev[0].record()
        for _ in range(calls):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        us.append(ev[0].elapsed_time(ev[1]) * 1e3 / calls)
    return {"median_us": round(float(np.median(us)), 2), "min_us": round(float(np.min(us)), 2),
            "max_us": round(float(np.max(us)), 2)}


def topk_loop(batch, logits):
    """the per-instance host loop of the reference (linear_program_experiment.py:146-148), as train_angle still does"""
    out = []
    for z, m in zip(batch.logits_per_instance(logits), batch.inst_m):
        idx = torch.topk(z, k=min(m, z.numel()))[-1].cpu().numpy()
        pred = np.zeros(z.numel(), np.int32)
        pred[idx] = 1
        out.append(pred)
    return out


def host_us(fn, iters):
    fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0) * 1e6)
    return {"median_us": round(float(np.median(us)), 1), "min_us": round(float(np.min(us)), 1),
            "max_us": round(float(np.max(us)), 1)}


def measure(batch, logits, iters, calls):
    from mllp_amd import _lib
    bufs = batch.predict_basis(logits)         # the outputs are allocated once: the windows time the launch alone
    met = batch.topm_metrics(logits)
    raw, s = _lib.lib(), _lib.current_stream()

    def select(mask=True, index=True, stats=True):
        _lib.check(raw.mllp_topm_select(batch._h, _lib.ptr(logits), _lib.ptr(bufs.mask if mask else None),
                                        _lib.ptr(bufs.index if index else None), _lib.ptr(bufs.stats if stats else None), s))
    return {
        "instances": batch.n_inst, "columns": batch.N, "selected": int(sum(min(m, n) for m, n in zip(batch.inst_m, batch.inst_n))),
        "largest_instance_columns": max(batch.inst_n),
        "topm_select": device_us(select, iters, calls),
        "topm_select_mask_only": device_us(lambda: select(True, False, False), iters, calls),
        "topm_metrics": device_us(lambda: batch.topm_metrics(logits, met), iters, calls),
        "torch_topk_loop_with_copy_back": host_us(lambda: topk_loop(batch, logits), max(iters // 6, 3)),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--row-nnz", type=float, default=4.0, help="mean nonzeros per row of the synthetic matrix")
    args = ap.parse_args()
    from mllp_amd.data import load_packed
    from mllp_amd.graph import LPBatch, synthetic_batch
    assert torch.cuda.is_available(), "bench_predict needs the GPU: there is no CPU path"
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "subset5.npz"))
    params = torch.tensor(gold["weights_flat"], dtype=torch.float32, device="cuda")
    out = {"iters": args.iters, "calls_per_window": args.calls}
    b = LPBatch.from_instances(load_packed())
    out["netlib97"] = measure(b, b.forward(params), args.iters, args.calls)
    del b
    sb = synthetic_batch(n_inst=256, m=10000, n=20000, mean_row_nnz=args.row_nnz)
    z = torch.randn(sb.N, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    out["synthetic256"] = measure(sb, z, args.iters, args.calls)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
