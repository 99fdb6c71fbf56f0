#!/usr/bin/env python3
"""bench_small_step.py -- the one-launch step (mllp_gnn_train_step_small) against the default step on the 97 Netlib singles.

  python tools/bench_small_step.py [--out profiles/small_step_bench.json] [--ladder-only | --loop-only]
                                   [--nodes K --nnz E]

ladder   every instance its own batch, sorted by nnz: device-event time of 20 back-to-back steps of mllp_gnn_train_step
         (as LPBatch.train_step issues it, with the folded-weights flag) and of the new call, the two alternating, median
         of 5 windows each.  `crossover`: the largest (nodes, nnz) below which the new call is faster on EVERY instance
         of the ladder (instances beyond the library's limits count as "not faster").
loop     the loop of bench.py's per_instance_steps: a warm epoch, then 3 epochs over the 97 singles, one Adam step per
         instance, host clock.  Both arms call the library directly with the same buffers: `default` is
         LPBatch.train_step for every instance, `routed` takes LPBatch.train_step_small for the instances within
         --nodes / --nnz (default: this run's ladder crossover, or the library's limits with --loop-only).  Five
         alternating runs in one process, median and min-max of each; `accepted`: the routed median is above the default's
         by more than the default's own min-max spread.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

from mllp_amd.data import load_packed  # noqa: E402
from mllp_amd.graph import LPBatch, small_step_limits  # noqa: E402
from mllp_amd.model import GNNModel  # noqa: E402

STEPS, WINDOWS = 20, 5


def _adam(p):
    return torch.zeros_like(p), torch.zeros_like(p), torch.tensor([0.0, 1e-3, 0.9, 0.999], device=p.device)


def _window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(STEPS):
        fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / STEPS      # us per step


def ladder(instances, params0):
    rows = []
    for inst in sorted(instances, key=lambda i: i.nnz):
        b = LPBatch.from_instances([inst])
        p = params0.clone()
        m, v, st = _adam(p)
        logits, loss = torch.empty(b.N, device="cuda"), torch.zeros(1, device="cuda")
        grads = torch.empty(p.numel(), device="cuda")
        gen = [0]

        def default():
            b.train_step(p, m, v, st, 1e-8, 1.0, logits, loss, grads, param_gen=gen[0])
            gen[0] += 1

        def small():
            b.train_step_small(p, m, v, st, 1e-8, 1.0, logits, loss, grads)

        fits = b.small_step_fits()
        default()
        if fits:
            small()
        torch.cuda.synchronize()
        td, ts = [], []
        for _ in range(WINDOWS):
            td.append(_window(default))
            if fits:
                ts.append(_window(small))
        rows.append(dict(name=inst.name, m=inst.m, n=inst.n, nodes=inst.m + inst.n, nnz=inst.nnz,
                         default_us=statistics.median(td), small_us=statistics.median(ts) if fits else None))
        del b
    # the largest prefix of each ordering on which the new call wins every time
    def bound(key):
        best = 0
        for r in sorted(rows, key=lambda r: r[key]):
            if r["small_us"] is None or r["small_us"] >= r["default_us"]:
                break
            best = r[key]
        return best
    return rows, dict(nodes=bound("nodes"), nnz=bound("nnz"))


def epoch_loop(instances, params0, nodes, nnz):
    """nodes / nnz: the routing thresholds; None = every instance takes the default step"""
    singles = [LPBatch.from_instances([i]) for i in instances]
    small = [nodes is not None and b.small_step_fits() and b.M + b.N <= nodes and b.nnz <= nnz for b in singles]
    p = params0.clone()
    m, v, st = _adam(p)
    logits = [torch.empty(b.N, device="cuda") for b in singles]
    loss, grads = torch.zeros(1, device="cuda"), torch.empty(p.numel(), device="cuda")

    def epoch():
        for b, z, s in zip(singles, logits, small):
            if s:
                b.train_step_small(p, m, v, st, 1e-8, 1.0, z, loss, grads)
            else:
                b.train_step(p, m, v, st, 1e-8, 1.0, z, loss, grads)

    epoch()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(3):
        epoch()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return 3 * len(singles) / dt, sum(small)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--ladder-only", action="store_true")
    ap.add_argument("--loop-only", action="store_true")
    ap.add_argument("--loop-runs", type=int, default=5)
    ap.add_argument("--nodes", type=int, default=None)
    ap.add_argument("--nnz", type=int, default=None)
    args = ap.parse_args()
    instances = load_packed()
    torch.manual_seed(0)
    params0 = GNNModel().flat_parameters().detach().float().cuda()
    out = dict(limits=small_step_limits(), steps_per_window=STEPS, windows=WINDOWS)
    if not args.loop_only:
        rows, cross = ladder(instances, params0)
        out["ladder"], out["crossover"] = rows, cross
        for r in rows:
            s = "-" if r["small_us"] is None else f"{r['small_us']:8.1f}"
            print(f"{r['name']:14s} nodes {r['nodes']:6d} nnz {r['nnz']:7d}  default {r['default_us']:8.1f} us  small {s} us")
        print("crossover:", cross)
    if not args.ladder_only:
        lim = out["limits"]
        base = out.get("crossover", dict(nodes=lim["max_nodes"], nnz=lim["max_nnz"]))
        nodes = base["nodes"] if args.nodes is None else args.nodes
        nnz = base["nnz"] if args.nnz is None else args.nnz
        runs = {"default": [], "routed": []}
        n_small = None
        for _ in range(args.loop_runs):
            runs["default"].append(epoch_loop(instances, params0, None, None)[0])
            v, n_small = epoch_loop(instances, params0, nodes, nnz)
            runs["routed"].append(v)
        out["loop"] = {k: dict(median=statistics.median(v), min=min(v), max=max(v), runs=v) for k, v in runs.items() if v}
        out["loop"]["instances_on_small_step"] = n_small
        out["loop"]["thresholds"] = dict(nodes=nodes, nnz=nnz)
        if args.loop_runs > 0:
            d, s = out["loop"]["default"], out["loop"]["routed"]
            out["loop"]["accepted"] = bool(s["median"] - d["median"] > d["max"] - d["min"])
        print(json.dumps(out["loop"]))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
