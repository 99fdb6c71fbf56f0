#!/usr/bin/env python3
"""bench_optim.py -- what mllp_optim_step costs.

  python tools/bench_optim.py [--out profiles/optim_bench.json]

kernels  mllp_adam_step against mllp_optim_step at n = 4721 (one workgroup) and n = mllp_angle_num_params(256) (the sliced
         launches): `optim_off` = neutral settings without info, so the norm pass is not run; `optim_on` = weight decay, a clip
         norm and info, so it is.  Device events around 1000 back-to-back calls on one stream, the three arms alternating,
         median and min-max of 7 windows after a warm-up of every arm.
trainer  the LPTrainer step on the Netlib batch (all 97 instances, the batch of bench.py): the default whole step, whose
         tail is one launch with plain Adam in it, against the step with the three options on (loss step, then
         mllp_optim_step).  50 steps per window, the two alternating, median and min-max of 7 windows.  The difference is the
         price of leaving the one-launch tail.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

from mllp_amd import _lib  # noqa: E402
from mllp_amd.data import load_packed  # noqa: E402
from mllp_amd.graph import LPBatch, adam_step, optim_scratch_floats, optim_step  # noqa: E402
from mllp_amd.model import GNNModel  # noqa: E402
from mllp_amd.trainer import LPTrainer  # noqa: E402

WINDOWS = 7


def window(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / steps      # us per call


def alternate(arms, steps):
    """arms: name -> callable.  dict(name -> median / min / max us per call) over WINDOWS alternating windows"""
    for fn in arms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(WINDOWS):
        for k, fn in arms.items():
            times[k].append(window(fn, steps))
    return {k: dict(median_us=statistics.median(v), min_us=min(v), max_us=max(v)) for k, v in times.items()}


def kernels(n, steps=1000):
    g = torch.randn(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(n))

    def bufs(words):
        p = torch.randn(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
        st = torch.tensor([0.0, 1e-3, 0.9, 0.999, 100.0, 100000.0, 0.1, 0.0][:words], device="cuda")
        return p, torch.zeros_like(p), torch.zeros_like(p), st

    ns = optim_scratch_floats(n)
    scratch = torch.empty(ns, device="cuda") if ns else None
    info = torch.zeros(4, device="cuda")
    a, off, on = bufs(4), bufs(8), bufs(8)
    off[3][4:] = 0.0
    arms = {
        "adam_step": lambda: adam_step(a[0], g, a[1], a[2], a[3], 1e-8, 1.0),
        "optim_off": lambda: optim_step(off[0], g, off[1], off[2], off[3], 1e-8, 1.0, 0.0, 0.0, scratch, None),
        "optim_on": lambda: optim_step(on[0], g, on[1], on[2], on[3], 1e-8, 1.0, 0.01, 1.0, scratch, info),
    }
    out = alternate(arms, steps)
    assert float(on[3][0]) == float(a[3][0]) and float(info[3]) == 0.0      # every call took its step
    return dict(n=n, calls_per_window=steps, **out)


def trainer(steps=50):
    instances = load_packed()
    torch.manual_seed(0)
    params0 = GNNModel().flat_parameters().detach().float().cuda()
    opts = dict(weight_decay=0.01, clip_norm=1.0, lr_schedule=dict(warmup=100, total=100000, min_ratio=0.1))
    pairs = {}
    for name, kw in (("whole_step", {}), ("options_on", opts)):
        pairs[name] = (LPTrainer(params0, lr=1e-3, use_hip_graph=False, **kw), LPBatch.from_instances(instances))
    arms = {k: (lambda t=t, b=b: t.step(b)) for k, (t, b) in pairs.items()}
    out = alternate(arms, steps)
    skipped = float(pairs["options_on"][0].opt.info[3])
    return dict(instances=len(instances), nnz=int(pairs["whole_step"][1].nnz), steps_per_window=steps, last_step_skipped=skipped,
                **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim.py measures on the GPU: no device, no figures")
    n_angle = ctypes.c_int64()
    _lib.check(_lib.lib().mllp_angle_num_params(256, ctypes.byref(n_angle)))
    out = dict(windows=WINDOWS, device=torch.cuda.get_device_name(0),
               kernels=[kernels(_lib.NUM_PARAMS), kernels(int(n_angle.value))], trainer=trainer())
    for row in out["kernels"]:
        print(f"n {row['n']:7d}: " + ", ".join(f"{k} {row[k]['median_us']:.2f} us [{row[k]['min_us']:.2f}, {row[k]['max_us']:.2f}]"
                                                for k in ("adam_step", "optim_off", "optim_on")))
    t = out["trainer"]
    print("trainer: " + ", ".join(f"{k} {t[k]['median_us']:.1f} us [{t[k]['min_us']:.1f}, {t[k]['max_us']:.1f}]"
                                  for k in ("whole_step", "options_on")))
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
