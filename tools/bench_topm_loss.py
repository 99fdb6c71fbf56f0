"""Cost of the soft top-m loss head (mllp_topm_loss) beside the weighted head it replaces (mllp_weighted_loss) on the same
logits, and of the whole step with either head (loss_step_topm against loss_step_weighted).  Prints one JSON line
(profiles/topm_loss_bench.json).

    python tools/bench_topm_loss.py [--calls 8] [--windows 7] [--samples 10]

Batches: the full Netlib batch and `planted 1024 x (50 x 120)`.  Logits: those of the model's forward with the golden
weights.  The head at S = 0 and at S = --samples (sigma 0.05, the yaml's gumbel_sigma), each with dlogits, inst_loss and loss
as outputs (what a training step asks for).

DEVICE figures, in the protocol of tools/bench_simplex.py: device events around `calls` back-to-back calls into outputs
allocated once, after two warm-up calls; the median, min and max over `windows` windows, per call.  No bar is set.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_basis_repair import device_window  # noqa: E402


def timed(fn, calls, windows):
    fn()
    fn()
    torch.cuda.synchronize()
    dev = [device_window(fn, calls) for _ in range(windows)]
    return {"median": round(float(np.median(dev)) * 1e6, 2), "min": round(min(dev) * 1e6, 2), "max": round(max(dev) * 1e6, 2)}


def measure(name, b, params, calls, windows, samples, sigma):
    from mllp_amd import _lib
    L, p, s = _lib.lib(), _lib.ptr, _lib.current_stream
    dev = b.x1.device
    z = b.forward(params).clone()
    dz, il, ls = torch.empty(b.N, device=dev), torch.empty(b.n_inst, device=dev), torch.empty(1, device=dev)
    info = torch.empty(b.n_inst, 4, device=dev)
    iw = torch.full((b.n_inst,), 1.0 / b.n_inst, device=dev)
    y = b.labels

    def weighted():
        _lib.check(L.mllp_weighted_loss(b._h, p(z), p(y), p(iw), None, p(dz), p(il), p(ls), s()))

    def topm(S, with_info=False):
        def call():
            _lib.check(L.mllp_topm_loss(b._h, p(z), p(y), p(iw), None, None, 1.0, sigma if S else 0.0, S, 1, p(dz), p(il), p(ls), None,
                                        p(info) if with_info else None, s()))
        return call
    topm(0, True)()
    torch.cuda.synchronize()
    it = info[:, 3].cpu().numpy()
    rooted = it >= 0
    out = {"batch": name, "instances": b.n_inst, "columns": b.N, "longest_instance": int(max(b.inst_n)), "calls_per_window": calls,
           "windows": windows, "root_iterations": {"mean": round(float(it[rooted].mean()), 2), "max": int(it.max())},
           "instances_without_a_root": int((~rooted).sum()),
           "device_us_per_call": {"weighted_loss": timed(weighted, calls, windows), "topm_loss_S0": timed(topm(0), calls, windows),
                                  f"topm_loss_S{samples}": timed(topm(samples), calls, windows)}}
    grads, logits = torch.empty_like(params), torch.empty(b.N, device=dev)
    out["device_us_per_call"]["loss_step_weighted"] = timed(lambda: b.loss_step_weighted(params, iw, None, logits, ls, il, grads), calls, windows)
    out["device_us_per_call"]["loss_step_topm_S0"] = timed(
        lambda: b.loss_step_topm(params, 1.0, 0.0, 0, 1, iw, None, logits, ls, il, grads), calls, windows)
    out["device_us_per_call"][f"loss_step_topm_S{samples}"] = timed(
        lambda: b.loss_step_topm(params, 1.0, sigma, samples, 1, iw, None, logits, ls, il, grads), calls, windows)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--sigma", type=float, default=0.05)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_topm_loss needs the GPU: there is no CPU path"
    from mllp_amd import _lib
    from mllp_amd.data import load_packed
    from mllp_amd.graph import LPBatch
    from mllp_amd.planted import planted_batch
    golden = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "subset5.npz"))
    params = torch.tensor(golden["weights_flat"], dtype=torch.float32, device="cuda")
    lim = (__import__("ctypes").c_int64 * 2)()
    _lib.check(_lib.lib().mllp_topm_loss_limits(lim))
    net = LPBatch.from_instances(load_packed())
    pl, _, _ = planted_batch(1024, 50, 120, 6.0, 1)
    res = [measure(f"Netlib {net.n_inst} instances", net, params, args.calls, args.windows, args.samples, args.sigma),
           measure("planted 1024 x (50 x 120)", pl, params, args.calls, args.windows, args.samples, args.sigma)]
    print(json.dumps({"lds_max_columns": int(lim[0]), "threads": int(lim[1]), "samples": args.samples, "sigma": args.sigma, "results": res}))


if __name__ == "__main__":
    main()
