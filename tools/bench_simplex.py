"""Cost of pivoting a repaired basis to the optimum on the device (mllp_basis_simplex), and the one comparison that means
something: pivots from a WARM start (the optimal basis with k columns swapped, repaired) against pivots from the same LP's
COLD start (the repair of a seeded random ranking).  Prints one JSON line (profiles/simplex_bench.json).

    python tools/bench_simplex.py [--calls 8] [--windows 7] [--swap 10] [--max-pivots 2000] [--refactor R] [--stall S]

--refactor R / --stall S (either above 0) measure mllp_basis_simplex_guarded instead: a fresh factorization every R pivots,
Bland's rule after S degenerate pivots of a stage; every row then has `refactorizations_per_call` and `bland_pivots_per_call`,
the sums of d_guard over the batch (0 and 0 on the plain entry point).  (profiles/simplex_guarded_bench.json)

Batches:  planted 64 and 1024 x (50 x 120);  one planted batch across the LDS threshold (32 x (160 x 400) with T in LDS, 32 x
(256 x 600) with T in scratch);  the Netlib batch with max_m at the threshold, from a seeded random ranking, with the
distribution of codes (degenerate LPs may stop at the limit: the rule has no anti-cycling device).

DEVICE figures, in the protocol of tools/bench_basis_repair.py: device events around `calls` back-to-back launches into
outputs allocated once, after a warm-up; the median, min and max over `windows` windows, per call.  One workgroup works on
one instance, so a call lasts as long as its slowest instance: `us_per_pivot_longest` is the call time over the largest pivot
count of an instance (an upper bound of the time of one pivot: the factorization of the start is inside it), and
`instance_pivots_per_s` the batch's pivots over the call time.  No bar is set: this is an evaluation call.
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_basis_repair import device_window  # noqa: E402


class Call:
    """mllp_basis_simplex on one batch and one start mask, outputs and scratch allocated once"""

    def __init__(self, b, start, max_pivots, max_m=None, refactor=0, stall=0):
        from mllp_amd import _lib
        self.lib, self.b, self.start, self.max_pivots = _lib, b, start.to(torch.float32).contiguous(), int(max_pivots)
        self.refactor, self.stall = int(refactor), int(stall)
        self.max_m = max(b.inst_m) if max_m is None else int(max_m)
        n = ctypes.c_int64()
        _lib.check(_lib.lib().mllp_basis_simplex_scratch_bytes(b._h, self.max_m, ctypes.byref(n)))
        self.scratch_bytes = n.value
        dev = b.x1.device
        self.scratch = torch.empty(max(n.value // 4, 1), device=dev)
        self.basis = torch.empty(b.N, device=dev)
        self.status = torch.empty(b.n_inst, 4, device=dev, dtype=torch.int32)
        self.guard = torch.zeros(b.n_inst, 2, device=dev, dtype=torch.int32)

    def __call__(self):
        p = self.lib.ptr
        if self.refactor or self.stall:     # the guarded entry point; with both 0 the plain one, as ever
            self.lib.check(self.lib.lib().mllp_basis_simplex_guarded(
                self.b._h, p(self.b.x1), p(self.b.x2), p(self.start), 2.0 ** -12, 2.0 ** -10, 2.0 ** -10, 2.0 ** -10, 2.0 ** -4,
                self.max_pivots, self.max_m, self.refactor, self.stall, p(self.basis), None, None, p(self.status), p(self.guard),
                p(self.scratch), self.lib.current_stream()))
            return
        self.lib.check(self.lib.lib().mllp_basis_simplex(self.b._h, p(self.b.x1), p(self.b.x2), p(self.start), 2.0 ** -12, 2.0 ** -10,
                                                         2.0 ** -10, 2.0 ** -10, 2.0 ** -4, self.max_pivots, self.max_m, p(self.basis),
                                                         None, None, p(self.status), p(self.scratch), self.lib.current_stream()))


def swapped_start(b, k, seed):
    """the labels with k basic columns swapped for k nonbasic ones per instance, ranked `kept, added, the rest` and repaired
    on the device: a start k columns away from the optimum (less where the repair rejects an added column)"""
    lab = b.labels.cpu().numpy() != 0
    pn = np.concatenate([[0], np.cumsum(b.inst_n)])
    order = np.empty(b.N, np.int32)
    rng = np.random.default_rng(seed)
    for i in range(b.n_inst):
        on, off = np.flatnonzero(lab[pn[i]:pn[i + 1]]), np.flatnonzero(~lab[pn[i]:pn[i + 1]])
        kk = min(k, len(on), len(off))
        kept = np.setdiff1d(on, rng.choice(on, size=kk, replace=False))
        add = rng.choice(off, size=kk, replace=False)
        order[pn[i]:pn[i + 1]] = np.concatenate([kept, add, np.setdiff1d(np.arange(pn[i + 1] - pn[i]), np.concatenate([kept, add]))])
    return b.repair_basis(order=torch.from_numpy(order).cuda(), want=("basis",)).basis


def random_start(b, seed, max_m=None):
    z = torch.randn(b.N, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))
    return b.repair_basis(logits=z, max_m=max_m, want=("basis",)).basis


def measure(name, b, start, what, calls, windows, max_pivots, max_m=None, certify=True, refactor=0, stall=0):
    call = Call(b, start, max_pivots, max_m, refactor, stall)
    call()
    call()
    torch.cuda.synchronize()
    st, gd = call.status.cpu().numpy(), call.guard.cpu().numpy()
    dev = [device_window(call, calls) for _ in range(windows)]
    med = float(np.median(dev))
    piv = (st[:, 1] + st[:, 2]).astype(np.int64)
    done = st[:, 0] == 0
    out = {"batch": name, "start": what, "instances": b.n_inst, "max_m": call.max_m, "max_pivots": max_pivots,
           "refactor_every": call.refactor, "stall_pivots": call.stall,
           "scratch_bytes": call.scratch_bytes, "codes": {str(c): int((st[:, 0] == c).sum()) for c in range(8)},
           "refactorizations_per_call": int(gd[:, 0].sum()), "bland_pivots_per_call": int(gd[:, 1].sum()),
           "pivots": {"total": int(piv.sum()), "stage_D": int(st[:, 1].sum()), "stage_P": int(st[:, 2].sum()), "largest": int(piv.max(initial=0)),
                      "mean_of_the_optimal": round(float(piv[done].mean()), 2) if done.any() else None},
           "calls_per_window": calls, "windows": windows,
           "device_us_per_call": {"median": round(med * 1e6, 1), "min": round(min(dev) * 1e6, 1), "max": round(max(dev) * 1e6, 1)},
           "us_per_pivot_longest": round(med * 1e6 / max(int(piv.max(initial=0)), 1), 2),
           "instance_pivots_per_s": round(float(piv.sum()) / med, 0)}
    # the start's factorization is solve_basis' (the same list, the same rule): code 1 where that call finds rank < m
    sb = b.solve_basis(call.start, max_m=max_m, want=()).status.cpu().numpy()
    out["singular_starts_by_solve_basis"] = int((sb[:, 3] == 1).sum())
    out["code_1_is_solve_basis_code_1"] = bool(np.array_equal(sb[:, 3] == 1, st[:, 0] == 1))
    if certify:     # the final bases, factorized afresh and certified
        from mllp_amd.graph import BasisSimplex
        got = b.simplex_solved(BasisSimplex(call.basis, None, None, call.status), 1e-3, 1e-3, max_m=max_m)
        out["certified_optimal"] = int((got["optimal"] & (call.status[:, 0] == 0)).sum())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--swap", type=int, default=10)
    ap.add_argument("--max-pivots", type=int, default=2000)
    ap.add_argument("--refactor", type=int, default=0, help="refactor_every of mllp_basis_simplex_guarded (0: never)")
    ap.add_argument("--stall", type=int, default=0, help="stall_pivots of mllp_basis_simplex_guarded (0: no Bland mode)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_simplex needs the GPU: there is no CPU path"
    from mllp_amd.data import load_packed
    from mllp_amd.graph import LPBatch
    from mllp_amd.planted import batch_to_instances, planted_batch
    from mllp_amd._lib import HEADER_PATH
    internal = open(os.path.join(os.path.dirname(HEADER_PATH), "..", "mllp_amd", "csrc", "internal.h")).read()
    lds_max = int(internal.split("SIMPLEX_LDS_MAX_M =")[1].split(";")[0])
    res = []
    guards = dict(refactor=args.refactor, stall=args.stall)
    batches = []
    for n_inst in (64, 1024):
        b, _, _ = planted_batch(n_inst, 50, 120, 6.0, 1)
        batches.append((f"planted {n_inst} x (50 x 120)", b))
    lo, _, _ = planted_batch(32, 160, 400, 6.0, 2)
    hi, _, _ = planted_batch(32, 256, 600, 6.0, 3)
    batches.append(("planted 32 x (160 x 400) + 32 x (256 x 600)", LPBatch.from_instances(batch_to_instances(lo) + batch_to_instances(hi))))
    for name, b in batches:
        res.append(measure(name, b, swapped_start(b, args.swap, 11), f"warm: {args.swap} columns swapped, repaired", args.calls,
                           args.windows, args.max_pivots, **guards))
        res.append(measure(name, b, random_start(b, 5), "cold: the repair of a random ranking", 2, 3, args.max_pivots, **guards))
    net = LPBatch.from_instances(load_packed())
    res.append(measure(f"Netlib {net.n_inst} instances, max_m {lds_max}", net, random_start(net, 5, lds_max),
                       "cold: the repair of a random ranking", 1, 3, args.max_pivots, max_m=lds_max, **guards))
    print(json.dumps({"lds_max_m": lds_max, "refactor_every": args.refactor, "stall_pivots": args.stall, "results": res}))


if __name__ == "__main__":
    main()
