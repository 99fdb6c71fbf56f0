"""Cost of repairing and solving a basis on the device (mllp_basis_repair), beside the host alternative in the same process:
copy the batch back, then scipy.linalg.lu_factor / lu_solve per instance.  Prints one JSON line
(profiles/basis_repair_bench.json).

    python tools/bench_basis_repair.py [--calls 8] [--windows 7] [--netlib-max-m 1024]

Batches:  planted 64 and 1024 x (50 x 120);  one planted batch across the LDS threshold (32 x (160 x 400) with T in LDS, 32 x
(256 x 600) with T in scratch);  the Netlib batch with max_m at the threshold and at --netlib-max-m (every instance would
need the reported scratch; the cost grows with m^3, so the largest ones are an offline job, not a benchmark window).
Planted batches are solved with the labels first (no rejections: the cost of solving a given basis); the Netlib batch with
a seeded random ranking (a repair: rejections included).

DEVICE figures: device events around `calls` back-to-back launches into outputs allocated once, after a warm-up; the median,
min and max over `windows` windows, per call.  HOST figures: a host clock around export (synchronises) + per-instance dense
LU, alternating with the device windows.  No bar is set: this is an evaluation call.

WORK of one instance of m rows that accepts m columns without rejections: the update of acceptance k touches (k + 1) m
elements of T (read + write, 8 bytes in scratch), m^3 / 2 in all, plus sum_j m nnz(a_j) for the candidates' columns and
2 m^2 for x and y.  `update_GBps` is 8 bytes x m^3 / 2 x instances over the call time: what one workgroup per instance
streams through LDS (m <= threshold) or through its CU's L2 path (above).
"""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np  # noqa: E402
import torch  # noqa: E402


class Call:
    """mllp_basis_repair on one batch and one candidate list, outputs and scratch allocated once"""

    def __init__(self, b, order, max_m=None, tol=2.0 ** -12):
        from mllp_amd import _lib
        self.lib, self.b, self.order, self.tol = _lib, b, order, tol
        self.max_m = max(b.inst_m) if max_m is None else int(max_m)
        n = ctypes.c_int64()
        _lib.check(_lib.lib().mllp_basis_repair_scratch_bytes(b._h, self.max_m, ctypes.byref(n)))
        self.scratch_bytes = n.value
        dev = b.x1.device
        self.scratch = torch.empty(max(n.value // 4, 1), device=dev)
        self.basis, self.x = torch.empty(b.N, device=dev), torch.empty(b.N, device=dev)
        self.y, self.col_of_row = torch.empty(b.M, device=dev), torch.empty(b.M, device=dev, dtype=torch.int32)
        self.status = torch.empty(b.n_inst, 4, device=dev, dtype=torch.int32)
        self.quality = torch.empty(b.n_inst, 2, device=dev)

    def __call__(self):
        p = self.lib.ptr
        self.lib.check(self.lib.lib().mllp_basis_repair(self.b._h, p(self.b.x1), p(self.b.x2), p(self.order), self.tol, self.max_m,
                                                        p(self.basis), p(self.col_of_row), p(self.x), p(self.y), p(self.status),
                                                        p(self.quality), p(self.scratch), self.lib.current_stream()))


def device_window(fn, calls):
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    e.record()
    e.synchronize()
    return a.elapsed_time(e) * 1e-3 / calls


def host_solve(b):
    """the host alternative: the batch copied back, a dense LU of every instance's labelled basis, x and y"""
    import scipy.linalg
    ptr, idx, val = b.export(0).astype(np.int64), b.export(1), b.export(2)
    c, rhs, lab = b.x1.cpu().numpy().astype(np.float64), b.x2.cpu().numpy().astype(np.float64), b.labels.cpu().numpy()
    pm, pn = np.concatenate([[0], np.cumsum(b.inst_m)]), np.concatenate([[0], np.cumsum(b.inst_n)])
    rows = np.repeat(np.arange(b.M), np.diff(ptr))
    out = []
    for k in range(b.n_inst):
        e = slice(ptr[pm[k]], ptr[pm[k + 1]])
        A = np.zeros((b.inst_m[k], b.inst_n[k]))
        A[rows[e] - pm[k], idx[e] - pn[k]] = val[e]
        on = lab[pn[k]:pn[k + 1]] != 0
        lu = scipy.linalg.lu_factor(A[:, on])
        out.append((scipy.linalg.lu_solve(lu, rhs[pm[k]:pm[k + 1]]), scipy.linalg.lu_solve(lu, c[pn[k]:pn[k + 1]][on], trans=1)))
    return out


def measure(name, b, order, calls, windows, max_m=None, host=True):
    call = Call(b, order, max_m)
    call()
    call()
    torch.cuda.synchronize()
    st = call.status.cpu().numpy()
    dev, hst = [], []
    for _ in range(windows):
        dev.append(device_window(call, calls))
        if host:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host_solve(b)
            hst.append(time.perf_counter() - t0)
    ran = st[:, 3] != 2
    m = np.asarray(b.inst_m, np.float64)
    med = float(np.median(dev))
    out = {"batch": name, "instances": b.n_inst, "m_max_run": int(m[ran].max(initial=0)), "max_m": call.max_m,
           "scratch_bytes": call.scratch_bytes, "codes": {str(c): int((st[:, 3] == c).sum()) for c in range(4)},
           "examined": int(st[:, 1].sum()), "accepted": int(st[:, 0].sum()), "calls_per_window": calls, "windows": windows,
           "device_us_per_call": {"median": round(med * 1e6, 1), "min": round(min(dev) * 1e6, 1), "max": round(max(dev) * 1e6, 1)},
           "device_us_per_instance_run": round(med * 1e6 / max(int(ran.sum()), 1), 2),
           "update_GBps": round(float(8 * (m[ran] ** 3).sum() / 2 / med / 1e9), 1)}
    if host:
        out["host_us_per_call"] = {"median": round(float(np.median(hst)) * 1e6, 1), "min": round(min(hst) * 1e6, 1),
                                   "max": round(max(hst) * 1e6, 1)}
        out["host_over_device"] = round(float(np.median(hst)) / med, 1)
    return out


def labels_first(b):
    lab = b.labels
    pn = np.concatenate([[0], np.cumsum(b.inst_n)])
    inst = torch.repeat_interleave(torch.arange(b.n_inst, device=lab.device), torch.tensor(b.inst_n, device=lab.device))
    cols = torch.sort(inst * 2 + (lab == 0).long(), stable=True)[1]
    return (cols - torch.tensor(pn[:-1], device=lab.device)[inst[cols]]).to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--netlib-max-m", type=int, default=1024)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_basis_repair needs the GPU: there is no CPU path"
    from mllp_amd.data import load_packed
    from mllp_amd.graph import LPBatch
    from mllp_amd.planted import batch_to_instances, planted_batch
    from mllp_amd._lib import HEADER_PATH
    internal = open(os.path.join(os.path.dirname(HEADER_PATH), "..", "mllp_amd", "csrc", "internal.h")).read()
    lds_max = int(internal.split("BASIS_LDS_MAX_M =")[1].split(";")[0])
    res = []
    for n_inst in (64, 1024):
        b, _, _ = planted_batch(n_inst, 50, 120, 6.0, 1)
        res.append(measure(f"planted {n_inst} x (50 x 120)", b, labels_first(b), args.calls, args.windows))
    lo, _, _ = planted_batch(32, 160, 400, 6.0, 2)
    hi, _, _ = planted_batch(32, 256, 600, 6.0, 3)
    b = LPBatch.from_instances(batch_to_instances(lo) + batch_to_instances(hi))
    res.append(measure("planted 32 x (160 x 400) + 32 x (256 x 600)", b, labels_first(b), args.calls, args.windows))
    for name, one in (("planted 32 x (160 x 400) alone", lo), ("planted 32 x (256 x 600) alone", hi)):
        res.append(measure(name, one, labels_first(one), args.calls, args.windows, host=False))
    big, _, _ = planted_batch(1, 1200, 2400, 8.0, 4)
    res.append(measure("planted 1 x (1200 x 2400)", big, labels_first(big), 2, args.windows))
    net = LPBatch.from_instances(load_packed())
    order = net.ranking(torch.randn(net.N, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5)))
    n_all = ctypes.c_int64()
    from mllp_amd import _lib
    _lib.check(_lib.lib().mllp_basis_repair_scratch_bytes(net._h, max(net.inst_m), ctypes.byref(n_all)))
    for max_m in (lds_max, args.netlib_max_m):
        res.append(measure(f"Netlib {net.n_inst} instances, random ranking, max_m {max_m}", net, order, 1, 3, max_m=max_m, host=False))
    print(json.dumps({"lds_max_m": lds_max, "netlib_largest_m": max(net.inst_m), "netlib_scratch_bytes_all_instances": n_all.value,
                      "results": res}))


if __name__ == "__main__":
    main()
