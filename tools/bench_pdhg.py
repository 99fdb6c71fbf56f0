"""Cost and reach of restarted PDHG on the resident batch (mllp_lp_pdhg; with --scaled: mllp_lp_pdhg_scaled; with --halpern:
mllp_lp_pdhg_halpern; with --wide: mllp_lp_pdhg_wide against mllp_lp_pdhg_halpern; with --rays: mllp_lp_pdhg_rays against
mllp_lp_pdhg_wide; with --spectral: mllp_lp_pdhg_spectral against mllp_lp_pdhg_wide, profiles/pdhg_spectral_bench.json).
Prints one JSON line (profiles/pdhg_bench.json; profiles/pdhg_scaled_bench.json holds the --scaled runs,
profiles/pdhg_halpern_bench.json the --halpern ones, profiles/pdhg_wide_bench.json the --wide ones, profiles/pdhg_rays_bench.json
the --rays ones).

    python tools/bench_pdhg.py [--calls 2] [--windows 5] [--plain-iters 256] [--netlib-iters 60000] [--synthetic 4]
                               [--scaled | --halpern [--no-reflect]] [--ruiz 10] [--no-pock-chambolle] [--no-weight] [--span 16]
                               [--wide [--rows R] [--poll P]] [--rays [--ray-eps E] [--runs NAME,...]] [--spectral [--power P]]
                               [--only PART,...]

  --scaled        the same batches and the same Netlib table through LPBatch.pdhg_scaled with the options given; the output
                  gains "call" and "options".  --only per_iteration,netlib,cold_warm,oracle runs the named parts alone.
  --halpern       the same through LPBatch.pdhg_halpern, with the --scaled options and --no-reflect.
  --wide          LPBatch.pdhg_wide (the --halpern options; --rows: rows_per_item, --poll: poll_every of the netlib part) AGAINST
                  LPBatch.pdhg_halpern from the same build: per_iteration times both calls on every batch, alternating window by
                  window ("persistent" beside the wide figures, and "wide_max_below_persistent_min"); netlib (eps 1e-3 alone)
                  runs both under --netlib-iters and reports the wall time of each and whether the converged sets are equal.
  --rays          what certificates cost (the --wide options): on Netlib, planted 64 x (500 x 1200) and planted 256 x (50 x 120),
                  --plain-iters iterations at check_every 64 and at check_every 0, with eps = 0 so that no instance stops, through
                  LPBatch.pdhg_wide ("wide"), LPBatch.pdhg_rays with ray_eps = -1 ("rays_off": the wide call's kernels) and with
                  ray_eps = 0 ("rays_on": every check evaluates the rays and none decides), alternating window by window; per run
                  the figures of per_iteration and "us_per_check", (the median at 64 - the median at 0) x 64 / iterations.  --runs
                  wide times that call alone, which is all a tree from before the call has.  --ray-eps E: the detection part,
                  Netlib at eps 1e-3 under --netlib-iters with ray_eps E against the wide call (codes and iterations equal?).
  --spectral      what the spectral step costs and reaches (the --wide options; --power P: power_iters, default 40).  per_iteration:
                  on Netlib, planted 64 x (500 x 1200) and the synthetic batch, LPBatch.pdhg_wide and LPBatch.pdhg_spectral from the
                  same build alternate window by window, each also with no iterations (the set-up alone; the spectral call also at
                  power_iters = 0); an iteration's time is a window less the median set-up of the same call, and the bar of DESIGN
                  4.21 is evaluated on it (each median inside the other call's smallest window - 1 % .. largest + 1 %).  netlib: the 97
                  instances under --netlib-iters and --poll at eps 1e-3 and 1e-4 with power_iters 0 and P: converged counts, gains
                  and losses by name, iterations on the instances both solve, and the instances whose estimate fell back.

  per_iteration   plain PDHG (check_every = 0) for --plain-iters iterations on the Netlib batch, on planted batches (256 and
                  1024 x (50 x 120), all in LDS; 64 x (500 x 1200); the same 64 with max_lds_words = 0, all in scratch) and on
                  --synthetic instances of the synthetic batch's size (10 000 x 20 000, about 2 M nonzeros each).  DEVICE
                  figures in the protocol of tools/bench_basis_repair.py: device events around `calls` back-to-back launches
                  into outputs allocated once, after a warm-up; the median, min and max over `windows` windows, per call and
                  per iteration.  One workgroup works on one instance, so a call lasts as long as its slowest instance.
  netlib          per instance at eps 1e-3 and 1e-4 under --netlib-iters: code, iterations, restarts and the three errors.
  cold_warm       planted 256 x (50 x 120): iterations from zeros against iterations from repair_basis(labels)'s x and y.
  oracle_deviation  the figure behind the bars of tests/test_pdhg.py: the fp32 numpy oracle against the fp64 one (CPU code
                  both) after 64 and 512 plain iterations, in units of 2^-24 max|.|, on that test's shapes.
No number here is a gate.
"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_basis_repair import device_window  # noqa: E402


SOLVE = {"call": "pdhg", "options": {}}       # set by main: which call `solve` makes


def solve(b, iters, **kw):
    return getattr(b, SOLVE["call"])(iters, **SOLVE["options"], **kw)


def figures(dev, iters):
    med = float(np.median(dev))
    return {"device_ms_per_call": {"median": round(med * 1e3, 3), "min": round(min(dev) * 1e3, 3), "max": round(max(dev) * 1e3, 3)},
            "us_per_iteration": {"median": round(med * 1e6 / iters, 3), "min": round(min(dev) * 1e6 / iters, 3),
                                 "max": round(max(dev) * 1e6 / iters, 3)}}


def timed(b, iters, calls, windows, max_lds_words=None, **kw):
    head = {"iterations": iters, "calls_per_window": calls, "windows": windows}
    if SOLVE["call"] == "pdhg_wide":
        # both calls from the same build, alternating window by window; the persistent call takes the same options
        opts = {k: v for k, v in SOLVE["options"].items() if k != "rows_per_item"}
        runs = {"persistent": lambda: b.pdhg_halpern(iters, max_lds_words=max_lds_words, **opts, **kw), "wide": lambda: solve(b, iters, **kw)}
        for run in runs.values():
            run()
            run()
        torch.cuda.synchronize()
        dev = {name: [] for name in runs}
        for _ in range(windows):
            for name, run in runs.items():
                dev[name].append(device_window(run, calls))
        return {**head, **figures(dev["wide"], iters), "persistent": figures(dev["persistent"], iters),
                "wide_max_below_persistent_min": bool(max(dev["wide"]) < min(dev["persistent"]))}
    run = lambda: solve(b, iters, max_lds_words=max_lds_words, **kw)      # noqa: E731
    run()
    run()
    torch.cuda.synchronize()
    dev = [device_window(run, calls) for _ in range(windows)]
    return {**head, **figures(dev, iters)}


def shape_of(b):
    from mllp_amd.graph import pdhg_limits
    words = [3 * n + 2 * m for m, n in zip(b.inst_m, b.inst_n)]
    return {"instances": b.n_inst, "nnz": b.dims()["nnz"], "largest_m": max(b.inst_m), "largest_n": max(b.inst_n),
            "instances_in_lds": int(sum(w <= pdhg_limits()[0] for w in words))}


def oracle_deviation():
    import pdhg_oracle as pg
    import planted_oracle as po
    import test_basis_repair as tb
    out = {}
    insts = pg.cpu_planted(tb.planted_shapes([(1, 1), (3, 3), (5, 12), (40, 100)], 20)) + pg.cpu_planted(po.ragged_case(which=[4]))
    for K in (64, 512):
        worst = 0.0
        for i in insts:
            a = pg.solve(i["A"], i["b"], i["c"], K, check_every=0)
            f = pg.solve(i["A"], i["b"], i["c"], K, check_every=0, dtype=np.float32)
            for v in ("x", "y"):
                worst = max(worst, float(np.abs(a[v] - f[v]).max() / (2.0 ** -24 * np.abs(a[v]).max())))
        out[str(K)] = round(worst, 2)
    return out


def rays_bench(args, opts):
    """--rays: see the module's docstring"""
    from mllp_amd.data import load_packed
    from mllp_amd.graph import LPBatch
    from mllp_amd.planted import planted_batch
    names = args.runs.split(",")
    calls = {"wide": lambda b, it, ce: b.pdhg_wide(it, check_every=ce, eps=0.0, **opts),
             "rays_off": lambda b, it, ce: b.pdhg_rays(it, check_every=ce, eps=0.0, ray_eps=-1.0, **opts),
             "rays_on": lambda b, it, ce: b.pdhg_rays(it, check_every=ce, eps=0.0, ray_eps=0.0, **opts)}
    net = LPBatch.from_instances(load_packed())
    mid, _, _ = planted_batch(64, 500, 1200, 6.0, 2)
    small, _, _ = planted_batch(256, 50, 120, 6.0, 1)
    out = {"call": "mllp_lp_pdhg_rays", "against": "mllp_lp_pdhg_wide", "options": opts, "runs": names, "per_iteration": []}
    iters = args.plain_iters
    for name, b in ((f"Netlib {net.n_inst} instances", net), ("planted 64 x (500 x 1200)", mid), ("planted 256 x (50 x 120)", small)):
        runs = {(n, ce): (lambda n=n, ce=ce: calls[n](b, iters, ce)) for ce in (64, 0) for n in names}
        for run in runs.values():
            run()
            run()
        torch.cuda.synchronize()
        dev = {key: [] for key in runs}
        for _ in range(args.windows):
            for key, run in runs.items():
                dev[key].append(device_window(run, args.calls))
        row = {"batch": name, "instances": b.n_inst, "nnz": b.dims()["nnz"], "iterations": iters, "calls_per_window": args.calls, "windows": args.windows}
        for n in names:
            with_checks, without = figures(dev[n, 64], iters), figures(dev[n, 0], iters)
            running = int((calls[n](b, iters, 64).status[:, 0] == 6).sum().item())
            row[n] = {"check_every_64": with_checks, "check_every_0": without, "still_running": running,
                      "us_per_check": round((with_checks["us_per_iteration"]["median"] - without["us_per_iteration"]["median"]) * 64, 3)}
        out["per_iteration"].append(row)
    if args.ray_eps is not None and "rays_on" in names:
        import time
        res = {}
        for n, run in (("wide", lambda: net.pdhg_wide(args.netlib_iters, eps=1e-3, poll_every=args.poll, **opts)),
                       ("rays", lambda: net.pdhg_rays(args.netlib_iters, eps=1e-3, ray_eps=args.ray_eps, poll_every=args.poll, **opts))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = run()
            torch.cuda.synchronize()
            res[n] = (r, time.perf_counter() - t0)
        (w, tw), (r, tr) = res["wide"], res["rays"]
        st, ws = r.status.cpu().numpy(), w.status.cpu().numpy()
        cert = r.cert.cpu().numpy()
        out["netlib_detection"] = {
            "eps": 1e-3, "ray_eps": args.ray_eps, "max_iters": args.netlib_iters, "poll_every": args.poll, "wide_wall_s": round(tw, 3),
            "rays_wall_s": round(tr, 3), "calls": [w.calls, r.calls], "codes": {str(c): int((st[:, 0] == c).sum()) for c in sorted(set(st[:, 0]))},
            "status_equal_to_wide": bool((st == ws).all()), "x_bits_equal_to_wide": bool(torch.equal(r.x.view(torch.int32), w.x.view(torch.int32))),
            "stopped_by_a_ray": {net.names[k]: [int(v) for v in st[k]] for k in np.flatnonzero((st[:, 0] == 4) | (st[:, 0] == 5))},
            "smallest_quality_at_the_last_check": float(f"{np.minimum(cert[:, 0], cert[:, 2]).min():.3g}")}
        # a certificate of code 4 says |x|_1 >= 1 / qp for every feasible x: where the wide call SOLVED the instance, compare with its x
        off = np.concatenate([[0], np.cumsum(net.inst_n)])
        wx = w.x.cpu().numpy()
        out["netlib_detection"]["code_4_on_instances_the_wide_call_solves"] = {
            net.names[k]: {"iterations": int(st[k, 1]), "bound_on_x_1norm": float(f"{1.0 / cert[k, 0]:.4g}"),
                           "x_1norm_of_the_wide_solution": float(f"{np.abs(wx[off[k]:off[k + 1]]).sum():.4g}")}
            for k in np.flatnonzero((st[:, 0] == 4) & (ws[:, 0] == 0))}
        out["netlib_detection"]["converged_wide"] = int((ws[:, 0] == 0).sum())
    print(json.dumps(out))


def spectral_bench(args, opts):
    """--spectral: see the module's docstring"""
    import time
    from mllp_amd.data import load_packed
    from mllp_amd.graph import LPBatch, synthetic_batch
    from mllp_amd.planted import planted_batch
    P, iters = args.power, args.plain_iters
    net = LPBatch.from_instances(load_packed())
    out = {"call": "mllp_lp_pdhg_spectral", "against": "mllp_lp_pdhg_wide", "options": opts, "power_iters": P, "per_iteration": [], "set_up": []}
    batches = [(f"Netlib {net.n_inst} instances", net, iters, args.calls, args.windows), ("planted 64 x (500 x 1200)", planted_batch(64, 500, 1200, 6.0, 2)[0], iters, args.calls, args.windows)]
    if args.synthetic > 0:
        batches.append((f"synthetic {args.synthetic} x (10000 x 20000)", synthetic_batch(n_inst=args.synthetic), 16, 1, 3))
    for name, b, K, n_calls, windows in () if "per_iteration" not in args.parts else batches:
        runs = {"wide": lambda K=K: b.pdhg_wide(K, check_every=0, **opts), "spectral": lambda K=K: b.pdhg_spectral(K, check_every=0, power_iters=P, **opts),
                "wide_set_up": lambda: b.pdhg_wide(0, check_every=0, **opts), "spectral_set_up_P0": lambda: b.pdhg_spectral(0, check_every=0, power_iters=0, **opts),
                "spectral_set_up": lambda: b.pdhg_spectral(0, check_every=0, power_iters=P, **opts)}
        for run in runs.values():
            run()
            run()
        torch.cuda.synchronize()
        dev = {key: [] for key in runs}
        for _ in range(windows):
            for key, run in runs.items():
                dev[key].append(device_window(run, n_calls))
        head = {"batch": name, "instances": b.n_inst, "nnz": b.dims()["nnz"], "iterations": K, "calls_per_window": n_calls, "windows": windows}
        # an iteration: the call's windows less the median set-up of the SAME call (the spectral call's set-up has 3 P + 1 launches more)
        net_dev = {n: [w - float(np.median(dev[s])) for w in dev[n]] for n, s in (("wide", "wide_set_up"), ("spectral", "spectral_set_up"))}
        fig = {n: figures(v, K)["us_per_iteration"] for n, v in net_dev.items()}
        inside = all(fig[o]["min"] * 0.99 <= fig[n]["median"] <= fig[o]["max"] * 1.01 for n, o in (("wide", "spectral"), ("spectral", "wide")))
        out["per_iteration"].append({**head, "us_per_iteration_without_set_up": fig, "whole_call": {n: figures(dev[n], K) for n in ("wide", "spectral")},
                                     "each_median_inside_the_others_windows_1pct": bool(inside)})
        out["set_up"].append({"batch": name, "calls_per_window": n_calls, "windows": windows,
                              **{n: figures(dev[n], 1)["device_ms_per_call"] for n in ("wide_set_up", "spectral_set_up_P0", "spectral_set_up")}})
    table, summary = {}, {}
    for eps in (1e-3, 1e-4) if "netlib" in args.parts else ():
        got = {}
        for power in (0, P):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = net.pdhg_spectral(args.netlib_iters, eps=eps, power_iters=power, poll_every=args.poll, **opts)
            torch.cuda.synchronize()
            got[power] = (r.status.cpu().numpy(), r.norm.cpu().numpy(), round(time.perf_counter() - t0, 3), r.calls)
        (s0, _, t_0, c0), (s1, nm, t_1, c1) = got[0], got[P]
        both = (s0[:, 0] == 0) & (s1[:, 0] == 0)
        fell = ~((nm[:, 0] > 0) & (nm[:, 0] <= nm[:, 1]))
        key = f"eps_{eps:g}"
        summary[key] = {"converged": {"P0": int((s0[:, 0] == 0).sum()), f"P{P}": int((s1[:, 0] == 0).sum())},
                        "gained": [net.names[k] for k in np.flatnonzero((s0[:, 0] != 0) & (s1[:, 0] == 0))],
                        "lost": [net.names[k] for k in np.flatnonzero((s0[:, 0] == 0) & (s1[:, 0] != 0))],
                        "iterations_on_those_both_solve": {"P0": int(s0[both, 1].sum()), f"P{P}": int(s1[both, 1].sum())},
                        "fewer_equal_more": [int((s1[both, 1] < s0[both, 1]).sum()), int((s1[both, 1] == s0[both, 1]).sum()), int((s1[both, 1] > s0[both, 1]).sum())],
                        "fell_back": [net.names[k] for k in np.flatnonzero(fell)], "wall_s": {"P0": t_0, f"P{P}": t_1}, "calls": {"P0": c0, f"P{P}": c1},
                        "bound_over_estimate": {"min": float(f"{(nm[~fell, 1] / nm[~fell, 0]).min():.3g}"), "max": float(f"{(nm[~fell, 1] / nm[~fell, 0]).max():.3g}")}}
        for k, name in enumerate(net.names):
            table.setdefault(name, {"m": net.inst_m[k], "n": net.inst_n[k], "sigma_est": float(f"{nm[k, 0]:.4g}"), "bound": float(f"{nm[k, 1]:.4g}")})[key] = {
                "P0": [int(s0[k, 0]), int(s0[k, 1])], f"P{P}": [int(s1[k, 0]), int(s1[k, 1])]}
    out.update(netlib_max_iters=args.netlib_iters, poll_every=args.poll, netlib_summary=summary, netlib=table)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--plain-iters", type=int, default=256)
    ap.add_argument("--netlib-iters", type=int, default=60000)
    ap.add_argument("--synthetic", type=int, default=4)
    ap.add_argument("--scaled", action="store_true")
    ap.add_argument("--halpern", action="store_true")
    ap.add_argument("--no-reflect", action="store_true")
    ap.add_argument("--wide", action="store_true")
    ap.add_argument("--rays", action="store_true")
    ap.add_argument("--spectral", action="store_true")
    ap.add_argument("--power", type=int, default=40)
    ap.add_argument("--ray-eps", type=float, default=None)
    ap.add_argument("--runs", default="wide,rays_off,rays_on")
    ap.add_argument("--rows", type=int, default=None)
    ap.add_argument("--poll", type=int, default=None)
    ap.add_argument("--ruiz", type=int, default=10)
    ap.add_argument("--no-pock-chambolle", action="store_true")
    ap.add_argument("--no-weight", action="store_true")
    ap.add_argument("--span", type=float, default=16.0)
    ap.add_argument("--only", default="per_iteration,netlib,cold_warm,oracle")
    args = ap.parse_args()
    parts = set(args.only.split(","))
    if args.scaled + args.halpern + args.wide + args.rays + args.spectral > 1:
        ap.error("--scaled, --halpern, --wide, --rays and --spectral name five calls: give one")
    if args.spectral:
        assert torch.cuda.is_available(), "bench_pdhg needs the GPU: there is no CPU path"
        args.parts = parts
        return spectral_bench(args, {"ruiz": args.ruiz, "pock_chambolle": not args.no_pock_chambolle, "primal_weight": not args.no_weight,
                                     "weight_span": args.span, "reflect": not args.no_reflect, "rows_per_item": args.rows})
    if args.rays:
        assert torch.cuda.is_available(), "bench_pdhg needs the GPU: there is no CPU path"
        return rays_bench(args, {"ruiz": args.ruiz, "pock_chambolle": not args.no_pock_chambolle, "primal_weight": not args.no_weight,
                                 "weight_span": args.span, "reflect": not args.no_reflect, "rows_per_item": args.rows})
    if args.scaled or args.halpern or args.wide:
        SOLVE.update(call="pdhg_wide" if args.wide else "pdhg_halpern" if args.halpern else "pdhg_scaled",
                     options={"ruiz": args.ruiz, "pock_chambolle": not args.no_pock_chambolle, "primal_weight": not args.no_weight,
                              "weight_span": args.span, **({"reflect": not args.no_reflect} if args.halpern or args.wide else {}),
                              **({"rows_per_item": args.rows} if args.wide else {})})
    assert torch.cuda.is_available(), "bench_pdhg needs the GPU: there is no CPU path"
    from mllp_amd.data import load_packed
    from mllp_amd.graph import LPBatch, pdhg_limits, synthetic_batch
    from mllp_amd.planted import planted_batch
    out = {"call": "mllp_lp_" + SOLVE["call"], "options": SOLVE["options"],
           "limits": {"lds_words": pdhg_limits()[0], "threads": pdhg_limits()[1]}}
    if args.wide and "cold_warm" in parts:
        parts.discard("cold_warm")          # (the rule's reach is --halpern's: the same bits)
    if "oracle" in parts:
        out["oracle_deviation_units"] = oracle_deviation()
    net = LPBatch.from_instances(load_packed())
    per_it = []
    small, _, _ = planted_batch(256, 50, 120, 6.0, 1)
    many, _, _ = planted_batch(1024, 50, 120, 6.0, 1)
    mid, _, _ = planted_batch(64, 500, 1200, 6.0, 2)
    for name, b, lds in () if "per_iteration" not in parts else ((f"Netlib {net.n_inst} instances", net, None), ("planted 256 x (50 x 120)", small, None),
                         ("planted 1024 x (50 x 120)", many, None), ("planted 64 x (500 x 1200)", mid, None),
                         ("planted 64 x (500 x 1200), vectors in scratch", mid, 0)):
        per_it.append({"batch": name, **shape_of(b), **timed(b, args.plain_iters, args.calls, args.windows, lds, check_every=0)})
    if args.synthetic > 0 and "per_iteration" in parts:
        syn = synthetic_batch(n_inst=args.synthetic)
        per_it.append({"batch": f"synthetic {args.synthetic} x (10000 x 20000)", **shape_of(syn), **timed(syn, 16, 1, 3, None, check_every=0)})
        del syn
    out["per_iteration"] = per_it
    # Netlib: where the baseline gets within --netlib-iters
    table = {}
    for eps in ((1e-3,) if args.wide else (1e-3, 1e-4)) if "netlib" in parts else ():
        import time
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = solve(net, args.netlib_iters, eps=eps, **({"poll_every": args.poll} if args.wide else {}))
        torch.cuda.synchronize()
        st, kkt = res.status.cpu().numpy(), res.kkt.cpu().numpy()
        if args.wide:
            wall = time.perf_counter() - t0
            t0 = time.perf_counter()
            ref = net.pdhg_halpern(args.netlib_iters, eps=eps, **{k: v for k, v in SOLVE["options"].items() if k != "rows_per_item"})
            torch.cuda.synchronize()
            ref_st = ref.status.cpu().numpy()
            out["netlib_wide_against_persistent"] = {
                "eps": eps, "poll_every": args.poll, "calls": res.calls, "wide_wall_s": round(wall, 3),
                "persistent_wall_s": round(time.perf_counter() - t0, 3), "converged_sets_equal": bool(((st[:, 0] == 0) == (ref_st[:, 0] == 0)).all()),
                "status_equal": bool((st == ref_st).all()), "x_bits_equal": bool(torch.equal(res.x.view(torch.int32), ref.x.view(torch.int32)))}
        for k, name in enumerate(net.names):
            table.setdefault(name, {"m": net.inst_m[k], "n": net.inst_n[k]})[f"eps_{eps:g}"] = {
                "code": int(st[k, 0]), "iterations": int(st[k, 1]), "restarts": int(st[k, 2]),
                "primal": float(f"{kkt[k, 0]:.3g}"), "dual": float(f"{kkt[k, 1]:.3g}"), "gap": float(f"{kkt[k, 2]:.3g}")}
        out.setdefault("netlib_converged", {})[f"eps_{eps:g}"] = int((st[:, 0] == 0).sum())
    out["netlib_max_iters"] = args.netlib_iters
    out["netlib"] = table
    if "cold_warm" not in parts:
        print(json.dumps(out))
        return
    # cold against warm on a planted batch
    cold = solve(small, 8192)
    warm = solve(small, 8192, start=small.solve_basis(small.labels))
    far = solve(small, 8192, start=small.repair_basis(torch.randn(small.N, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))))
    torch.cuda.synchronize()
    rows = {}
    for name, r in (("cold", cold), ("warm_from_repair_basis_of_the_labels", warm), ("warm_from_repair_basis_of_a_random_ranking", far)):
        st = r.status.cpu().numpy()
        rows[name] = {"converged": int((st[:, 0] == 0).sum()), "iterations_mean": round(float(st[:, 1].mean()), 1),
                      "iterations_max": int(st[:, 1].max())}
    got = small.solved(small.pdhg_basis(cold), 1e-3, 1e-3)
    rows["cold"]["optimal_after_pdhg"] = int(got["optimal"].sum())
    out["cold_warm"] = {"batch": "planted 256 x (50 x 120)", "eps": 2.0 ** -10, "max_iters": 8192, **rows}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
