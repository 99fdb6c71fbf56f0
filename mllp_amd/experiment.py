"""Training driver with the CLI, outputs and loop semantics of the reference's
`linear_program_experiment.py` for the sparse bipartite methods ('gs-topk', 'soft-topk').

    python linear_program_experiment.py --cfg linear_program_netlib.yaml

reference linear_program_experiment.py:17-46 (config, seed, dataset, criterion), :115-157 (loop:
graph -> forward -> BCEWithLogitsLoss -> backward -> Adam step -> top-m F1 / correct count ->
print / train_log.json), :176-177 (torch.save(state_dict) to linear_program_<data>_<method>.pt).

What differs, by design: the graph of an instance is built once and stays in HBM (the reference
rebuilds it in Python every step, :124); forward/BCE/backward/Adam/metrics run in libmllp_hip.so;
`batch_size` (optional yaml key) > 1 groups instances into block-diagonal batches with ONE Adam step
per batch; with WORLD_SIZE > 1 (torchrun) each batch is sharded over the ranks and the flat gradient is
all-reduced over RCCL.  `batch_size: 1` on one GPU reproduces the reference's update sequence.
"""
import json
import os
import sys
import time

import numpy as np
import torch

from .config import load_config
from .data import LPInstance, get_netlib_dataset
from .model import GNNModel, set_seed

SPARSE_METHODS = ("gs-topk", "soft-topk")


def _dist_setup():
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        local = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(local)
        if not dist.is_initialized():
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        return dist.get_rank(), world
    return 0, 1


def plan_batches(instances, batch_size, rank, world):
    """Groups of `batch_size` consecutive instances (0 = the whole dataset); with world > 1 every group is sharded
    over the ranks by nnz (trainer.shard_instances).  Returns [(global ids owned by this rank, global group size)]."""
    from .trainer import shard_instances
    bs = int(batch_size)
    if bs <= 0:
        bs = len(instances)
    plan = []
    for i in range(0, len(instances), bs):
        grp = list(range(i, min(i + bs, len(instances))))
        mine = grp if world == 1 else [grp[j] for j in shard_instances([instances[k].nnz for k in grp], world)[rank]]
        plan.append((mine, len(grp)))
    return plan


def holdout_by_fraction(n, f):
    """The held-out instances of a dataset of `n` for the yaml key `holdout: f`, 0 < f < 1: with the instances in dataset
    order, instance i is held out iff floor((i + 1) f) > floor(i f) -- floor(n f) of them, evenly spread, the same ones
    on every run and every rank."""
    f = float(f)
    if not 0.0 < f < 1.0:
        raise ValueError(f"holdout: a fraction must lie in (0, 1), got {f!r}")
    return [i for i in range(int(n)) if int(np.floor((i + 1) * f)) > int(np.floor(i * f))]


def split_holdout(names, holdout):
    """(trained ids, held-out ids) of the instances `names` (dataset order) for the yaml key `holdout`: None / an empty
    list (nothing held out), a list of instance names (an unknown name raises), or a fraction (`holdout_by_fraction`)."""
    names = list(names)
    if holdout is None or (isinstance(holdout, (list, tuple)) and not holdout):
        return list(range(len(names))), []
    if isinstance(holdout, bool) or isinstance(holdout, str):
        raise ValueError(f"holdout: expected a list of instance names or a fraction in (0, 1), got {holdout!r}")
    if isinstance(holdout, (int, float)):
        held = holdout_by_fraction(len(names), holdout)
    else:
        unknown = [h for h in holdout if h not in names]
        if unknown:
            raise ValueError(f"holdout: unknown instance name(s) {unknown} (the dataset has {names})")
        held = sorted({names.index(h) for h in holdout})
    heldset = set(held)
    return [i for i in range(len(names)) if i not in heldset], held


def plan_split_batches(instances, ids, batch_size, rank, world):
    """`plan_batches` over the sub-list `ids` of `instances`, in GLOBAL ids."""
    sub = [instances[i] for i in ids]
    return [([ids[j] for j in mine], gcount) for mine, gcount in plan_batches(sub, batch_size, rank, world)]


def run_epochs(cfg, instances, train_dict, trainer, batches, rank, world, device, start_epoch=0, out=print,
               save_all=None, holdout=(), n_holdout=0):
    """The epoch loop of reference linear_program_experiment.py:120-157 over prebuilt batches, for any trainer
    with `step(batch) -> (loss, logits)`, `step_empty()` and `metrics_of(batch) -> [n, 2]` (correct_num, f1).

    `batches` = [(global instance ids of THIS rank, batch or None, global instance count of the group)].
    With world > 1 the per-instance metrics of every rank are summed into one dense [n_instances, 2] tensor
    (each instance is owned by exactly one rank), so rank 0 prints and logs the complete epoch; the other
    ranks print nothing and write no files.

    `holdout` = [(global instance ids of THIS rank, batch)] of held-out instances, `n_holdout` their number over all
    ranks: never passed to `step`; on every logging epoch `trainer.evaluate(batch)` -> dict(inst_loss [n], metrics
    [n, 2]) gives their correct counts (logged under their names like everyone's) and `val_obj`, the mean of their
    losses.  `obj` stays the mean over the trained instances."""
    n_holdout = int(n_holdout)
    if n_holdout and not hasattr(trainer, "evaluate"):
        raise ValueError(f"holdout: {n_holdout} held-out instance(s), but {type(trainer).__name__} has no evaluate(batch)")
    n_train = len(instances) - n_holdout
    dist = None
    if world > 1:
        import torch.distributed as dist
    log_every = max(int(cfg.get_default("log_every")), 1)
    report = cfg.get_default("report_solved")
    save_every = int(cfg.get_default("save_every"))
    optim_log = OptimLog(trainer)
    for epoch in range(start_epoch, cfg.train_iter):                                # reference :120
        obj_sum = torch.zeros(1, device=device)
        optim_log.reset()
        logging = epoch % log_every == 0
        table = torch.zeros(len(instances), 2, device=device) if logging else None
        train_solved = torch.zeros(len(report_keys(report)), device=device) if logging and report is not None and not n_holdout else None
        for mine, b, gcount in batches:
            if b is None:      # a rank without instances in this batch still joins the all-reduce
                trainer.step_empty()
                optim_log.add()
                continue
            trainer.global_instances = gcount
            loss, step_logits = trainer.step(b)                                     # reference :124-144
            optim_log.add()
            if train_solved is not None:            # (the logits of the step's forward, valid until the next step)
                train_solved += report_counts(b, step_logits, report).to(device)
            obj_sum += loss.to(device) * gcount     # loss is the batch mean over gcount instances (this rank's share)
            if logging:
                table[torch.as_tensor(mine, device=device)] = trainer.metrics_of(b).to(device)
        val_sum = torch.zeros(1, device=device) if logging and n_holdout else None
        if val_sum is not None:
            for mine, b in holdout:
                if b is None:
                    continue
                ev = trainer.evaluate(b)
                val_sum += ev["inst_loss"].to(device).sum()
                table[torch.as_tensor(mine, device=device)] = ev["metrics"].to(device)
        solved = None
        if logging and report is not None:      # held-out instances, or the trained ones without a holdout
            solved = train_solved if train_solved is not None else torch.zeros(len(report_keys(report)), device=device)
            for _, b in (holdout if n_holdout else ()):
                if b is not None:
                    solved += report_counts(b, trainer.evaluate(b)["logits"], report).to(device)
        if dist is not None:
            dist.all_reduce(obj_sum)
            if logging:
                dist.all_reduce(table)
            if solved is not None:
                dist.all_reduce(solved)
            if val_sum is not None:
                dist.all_reduce(val_sum)
        obj = float(obj_sum[0]) / n_train
        if logging:
            met = table.cpu().numpy()
            for gi, inst in enumerate(instances):      # groups are consecutive id ranges: this is the dataset order
                correct_num, f1 = float(met[gi, 0]), float(met[gi, 1])              # reference :146-153
                if rank == 0:
                    out("%8d, %8d, %8d, %5f" % (correct_num, inst.m, inst.n, f1))
                train_dict[inst.name].append(correct_num)
        if solved is not None:
            for key, v in zip(report_keys(report), solved.cpu().tolist()):
                train_dict.setdefault(key, []).append(int(v))
        train_dict["obj"].append(obj)                  # plain float: the reference's numpy.float32 breaks json.dump
        if logging:
            optim_log.log(train_dict)
        val_obj = None
        if val_sum is not None:
            val_obj = float(val_sum[0]) / n_holdout
            train_dict.setdefault("val_obj", []).append(val_obj)
        if rank == 0:
            with open("train_log.json", "w") as json_file:                          # reference :155-156
                json.dump(train_dict, json_file)
            out(f"epoch {epoch}, obj={obj}" + ("" if val_obj is None else f", val_obj={val_obj}"))    # reference :157
        if save_all is not None and save_every and (epoch + 1) % save_every == 0:
            save_all(epoch)
    return train_dict


SOLVED_KEYS = ("usable", "feasible", "optimal", "skipped")


def solved_counts(batch, logits, report):
    """[4] device counts over a batch's instances, by SOLVED_KEYS: the predicted ranking repaired into a nonsingular basis
    and solved on the device (LPBatch.repair_basis), then certified (LPBatch.solved) under the yaml block `report_solved`
    {feas_tol, opt_tol, max_m}.  Instances with m > max_m are `skipped` and in no other count.  No sync."""
    for key in ("feas_tol", "opt_tol"):
        if key not in report:
            raise ValueError(f"report_solved: {key} is required")
    rep = batch.repair_basis(logits, max_m=report.get("max_m"), want=("basis", "x", "y"))
    got = batch.solved(rep, report["feas_tol"], report["opt_tol"])
    return torch.stack([got["usable"].sum(), got["primal_feasible"].sum(), got["optimal"].sum(), got["skipped"].sum()]).float()


PIVOT_KEYS = ("optimal_after_pivots", "pivots")


def pivot_counts(batch, logits, report):
    """[2] device counts over a batch's instances, by PIVOT_KEYS, under `report_solved` {..., pivots: K}: the repaired
    prediction pivoted to the optimum on the device (LPBatch.simplex, at most K pivots per instance), the final basis
    factorized afresh and certified (LPBatch.simplex_solved) -- the instances certified optimal, and the pivots they took
    in all.  `refactor: R` and `stall: S` in the block are LPBatch.simplex's refactor_every and stall_pivots; without them
    the call is the one it was.  No sync."""
    max_m = report.get("max_m")
    rep = batch.repair_basis(logits, max_m=max_m, want=("basis",))
    guards = {key: int(report[name]) for name, key in (("refactor", "refactor_every"), ("stall", "stall_pivots")) if report.get(name) is not None}
    res = batch.simplex(rep, int(report["pivots"]), max_m=max_m, want=(), **guards)
    got = batch.simplex_solved(res, report["feas_tol"], report["opt_tol"], max_m=max_m)
    done = got["optimal"] & (res.status[:, 0] == 0)
    return torch.stack([done.sum(), (got["pivots"] * done).sum()]).float()


PDHG_KEYS = ("pdhg_converged", "pdhg_iterations", "optimal_after_pdhg")
PDHG_RAY_KEYS = ("pdhg_infeasible", "pdhg_unbounded")       # with `rays` inside the pdhg block


def _pdhg_rays(opt):
    """the `rays` option of the pdhg block: None when absent or false, else ray_eps"""
    rays = opt.get("rays")
    if rays is None or rays is False:
        return None
    own = {} if rays is True else dict(rays)
    if set(own) - {"eps"}:
        raise ValueError(f"report_solved: pdhg: rays: unknown keys {sorted(set(own) - {'eps'})}")
    ray_eps = float(own.get("eps", 2.0 ** -10))
    if not ray_eps >= 0.0 or ray_eps == float("inf"):
        raise ValueError("report_solved: pdhg: rays: eps must be finite and not negative")
    return ray_eps


def _pdhg_spectral(opt):
    """the `spectral` option of the pdhg block: None when absent or false, else power_iters"""
    spectral = opt.get("spectral")
    if spectral is None or spectral is False:
        return None
    own = {} if spectral is True else dict(spectral)
    if set(own) - {"iters"}:
        raise ValueError(f"report_solved: pdhg: spectral: unknown keys {sorted(set(own) - {'iters'})}")
    power = int(own.get("iters", 40))
    if power < 0:
        raise ValueError("report_solved: pdhg: spectral: iters must not be negative")
    return power


def pdhg_counts(batch, logits, report):
    """[3] device counts over a batch's instances, by PDHG_KEYS, under `report_solved` {..., pdhg: {iters: K, eps: E}}
    (optional: `check`, default 64, and `warm`, default true): every instance solved by restarted PDHG on the device
    (LPBatch.pdhg, at most K iterations, relative KKT error E) -- the instances that converged, the iterations all of them
    took, and the instances whose iterate points at a vertex that is certified optimal (LPBatch.pdhg_basis + solved, under
    the block's tolerances and max_m).  With `warm` the start is the repaired prediction's basic solution where it is
    usable and cold (zeros, which is what repair_basis leaves) otherwise.  PDHG itself has no row limit.  `scaled: true`
    selects the preconditioned call (LPBatch.pdhg_scaled) with its defaults; a mapping {ruiz, pock_chambolle, weight, span}
    sets its options.  `halpern: true` selects Halpern's iteration (LPBatch.pdhg_halpern), `halpern: {reflect: false}` its
    unreflected form; it takes the `scaled:` options too (`scaled: false` beside it is refused: the call is preconditioned).
    `wide: true` runs Halpern's iteration across the whole device (LPBatch.pdhg_wide: the same rule and the same bits, for
    instances too long for one workgroup), `wide: {rows: R, poll: P}` with R rows per work item and the codes polled every
    P iterations (one sync per poll; an early stop then costs nothing); it takes the `halpern:` and `scaled:` options, and
    `scaled: false` beside it is refused likewise.  `rays: true` or `rays: {eps: E}` selects the wide call with certificates
    of infeasibility and unboundedness (LPBatch.pdhg_rays, ray_eps E, default 2^-10): it implies `wide` (`wide: false` beside
    it is refused), takes its options, and two more counts are returned, by PDHG_RAY_KEYS: the instances that ended with
    code 4 and with code 5 -- "no feasible point with a 1-norm below 1 / E" and its dual, which is infeasibility only where E
    is small against the solutions' size.  `spectral: true` or `spectral: {iters: P}` selects the wide call whose step comes
    from P rounds (default 40) of power iteration on the device (LPBatch.pdhg_spectral): it implies `wide` (`wide: false` or
    `scaled: false` beside it is refused), takes its options, and combines with `rays` (without `rays` detection is off and
    the log keys are the ones they were).  Without any of the five keys (or with `false`) the call is LPBatch.pdhg.  No sync
    unless `poll` is given."""
    opt = report["pdhg"]
    for key in ("iters", "eps"):
        if key not in opt:
            raise ValueError(f"report_solved: pdhg: {key} is required")
    max_m = report.get("max_m")
    start = batch.repair_basis(logits, max_m=max_m, want=("basis", "x", "y")) if opt.get("warm", True) else None
    scaled, halpern, wide = opt.get("scaled"), opt.get("halpern"), opt.get("wide")
    ray_eps = _pdhg_rays(opt)
    if ray_eps is not None and wide is False:
        raise ValueError("report_solved: pdhg: rays runs on the wide call: it cannot go with wide: false")
    power = _pdhg_spectral(opt)
    if power is not None and wide is False:
        raise ValueError("report_solved: pdhg: spectral runs on the wide call: it cannot go with wide: false")
    halpern = None if halpern is False else halpern
    wide = None if wide is False else wide
    if (ray_eps is not None or power is not None) and wide is None:
        wide = True                 # the call with certificates, and the one with the spectral step, ARE the wide call
    if wide is not None and scaled is False:
        raise ValueError("report_solved: pdhg: wide is a preconditioned call: it cannot go with scaled: false")
    if wide is not None and halpern is None:
        halpern = True              # the wide call IS Halpern's iteration
    if halpern is not None and scaled is False:
        raise ValueError("report_solved: pdhg: halpern is a preconditioned call: it cannot go with scaled: false")
    if halpern is None and (scaled is None or scaled is False):
        res = batch.pdhg(int(opt["iters"]), eps=float(opt["eps"]), check_every=int(opt.get("check", 64)), start=start)
    else:
        more = {} if scaled is True or scaled is None else dict(scaled)
        unknown = set(more) - {"ruiz", "pock_chambolle", "weight", "span"}
        if unknown:
            raise ValueError(f"report_solved: pdhg: scaled: unknown keys {sorted(unknown)}")
        kw = dict(ruiz=int(more.get("ruiz", 10)), pock_chambolle=bool(more.get("pock_chambolle", True)),
                  primal_weight=bool(more.get("weight", True)), weight_span=float(more.get("span", 16.0)))
        if halpern is not None:
            own = {} if halpern is True else dict(halpern)
            if set(own) - {"reflect"}:
                raise ValueError(f"report_solved: pdhg: halpern: unknown keys {sorted(set(own) - {'reflect'})}")
            kw["reflect"] = bool(own.get("reflect", True))
        if wide is not None:
            own = {} if wide is True else dict(wide)
            if set(own) - {"rows", "poll"}:
                raise ValueError(f"report_solved: pdhg: wide: unknown keys {sorted(set(own) - {'rows', 'poll'})}")
            rows, poll = own.get("rows"), own.get("poll")
            if rows is not None and (int(rows) <= 0 or int(rows) % 64):
                raise ValueError("report_solved: pdhg: wide: rows must be a positive multiple of 64")
            if poll is not None and int(poll) <= 0:
                raise ValueError("report_solved: pdhg: wide: poll must be positive")
            kw.update(rows_per_item=None if rows is None else int(rows), poll_every=None if poll is None else int(poll))
        if ray_eps is not None:
            kw["ray_eps"] = ray_eps
        if power is not None:
            kw["power_iters"] = power
        call = (batch.pdhg_spectral if power is not None else batch.pdhg_rays if ray_eps is not None else batch.pdhg_wide if wide is not None else batch.pdhg_scaled if halpern is None
                else batch.pdhg_halpern)
        res = call(int(opt["iters"]), eps=float(opt["eps"]), check_every=int(opt.get("check", 64)), start=start, **kw)
    got = batch.solved(batch.pdhg_basis(res, max_m=max_m), report["feas_tol"], report["opt_tol"])
    counts = [(res.status[:, 0] == 0).sum(), res.status[:, 1].sum(), got["optimal"].sum()]
    if ray_eps is not None:
        counts += [(res.status[:, 0] == 4).sum(), (res.status[:, 0] == 5).sum()]
    return torch.stack(counts).float()


def report_keys(report):
    """the keys `report_solved` adds to the log: SOLVED_KEYS, PIVOT_KEYS when the block has `pivots`, PDHG_KEYS when it
    has `pdhg`, and PDHG_RAY_KEYS when that has `rays`"""
    pdhg = report.get("pdhg")
    return (SOLVED_KEYS + (PIVOT_KEYS if report.get("pivots") is not None else ()) + (PDHG_KEYS if pdhg is not None else ())
            + (PDHG_RAY_KEYS if pdhg is not None and _pdhg_rays(pdhg) is not None else ()))


def report_counts(batch, logits, report):
    counts = [solved_counts(batch, logits, report)]
    if report.get("pivots") is not None:
        counts.append(pivot_counts(batch, logits, report))
    if report.get("pdhg") is not None:
        counts.append(pdhg_counts(batch, logits, report))
    return counts[0] if len(counts) == 1 else torch.cat(counts)


def train_method(cfg, method_name, train_dataset, train_dict, out=print):
    from .graph import LPBatch
    from .trainer import LPTrainer
    rank, world = _dist_setup()
    model_path = f"linear_program_{cfg.train_data_type}_{method_name}.pt"
    ckpt_path = f"linear_program_{cfg.train_data_type}_{method_name}.ckpt"
    if rank == 0:
        out(f"Training the model weights for {method_name}...")
    if str(cfg.get_default("dtype")).lower() not in ("f32", "fp32", "float32"):
        raise NotImplementedError(
            f"dtype: {cfg.get_default('dtype')!r}: the training step computes and stores fp32 (the reference's arithmetic, "
            "north_star's 1e-5 parity bar); the opt-in bf16 feature image exists for the plain SpMM only "
            "(LPBatch.spmm_bf16 / mllp_spmm_csr_bf16), where it measured slower than fp32 (DESIGN.md section 6)")
    device = torch.device(cfg.get_default("device"))
    if device.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError("this build runs the learned-LP path on MI355X through HIP only (device: 'cuda'); "
                           "there is no CPU fallback")
    model = GNNModel().to(device)                     # reference :117
    if world > 1:                                     # same initial weights on every rank
        import torch.distributed as dist
        flat0 = model.flat_parameters().detach().clone()
        dist.broadcast(flat0, src=0)
        model.load_flat(flat0)
    instances = [LPInstance.from_reference_tuple(t) for t in train_dataset]
    make = lambda mine: LPBatch.from_instances([instances[i] for i in mine]) if mine else None  # noqa: E731
    train_ids, held_ids = split_holdout([i.name for i in instances], cfg.get_default("holdout"))
    extra = {}
    if not held_ids:           # (no holdout: the calls of a build without the key)
        batches = [(mine, make(mine), gcount)
                   for mine, gcount in plan_batches(instances, cfg.get_default("batch_size"), rank, world)]
    else:
        if not train_ids:
            raise ValueError("holdout: every instance is held out, nothing is left to train on")
        batches = [(mine, make(mine), gcount)
                   for mine, gcount in plan_split_batches(instances, train_ids, cfg.get_default("batch_size"), rank, world)]
        extra = dict(n_holdout=len(held_ids),
                     holdout=[(mine, make(mine)) for mine, _ in
                              plan_split_batches(instances, held_ids, cfg.get_default("batch_size"), rank, world)])
    pos_weight = cfg.get_default("pos_weight")
    trainer = LPTrainer(model.flat_parameters().detach(), lr=cfg.train_lr,
                        use_hip_graph=cfg.get_default("use_hip_graph"), with_metrics=True,
                        tiled_copies=cfg.get_default("tiled_copies"),
                        **({} if pos_weight is None else dict(pos_weight=pos_weight)), **topm_head(cfg, method_name),
                        **optimizer_options(cfg))
    start_epoch = 0
    if cfg.get_default("resume") and os.path.exists(ckpt_path):
        start_epoch = load_checkpoint(ckpt_path, trainer, train_dict, device)
        if rank == 0:
            out(f"resumed from {ckpt_path} at epoch {start_epoch}")

    def save_all(epoch):
        if rank != 0:
            return
        model.load_flat(trainer.params)
        torch.save(model.state_dict(), model_path)                                   # reference :176
        save_checkpoint(ckpt_path, trainer, train_dict, epoch)

    run_epochs(cfg, instances, train_dict, trainer, batches, rank, world, device, start_epoch, out, save_all, **extra)
    save_all(cfg.train_iter - 1)
    if rank == 0:
        out(f"Model saved to {model_path}.")
    return model_path


def topm_head(cfg, method_name):
    """LPTrainer's arguments for the yaml key `loss_head`: {} for 'bce' (or no key: the trainer of a build without it); for
    'topm' the soft top-m head at `topm_tau` -- without noise under the method 'soft-topk', with `train_gumbel_sample_num`
    Gumbel samples of scale `gumbel_sigma` under 'gs-topk' (the reference's yaml keys, linear_program_netlib.yaml)."""
    head = cfg.get_default("loss_head")
    if head in (None, "bce"):
        return {}
    if head != "topm":
        raise ValueError(f"loss_head: 'bce' or 'topm', got {head!r}")
    out = dict(loss_head="topm", topm_tau=float(cfg.get_default("topm_tau")))
    if method_name == "gs-topk":
        for key in ("train_gumbel_sample_num", "gumbel_sigma"):
            if key not in cfg:
                raise ValueError(f"loss_head 'topm' with method 'gs-topk' reads the yaml key {key}")
        out.update(topm_samples=int(cfg["train_gumbel_sample_num"]), topm_sigma=float(cfg["gumbel_sigma"]))
    return out


def optimizer_options(cfg):
    """LPTrainer's / AngleStepper's arguments for the yaml keys `weight_decay`, `clip_norm` and `lr_schedule` {warmup, total,
    min_ratio}: {} with none of them set (the trainer of a build without the keys); ValueError for a bad value."""
    from .trainer import check_optim_options, lr_schedule_args
    wd, clip, sched = cfg.get_default("weight_decay"), cfg.get_default("clip_norm"), cfg.get_default("lr_schedule")
    wd, clip = 0.0 if wd is None else wd, 0.0 if clip is None else clip
    check_optim_options(wd, clip, *lr_schedule_args(sched))
    if not wd and not clip and sched is None:
        return {}
    return dict(weight_decay=float(wd), clip_norm=float(clip), lr_schedule=None if sched is None else dict(sched))


class OptimLog:
    """`grad_norm` and `lr` of train_log.json for an optimizer with `info` (FlatAdamW): the mean of info[0] over the steps
    an epoch took (skipped steps apart) and the last info[2], accumulated on the device -- `add` never synchronises."""

    def __init__(self, trainer):
        self.info = getattr(getattr(trainer, "opt", None), "info", None)
        self.reset()

    def reset(self):
        if self.info is not None:
            self.acc = torch.zeros(2, device=self.info.device)      # {sum of norms, steps taken}

    def add(self):
        if self.info is not None:
            taken = 1.0 - self.info[3]
            self.acc += torch.stack([torch.where(taken > 0, self.info[0], torch.zeros_like(taken)), taken])

    def log(self, train_dict):
        if self.info is not None:
            total, steps = self.acc.tolist()
            train_dict.setdefault("grad_norm", []).append(total / max(steps, 1.0))
            train_dict.setdefault("lr", []).append(float(self.info[2]))


def save_checkpoint(path, trainer, train_dict, epoch):
    """Everything a restart needs: weights, Adam moments + step counter, the epoch, the log so far (and, under the top-m
    head, the step count that seeds the next step's noise).  Under weight_decay / clip_norm / lr_schedule the optimizer's
    state has 8 words (FlatAdamW: the schedule travels with it and a resume continues it); a checkpoint from before those
    keys holds 4, which FlatAdamW.load_state_dict continues under the schedule of the yaml file."""
    extra = {"topm_step": int(trainer.topm_step)} if getattr(trainer, "loss_head", "bce") == "topm" else {}
    torch.save({"params": trainer.params, "opt": trainer.opt.state_dict(), "epoch": epoch,
                "train_dict": json.dumps(train_dict), **extra}, path)


def load_checkpoint(path, trainer, train_dict, device):
    ck = torch.load(path, map_location=device, weights_only=True)
    trainer.params.copy_(ck["params"])
    trainer.opt.load_state_dict(ck["opt"])
    if "topm_step" in ck:
        trainer.topm_step = int(ck["topm_step"])
    train_dict.update({k: list(v) for k, v in json.loads(ck["train_dict"]).items()})
    return int(ck["epoch"]) + 1


def train_angle(cfg, method_name, train_dataset, train_dict, out=print):
    """reference linear_program_experiment.py:81-114: AngleModel(feat_dim=256) on the complete angle graph of the
    dense dataset's instance, BCEWithLogits + Adam, top-k metrics, train_log.json, state_dict .pt."""
    from .angle import AngleModel, AngleStepper, get_netlib_dataloader
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        # one instance, one dense graph: nothing to shard, and N ranks would all write the same files
        raise RuntimeError("the angleNet method trains a single instance: run it with one rank")
    out(f"Training the model weights for {method_name}...")
    device = torch.device(cfg.get_default("device"))
    if device.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError("this build runs the learned-LP path on MI355X through HIP only (device: 'cuda'); "
                           "there is no CPU fallback")
    train_loader = get_netlib_dataloader(train_dataset, device)                     # reference :33
    model = AngleModel(feat_dim=int(cfg.get_default("angle_feat_dim"))).to(device)  # reference :83
    # reference :41, :87-96: BCEWithLogitsLoss + torch.optim.Adam around autograd -- here the same arithmetic on flat
    # parameters without autograd (AngleStepper: C ABI forward / backward, the library's Adam kernel; tests/test_angle.py
    # checks it step for step against the nn.Module + torch.optim loop), 2-3 x faster per step on small instances
    stepper = AngleStepper(model, lr=cfg.train_lr, **optimizer_options(cfg))
    optim_log = OptimLog(stepper)
    for epoch in range(cfg.train_iter):
        obj_sum = 0.0
        optim_log.reset()
        for graph in train_loader:
            name, basis_num, var_num = graph.name, graph.basis_num, graph.var_num
            basis_opt = torch.tensor(np.asarray(graph.basis_opt), dtype=torch.float, device=device)
            obj, latent_vars = stepper.step(graph, basis_opt)
            optim_log.add()
            obj_sum += float(obj.detach())
            pred_indices = torch.topk(latent_vars, k=basis_num)[-1].cpu().detach().numpy()
            pred = np.zeros(var_num)
            pred[pred_indices] = 1
            truth = basis_opt.cpu().numpy()
            correct_num = float(pred @ truth)
            tp = correct_num
            f1 = 2.0 * tp / max(pred.sum() + truth.sum(), 1.0)                      # sklearn f1_score on {0,1} vectors
            out("%8d, %8d, %8d, %5f" % (correct_num, basis_num, var_num, f1))
            train_dict[name].append(correct_num)
        train_dict["obj"].append(obj_sum / len(train_dataset))
        optim_log.log(train_dict)
        with open("train_log.json", "w") as json_file:
            json.dump(train_dict, json_file)
        out(f"epoch {epoch}, obj={obj_sum / len(train_dataset)}")
    model_path = f"linear_program_{cfg.train_data_type}_{method_name}.pt"
    model.load_flat(stepper.params)
    torch.save(model.state_dict(), model_path)                                      # reference :176
    out(f"Model saved to {model_path}.")
    return train_dict


def main(argv=None):
    cfg = load_config(argv)                                                         # reference :17
    set_seed()                                                                      # reference :19
    if cfg.train_data_type == "netlib":                                             # reference :28-35
        names = cfg.get_default("instances")
        if cfg.methods[0] == "invariant":
            raise NotImplementedError(
                "method 'invariant' is the reference's InvariantModel research path (reference "
                f"linear_program_methods.py:136-185), not built: use 'angleNet' or one of {SPARSE_METHODS}")
        if cfg.methods[0] == "angleNet":                                            # reference :31-33
            from .data import get_netlib_dataset_dense
            train_dataset, train_dict = get_netlib_dataset_dense(normalize=True, names=names)
        else:
            train_dataset, train_dict = get_netlib_dataset(normalize=True, names=names)
    elif cfg.train_data_type == "planted":          # labelled LPs built on the device (mllp_amd/planted.py)
        unsupported = [m for m in cfg.methods if m not in SPARSE_METHODS]
        if unsupported:
            raise ValueError(f"train_data_type 'planted' feeds the sparse bipartite methods {SPARSE_METHODS} only, "
                             f"not {unsupported}")
        from .planted import planted_dataset
        train_dataset, train_dict = planted_dataset(cfg.get_default("planted"), cfg.get_default("device"))
    else:
        raise ValueError(f"Unknown training dataset {cfg.train_data_type}!")
    for method_name in cfg.methods:                                                 # reference :45
        if method_name in SPARSE_METHODS:
            train_method(cfg, method_name, train_dataset, train_dict)
        elif method_name == "angleNet":
            train_angle(cfg, method_name, train_dataset, train_dict)
        else:
            raise NotImplementedError(f"method {method_name!r} is outside the sparse bipartite hot path of this "
                                      f"build (supported: {SPARSE_METHODS})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
