"""Batched training step of the learned-LP path: forward + BCE + backward in ONE library call,
gradient all-reduce across data-parallel ranks (RCCL over xGMI through torch.distributed), flat Adam.

Replaces the inner loop of reference linear_program_experiment.py:120-157 (graph rebuild, forward,
BCEWithLogitsLoss, autograd backward, Adam step, top-m metrics -- all per instance on the CPU).

Data parallelism: LP instances are independent blocks of the block-diagonal
batch, so a rank owns a subset of instances and builds its own LPBatch; the loss is the sum over
instances of the per-instance mean BCE divided by the GLOBAL instance count, hence summed per-rank
gradients equal the single-GPU batch gradient.  One all-reduce of the flat 4721-float gradient buffer
(18.9 KB, latency bound) per step; weights stay replicated because every rank applies the same Adam.
"""
import os
from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .graph import LPBatch, adam_step, optim_scratch_floats, optim_step

NUM_PARAMS = _lib.NUM_PARAMS


def shard_instances(sizes: Sequence[int], world_size: int) -> List[List[int]]:
    """Greedy longest-processing-time assignment of instances (weights = nnz) to ranks.
    Returns per-rank lists of instance indices (each sorted ascending); deterministic."""
    order = sorted(range(len(sizes)), key=lambda i: (-int(sizes[i]), i))
    loads = [0] * world_size
    out = [[] for _ in range(world_size)]
    for i in order:
        r = min(range(world_size), key=lambda q: (loads[q], q))
        out[r].append(i)
        loads[r] += int(sizes[i])
    return [sorted(v) for v in out]


class FlatAdam:
    """torch.optim.Adam(lr, betas=(0.9, 0.999), eps=1e-8) on flat buffers, backend-agnostic:
    `backend='hip'` uses mllp_adam_step, `backend='torch'` is the same arithmetic in torch ops
    (used by the CPU/gloo tests of the data-parallel logic)."""

    def __init__(self, params: torch.Tensor, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, backend="hip"):
        self.params = params
        self.m = torch.zeros_like(params)
        self.v = torch.zeros_like(params)
        self.eps = eps
        self.backend = backend
        self.state = torch.tensor([0.0, lr, betas[0], betas[1]], dtype=torch.float32, device=params.device)

    def step(self, grads, grad_scale=1.0):
        if self.backend == "hip":
            adam_step(self.params, grads, self.m, self.v, self.state, self.eps, grad_scale)
            return
        step = float(self.state[0]) + 1.0
        lr, b1, b2 = float(self.state[1]), float(self.state[2]), float(self.state[3])
        g = grads * grad_scale
        self.m.mul_(b1).add_(g, alpha=1 - b1)
        self.v.mul_(b2).addcmul_(g, g, value=1 - b2)
        bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
        denom = self.v.sqrt() / (bc2 ** 0.5) + self.eps
        self.params.addcdiv_(self.m, denom, value=-lr / bc1)
        self.state[0] = step

    def state_dict(self):
        return dict(m=self.m.clone(), v=self.v.clone(), state=self.state.clone())

    def load_state_dict(self, sd):
        self.m.copy_(sd["m"])
        self.v.copy_(sd["v"])
        self.state.copy_(sd["state"])


def lr_schedule_args(lr_schedule):
    """(warmup W, total T, min_ratio r) of the yaml block / keyword `lr_schedule`: None (the constant rate) or a mapping
    with any of the keys warmup, total, min_ratio.  ValueError for anything else or an unknown key (the values are checked by
    `check_optim_options`)."""
    if lr_schedule is None:
        return 0, 0, 0.0
    if not hasattr(lr_schedule, "items"):
        raise ValueError(f"lr_schedule: a mapping {{warmup, total, min_ratio}} or None, got {lr_schedule!r}")
    unknown = sorted(set(lr_schedule) - {"warmup", "total", "min_ratio"})
    if unknown:
        raise ValueError(f"lr_schedule: unknown key(s) {unknown} (known: warmup, total, min_ratio)")
    return lr_schedule.get("warmup", 0), lr_schedule.get("total", 0), lr_schedule.get("min_ratio", 0.0)


def _number(name, v, integral=False):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
        raise ValueError(f"{name}: a finite number, got {v!r}")
    if integral and float(v) != int(v):
        raise ValueError(f"{name}: a whole number of steps, got {v!r}")
    return float(v)


def check_optim_options(weight_decay=0.0, clip_norm=0.0, warmup_steps=0, total_steps=0, lr_min_ratio=0.0):
    """The five numbers as floats, or ValueError: weight_decay >= 0, clip_norm >= 0, whole W >= 0 and T >= 0, 0 <= r <= 1.
    (W, T and r live in the device state, which mllp_optim_step cannot check: this is where they are checked.)"""
    wd, clip = _number("weight_decay", weight_decay), _number("clip_norm", clip_norm)
    W, T = _number("warmup_steps", warmup_steps, True), _number("total_steps", total_steps, True)
    r = _number("lr_min_ratio", lr_min_ratio)
    if wd < 0 or clip < 0:
        raise ValueError(f"weight_decay and clip_norm must not be negative, got {weight_decay!r}, {clip_norm!r}")
    if W < 0 or T < 0:
        raise ValueError(f"warmup_steps and total_steps must not be negative, got {warmup_steps!r}, {total_steps!r}")
    if W >= 1 << 24 or T >= 1 << 24:
        raise ValueError("warmup_steps and total_steps: the step counter is a float, whole numbers end at 2^24")
    if not 0.0 <= r <= 1.0:
        raise ValueError(f"lr_min_ratio must lie in [0, 1], got {lr_min_ratio!r}")
    return wd, clip, W, T, r


class FlatAdamW:
    """torch.optim.AdamW + clip_grad_norm_(clip_norm) + a warm-up / cosine LambdaLR on flat buffers, every decision on the
    device (mllp_optim_step; include/mllp_hip.h states the rule): the rate of step t is lr * t / W up to step W, then
    lr * (r + (1 - r) (1 + cos(pi (t - W) / (T - W))) / 2) down to r * lr at step T and constant after it; W = T = 0 is the
    constant rate.  A step whose gradient norm is not finite is skipped (nothing moves, info[3] = 1).  Elements whose
    gradient is 0 with zero moments are not touched, and not decayed either (a parameter without a gradient).

    `backend='hip'` uses mllp_optim_step, `backend='torch'` is the same arithmetic in torch ops (the CPU tests and the gloo
    driver).  `info` = float tensor [4] {gradient norm, clip coefficient, rate, skipped} of the last step, on the
    parameters' device.  With everything at its default the parameters get FlatAdam's bits."""

    def __init__(self, params: torch.Tensor, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, clip_norm=0.0,
                 warmup_steps=0, total_steps=0, lr_min_ratio=0.0, backend="hip"):
        wd, clip, W, T, r = check_optim_options(weight_decay, clip_norm, warmup_steps, total_steps, lr_min_ratio)
        self.params = params
        self.m = torch.zeros_like(params)
        self.v = torch.zeros_like(params)
        self.eps = eps
        self.weight_decay, self.clip_norm = wd, clip
        self.backend = backend
        self.state = torch.tensor([0.0, lr, betas[0], betas[1], W, T, r, 0.0], dtype=torch.float32, device=params.device)
        self.info = torch.zeros(4, dtype=torch.float32, device=params.device)
        self.scratch = None
        if backend == "hip":
            n_scratch = optim_scratch_floats(params.numel())
            if n_scratch:
                self.scratch = torch.empty(n_scratch, dtype=torch.float32, device=params.device)

    def step(self, grads, grad_scale=1.0):
        if self.backend == "hip":
            optim_step(self.params, grads, self.m, self.v, self.state, self.eps, grad_scale, self.weight_decay,
                       self.clip_norm, self.scratch, self.info)
            return
        f = np.float32
        step, lr0, b1, b2, W, T, r, _ = (f(x) for x in self.state.tolist())
        t = step + f(1)
        if W > 0 and t <= W:
            lr = lr0 * t / W
        elif T > W:
            x = min(f(1), (t - W) / (T - W))
            lr = lr0 * (r + (f(1) - r) * (f(0.5) * (f(1) + np.cos(f(np.pi) * x, dtype=f))))
        else:
            lr = lr0
        g = grads * float(f(grad_scale))
        norm = f(float(g.square().sum().sqrt()))
        if not np.isfinite(norm):
            self.info.copy_(torch.tensor([float(norm), 0.0, float(lr), 1.0]))
            return
        c = min(f(1), f(self.clip_norm) / (norm + f(1e-6))) if self.clip_norm > 0 else f(1)
        live = (g != 0) | (self.m != 0) | (self.v != 0)
        g = g * float(c)
        p = self.params - float(lr * f(self.weight_decay)) * self.params
        m = self.m * float(b1) + g * float(f(1) - b1)
        v = self.v * float(b2) + g * g * float(f(1) - b2)
        bc1, bc2 = f(1) - np.power(b1, t, dtype=f), f(1) - np.power(b2, t, dtype=f)
        denom = v.sqrt() * float(f(1) / np.sqrt(bc2)) + float(f(self.eps))
        p = p - float(lr / bc1) * (m / denom)
        self.params.copy_(torch.where(live, p, self.params))
        self.m.copy_(torch.where(live, m, self.m))
        self.v.copy_(torch.where(live, v, self.v))
        self.state[0] = float(t)
        self.info.copy_(torch.tensor([float(norm), float(c), float(lr), 0.0]))

    def state_dict(self):
        return dict(m=self.m.clone(), v=self.v.clone(), state=self.state.clone())

    def load_state_dict(self, sd):
        """An 8-word state continues its own schedule; the 4-word state of a FlatAdam checkpoint continues its step count,
        rate and betas under the schedule this optimizer was built with."""
        st = sd["state"]
        if st.numel() not in (4, 8):
            raise ValueError(f"optimizer state: 4 or 8 words, got {st.numel()}")
        self.m.copy_(sd["m"])
        self.v.copy_(sd["v"])
        self.state[:st.numel()].copy_(st)


def make_optimizer(params, lr, weight_decay=0.0, clip_norm=0.0, lr_schedule=None, backend="hip"):
    """FlatAdam with nothing set (every call is the one it was), else a FlatAdamW"""
    if not weight_decay and not clip_norm and lr_schedule is None:
        return FlatAdam(params, lr=lr, backend=backend)
    W, T, r = lr_schedule_args(lr_schedule)
    return FlatAdamW(params, lr=lr, weight_decay=weight_decay, clip_norm=clip_norm, warmup_steps=W, total_steps=T,
                     lr_min_ratio=r, backend=backend)


def allreduce_sum_(t: torch.Tensor):
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and (
            dist.get_world_size() > 1 or os.environ.get("MLLP_BENCH_FORCE_DIST") == "1"):
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return t


class DataParallelStep:
    """grad function -> all-reduce -> identical Adam on every rank.  `grad_fn(params) -> (loss, grads)`
    must already scale by 1 / global instance count."""

    def __init__(self, params, grad_fn: Callable, lr=1e-3, adam_backend="hip"):
        self.params = params
        self.grad_fn = grad_fn
        self.opt = FlatAdam(params, lr=lr, backend=adam_backend)

    def step(self):
        loss, grads = self.grad_fn(self.params)
        allreduce_sum_(grads)
        allreduce_sum_(loss)
        self.opt.step(grads)
        return loss


class LPTrainer:
    """HIP fast path: one `mllp_gnn_loss_step` + all-reduce + `mllp_adam_step` per batch, launched eagerly on one
    stream (the latency-regime step of the Netlib batch is 13 back-to-back launches), optionally captured in hipGraphs."""

    # "auto": capture batches up to this many nonzeros.  0 = never: the fused step's launches already run back to back,
    # a single-stream capture replays within 1.5 % of eager (0.4755 vs 0.4687 ms), and the
    # per-instance loop is slower replayed (6.0 k vs 7.6 k instances/s).  `use_hip_graph=True` still forces capture.
    GRAPH_NNZ_LIMIT = 0

    # "auto": batches of at least this many nonzeros get the re-blocked copies of the attention sweeps, both orientations
    # (the throughput regime of the library's row tiers starts at the same size): the STREAMED copies for the 16-channel
    # sweeps and the lane-per-row copies for the 1-channel sweeps of layer 1 (round 4, LPBatch.enable_stream_step); with
    # `stream_copies=False` all sweeps run on LDS-tiled copies (round 2-3, LPBatch.enable_tiled_step); smaller batches run
    # the fused latency-regime kernels
    TILED_NNZ_MIN = 32 << 20

    def __init__(self, params_flat: torch.Tensor, lr=1e-3, use_hip_graph="auto",
                 global_instances: Optional[int] = None, with_metrics=False, tiled_copies="auto", stream_copies=True,
                 pos_weight=None, loss_head="bce", topm_tau=1.0, topm_sigma=0.0, topm_samples=0,
                 weight_decay=0.0, clip_norm=0.0, lr_schedule=None):
        assert params_flat.is_cuda and params_flat.numel() == NUM_PARAMS
        if loss_head not in ("bce", "topm"):
            raise ValueError(f"loss_head: 'bce' or 'topm', got {loss_head!r}")
        self.params = params_flat.detach().clone().float().contiguous()
        # weight_decay, clip_norm, lr_schedule {warmup, total, min_ratio}: with any of them set the optimizer is a FlatAdamW
        # (mllp_optim_step) and `step` takes the loss step -> all-reduce -> optimizer route, never the whole step, whose fused
        # tail contains plain Adam.  With none of them every call is the one it was
        self.opt = make_optimizer(self.params, lr, weight_decay, clip_norm, lr_schedule)
        self.split_opt = isinstance(self.opt, FlatAdamW)
        self.use_graph = use_hip_graph
        self.global_instances = global_instances
        self.with_metrics = with_metrics
        self.tiled_copies = tiled_copies
        self.stream_copies = stream_copies
        # None: the unweighted loss of mllp_gnn_train_step / mllp_gnn_loss_step.  A float, a tensor [n_inst] or 'balanced':
        # BCEWithLogitsLoss(pos_weight) through LPBatch.loss_step_weighted, per-instance losses in `inst_loss_of`
        self.pos_weight = pos_weight
        # 'bce': the heads above.  'topm': the soft top-m head through LPBatch.loss_step_topm (probabilities that sum to
        # m_k; topm_samples = 0 without noise, S >= 1 the mean of S evaluations with Gumbel noise of scale topm_sigma).  The
        # noise of a step is seeded by `topm_step`, the number of steps taken so far: a checkpoint keeps it
        self.loss_head = loss_head
        self.topm = dict(tau=float(topm_tau), sigma=float(topm_sigma), n_samples=int(topm_samples))
        self.topm_step = 0
        self._plans = {}
        self._gen = 0                  # bumped at every library-side write of the parameters (LPBatch.train_step)

    def _plan(self, batch: LPBatch):
        key = batch.token          # unique per LPBatch for the life of the process (id() can be reused after a free)
        p = self._plans.get(key)
        if p is None:
            dev = self.params.device
            graph = (batch.nnz <= self.GRAPH_NNZ_LIMIT) if self.use_graph == "auto" else bool(self.use_graph)
            if self.loss_head == "topm" and self.topm["n_samples"] > 0:
                graph = False          # (the seed is an argument by value and changes every step: a replay would repeat the noise)
            want_tiled = (batch.nnz >= self.TILED_NNZ_MIN) if self.tiled_copies == "auto" else bool(self.tiled_copies)
            if want_tiled and self.stream_copies:
                if not batch._streams:
                    batch._streams = batch.enable_stream_step()
            elif want_tiled and not batch._tiled:
                batch.enable_tiled_step()
            p = dict(batch=batch, logits=torch.empty(batch.N, device=dev), loss=torch.zeros(1, device=dev),
                     grads=torch.zeros(NUM_PARAMS, device=dev), metrics=torch.zeros(batch.n_inst, 2, device=dev),
                     g_fwd=None, g_opt=None, warm=0, graph=graph)
            if self.pos_weight is not None or self.loss_head == "topm":
                p["inst_loss"] = torch.zeros(max(batch.n_inst, 1), device=dev)[:batch.n_inst]
            self._plans[key] = p
        return p

    def inst_loss_of(self, batch: LPBatch) -> torch.Tensor:
        """[n_inst] per-instance losses L_k of the last step on `batch` (trainers with a pos_weight); device tensor."""
        return self._plans[batch.token]["inst_loss"]

    def evaluate(self, batch: LPBatch):
        """`LPBatch.evaluate` under this trainer's parameters and pos_weight: dict(logits, inst_loss, metrics).  No
        gradient, no optimizer step, no sync; parameters and Adam state are not touched."""
        if self.loss_head == "topm":       # the noise-free head, whatever the training samples
            logits = batch.forward(self.params)
            inst = batch.topm_loss(logits, self.topm["tau"], pos_weight=self.pos_weight, want="inst_loss")["inst_loss"]
            return dict(logits=logits, inst_loss=inst, metrics=batch.topm_metrics(logits))
        return batch.evaluate(self.params, self.pos_weight)

    def metrics_of(self, batch: LPBatch) -> torch.Tensor:
        """[n_inst, 2] (correct_num, f1) of the last step on `batch` (with_metrics=True); device tensor."""
        return self._plans[batch.token]["metrics"]

    def last_loss(self, batch: LPBatch) -> torch.Tensor:
        return self._plans[batch.token]["loss"]

    def uses_graph(self, batch: LPBatch) -> bool:
        return bool(self._plans[batch.token]["graph"])

    def release(self, batch: LPBatch):
        """Drop the buffers (and the reference to the batch) kept for `batch`."""
        self._plans.pop(batch.token, None)

    def _whole_step(self, p):
        """single rank: forward + loss + backward + Adam in one library call (the tail of the fused path is one launch
        that leaves the folded weights of the NEXT step in the batch's workspace: valid for the next step when it is on
        the same batch and nobody else wrote the parameters -- this trainer owns them)"""
        b = p["batch"]
        inv = 1.0 / float(self.global_instances or b.n_inst)
        b.train_step(self.params, self.opt.m, self.opt.v, self.opt.state, self.opt.eps, inv, p["logits"], p["loss"],
                     p["grads"], param_gen=self._gen)
        self._gen += 1
        if self.with_metrics:
            b.topm_metrics(p["logits"], p["metrics"])

    def _fwd_bwd(self, p):
        b = p["batch"]
        inv = 1.0 / float(self.global_instances or b.n_inst)
        if self.loss_head == "topm":
            b.loss_step_topm(self.params, self.topm["tau"], self.topm["sigma"], self.topm["n_samples"], self.topm_step, inv,
                             self.pos_weight, p["logits"], p["loss"], p["inst_loss"], p["grads"])
            self.topm_step += 1
        elif self.pos_weight is not None:
            b.loss_step_weighted(self.params, inv, self.pos_weight, p["logits"], p["loss"], p["inst_loss"], p["grads"])
        else:
            b.loss_step(self.params, inv, p["logits"], p["loss"], p["grads"])
        if self.with_metrics:
            b.topm_metrics(p["logits"], p["metrics"])

    def _opt(self, p):
        self.opt.step(p["grads"])

    def step_empty(self):
        """A rank that owns no instance of the current batch: contribute a zero gradient and apply the same Adam."""
        if not hasattr(self, "_zero"):
            self._zero = torch.zeros(NUM_PARAMS, device=self.params.device)
        self._zero.zero_()
        allreduce_sum_(self._zero)
        self.opt.step(self._zero)
        self._gen += 1

    def step(self, batch: LPBatch):
        """One optimizer step on `batch`; returns (loss, logits) device tensors (valid until the next step)."""
        import torch.distributed as dist
        p = self._plan(batch)
        multi = dist.is_available() and dist.is_initialized() and (
            dist.get_world_size() > 1 or os.environ.get("MLLP_BENCH_FORCE_DIST") == "1")
        if not p["graph"] or p["warm"] < 1:
            if multi or self.pos_weight is not None or self.loss_head == "topm" or self.split_opt:      # (one rank: the all-reduce is a no-op)
                self._fwd_bwd(p)
                allreduce_sum_(p["grads"])
                self._opt(p)
                self._gen += 1
            else:
                self._whole_step(p)
            p["warm"] += 1
            return p["loss"], p["logits"]
        if p["g_fwd"] is None:
            torch.cuda.synchronize()
            if multi:
                p["g_fwd"], p["g_opt"] = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
                with torch.cuda.graph(p["g_fwd"]):
                    self._fwd_bwd(p)
                with torch.cuda.graph(p["g_opt"]):
                    self._opt(p)
            else:
                p["g_fwd"] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(p["g_fwd"]):
                    self._fwd_bwd(p)
                    self._opt(p)
            # capture does not execute: the captured step runs below
        self._gen += 1
        p["g_fwd"].replay()
        if multi:
            allreduce_sum_(p["grads"])
            p["g_opt"].replay()
        return p["loss"], p["logits"]
