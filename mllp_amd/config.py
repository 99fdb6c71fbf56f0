"""Experiment configuration: `--cfg <yaml>` -> attribute-style nested dict.

Mirrors the surface of the reference's `config.py` (reference `config.py:6-25`):
`load_config()` parses `--cfg/--config`, raises ``ValueError('Please specify path
to the configuration file!')`` when absent, and returns the yaml merged into an
attribute dict.  The reference depends on `easydict`; this build carries its own
small `AttrDict` so nothing outside the standard library + pyyaml is needed.

Keys read on the hot path (reference `linear_program_netlib.yaml:1-15`):
``train_data_type, train_lr, train_iter, methods, verbose``.  Optional keys
added by this build (all default to reference behaviour when absent) are listed
in `HOT_PATH_DEFAULTS`.
"""
import argparse

import yaml

# optional keys this build understands; absent -> reference semantics
HOT_PATH_DEFAULTS = {
    "device": "cuda",        # the reference hard-wires cpu (experiment.py:18); the product path is HIP
    "batch_size": 1,         # instances per Adam step; 1 == reference (experiment.py:123-144); 0 == whole dataset
    "instances": None,       # optional list of instance names (e.g. ['afiro.mps', ...]); None == all
    "log_every": 1,          # print per-instance metrics every k epochs
    "save_every": 0,         # extra checkpoints every k epochs (0 == only at the end, as the reference)
    "resume": False,         # resume from linear_program_<data>_<method>.ckpt if present
    "tiled_copies": "auto",  # LDS-tiled copies of the batch for the large-batch kernels: True | False | 'auto' (>= 32 M nonzeros)
    "use_hip_graph": "auto", # capture the training step into a hipGraph: True | False | 'auto' (= False: eager launches measured faster)
    "angle_feat_dim": 256,   # feat_dim of AngleModel for the 'angleNet' method (the reference hard-codes 256, experiment.py:83)
    "dtype": "f32",          # feature precision of the training step.  'f32' is the reference's arithmetic and the only one the
                             # step implements; 'bf16' exists for the plain SpMM only (LPBatch.spmm_bf16 / mllp_spmm_csr_bf16)
    "pos_weight": None,      # weight of the positive labels in the loss: a float | 'balanced' (negatives / positives of each
                             # instance); None == the reference's unweighted BCEWithLogitsLoss (experiment.py:41)
    "loss_head": "bce",      # 'bce': the per-column BCEWithLogitsLoss above.  'topm': the soft top-m head (LPBatch.loss_step_topm):
                             # probabilities that sum to the instance's m.  Method 'soft-topk' then runs it without noise,
                             # 'gs-topk' with train_gumbel_sample_num Gumbel samples of scale gumbel_sigma per step
    "topm_tau": 1.0,         # temperature of the 'topm' head: p = sigmoid(z / topm_tau + nu) (= sinkhorn_tau / 2 of the reference)
    "holdout": None,         # instances evaluated every logging epoch and never trained on: a list of instance names, or a
                             # fraction f in (0, 1) (mllp_amd.experiment.holdout_by_fraction); None == train on everything
    "planted": None,         # with train_data_type: 'planted', the block {instances, m, n, row_nnz, seed} of the planted-basis
                             # LPs built on the device (mllp_amd.planted.PLANTED_DEFAULTS); None == those defaults
    "report_solved": None,   # the block {feas_tol, opt_tol, max_m}: every logging epoch the predicted ranking of the held-out
                             # instances (the trained ones without `holdout`) is repaired into a basis, solved and certified on
                             # the device, and train_log.json gains the counts usable / feasible / optimal / skipped (m > max_m;
                             # max_m absent == none skipped); None == not computed, the log as before
                             # `pivots: K` in the block adds optimal_after_pivots / pivots: the repaired prediction pivoted to
                             # the optimum with at most K simplex pivots per instance (LPBatch.simplex), and their total;
                             # `refactor: R` / `stall: S` beside it are that call's refactor_every / stall_pivots (a fresh
                             # factorization every R pivots, Bland's rule after S degenerate pivots); absent == the plain call
                             # `pdhg: {iters: K, eps: E}` in the block (optional `check`, default 64, and `warm`, default true)
                             # adds pdhg_converged / pdhg_iterations / optimal_after_pdhg: every instance solved by restarted
                             # PDHG (LPBatch.pdhg) from the repaired prediction's basic solution (warm) or from zeros, and the
                             # vertex its iterate points at certified (LPBatch.pdhg_basis + solved);  `scaled: true` inside
                             # `pdhg` solves by the preconditioned call instead (LPBatch.pdhg_scaled: Ruiz and Pock-Chambolle
                             # scaling, a clamped primal weight) under the same three keys, or `scaled: {ruiz: 10,
                             # pock_chambolle: true, weight: true, span: 16}` with any of its options; absent == LPBatch.pdhg;
                             # `halpern: true` (or `halpern: {reflect: false}`) inside `pdhg` solves by the preconditioned call
                             # with Halpern's iteration (LPBatch.pdhg_halpern), with the `scaled:` options if they are given;
                             # `wide: true` (or `wide: {rows: 64, poll: 256}`) inside `pdhg` runs that same rule, bit for bit,
                             # across the whole device (LPBatch.pdhg_wide: for instances too long for one workgroup), with the
                             # `halpern:` and `scaled:` options if they are given; `poll` reads the codes back every so many
                             # iterations and stops once every instance has; `rays: true` (or `rays: {eps: 1.e-3}`) inside
                             # `pdhg` runs the wide call with certificates (LPBatch.pdhg_rays; implies `wide`) and adds
                             # pdhg_infeasible / pdhg_unbounded: the instances that ended with code 4 and with code 5.  Both are
                             # relative to eps: code 4 says "no feasible point with a 1-norm below 1 / eps", which feasible LPs
                             # with large solutions meet too (at 2^-10: 46 of the 97 Netlib LPs), so choose eps against them;
                             # `spectral: true` (or `spectral: {iters: 40}`) inside `pdhg` runs the wide call with the step
                             # from power iteration on the device (LPBatch.pdhg_spectral; implies `wide`, combines with `rays`)
    "weight_decay": 0.0,     # decoupled weight decay of the optimizer (torch.optim.AdamW); 0 == the reference's Adam
    "clip_norm": 0.0,        # cap on the global gradient norm of a step (torch.nn.utils.clip_grad_norm_); 0 == no clipping
    "lr_schedule": None,     # the block {warmup: W, total: T, min_ratio: r}: the rate rises linearly over the first W steps, then
                             # falls along half a cosine to r * train_lr at step T and stays there; None == constant train_lr.
                             # With any of the three keys set the step runs mllp_optim_step (everything decided on the device),
                             # a step with a non-finite gradient norm is skipped, and train_log.json gains grad_norm and lr
}


class AttrDict(dict):
    """dict with attribute access; nested dicts are converted recursively."""

    def __init__(self, *args, **kwargs):
        super().__init__()
        for k, v in dict(*args, **kwargs).items():
            self[k] = v

    @staticmethod
    def _wrap(v):
        if isinstance(v, dict) and not isinstance(v, AttrDict):
            return AttrDict(v)
        if isinstance(v, (list, tuple)):
            return type(v)(AttrDict._wrap(x) for x in v)
        return v

    def __setitem__(self, k, v):
        super().__setitem__(k, AttrDict._wrap(v))

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            # a missing key is an AttributeError at use, as with easydict
            raise AttributeError(k) from None

    def __setattr__(self, k, v):
        self[k] = v

    def get_default(self, k):
        """Value of an optional build key, falling back to HOT_PATH_DEFAULTS."""
        return self[k] if k in self else HOT_PATH_DEFAULTS[k]


def _merge_a_into_b(a, b, strict=False):
    """Merge mapping `a` into `b`, overwriting `b`'s entries (reference config.py:28-57).

    With ``strict`` every key of `a` must already exist in `b` with the same type
    (int -> float promotion allowed).
    """
    if not isinstance(a, AttrDict):
        return
    for key, val in a.items():
        if strict:
            if key not in b:
                raise KeyError("{} is not a valid config key".format(key))
            want, got = type(b[key]), type(val)
            if want is not got:
                if want is float and got is int:
                    val = float(val)
                elif key not in ("CLASS",):
                    raise ValueError("Type mismatch ({} vs. {}) for config key: {}".format(want, got, key))
        if isinstance(val, AttrDict) and isinstance(b.get(key), AttrDict):
            try:
                _merge_a_into_b(val, b[key], strict)
            except Exception:
                print("Error under config key: {}".format(key))
                raise
        else:
            b[key] = val


def cfg_from_file(filename, cfg=None):
    """Load a yaml file and merge it into `cfg` (a fresh AttrDict when None)."""
    with open(filename, "r") as fh:
        loaded = AttrDict(yaml.safe_load(fh) or {})
    if cfg is None:
        cfg = AttrDict()
    _merge_a_into_b(loaded, cfg)
    return cfg


def load_config(argv=None):
    parser = argparse.ArgumentParser(description="mllp learned-LP experiment protocol (MI355X build).")
    parser.add_argument("--cfg", "--config", dest="cfg_file", default=None, type=str,
                        help="path to the configuration file")
    args, _unknown = parser.parse_known_args(argv)
    if args.cfg_file is None:
        raise ValueError("Please specify path to the configuration file!")
    return cfg_from_file(args.cfg_file)
