"""Inference driver: trained weights + LP files in, predicted bases out, without labels.

    python linear_program_predict.py --cfg linear_program_netlib.yaml --model linear_program_netlib_gs-topk.pt \\
        --mps netlib_mps/ --out predictions/ [--labels dataset/netlib_mps_norm/]

The reference's training loop forms the prediction of an instance as a 0/1 vector (`pred[pred_indices] = 1`,
linear_program_experiment.py:146-148) only to score it against the label; its "testing" half was never finished.  This
is that half: every `.mps` file is read and normalised by the library (`mllp_amd.mps.read_mps(normalize=True)`), the
instances are grouped into block-diagonal batches of the yaml's `batch_size` (0 = all in one batch), and per batch the
model's forward and the device top-m selection (`mllp_topm_select`; m = the instance's constraints) run back to back,
followed by ONE copy to the host.  No gradient, optimizer state or autograd graph is made.

Written to --out:
  <name>_basis_pred.npy   int32 [n], 0/1: the format of the reference's `<name>_basis.npy` (name = the file's name)
  predictions.json        name -> {m, n, threshold, runner_up, margin}: the m-th largest logit, the largest logit left
                          out, and their difference (0 with equal bits = a tie, broken towards the lower index).  A value
                          that is not finite (runner_up = -inf when every column is selected) is written as the string
                          float() parses ("inf", "-inf", "nan").  With --labels (a directory of `<name>_basis.npy`),
                          also `correct` and `f1`, from `mllp_topm_metrics` for the sparse methods.
  <name>_basis_prob.npy   only with --prob (sparse methods): float32 [n], the soft basis p_i = sigmoid(z_i / topm_tau + nu)
                          whose sum is m (`LPBatch.topm_prob`; topm_tau from the yaml, 1 when absent)

Method (the yaml's first entry): 'gs-topk' / 'soft-topk' -> GNNModel; 'angleNet' -> AngleModel on the dense angle graph
of each instance (m = the rank of its Q factor, as in training); 'invariant' is not built.  There is no CPU path.
"""
import argparse
import json
import math
import os
import sys

import numpy as np

from .config import cfg_from_file

SPARSE_METHODS = ("gs-topk", "soft-topk")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="predict the optimal simplex basis of LP files with trained weights (MI355X build)")
    p.add_argument("--cfg", "--config", dest="cfg_file", required=True, help="the experiment's yaml (methods, device, batch_size)")
    p.add_argument("--model", required=True, help="state_dict saved by linear_program_experiment.py (linear_program_<data>_<method>.pt)")
    p.add_argument("--mps", required=True, nargs="+", help="a directory of .mps files, or .mps files")
    p.add_argument("--out", required=True, help="output directory")
    p.add_argument("--labels", default=None, help="directory of <name>_basis.npy: also report correct / f1")
    p.add_argument("--prob", action="store_true",
                   help="also write <name>_basis_prob.npy: the soft basis of the top-m head (sparse methods; yaml key topm_tau)")
    return p.parse_args(argv)


def mps_files(paths):
    """The .mps files named by --mps: every file of a directory (sorted), or the files themselves."""
    out = []
    for p in paths:
        if os.path.isdir(p):
            found = sorted(f for f in os.listdir(p) if f.lower().endswith(".mps"))
            if not found:
                raise FileNotFoundError(f"--mps {p}: no .mps files in this directory")
            out += [os.path.join(p, f) for f in found]
        elif os.path.isfile(p):
            out.append(p)
        else:
            raise FileNotFoundError(f"--mps {p}: no such file or directory")
    names = [os.path.basename(f) for f in out]
    if len(set(names)) != len(names):
        raise ValueError("--mps: two files with the same name would write the same output")
    return out


def load_labels(labels_dir, name, n):
    path = os.path.join(labels_dir, name + "_basis.npy")
    if not os.path.exists(path):
        raise FileNotFoundError(f"--labels: {path} not found")
    y = np.load(path).astype(np.int32).reshape(-1)
    if y.shape[0] != n:
        raise ValueError(f"{path}: {y.shape[0]} labels for {n} columns")
    return y


def _num(v):
    v = float(v)
    return v if math.isfinite(v) else repr(v)


def _record(m, n, thr, run, extra=None):
    with np.errstate(invalid="ignore"):
        rec = {"m": int(m), "n": int(n), "threshold": _num(thr), "runner_up": _num(run),
               "margin": _num(np.float32(thr) - np.float32(run))}
    rec.update(extra or {})
    return rec


def predict_sparse(model, instances, batch_size, have_labels, prob_tau=None):
    """[(instance, 0/1 int32 [n], record)] for the bipartite GNNModel, `batch_size` instances per block-diagonal batch.
    With `prob_tau` the tuples end in a fourth element, the soft basis float32 [n] at that temperature."""
    import torch
    from .graph import LPBatch
    bs = int(batch_size) if int(batch_size) > 0 else len(instances)
    flat = model.flat_parameters().detach().contiguous()
    out = []
    for i in range(0, len(instances), bs):
        grp = instances[i:i + bs]
        b = LPBatch.from_instances(grp)
        logits = b.forward(flat)
        pred = b.predict_basis(logits, ("mask", "stats"))
        parts = [pred.mask, pred.stats.reshape(-1).view(torch.uint8)]
        if have_labels:
            parts.append(b.topm_metrics(logits).reshape(-1).view(torch.uint8))
        if prob_tau is not None:
            parts.append(b.topm_prob(logits, prob_tau).view(torch.uint8))
        host = torch.cat(parts).cpu().numpy()                 # the batch's one copy back
        k = len(grp)
        mask = host[:b.N].astype(np.int32)
        stats = host[b.N:b.N + 8 * k].view(np.float32).reshape(k, 2)
        end = b.N + 8 * k + (8 * k if have_labels else 0)
        met = host[b.N + 8 * k:end].view(np.float32).reshape(k, 2) if have_labels else None
        prob = host[end:].view(np.float32) if prob_tau is not None else None
        off = np.concatenate([[0], np.cumsum(b.inst_n)])
        for j, inst in enumerate(grp):
            extra = {"correct": float(met[j, 0]), "f1": float(met[j, 1])} if have_labels else None
            row = (inst, mask[off[j]:off[j + 1]], _record(inst.m, inst.n, stats[j, 0], stats[j, 1], extra))
            out.append(row if prob is None else row + (prob[off[j]:off[j + 1]].copy(),))
    return out


def predict_angle(model, instances, device, have_labels):
    """The same for AngleModel: one dense angle graph per instance."""
    import torch
    from .angle import build_graph_from_Q_sets, dense_instance_tensors
    out = []
    for inst in instances:
        Q, coefs, basis = dense_instance_tensors(inst)
        g = build_graph_from_Q_sets(Q, coefs, device, inst.name, basis)
        pred = model.predict(g, ("mask", "stats"))
        parts = [pred.mask, pred.stats.reshape(-1).view(torch.uint8)]
        host = torch.cat(parts).cpu().numpy()
        n = g.var_num
        mask = host[:n].astype(np.int32)
        stats = host[n:n + 8].view(np.float32)
        extra = None
        if have_labels:     # sklearn's f1_score on 0/1 vectors, as train_angle reports it
            tp = float(mask @ np.asarray(basis, np.int32))
            extra = {"correct": tp, "f1": 2.0 * tp / max(float(mask.sum() + np.asarray(basis).sum()), 1.0)}
        out.append((inst, mask, _record(g.basis_num, n, stats[0], stats[1], extra)))
    return out


def main(argv=None):
    args = parse_args(argv)
    cfg = cfg_from_file(args.cfg_file)
    method = cfg.methods[0]
    if method == "invariant":
        raise NotImplementedError(
            "method 'invariant' is the reference's InvariantModel research path (reference "
            f"linear_program_methods.py:136-185), not built: use 'angleNet' or one of {SPARSE_METHODS}")
    if method not in SPARSE_METHODS + ("angleNet",):
        raise NotImplementedError(f"method {method!r} is outside this build (supported: {SPARSE_METHODS + ('angleNet',)})")
    if str(cfg.get_default("device")).split(":")[0] != "cuda":
        raise RuntimeError("this build runs the learned-LP path on MI355X through HIP only (device: 'cuda'); "
                           "there is no CPU fallback")
    if not os.path.isfile(args.model):
        raise FileNotFoundError(f"--model {args.model}: no such file")
    if args.prob and method not in SPARSE_METHODS:
        raise NotImplementedError(f"--prob: the soft basis is the top-m head's, for the sparse methods {SPARSE_METHODS} only")
    files = mps_files(args.mps)
    if args.labels is not None and not os.path.isdir(args.labels):
        raise FileNotFoundError(f"--labels {args.labels}: no such directory")
    import torch
    device = torch.device(cfg.get_default("device"))
    if not torch.cuda.is_available():
        raise RuntimeError("no HIP device: this build runs the learned-LP path on MI355X only; there is no CPU fallback")
    from .mps import read_mps
    instances = []
    for f in files:
        inst, _ = read_mps(f, normalize=True)
        inst.basis = (load_labels(args.labels, inst.name, inst.n) if args.labels is not None
                      else np.zeros(inst.n, np.int32))
        instances.append(inst)
    state = torch.load(args.model, map_location=device, weights_only=True)
    if method == "angleNet":
        from .angle import AngleModel
        model = AngleModel(feat_dim=int(cfg.get_default("angle_feat_dim"))).to(device)
        model.load_state_dict(state)
        results = predict_angle(model, instances, device, args.labels is not None)
    else:
        from .model import GNNModel
        model = GNNModel().to(device)
        model.load_state_dict(state)
        results = predict_sparse(model, instances, cfg.get_default("batch_size"), args.labels is not None,
                                 float(cfg.get_default("topm_tau")) if args.prob else None)
    os.makedirs(args.out, exist_ok=True)
    table = {}
    for inst, mask, rec, *prob in results:
        np.save(os.path.join(args.out, inst.name + "_basis_pred.npy"), mask)
        if prob:
            np.save(os.path.join(args.out, inst.name + "_basis_prob.npy"), prob[0])
        table[inst.name] = rec
    with open(os.path.join(args.out, "predictions.json"), "w") as fh:
        json.dump(table, fh, indent=1)
    print(f"{len(results)} predicted bases written to {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
