"""CPU: the held-out split of the experiment driver (yaml keys `holdout`, `pos_weight`; mllp_amd.experiment.
holdout_by_fraction, split_holdout, plan_split_batches, run_epochs(holdout=..., n_holdout=...)) with fake trainers."""
import json
import math
from types import SimpleNamespace

import pytest
import torch

from mllp_amd.config import HOT_PATH_DEFAULTS, AttrDict
from mllp_amd.experiment import holdout_by_fraction, plan_batches, plan_split_batches, run_epochs, split_holdout


def test_fraction_rule_counts_determinism_and_limits():
    for n in (0, 1, 5, 10, 97):
        for f in (0.1, 0.2, 0.25, 1.0 / 3.0, 0.5, 0.9):
            held = holdout_by_fraction(n, f)
            assert held == [i for i in range(n) if math.floor((i + 1) * f) > math.floor(i * f)]
            assert len(held) == math.floor(n * f) and held == sorted(set(held))
            assert held == holdout_by_fraction(n, f)                       # a pure function
            if held:
                assert 0 <= held[0] and held[-1] < n
    assert holdout_by_fraction(10, 0.2) == [4, 9]
    assert holdout_by_fraction(97, 1e-9) == []                             # f -> 0: nobody
    assert holdout_by_fraction(97, 1.0 - 1e-9) == list(range(1, 97))       # f -> 1: everybody but the first
    for bad in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            holdout_by_fraction(10, bad)


def test_split_by_names_and_by_fraction():
    names = [f"lp{i}.mps" for i in range(10)]
    assert split_holdout(names, None) == (list(range(10)), [])
    assert split_holdout(names, []) == (list(range(10)), [])
    train, held = split_holdout(names, ["lp7.mps", "lp2.mps"])
    assert held == [2, 7] and train == [0, 1, 3, 4, 5, 6, 8, 9]
    train, held = split_holdout(names, 0.2)
    assert held == [4, 9] and sorted(train + held) == list(range(10))
    with pytest.raises(ValueError, match="nosuch.mps"):
        split_holdout(names, ["lp1.mps", "nosuch.mps"])
    with pytest.raises(ValueError):
        split_holdout(names, "lp1.mps")
    assert HOT_PATH_DEFAULTS["holdout"] is None and HOT_PATH_DEFAULTS["pos_weight"] is None
    assert AttrDict(train_iter=1).get_default("holdout") is None


class Batch:
    def __init__(self, ids):
        self.ids = list(ids)
        self.n_inst = len(self.ids)


class PlainTrainer:
    """LPTrainer's driver-facing surface without `evaluate`; instance i has loss 0.5 + i and correct count 10 i"""

    def __init__(self):
        self.global_instances = None
        self.stepped = []

    def step(self, batch):
        self.stepped.append(batch)
        return torch.tensor([sum(0.5 + i for i in batch.ids) / self.global_instances]), None

    def step_empty(self):
        pass

    def metrics_of(self, batch):
        return torch.tensor([[10.0 * i, 0.5] for i in batch.ids])


class EvalTrainer(PlainTrainer):
    def __init__(self):
        super().__init__()
        self.evaluated = []

    def evaluate(self, batch):
        self.evaluated.append(batch)
        return dict(logits=None, inst_loss=torch.tensor([100.0 + i for i in batch.ids]),
                    metrics=torch.tensor([[10.0 * i + 1.0, 0.25] for i in batch.ids]))


def _dataset(n=7):
    inst = [SimpleNamespace(name=f"lp{i}.mps", m=3 + i, n=5 + i, nnz=10 + i) for i in range(n)]
    return inst, dict(obj=[], **{i.name: [] for i in inst})


def _run(tmp_path, monkeypatch, trainer, holdout, epochs=3, log_every=1):
    monkeypatch.chdir(tmp_path)
    inst, train_dict = _dataset()
    cfg = AttrDict(train_iter=epochs, log_every=log_every, save_every=0)
    train_ids, held_ids = split_holdout([i.name for i in inst], holdout)
    lines = []
    if not held_ids:
        batches = [(mine, Batch(mine), g) for mine, g in plan_batches(inst, 2, 0, 1)]
        run_epochs(cfg, inst, train_dict, trainer, batches, 0, 1, torch.device("cpu"), 0, lines.append)
    else:
        batches = [(mine, Batch(mine), g) for mine, g in plan_split_batches(inst, train_ids, 2, 0, 1)]
        held = [(mine, Batch(mine)) for mine, _ in plan_split_batches(inst, held_ids, 2, 0, 1)]
        run_epochs(cfg, inst, train_dict, trainer, batches, 0, 1, torch.device("cpu"), 0, lines.append,
                   holdout=held, n_holdout=len(held_ids))
    return inst, train_dict, lines, json.load(open(tmp_path / "train_log.json")), train_ids, held_ids


def test_without_the_keys_the_log_is_todays(tmp_path, monkeypatch):
    tr = PlainTrainer()                        # a trainer without `evaluate` keeps working
    inst, train_dict, lines, log, train_ids, held_ids = _run(tmp_path, monkeypatch, tr, None, epochs=2)
    assert held_ids == [] and train_ids == list(range(7))
    assert set(log) == {"obj"} | {i.name for i in inst} and log == train_dict
    assert "val_obj" not in log
    obj = sum(0.5 + i for i in range(7)) / 7
    assert log["obj"] == pytest.approx([obj, obj]) and all(log[f"lp{i}.mps"] == [10.0 * i] * 2 for i in range(7))
    assert [b.ids for b in tr.stepped] == [[0, 1], [2, 3], [4, 5], [6]] * 2
    epoch_lines = [x for x in lines if x.startswith("epoch")]
    assert len(epoch_lines) == 2 and all(", obj=" in x and "val_obj" not in x for x in epoch_lines)
    assert len(lines) == 2 * (7 + 1)


def test_held_out_instances_are_evaluated_logged_and_never_stepped(tmp_path, monkeypatch):
    tr = EvalTrainer()
    holdout = ["lp1.mps", "lp4.mps", "lp5.mps"]
    inst, train_dict, lines, log, train_ids, held_ids = _run(tmp_path, monkeypatch, tr, holdout, epochs=3)
    assert held_ids == [1, 4, 5] and train_ids == [0, 2, 3, 6]
    # trained batches hold trained instances only, in groups of batch_size; held-out ones have batches of their own
    assert [b.ids for b in tr.stepped] == [[0, 2], [3, 6]] * 3
    assert [b.ids for b in tr.evaluated] == [[1, 4], [5]] * 3
    assert not {id(b) for b in tr.stepped} & {id(b) for b in tr.evaluated}
    assert set(log) == {"obj", "val_obj"} | {i.name for i in inst} and log == train_dict
    obj = sum(0.5 + i for i in train_ids) / len(train_ids)                 # the mean over TRAINED instances
    val = sum(100.0 + i for i in held_ids) / len(held_ids)
    assert log["obj"] == pytest.approx([obj] * 3) and log["val_obj"] == pytest.approx([val] * 3)
    for i in range(7):
        assert log[f"lp{i}.mps"] == [10.0 * i + (1.0 if i in held_ids else 0.0)] * 3
    epoch_lines = [x for x in lines if x.startswith("epoch")]
    assert len(epoch_lines) == 3 and all(", obj=" in x and ", val_obj=" in x for x in epoch_lines)
    assert len(lines) == 3 * (7 + 1)                                       # every instance prints its row, in dataset order


def test_held_out_instances_are_evaluated_on_logging_epochs_only(tmp_path, monkeypatch):
    tr = EvalTrainer()
    _, _, lines, log, _, _ = _run(tmp_path, monkeypatch, tr, 0.3, epochs=4, log_every=2)
    assert [b.ids for b in tr.evaluated] == [[3, 6]] * 2                   # floor(7 * 0.3) = 2 instances, epochs 0 and 2
    assert len(log["val_obj"]) == 2 and len(log["obj"]) == 4 and len(log["lp3.mps"]) == 2
    assert sum("val_obj" in x for x in lines) == 2


def test_a_trainer_without_evaluate_is_refused_with_a_holdout(tmp_path, monkeypatch):
    with pytest.raises(ValueError, match="evaluate"):
        _run(tmp_path, monkeypatch, PlainTrainer(), ["lp2.mps"])


@pytest.mark.gpu
def test_driver_with_holdout_and_pos_weight_end_to_end(tmp_path, monkeypatch):
    """`linear_program_experiment.py --cfg <yaml>` with `holdout` and `pos_weight`: the log gains `val_obj` and the
    held-out instance's correct counts, and the held-out instance does not touch the training -- the run without it in
    the dataset ends with the same weights, bit for bit, and the same `obj`."""
    from mllp_amd import experiment
    names = ["afiro.mps", "sc50a.mps", "kb2.mps"]
    head = "train_data_type: 'netlib'\ntrain_lr: 1.e-3\ntrain_iter: 2\nmethods:\n  - 'gs-topk'\nbatch_size: 2\npos_weight: 'balanced'\n"
    runs = {}
    for tag, extra in (("held", f"instances: {names}\nholdout: ['sc50a.mps']\n"),
                       ("without", f"instances: {[n for n in names if n != 'sc50a.mps']}\n")):
        d = tmp_path / tag
        d.mkdir()
        (d / "cfg.yaml").write_text(head + extra)
        monkeypatch.chdir(d)
        assert experiment.main(["--cfg", str(d / "cfg.yaml")]) == 0
        sd = torch.load(d / "linear_program_netlib_gs-topk.pt", weights_only=True)
        runs[tag] = (json.load(open(d / "train_log.json")), torch.cat([v.reshape(-1) for v in sd.values()]).cpu())
    log, flat = runs["held"]
    assert set(log) == {"obj", "val_obj"} | set(names) and all(len(v) == 2 for v in log.values())
    assert all(math.isfinite(v) and v > 0.0 for v in log["val_obj"]) and log["val_obj"][0] != log["val_obj"][1]
    assert all(0 <= c <= 50 for c in log["sc50a.mps"])                    # sc50a has 50 constraints
    log0, flat0 = runs["without"]
    assert "val_obj" not in log0 and log0["obj"] == log["obj"]
    assert all(log0[n] == log[n] for n in names if n != "sc50a.mps")
    assert torch.equal(flat, flat0)
