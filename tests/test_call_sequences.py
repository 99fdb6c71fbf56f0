"""Call sequences on one resident batch against a stateless replay (include/mllp_hip.h, RECORDS).

The library keeps, per graph, a record of the forward whose activations the workspace holds and a record of the folded
weights a fused train step left behind.  tests/call_model.py states what those records must do as a pure-Python model
over an alphabet of 16 operations, and a fixed walk -- the order-3 de Bruijn sequence over the alphabet, every triple of
operations once, cut into segments that each start from the start state on a batch of their own.

CPU: the model itself, the walk's coverage, and the conditions the walk must meet to be worth running.

GPU: every call of the walk on a resident batch through the C ABI.  The library's accept / refuse must be the model's.  After
every accepted call every output is compared BIT FOR BIT with a replay that carries nothing: a newly built batch from the
instances with the current values, a new handle, a new NaN-filled workspace, the current path, copies of the current
parameter and optimizer bytes, and the call alone (after a forward, for the backward calls).  Equality is the bar because
the header promises that results do not depend on what the workspace held and are reproducible bit for bit.  After every
refused call: MLLP_EINVAL, a message, every output still its sentinel, workspace, parameters and optimizer state untouched.
The replay itself is compared once per case and path with the fp64 oracle, at the bars of the files that own them
(through tests/test_memory_contract.py's anchors: nothing is restated), so the chain of equalities ends in a high-precision
reference.
"""
import dataclasses
import hashlib

import numpy as np
import pytest
import torch

import call_model as cm
import test_memory_contract as mc
from call_model import ACCEPT, REFUSE, SKIP, START, State
from mllp_amd import _lib

gpu = pytest.mark.gpu
EINVAL = -1
WALK_CASES = ("holes", "one")


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the model and the walk
# ---------------------------------------------------------------------------------------------------------------------
def test_alphabet_is_the_sixteen_operations_in_the_walks_order():
    assert cm.OPS == ("SA", "LI", "P2", "S", "SW", "IG", "F", "T1", "V", "BI", "X", "LW", "P1", "B", "L", "T0")
    assert set(cm.CALLS) == set(cm.OPS) and len(set(cm.OPS)) == 16
    assert START == State(2, "A", None, None)


def test_de_bruijn_walk_covers_every_triple_once():
    seq = cm.de_bruijn(16, 3)
    assert len(seq) == 16 ** 3 and seq[:9] == [0, 0, 0, 1, 0, 0, 2, 0, 0]        # Lyndon words, smallest symbol first
    w = cm.walk()
    assert len(w) == 16 ** 3 + 2
    windows = [tuple(w[i:i + 3]) for i in range(len(w) - 2)]
    assert len(windows) == 16 ** 3 == len(set(windows))
    assert set(windows) == {(a, b, c) for a in cm.OPS for b in cm.OPS for c in cm.OPS}
    for k, small in ((2, 3), (3, 2), (4, 1)):                                     # the construction, at other sizes
        s = cm.de_bruijn(k, small)
        cyc = s + s[:small - 1]
        assert len({tuple(cyc[i:i + small]) for i in range(len(s))}) == k ** small == len(s)


def test_segments_lose_no_window_at_a_cut():
    segs = cm.segments()
    assert len(segs) == cm.SEGMENTS and all(len(s) == 4096 // cm.SEGMENTS + 2 for s in segs)
    assert sum(len(s) for s in segs) == 4096 + 2 * cm.SEGMENTS
    windows = {tuple(s[i:i + 3]) for s in segs for i in range(len(s) - 2)}
    assert len(windows) == 16 ** 3
    assert [op for s in segs for op in s[:-2]] + segs[-1][-2:] == cm.walk()


def test_walk_conditions():
    """Conditions on what the walk exercises, by the model alone -- not measurements.  A change of the model that breaks
    one is answered by another alphabet order, not by another threshold."""
    c = cm.census()
    assert c["calls"] == 4096 + 2 * cm.SEGMENTS
    assert c["refused"] <= 0.20 * c["calls"]
    for op in cm.BACKWARD_OPS:
        assert c["accepted"][op] >= 40 and c["refused_by_op"][op] >= 40, (op, c)
    assert c["x_issued"] >= 40 and c["x_skipped"] >= 1
    if cm.SEGMENTS == 16:       # the census of this alphabet order and cut, as the model gave it when the walk was fixed
        assert (c["refused"], c["accepted"], c["refused_by_op"], c["x_issued"], c["x_skipped"], c["max_adam_steps"]) == \
            (558, {"B": 88, "BI": 56, "IG": 73}, {"B": 170, "BI": 201, "IG": 187}, 165, 91, 113)


def _verdicts(ops, state=START):
    return [v for _, v, _ in cm.run(ops, state)]


# the four sequences that were accepted before the records knew the parameters and the loss / train steps knew the records
WHY = {
    "wrong_path": ("P1", "F", "P2", "L", "P1", "B"),
    "train_step_fused": ("F", "T0", "B"),
    "train_step_generic": ("P1", "F", "T0", "B"),
    "loss_step_other_params": ("F", "SW", "L", "SW", "IG"),
    "backward_other_params": ("F", "SW", "B"),
}


@pytest.mark.parametrize("name", list(WHY))
def test_model_refuses_the_stale_sequences(name):
    v = _verdicts(WHY[name])
    assert v[-1] == REFUSE and all(x == ACCEPT for x in v[:-1]), v


def test_model_accepts_what_carries_a_valid_forward():
    assert _verdicts(("F", "L", "IG")) == [ACCEPT] * 3                      # one parameter tensor, the fused path
    assert _verdicts(("F", "LI", "B", "B", "IG")) == [ACCEPT] * 5
    assert _verdicts(("F", "P1", "P2", "B")) == [ACCEPT] * 4                 # nothing wrote the workspace in between
    assert _verdicts(("F", "P1", "B"))[-1] == REFUSE
    assert _verdicts(("LW", "IG", "BI")) == [ACCEPT, ACCEPT, REFUSE]        # BI is the generic path's call
    assert _verdicts(("P1", "LW", "BI", "V", "BI")) == [ACCEPT] * 4 + [REFUSE]
    assert _verdicts(("F", "S", "B"))[-1] == REFUSE and _verdicts(("F", "SA", "B"))[-1] == REFUSE
    assert _verdicts(("F", "SW", "SW", "B"))[-1] == ACCEPT


def test_model_clobbers_only_where_nothing_is_carried():
    assert _verdicts(("X", "F", "X", "L", "X")) == [ACCEPT, ACCEPT, SKIP, ACCEPT, SKIP]
    assert _verdicts(("F", "SW", "L", "X")) == [ACCEPT] * 4                 # a loss step with other parameters forgets
    assert _verdicts(("T0", "X", "V", "X", "P1", "X")) == [ACCEPT, SKIP, ACCEPT, SKIP, ACCEPT, ACCEPT]
    assert _verdicts(("P1", "T0", "X")) == [ACCEPT] * 3                     # the generic train step folds nothing ahead
    s = cm.run(("T0", "SW", "T1"))[-1][2]
    assert s.folded == "B" and s.rec is None


# ---------------------------------------------------------------------------------------------------------------------
# GPU: one batch with everything the calls need, driven by operation name
# ---------------------------------------------------------------------------------------------------------------------
SENTINEL = -7.0e37
OUTPUTS = {
    "F": ("logits",), "B": ("grads",), "IG": ("grads", "dx1", "dx2", "dvalues"), "BI": ("grads", "dx1", "dx2", "dvalues"),
    "L": ("logits", "loss", "grads"), "LI": ("logits", "loss", "grads", "dx1", "dx2", "dvalues"),
    "LW": ("logits", "loss", "inst_loss", "grads", "dlogits_out"),
    "T0": ("logits", "loss", "grads"), "T1": ("logits", "loss", "grads"), "S": ("logits", "loss", "grads"),
    "SA": ("logits", "loss", "grads"),
}
WRITES_PARAMS = ("T0", "T1", "SA")
_VALUES, _REPLAYS = {}, {}


def _bits(t):
    return t.view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


def test_comparison_is_on_the_bits():
    nan = torch.tensor([float("nan"), 1.0])
    assert _same(nan, nan.clone()) and not _same(torch.tensor([0.0]), torch.tensor([-0.0]))
    assert not _same(torch.tensor([1.0]), torch.tensor([1.0 + 2.0 ** -23])) and not _same(nan, nan[:1])


def value_sets(case):
    """the two value sets of a case on one pattern, as fp32 in the CSR order of A: the instances' own, and those times a
    seeded factor in [0.9, 1.1] (the product is formed in fp32: both sets are exactly what the batch stores)"""
    if case not in _VALUES:
        v0 = np.concatenate([i.values for i in mc.case_instances(case)]).astype(np.float32)
        factor = np.random.default_rng(23).uniform(0.9, 1.1, v0.size).astype(np.float32)
        _VALUES[case] = (v0, (v0 * factor).astype(np.float32))
    return _VALUES[case]


def instances_with(case, vset):
    insts, vals, out, off = mc.case_instances(case), value_sets(case)[vset], [], 0
    for i in insts:
        out.append(dataclasses.replace(i, values=vals[off:off + i.nnz].astype(np.float64)))
        off += i.nnz
    return out


def parameter_sets():
    """A: the golden weights; B: those times a seeded factor in [0.9, 1.1]"""
    flat = mc._f32(mc._golden_flat())
    factor = np.random.default_rng(29).uniform(0.9, 1.1, flat.size).astype(np.float32)
    return {"A": flat, "B": (flat * factor).astype(np.float32)}


def fresh_adam():
    """exp_avg, exp_avg_sq, state {step, lr, beta1, beta2} as one host array"""
    return np.concatenate([np.zeros(2 * _lib.NUM_PARAMS, np.float32), mc._f32([0.0, 1e-3, 0.9, 0.999])])


class Machine:
    """One batch on the device in a given state, and the 16 operations on it.  `params`: {id: host array of the parameters
    followed by the optimizer buffers}; each id gets device buffers of its own."""

    def __init__(self, case, path, vset, params):
        from mllp_amd.graph import LPBatch
        self.case, self.ctx = case, mc.get_ctx(case, "generic")                 # (ctx: the case's dlogits and loss weights)
        self.b = LPBatch.from_instances(instances_with(case, vset))
        self.b.set_path(path)
        self.h, self.N, self.M, self.nnz, self.K = self.b._h, self.b.N, self.b.M, self.b.nnz, self.b.n_inst
        self.path, self.vset, self.cur = path, vset, sorted(params)[0]
        dev = lambda a: torch.tensor(a, dtype=torch.float32, device="cuda")  # noqa: E731
        n = _lib.NUM_PARAMS
        self.P, self.opt = {}, {}
        for k, host in params.items():
            assert host.size == 3 * n + 4
            self.P[k] = dev(host[:n])
            self.opt[k] = (dev(host[n:2 * n]), dev(host[2 * n:3 * n]), dev(host[3 * n:]))
        self.ws = torch.full((self.ctx.ws_floats,), float("nan"), device="cuda")
        self.dz, self.iw, self.pw = dev(self.ctx.dz), dev(self.ctx.iw), dev(self.ctx.pw)
        self.vals = [dev(v) for v in value_sets(case)]
        self.sizes = {"logits": self.N, "loss": 1, "grads": n, "dx1": self.N, "dx2": self.M, "dvalues": self.nnz,
                      "inst_loss": self.K, "dlogits_out": self.N}
        assert all(t.data_ptr() % 16 == 0 for t in (self.ws, self.b.x1, self.b.x2, *self.P.values()))

    def model_state(self, rec=None, folded=None):
        return State(self.path, self.cur, rec, folded)

    def snapshot(self, k=None):
        """parameters and optimizer buffers of one id as one device tensor (a copy)"""
        k = self.cur if k is None else k
        return torch.cat([self.P[k], *self.opt[k]])

    def issue(self, op):
        """(return code, {output: tensor}) of one operation; outputs start as the sentinel"""
        L, h, s, p = _lib.lib(), self.h, _lib.current_stream(), _lib.ptr
        P, (ea, es, st) = self.P[self.cur], self.opt[self.cur]
        x1, x2, y, ws, ib = self.b.x1, self.b.x2, self.b.labels, self.ws, 1.0 / self.K
        o = {k: torch.full((self.sizes[k],), SENTINEL, device="cuda") for k in OUTPUTS.get(op, ())}
        q = lambda k: p(o[k])  # noqa: E731
        rc = 0
        if op == "F":
            rc = L.mllp_gnn_forward(h, p(P), p(x1), p(x2), p(ws), q("logits"), s)
        elif op == "B":
            rc = L.mllp_gnn_backward(h, p(P), p(x1), p(x2), p(ws), p(self.dz), q("grads"), s)
        elif op in ("IG", "BI"):
            call = L.mllp_gnn_input_grads if op == "IG" else L.mllp_gnn_backward_inputs
            rc = call(h, p(P), p(x1), p(x2), p(ws), p(self.dz), q("grads"), q("dx1"), q("dx2"), q("dvalues"), None, s)
        elif op == "L":
            rc = L.mllp_gnn_loss_step(h, p(P), p(x1), p(x2), p(y), ib, p(ws), q("logits"), q("loss"), q("grads"), s)
        elif op == "LI":
            rc = L.mllp_gnn_loss_step_inputs(h, p(P), p(x1), p(x2), p(y), ib, p(ws), q("logits"), q("loss"), q("grads"),
                                             q("dx1"), q("dx2"), q("dvalues"), s)
        elif op == "LW":
            rc = L.mllp_gnn_loss_step_weighted(h, p(P), p(x1), p(x2), p(y), p(self.iw), p(self.pw), p(ws), q("logits"),
                                               q("loss"), q("inst_loss"), q("grads"), q("dlogits_out"), s)
        elif op in ("T0", "T1"):
            rc = L.mllp_gnn_train_step(h, p(P), p(x1), p(x2), p(y), ib, p(ws), q("logits"), q("loss"), q("grads"), p(ea), p(es),
                                       p(st), 1e-8, int(op[1]), s)
        elif op in ("S", "SA"):
            opt = (p(ea), p(es), p(st)) if op == "SA" else (None, None, None)
            rc = L.mllp_gnn_train_step_small(h, p(P), p(x1), p(x2), p(y), ib, p(ws), q("logits"), q("loss"), q("grads"), *opt,
                                             1e-8, s)
        elif op in ("P1", "P2"):
            self.path = int(op[1])
            rc = L.mllp_graph_set_path(h, self.path)
        elif op == "V":
            self.vset ^= 1
            rc = L.mllp_graph_set_values(h, p(self.vals[self.vset]), s)
        elif op == "SW":
            self.cur = "B" if self.cur == "A" else "A"
        elif op == "X":
            self.ws.fill_(float("nan"))
        else:
            raise ValueError(op)
        if op in WRITES_PARAMS and rc == 0:
            o["params+adam"] = self.snapshot()
        return rc, o


def replay(case, op, path, vset, snap):
    """the outputs of `op` from a state that carries nothing (memoised: the walk revisits states)"""
    host = snap.cpu().numpy()
    key = (case, op, path, vset, hashlib.blake2b(host.tobytes(), digest_size=16).hexdigest())
    if key not in _REPLAYS:
        m = Machine(case, path, vset, {"A": host})
        if op in cm.BACKWARD_OPS:
            rc, _ = m.issue("F")
            assert rc == 0
        rc, outs = m.issue(op)
        assert rc == 0, (op, _lib.lib().mllp_last_error())
        torch.cuda.synchronize()
        _REPLAYS[key] = outs
    return _REPLAYS[key]


def drive(m, ops, state, where=""):
    """Run `ops` on machine `m` from model state `state` with every check of the module docstring; returns the verdicts and
    the final state."""
    L, done, verdicts = _lib.lib(), [], []
    for pos, op in enumerate(ops):
        verdict, state = cm.step(state, op)
        verdicts.append(verdict)
        done.append(op)
        at = f"{where} position {pos}, last three operations {done[-3:]}"
        if verdict == SKIP:
            continue
        before = {k: m.snapshot(k) for k in m.P}
        cur, ws_before = m.cur, (m.ws.clone() if verdict == REFUSE else None)
        rc, outs = m.issue(op)
        if verdict == REFUSE:
            assert rc != 0, f"{at}: the library accepted {cm.CALLS[op]}, the model refuses it (stale workspace state)"
            assert rc == EINVAL and L.mllp_last_error(), f"{at}: return code {rc}"
            torch.cuda.synchronize()
            for k, t in outs.items():
                assert bool((t == SENTINEL).all()), f"{at}: the refused call wrote {k}"
            assert _same(m.ws, ws_before), f"{at}: the refused call wrote the workspace"
            for k in m.P:
                assert _same(m.snapshot(k), before[k]), f"{at}: the refused call wrote the parameters or optimizer buffers {k}"
            continue
        assert rc == 0, f"{at}: the library refused {cm.CALLS[op]}, the model accepts it: {L.mllp_last_error()}"
        assert (m.path, m.cur) == (state.path, state.cur)
        for k in m.P:                                       # only the train steps write parameters, and only the ones given
            if not (op in WRITES_PARAMS and k == cur):
                assert _same(m.snapshot(k), before[k]), f"{at}: {cm.CALLS[op]} wrote the parameters or optimizer buffers {k}"
        if op in OUTPUTS:
            want = replay(m.case, op, m.path, m.vset, before[cur])
            assert set(want) == set(outs)
            for k in want:
                assert _same(outs[k], want[k]), (f"{at}: {k} of {cm.CALLS[op]} differs from the stateless replay in "
                                                 f"{int((_bits(outs[k]) != _bits(want[k])).sum())} of {want[k].numel()} words")
    return verdicts, state


def start_machine(case):
    ps = parameter_sets()
    return Machine(case, START.path, 0, {k: np.concatenate([ps[k], fresh_adam()]) for k in ("A", "B")})


@gpu
@pytest.mark.parametrize("segment", range(cm.SEGMENTS))
@pytest.mark.parametrize("case", WALK_CASES)
def test_walk_segment(case, segment):
    ops = cm.segments()[segment]
    verdicts, _ = drive(start_machine(case), ops, START, f"{case} segment {segment}")
    assert len(verdicts) == len(ops)


# ---- the replay against the fp64 oracle ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("case", WALK_CASES)
def test_replay_against_the_oracle(case, path):
    """the fresh results in the start state, at the bars of the files that own them (tests/test_memory_contract.py's anchors)"""
    ctx = mc.get_ctx(case, "fused" if path == 2 else "generic")
    snap = torch.tensor(np.concatenate([parameter_sets()["A"], fresh_adam()]))
    assert np.array_equal(ctx.flat, parameter_sets()["A"])
    m = Machine(case, path, 0, {"A": snap.numpy()})
    assert np.array_equal(m.b.export(2).view(np.int32)[:m.nnz], value_sets(case)[0].view(np.int32))
    assert mc.get_ctx(case, "generic").b.small_step_fits()
    bits = lambda outs: {k: _bits(t).cpu().numpy() for k, t in outs.items()}  # noqa: E731
    f = bits(replay(case, "F", path, 0, snap))
    mc.anchor_forward(ctx)(f)
    mc.anchor_forward_backward(ctx)(dict(f, **bits(replay(case, "B", path, 0, snap))))
    for op in ("L", "S"):
        mc.anchor_loss_step(ctx)(bits(replay(case, op, path, 0, snap)))
    mc.anchor_loss_step_inputs(ctx)(bits(replay(case, "LI", path, 0, snap)))
    lw = bits(replay(case, "LW", path, 0, snap))
    mc.anchor_weighted(ctx)(dict(lw, dlogits=lw["dlogits_out"]))
    for op in ("IG", "BI") if path == 1 else ("IG",):
        mc.anchor_input_grads(ctx)(dict(f, **bits(replay(case, op, path, 0, snap))))


# ---- named sequences ----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", list(WHY))
def test_stale_sequence_is_refused_and_nothing_is_written(name):
    """each was accepted, and returned gradients of no model, before the workspace record knew the parameters and before the
    loss and train steps kept it"""
    verdicts, _ = drive(start_machine("one"), WHY[name], START, name)
    assert verdicts[-1] == REFUSE


@gpu
def test_input_grads_after_forward_and_loss_step_with_the_same_parameters():
    """the fused loss step leaves layer 3's saved state to the forward before it: with the same parameters those are the same
    bits, and mllp_gnn_input_grads returns what it returns straight after a forward"""
    for case in WALK_CASES:
        verdicts, state = drive(start_machine(case), ("F", "L", "IG", "LI", "B", "IG"), START, case)
        assert verdicts == [ACCEPT] * 6 and state.rec == (2, "A")


@gpu
def test_backward_after_switching_the_path_there_and_back():
    verdicts, _ = drive(start_machine("one"), ("F", "P1", "P2", "B", "P1", "B"), START)
    assert verdicts == [ACCEPT] * 5 + [REFUSE]


@gpu
@pytest.mark.parametrize("between", ["train_step", "loss_step"])
def test_module_backward_after_a_step_on_the_same_batch_raises(between):
    """z = model(g); a train step (or a loss step, which can only be with another parameter tensor) on g.lp_batch(); then
    z.sum().backward() raises instead of returning gradients of no model"""
    from mllp_amd.model import GNNModel, build_graph_from_weights_sets
    inst = mc.case_instances("one")[0]
    _, constrs, w, coefs, rhs, _ = inst.as_reference_tuple()
    flat = parameter_sets()["A"]
    model = GNNModel().to("cuda")
    model.load_flat(torch.tensor(flat, device="cuda"))
    g = build_graph_from_weights_sets(constrs, w, rhs, coefs, torch.device("cuda"))
    z = model(g)
    p = torch.tensor(flat, device="cuda")
    if between == "train_step":
        ea, es, st = (torch.tensor(a, device="cuda") for a in np.split(fresh_adam(), [_lib.NUM_PARAMS, 2 * _lib.NUM_PARAMS]))
        g.lp_batch().train_step(p, ea, es, st)
    else:
        g.lp_batch().loss_step(p)
    with pytest.raises(RuntimeError, match="mllp_gnn_backward"):
        z.sum().backward()
    assert all(q.grad is None for q in model.parameters())
    z = model(g)                                                     # the batch works afterwards
    z.sum().backward()
    assert model.fc.weight.grad is not None and bool(torch.isfinite(model.fc.weight.grad).all())
