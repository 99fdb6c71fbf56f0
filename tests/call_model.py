"""A model of what the library remembers about one graph between whole-model calls (include/mllp_hip.h, "RECORDS"; DESIGN.md
4.17), and the fixed walk over call sequences that tests/test_call_sequences.py drives.  Pure Python: no GPU, no library.

State: (path, cur, rec, folded)
  path    1 generic / LDS-tiled sweeps, 2 fused latency-regime kernels (mllp_graph_set_path)
  cur     which of the caller's two parameter tensors, "A" or "B", the next call is given
  rec     the workspace record: None, or (path, params id) of the forward whose activations the workspace holds
  folded  the folded-weights record: None, or the params id whose folded weights a fused train step left behind

The caller has ONE workspace per graph, so the records' workspace pointer never differs and is not modelled.
"""
from collections import namedtuple

State = namedtuple("State", "path cur rec folded")
START = State(2, "A", None, None)

# the alphabet, in the order the walk numbers it (the order decides which states the walk visits: see CONDITIONS)
OPS = ("SA", "LI", "P2", "S", "SW", "IG", "F", "T1", "V", "BI", "X", "LW", "P1", "B", "L", "T0")
CALLS = {
    "F": "mllp_gnn_forward", "B": "mllp_gnn_backward", "IG": "mllp_gnn_input_grads", "BI": "mllp_gnn_backward_inputs",
    "L": "mllp_gnn_loss_step", "LI": "mllp_gnn_loss_step_inputs", "LW": "mllp_gnn_loss_step_weighted",
    "T0": "mllp_gnn_train_step flags 0", "T1": "mllp_gnn_train_step flags 1", "S": "mllp_gnn_train_step_small, loss step",
    "SA": "mllp_gnn_train_step_small with Adam", "P1": "mllp_graph_set_path 1", "P2": "mllp_graph_set_path 2",
    "V": "mllp_graph_set_values, the other value set", "SW": "the caller's other parameter tensor",
    "X": "the caller fills the workspace with NaN",
}
BACKWARD_OPS = ("B", "BI", "IG")
ACCEPT, REFUSE, SKIP = "accept", "refuse", "skip"


def step(s, op):
    """(verdict, next state).  REFUSE: the library returns MLLP_EINVAL and writes nothing.  SKIP: the caller does not issue
    the operation (X while a record is set: MEMORY CONTRACT point 4 allows the clobber only where nothing is carried)."""
    here = (s.path, s.cur)
    if op == "F" or op == "LW":                     # (LW is forward, loss head, backward: its forward sets the record)
        return ACCEPT, s._replace(rec=here, folded=None)
    if op in ("B", "IG"):
        return (ACCEPT if s.rec == here else REFUSE), s
    if op == "BI":
        return (ACCEPT if s.rec == here and s.path == 1 else REFUSE), s
    if op in ("L", "LI"):
        return ACCEPT, s._replace(rec=s.rec if s.rec == here else None, folded=None)
    if op in ("T0", "T1"):
        return ACCEPT, s._replace(rec=None, folded=s.cur if s.path == 2 else None)
    if op in ("S", "SA"):
        return ACCEPT, s._replace(rec=None, folded=None)
    if op in ("P1", "P2"):
        return ACCEPT, s._replace(path=int(op[1]), folded=None)
    if op == "V":
        return ACCEPT, s._replace(rec=None)
    if op == "SW":
        return ACCEPT, s._replace(cur="B" if s.cur == "A" else "A")
    if op == "X":
        return (ACCEPT if s.rec is None and s.folded is None else SKIP), s
    raise ValueError(op)


def run(ops, state=START):
    """[(op, verdict, state after)] of a sequence from `state`"""
    out = []
    for op in ops:
        verdict, state = step(state, op)
        out.append((op, verdict, state))
    return out


def de_bruijn(k, n):
    """The de Bruijn sequence B(k, n) that concatenates the Lyndon words whose length divides n in lexicographic order (the
    construction of Fredricksen and Maiorana, smallest symbol first): every word of n symbols over range(k) occurs once
    as a cyclic window.  k ** n symbols."""
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
            return
        a[t] = a[t - p]
        db(t + 1, p)
        for j in range(a[t - p] + 1, k):
            a[t] = j
            db(t + 1, t)
    db(1, 1)
    return seq


ORDER = 3
SEGMENTS = 16


def walk():
    """the cyclic sequence opened up: extended by its first ORDER - 1 symbols, every triple of operations is a window"""
    seq = de_bruijn(len(OPS), ORDER)
    return [OPS[i] for i in seq + seq[:ORDER - 1]]


def segments(n=SEGMENTS):
    """the walk cut into n pieces that overlap by ORDER - 1 calls (no window is lost at a cut); each starts from START"""
    w = walk()
    size, rem = divmod(len(w) - (ORDER - 1), n)
    assert rem == 0
    return [w[i * size:(i + 1) * size + ORDER - 1] for i in range(n)]


def census(n=SEGMENTS):
    """what the walk exercises, by the model alone"""
    c = {"calls": 0, "refused": 0, "accepted": dict.fromkeys(BACKWARD_OPS, 0), "refused_by_op": dict.fromkeys(BACKWARD_OPS, 0),
         "x_issued": 0, "x_skipped": 0, "max_adam_steps": 0}
    for seg in segments(n):
        adam = 0
        for op, verdict, _ in run(seg):
            c["calls"] += 1
            if op in BACKWARD_OPS:
                c["accepted" if verdict == ACCEPT else "refused_by_op"][op] += 1
                c["refused"] += verdict == REFUSE
            if op == "X":
                c["x_issued" if verdict == ACCEPT else "x_skipped"] += 1
            adam += op in ("T0", "T1", "SA")
        c["max_adam_steps"] = max(c["max_adam_steps"], adam)
    return c
