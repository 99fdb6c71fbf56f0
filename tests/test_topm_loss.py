"""The soft top-m loss head (mllp_topm_loss, mllp_topm_loss_limits, mllp_topm_loss_math, mllp_gnn_loss_step_topm;
LPBatch.topm_loss / topm_prob / loss_step_topm; the trainer's and the driver's `loss_head: 'topm'`) against the fp64 oracle
of tests/topm_oracle.py.

Segments only for the head itself: instances without nonzeros, m_k rows and n_k columns each.
  PARITY batch   (n, m) = (1, 1), (3, 3), (7, 0) [no root], (12, 5), (100, 40), (2400, 1200), the lane-count edge
                 n = 1023 / 1024 / 1025, and both sides of the threshold mllp_topm_loss_limits reports (n = limit, limit + 1).
                 Every instance with a root has Q >= 1 and a derived bound on L_k below 1e-4 L_k (asserted from the oracle
                 before anything is compared).
  EDGE batch     m = 1 and m = n - 1 (Q = 1 - sum p^2 < 1 whatever the logits), and a sharp temperature: these finish, and
                 sum p = m within the bound of F; they are not parity cases.
TOLERANCES are the bounds of tests/topm_oracle.py (module docstring there), with no multiplier: the one constant the code
does not state is the ulp error of the device's expf / log1pf / logf, measured here on grids
(test_device_math_within_k_ulp) and used as topm_oracle.K_ULP.
"""
import ctypes
import json

import numpy as np
import pytest
import torch

import fused_cases as fc
import topm_oracle as to
from guarded import NAN, same_bits
from mllp_amd import _lib

gpu = pytest.mark.gpu
EINVAL = -1
TAUS = (1.0, 0.25)
S_NOISY, SIGMA, SEED = 3, 0.5, 20240607


def limits():
    lim = (ctypes.c_int64 * 2)()
    _lib.check(_lib.lib().mllp_topm_loss_limits(lim))
    return int(lim[0]), int(lim[1])


def parity_shapes():
    lds_max, threads = limits()
    assert threads == 1024
    return [(1, 1), (3, 3), (7, 0), (12, 5), (100, 40), (2400, 1200), (1023, 400), (1024, 600), (1025, 300),
            (lds_max, lds_max // 3), (lds_max + 1, lds_max // 2)]


def edge_shapes():
    lds_max, _ = limits()
    return [(12, 1), (12, 11), (1025, 1), (1025, 1024), (lds_max + 1, 1), (lds_max + 1, lds_max), (120, 50)]


def make_case(shapes, seed, labels="m", scale=1.0):
    """instances without nonzeros of the given (n, m), fp32 logits, 0/1 labels (`m`: sum y = m; `other`: sum y != m where
    the instance has room), instance weights (one of them 0) and pos_weights"""
    rng = np.random.default_rng(seed)
    insts, ys = [], []
    for k, (n, m) in enumerate(shapes):
        it = fc.empty_instance(m, n, seed=k)
        it.name = f"seg{k}_{n}_{m}"
        cnt = min(m, n) if labels == "m" else (min(m, n) // 2 if min(m, n) >= 2 else min(n, m + 1))
        y = np.zeros(n, np.int32)
        y[rng.permutation(n)[:cnt]] = 1
        it.basis = y
        insts.append(it)
        ys.append(y)
    seg_n, seg_m = [s[0] for s in shapes], [s[1] for s in shapes]
    N, K = sum(seg_n), len(shapes)
    z = (scale * rng.standard_normal(N)).astype(np.float32)
    iw = (0.25 + 1.5 * rng.random(K)).astype(np.float32)
    iw[4 % K] = 0.0                                                      # a held-out instance: dz = 0, its loss still reported
    pw = (0.5 + 2.0 * rng.random(K)).astype(np.float32)
    ids = (1000 + 7 * np.arange(K)).astype(np.int32)
    return dict(shapes=shapes, insts=insts, seg_n=seg_n, seg_m=seg_m, N=N, K=K, z=z, y=np.concatenate(ys).astype(np.float32), iw=iw,
                pw=pw, ids=ids, off=np.concatenate([[0], np.cumsum(seg_n)]))


_CASES, _BATCH, _ORACLE = {}, {}, {}


def case(labels):
    if labels not in _CASES:
        _CASES[labels] = make_case(parity_shapes(), 5 if labels == "m" else 6, labels)
    return _CASES[labels]


def batch_of(c):
    from mllp_amd.graph import LPBatch
    if id(c) not in _BATCH:
        _lib.lib()
        assert torch.cuda.is_available()
        _BATCH[id(c)] = LPBatch.from_instances(c["insts"])
    return _BATCH[id(c)]


def oracle(c, tau, S):
    """computed once per (case, tau, S), shared, never modified"""
    key = (id(c), tau, S)
    if key not in _ORACLE:
        _ORACLE[key] = to.batch(c["z"], c["y"], c["seg_n"], c["seg_m"], tau, SIGMA if S else 0.0, S, SEED, c["ids"], c["iw"], c["pw"])
    return _ORACLE[key]


def dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda")


def run_head(c, tau, S, want=("loss", "inst_loss", "dlogits", "prob", "info"), b=None, sl=None):
    b = b or batch_of(c)
    pick = (lambda a: a) if sl is None else (lambda a: a[sl])
    return b.topm_loss(dev(c["z"] if sl is None else c["z"][c["off"][sl.start]:c["off"][sl.stop]]), tau, SIGMA if S else 0.0, S, SEED,
                       dev(pick(c["iw"])), dev(pick(c["pw"])), want, dev(pick(c["ids"]), torch.int32))


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


def _worst(got, want, bound):
    """max over elements of |got - want| / bound (0 / 0 counts as 0): at most 1 when every element is within its bound"""
    err = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    bound = np.broadcast_to(np.asarray(bound, np.float64), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.max(r)) if r.size else 0.0


# ---- CPU: the surface -----------------------------------------------------------------------------------------------------
def test_symbols_limits_and_refusals_without_a_device():
    L = _lib.lib()
    lds_max, threads = limits()
    assert threads == 1024 and lds_max >= threads and lds_max * 4 <= 64 * 1024
    one = ctypes.c_void_p(16)
    assert L.mllp_topm_loss_limits(None) == EINVAL
    assert L.mllp_topm_loss(None, one, one, None, None, None, 1.0, 0.0, 0, 0, one, None, None, None, None, None) == EINVAL
    assert b"null" in L.mllp_last_error()
    assert L.mllp_gnn_loss_step_topm(None, one, one, one, one, None, None, None, 1.0, 0.0, 0, 0, one, one, None, None, one, one,
                                     None) == EINVAL
    assert L.mllp_topm_loss_math(3, 1, one, one, None) == EINVAL and L.mllp_topm_loss_math(0, 1, None, one, None) == EINVAL
    header = open(_lib.HEADER_PATH).read()
    for text in ("tau here = sinkhorn_tau / 2", "0x7feb352d", "0x846ca68b", "0x9E3779B9", "0x85EBCA6B", "at most 64", "2 ulp above lo"):
        assert text in header, text


def test_config_keys_default_to_the_run_without_them():
    from mllp_amd import experiment
    from mllp_amd.config import HOT_PATH_DEFAULTS, AttrDict
    assert HOT_PATH_DEFAULTS["loss_head"] == "bce" and HOT_PATH_DEFAULTS["topm_tau"] == 1.0
    assert experiment.topm_head(AttrDict(), "gs-topk") == {} and experiment.topm_head(AttrDict(loss_head="bce"), "soft-topk") == {}
    cfg = AttrDict(loss_head="topm", topm_tau=0.5, train_gumbel_sample_num=10, gumbel_sigma=0.05)
    assert experiment.topm_head(cfg, "soft-topk") == dict(loss_head="topm", topm_tau=0.5)
    assert experiment.topm_head(cfg, "gs-topk") == dict(loss_head="topm", topm_tau=0.5, topm_samples=10, topm_sigma=0.05)
    with pytest.raises(ValueError):
        experiment.topm_head(AttrDict(loss_head="sinkhorn"), "gs-topk")
    with pytest.raises(ValueError):
        experiment.topm_head(AttrDict(loss_head="topm"), "gs-topk")


# ---- GPU: the one measured constant --------------------------------------------------------------------------------------
@gpu
def test_device_math_within_k_ulp():
    """expf on [-104, 0] (the head's argument is -|u|), log1pf on [0, 1] (of e <= 1), logf on (0, 1) (of t and of -log t's
    range, and on [2^-24, 16] for logit(m / n)): the largest error in ulp of the fp32 result against fp64, printed, and at most
    topm_oracle.K_ULP, the figure every tolerance of this file uses."""
    L = _lib.lib()
    rng = np.random.default_rng(1)
    n = 1 << 18
    grids = {0: np.concatenate([-np.abs(rng.standard_normal(n)) * 4.0, -rng.random(n) * 104.0, -rng.random(n) * 2.0 ** -10]),
             1: np.concatenate([rng.random(n), np.exp(-rng.random(n) * 100.0), [0.0, 1.0]]),
             2: np.concatenate([(rng.integers(0, 1 << 23, n) + 0.5) * 2.0 ** -23, -np.log((rng.integers(0, 1 << 23, n) + 0.5) * 2.0 ** -23),
                                rng.random(n) * 16.0 + 2.0 ** -24])}
    f64 = {0: np.exp, 1: np.log1p, 2: np.log}
    worst = {}
    for which, x in grids.items():
        x = x.astype(np.float32)
        xd, yd = dev(x), torch.empty(len(x), device="cuda")
        _lib.check(L.mllp_topm_loss_math(which, len(x), _lib.ptr(xd), _lib.ptr(yd), _lib.current_stream()))
        got = yd.cpu().numpy()
        want = f64[which](x.astype(np.float64))
        keep = np.abs(want) >= 2.0 ** -126                                  # (ulp of a normal result)
        ulp = np.spacing(np.abs(want[keep]).astype(np.float32)).astype(np.float64)
        worst[which] = float(np.max(np.abs(got[keep].astype(np.float64) - want[keep]) / ulp))
    print("largest error in ulp: expf %.3f, log1pf %.3f, logf %.3f (K_ULP = %g)" % (worst[0], worst[1], worst[2], to.K_ULP))
    assert max(worst.values()) <= to.K_ULP, worst


# ---- GPU: parity ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("S", [0, S_NOISY])
@pytest.mark.parametrize("labels", ["m", "other"])
@pytest.mark.parametrize("tau", TAUS)
def test_parity_with_the_oracle(tau, labels, S):
    c = case(labels)
    res, loss, loss_bound, off = oracle(c, tau, S)
    # the conditions that keep the bound honest, from the oracle, first
    rooted = [k for k, r in enumerate(res) if not r["degenerate"]]
    assert len(rooted) == c["K"] - 3
    for k in rooted:
        r = res[k]
        assert r["Q"] >= 1.0, (c["shapes"][k], r["Q"])
        assert r["bound"]["L"] < 1e-4 * r["L"], (c["shapes"][k], r["bound"]["L"], r["L"])
        if labels == "other":
            assert c["y"][off[k]:off[k + 1]].sum() != c["seg_m"][k]
    out = run_head(c, tau, S)
    torch.cuda.synchronize()
    L, ls, dz = out["inst_loss"].cpu().numpy(), float(out["loss"][0]), out["dlogits"].cpu().numpy()
    p, info = out["prob"].cpu().numpy(), out["info"].cpu().numpy()
    assert all(np.isfinite(a).all() for a in (L, dz, p, info)) and np.isfinite(ls)
    worst = dict(L=0.0, dz=0.0, p=0.0, nu=0.0, Q=0.0, resid=0.0)
    for k, r in enumerate(res):
        s = slice(off[k], off[k + 1])
        if r["degenerate"]:
            assert L[k] == 0.0 and not dz[s].any() and (p[s] == r["p"]).all() and list(info[k]) == [0.0, 0.0, r["resid"], -1.0]
            continue
        b = r["bound"]
        worst["L"] = max(worst["L"], _worst(L[k], r["L"], b["L"]))
        worst["dz"] = max(worst["dz"], _worst(dz[s], r["dz"], b["dz"]))
        worst["p"] = max(worst["p"], _worst(p[s], r["p"], b["p"]))
        worst["nu"] = max(worst["nu"], _worst(info[k, 0], r["nu"], b["nu"]))
        worst["resid"] = max(worst["resid"], _worst(info[k, 2], 0.0, b["resid"]))
        worst["Q"] = max(worst["Q"], _worst(info[k, 1], r["Q"], b["Q"]))
        assert 1 <= info[k, 3] <= 64
        if c["iw"][k] == 0:
            assert not dz[s].any() and L[k] > 0                             # weight 0: exactly no gradient, its loss reported
    w_loss = _worst(ls, loss, loss_bound)
    print(f"tau {tau} labels {labels} S {S}: largest error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items())
          + f", loss {w_loss:.3f}; iterations {info[:, 3].astype(int).tolist()}")
    assert max(worst.values()) <= 1.0 and w_loss <= 1.0, (worst, w_loss)
    if S:                                                                    # the noise is there: far outside any tolerance
        free = oracle(c, tau, 0)[0]
        k = 5
        assert abs(res[k]["L"] - free[k]["L"]) > 100 * res[k]["bound"]["L"]


@gpu
def test_sharp_and_one_sided_instances_finish():
    """m = 1, m = n - 1 and tau = 0.02 on 50 of 120: Q < 1, so no parity; every evaluation ends within 64 iterations, everything
    is finite, and sum p = m within the bound of F"""
    c = make_case(edge_shapes(), 9, scale=0.1)
    b = batch_of(c)
    for tau, S in ((1.0, 0), (0.02, 0), (0.02, S_NOISY)):
        res = oracle(c, tau, S)[0]
        assert any(r["Q"] < 1.0 for r in res)
        out = run_head(c, tau, S, b=b)
        torch.cuda.synchronize()
        info, p = out["info"].cpu().numpy(), out["prob"].cpu().numpy().astype(np.float64)
        assert all(bool(torch.isfinite(out[k]).all()) for k in out)
        assert (info[:, 3] >= 1).all() and (info[:, 3] <= 64).all(), info[:, 3]
        for k, r in enumerate(res):
            s = slice(c["off"][k], c["off"][k + 1])
            assert abs(info[k, 2]) <= r["bound"]["resid"], (tau, S, c["shapes"][k], info[k], r["bound"]["resid"])
            assert abs(p[s].sum() - c["seg_m"][k]) <= r["bound"]["resid"] + to.U * c["seg_m"][k]
        print(f"tau {tau} S {S}: iterations {info[:, 3].astype(int).tolist()}, Q {[round(float(q), 3) for q in info[:, 1]]}")


# ---- GPU: determinism ----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("S", [0, S_NOISY])
def test_same_bits_again_alone_and_whatever_is_asked_for(S):
    from mllp_amd.graph import LPBatch
    c = case("other")
    b = batch_of(c)
    names = ("loss", "inst_loss", "dlogits", "prob", "info")
    r1, r2 = run_head(c, 0.25, S), run_head(c, 0.25, S)
    for name in names:
        assert _bits(r1[name]) == _bits(r2[name]), name
    off = c["off"]
    for k, inst in enumerate(c["insts"]):                                    # each instance alone, with its id
        one = run_head(c, 0.25, S, b=LPBatch.from_instances([inst]), sl=slice(k, k + 1))
        assert _bits(one["inst_loss"]) == _bits(r1["inst_loss"][k:k + 1]), inst.name
        assert _bits(one["dlogits"]) == _bits(r1["dlogits"][off[k]:off[k + 1]]), inst.name
        assert _bits(one["prob"]) == _bits(r1["prob"][off[k]:off[k + 1]]), inst.name
        assert _bits(one["info"]) == _bits(r1["info"][k:k + 1]), inst.name
    for want in ("loss", "inst_loss", "dlogits", "prob", "info", ("loss", "dlogits"), ("inst_loss", "prob"), ("dlogits", "info")):
        got = run_head(c, 0.25, S, want=want)
        for name in names:
            if name in ((want,) if isinstance(want, str) else want):
                assert _bits(got[name]) == _bits(r1[name]), (want, name)
            else:
                assert got[name] is None
    # d_loss without d_inst_loss: one workgroup takes the instances in turn, the same bits
    lo, z = torch.zeros(1, device="cuda"), dev(c["z"])
    iw, pw, ids = dev(c["iw"]), dev(c["pw"]), dev(c["ids"], torch.int32)     # (named: they must outlive the call)
    _lib.check(_lib.lib().mllp_topm_loss(b._h, _lib.ptr(z), _lib.ptr(b.labels), _lib.ptr(iw), _lib.ptr(pw), _lib.ptr(ids), 0.25,
                                         SIGMA if S else 0.0, S, SEED, None, None, _lib.ptr(lo), None, None, _lib.current_stream()))
    assert _bits(lo) == _bits(r1["loss"])
    # without ids instance k has id k; topm_prob is the noise-free p
    assert _bits(b.topm_prob(z, 0.25)) == _bits(run_head(c, 0.25, 0, want="prob")["prob"])
    if S:
        other = b.topm_loss(z, 0.25, SIGMA, S, SEED + 1, iw, pw, "inst_loss", ids)
        assert _bits(other["inst_loss"]) != _bits(r1["inst_loss"])           # another seed, another noise
    with pytest.raises(ValueError):
        b.topm_loss(z, tau=0.0)
    with pytest.raises(ValueError):
        b.topm_loss(z, want=())


# ---- GPU: memory and refusals ------------------------------------------------------------------------------------------------
class HeadCtx:
    """a batch of segments and the head's arguments, in the shape the cells of tests/test_stream_contract.py take"""
    config = "-"

    def __init__(self, name, c, tau, S, second=None, b=None):
        self.case, self.c, self.tau, self.S, self.second = name, c, tau, S, second
        self.b = b or batch_of(c)
        self.h = self.b._h


def ep_topm_loss(ctx, B):
    c = ctx.c
    z, y = B.ro("logits", c["z"]), B.ro("labels", c["y"])
    iw, pw, ids = B.ro("inst_weight", c["iw"]), B.ro("pos_weight", c["pw"]), B.ro("inst_id", c["ids"], dtype=torch.int32)
    o = dict(dlogits=B.rw("dlogits", c["N"]), inst_loss=B.rw("inst_loss", c["K"]), loss=B.rw("loss", 1), prob=B.rw("prob", c["N"]),
             info=B.rw("info", 4 * c["K"]))
    _lib.check(_lib.lib().mllp_topm_loss(ctx.h, z.ptr, y.ptr, iw.ptr, pw.ptr, ids.ptr, ctx.tau, SIGMA if ctx.S else 0.0, ctx.S, SEED,
                                         o["dlogits"].ptr, o["inst_loss"].ptr, o["loss"].ptr, o["prob"].ptr, o["info"].ptr,
                                         _lib.current_stream()))
    return o


def fl(a):
    return a.view(np.float32)


def anchor_topm_loss(ctx):
    """the oracle at its bounds, as test_parity_with_the_oracle"""
    c = ctx.c
    res, loss, loss_bound, off = to.batch(c["z"], c["y"], c["seg_n"], c["seg_m"], ctx.tau, SIGMA if ctx.S else 0.0, ctx.S, SEED, c["ids"],
                                          c["iw"], c["pw"])

    def check(out):
        L, dz, p, info = fl(out["inst_loss"]), fl(out["dlogits"]), fl(out["prob"]), fl(out["info"]).reshape(-1, 4)
        assert _worst(fl(out["loss"])[0], loss, loss_bound) <= 1.0
        for k, r in enumerate(res):
            s, b = slice(off[k], off[k + 1]), r["bound"]
            if r["degenerate"]:
                assert L[k] == 0.0 and not dz[s].any() and info[k, 3] == -1.0
                continue
            assert r["Q"] >= 1.0
            assert _worst(L[k], r["L"], b["L"]) <= 1.0 and _worst(dz[s], r["dz"], b["dz"]) <= 1.0, c["shapes"][k]
            assert _worst(p[s], r["p"], b["p"]) <= 1.0 and _worst(info[k, 0], r["nu"], b["nu"]) <= 1.0, c["shapes"][k]
    return check


@gpu
@pytest.mark.parametrize("S", [0, S_NOISY])
def test_memory_contract_and_refusals(S):
    import test_memory_contract as mc
    ctx = HeadCtx("parity", case("m"), 0.25, S)
    runs = {}
    for fill in ("zero", "nan", "huge"):                                     # the three poisons, under guard bands
        B = mc.Bufs(fill, shift=4 if fill == "huge" else 0)
        outs = ep_topm_loss(ctx, B)
        B.check()                                                            # guards intact, read-only inputs unchanged
        runs[fill] = {k: g.bits() for k, g in outs.items()}
    anchor_topm_loss(ctx)(runs["zero"])
    same_bits(runs["nan"], runs["zero"], "outputs after a NaN fill")
    same_bits(runs["huge"], runs["zero"], "outputs after a fill with the largest float, pointers shifted by 4 bytes")
    # every refusal leaves the poison in place
    L, c = _lib.lib(), ctx.c
    B = mc.Bufs("nan")
    z, y = B.ro("logits", c["z"]), B.ro("labels", c["y"])
    o = [B.rw(n, k) for n, k in (("dlogits", c["N"]), ("inst_loss", c["K"]), ("loss", 1), ("prob", c["N"]), ("info", 4 * c["K"]))]
    m = types_model(ctx, B)
    s = _lib.current_stream()
    nan, inf = float("nan"), float("inf")
    bad = [(0.0, 0.0, 0), (-1.0, 0.0, 0), (nan, 0.0, 0), (inf, 0.0, 0), (1.0, -0.5, 0), (1.0, nan, 0), (1.0, inf, 0), (1.0, 0.0, -1)]
    for tau, sigma, n_s in bad:
        assert L.mllp_topm_loss(ctx.h, z.ptr, y.ptr, None, None, None, tau, sigma, n_s, 0, *[g.ptr for g in o], s) == EINVAL, (tau, sigma, n_s)
        assert L.mllp_last_error()
        assert L.mllp_gnn_loss_step_topm(ctx.h, m["P"].ptr, m["x1"].ptr, m["x2"].ptr, y.ptr, None, None, None, tau, sigma, n_s, 0, m["ws"].ptr,
                                         m["logits"].ptr, o[2].ptr, o[1].ptr, m["grads"].ptr, o[0].ptr, s) == EINVAL, (tau, sigma, n_s)
    assert L.mllp_topm_loss(ctx.h, z.ptr, y.ptr, None, None, None, 1.0, 0.0, 0, 0, None, None, None, None, None, s) == EINVAL
    assert L.mllp_topm_loss(ctx.h, None, y.ptr, None, None, None, 1.0, 0.0, 0, 0, *[g.ptr for g in o], s) == EINVAL
    assert L.mllp_topm_loss(ctx.h, z.ptr, None, None, None, None, 1.0, 0.0, 0, 0, *[g.ptr for g in o], s) == EINVAL
    assert L.mllp_gnn_loss_step_topm(ctx.h, m["P"].ptr, m["x1"].ptr, m["x2"].ptr, y.ptr, None, None, None, 1.0, 0.0, 0, 0, m["ws"].ptr,
                                     m["logits"].ptr, o[2].ptr, o[1].ptr, m["grads"].ptr, None, s) == EINVAL
    B.check()
    for g in o + [m["ws"], m["logits"], m["grads"]]:
        assert (g.bits().view(np.uint32) == NAN).all(), f"{g.name}: a refused call wrote"


def types_model(ctx, B):
    """the model buffers of a step on the context's batch (refusals only: never computed on)"""
    n = ctypes.c_int64()
    _lib.check(_lib.lib().mllp_gnn_workspace_bytes(ctx.h, ctypes.byref(n)))
    b = ctx.b
    return dict(P=B.ro("params", np.zeros(_lib.NUM_PARAMS, np.float32), wide=True), x1=B.ro("x1", b.x1.cpu().numpy(), wide=True),
                x2=B.ro("x2", b.x2.cpu().numpy(), wide=True), ws=B.rw("ws", n.value // 4, wide=True), logits=B.rw("step_logits", b.N),
                grads=B.rw("grads", _lib.NUM_PARAMS))


# ---- GPU: the whole step ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("S", [0, S_NOISY])
def test_whole_step_equals_its_three_calls(subset5, golden, path, S):
    """mllp_gnn_loss_step_topm on the five Netlib fixtures, generic path (1) and fused path (2): logits, dlogits, loss and
    gradients are the bits of forward, mllp_topm_loss, backward; input_grads afterwards is accepted"""
    from mllp_amd.graph import LPBatch
    p = torch.tensor(golden["weights_flat"], dtype=torch.float32, device="cuda")
    b = LPBatch.from_instances(subset5).set_path(path)
    iw = torch.full((b.n_inst,), 1.0 / b.n_inst, device="cuda")
    sigma = SIGMA if S else 0.0
    z = b.forward(p).clone()
    head = b.topm_loss(z, 0.5, sigma, S, 77, iw, "balanced")
    g = b.backward(p, head["dlogits"]).clone()
    loss, logits, grads, inst_loss = b.loss_step_topm(p, 0.5, sigma, S, 77, iw, "balanced")
    torch.cuda.synchronize()
    assert _bits(logits) == _bits(z) and _bits(b.last_dlogits) == _bits(head["dlogits"]) and _bits(grads) == _bits(g)
    assert _bits(loss) == _bits(head["loss"]) and _bits(inst_loss) == _bits(head["inst_loss"])
    assert bool(torch.isfinite(grads).all()) and bool(grads.any()) and float(loss[0]) > 0
    g2, dx1, dx2, dv = b.input_grads(p, b.last_dlogits)                      # the workspace record allows it
    torch.cuda.synchronize()
    assert _bits(g2) == _bits(grads) and all(bool(torch.isfinite(t).all()) for t in (dx1, dx2, dv))
    # the head's loss against the oracle on the device's own logits (fp32 values, fp64 arithmetic)
    seg_n, seg_m = [i.n for i in subset5], [i.m for i in subset5]
    y = np.concatenate([np.asarray(i.basis, np.float64) for i in subset5])
    res, want, bound, _ = to.batch(z.cpu().numpy(), y, seg_n, seg_m, 0.5, sigma, S, 77, None, iw.cpu().numpy(),
                                   b.balanced_pos_weight().cpu().numpy())
    assert _worst(float(loss[0]), want, bound) <= 1.0, (float(loss[0]), want, bound)


# ---- GPU: trainer and driver ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("method", ["soft-topk", "gs-topk"])
def test_driver_trains_resumes_and_leaves_bce_alone(tmp_path, monkeypatch, method):
    from mllp_amd import experiment
    names = ["afiro.mps", "sc50a.mps", "adlittle.mps", "blend.mps", "kb2.mps"]
    base = (f"train_data_type: 'netlib'\ntrain_lr: 1.e-3\nmethods:\n  - '{method}'\ninstances: {names}\nbatch_size: 1\n"
            "train_gumbel_sample_num: 3\ngumbel_sigma: 0.05\n")

    def run(d, iters, resume, extra, save_every=0):
        d.mkdir(exist_ok=True)
        (d / "cfg.yaml").write_text(base + extra + f"train_iter: {iters}\nresume: {resume}\nsave_every: {save_every}\n")
        monkeypatch.chdir(d)
        assert experiment.main(["--cfg", str(d / "cfg.yaml")]) == 0
        ck = torch.load(d / f"linear_program_netlib_{method}.ckpt", map_location="cpu", weights_only=True)
        return json.load(open(d / "train_log.json")), ck

    topm = "loss_head: 'topm'\ntopm_tau: 0.5\n"
    log_s, ck_s = run(tmp_path / "straight", 2, False, topm)
    obj = log_s["obj"]
    assert len(obj) == 2 and all(np.isfinite(obj)) and obj[1] < obj[0], obj
    assert ck_s["topm_step"] == 10                                           # five steps an epoch: the seed of the next one
    log_1, ck_1 = run(tmp_path / "resumed", 1, False, topm, save_every=1)
    assert ck_1["topm_step"] == 5 and log_1["obj"] == obj[:1]
    log_r, ck_r = run(tmp_path / "resumed", 2, True, topm)
    assert log_r == log_s and ck_r["topm_step"] == 10
    assert torch.equal(ck_r["params"], ck_s["params"])                       # bit for bit: the seed was restored
    for k in ("m", "v", "state"):
        assert torch.equal(ck_r["opt"][k], ck_s["opt"][k]), k
    if method == "gs-topk":
        return
    # loss_head: 'bce' is the run without the key
    log_b, ck_b = run(tmp_path / "bce", 2, False, "loss_head: 'bce'\n")
    log_0, ck_0 = run(tmp_path / "nokey", 2, False, "")
    assert log_b == log_0 and torch.equal(ck_b["params"], ck_0["params"]) and "topm_step" not in ck_b and sorted(ck_b) == sorted(ck_0)
    assert log_b["obj"] != log_s["obj"]


@gpu
def test_trainer_evaluates_without_noise_and_predict_writes_the_soft_basis(subset5, golden):
    from mllp_amd.graph import LPBatch
    from mllp_amd.trainer import LPTrainer
    p = torch.tensor(golden["weights_flat"], dtype=torch.float32, device="cuda")
    t = LPTrainer(p, lr=1e-3, with_metrics=True, pos_weight="balanced", loss_head="topm", topm_tau=0.5, topm_sigma=0.3, topm_samples=2)
    b, held = LPBatch.from_instances(subset5), LPBatch.from_instances(subset5[:2])
    loss, logits = t.step(b)
    assert t.topm_step == 1 and not t.uses_graph(b) and bool(torch.isfinite(loss).all())
    before = [_bits(x) for x in (t.params, t.opt.m, t.opt.v, t.opt.state)]
    ev = t.evaluate(held)
    torch.cuda.synchronize()
    assert [_bits(x) for x in (t.params, t.opt.m, t.opt.v, t.opt.state)] == before and t.topm_step == 1
    assert _bits(ev["logits"]) == _bits(held.forward(t.params))
    assert _bits(ev["inst_loss"]) == _bits(held.topm_loss(ev["logits"], 0.5, pos_weight="balanced", want="inst_loss")["inst_loss"])
    assert _bits(ev["metrics"]) == _bits(held.topm_metrics(ev["logits"]))
    with pytest.raises(ValueError):
        LPTrainer(p, loss_head="sinkhorn")
    # the predict driver's soft basis: per instance it sums to m
    from mllp_amd import predict
    from mllp_amd.model import GNNModel
    model = GNNModel().to("cuda")
    model.load_flat(p)
    plain = predict.predict_sparse(model, list(subset5), 2, False)
    soft = predict.predict_sparse(model, list(subset5), 2, False, 0.5)
    assert all(len(r) == 3 for r in plain) and all(len(r) == 4 for r in soft)
    for (inst, mask, rec), (_, mask2, rec2, prob) in zip(plain, soft):
        assert np.array_equal(mask, mask2) and rec == rec2                   # without the flag the output is what it was
        assert prob.dtype == np.float32 and prob.shape == (inst.n,) and abs(prob.astype(np.float64).sum() - inst.m) < 1e-3 * inst.m
