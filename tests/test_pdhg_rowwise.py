"""GPU: the PDHG sweeps held to the fp64 rule row by row, each row on its own scale (tests/pdhg_rowwise.py).

THE BAR of the persistent calls (mllp_lp_pdhg, mllp_lp_pdhg_scaled, mllp_lp_pdhg_halpern) and of one run of mllp_lp_pdhg_wide:
every entry of x, y, dr, dc and every scalar of d_kkt within 2 x its own first-order bound of the fp64 reference, which
tests/test_pdhg_rowwise_oracle.py shows on the CPU to hold a correct fp32 execution (largest ratio 0.471) and to reject every
mutation of the list (smallest ratio 65.7).  Nothing of the bound is measured on a device.  K in {0, 1, 2} from (x0, y0) with
check_every = 0, and K = 3 for the Halpern call (w1 = w2 at k = 0: the third output is the first that tells them apart).

The wide calls keep their own bar -- the persistent call's bits -- now on the batches `tiers`, `mixed` and `many`, at
rows_per_item 64, 128, 4096 and the default, with more than 1024 instances and items behind instance 1024.

Largest ratio per call on an MI355X: see DESIGN.md 4.29 (recorded, not asserted).
"""
import numpy as np
import pytest
import torch

import pdhg_rowwise as rw
import test_basis_repair as tb
from guarded import same_bits
from test_basis_repair import LPBatch  # noqa: F401  (the fixture)
from test_pdhg_scaled import FIELDS, _bits, _host

pytestmark = pytest.mark.gpu

BATCHES = ("tiers", "mixed", "many")
SCRATCH_WORDS = 100         # 3 n + 2 m above it: `mixed` and every `tiers` instance from L = 63 (1 x L) or 33 (L x 1) in scratch
EPS_MANY = 2.0 ** -6        # the fp64 oracle's errors of `many` after 16 .. 64 iterations lie between 2^-2 and 2^-20


@pytest.fixture(scope="module")
def batches(LPBatch):
    """name -> dict(case, b: the device batch, x0, y0, ref: the references made so far)"""
    made = {}
    for name in BATCHES:
        case = getattr(rw, name)(tb.dense_case)
        c = case.dict
        made[name] = dict(case=case, b=tb._build(LPBatch, c, x1=tb._dev(c["c"]), x2=tb._dev(c["b"])), x0=tb._dev(case.x0),
                          y0=tb._dev(case.y0), ref={})
    return made


def _reference(g, call, kw, K):
    key = (call, tuple(sorted(kw.items())), K)
    if key not in g["ref"]:
        g["ref"][key] = rw.reference(g["case"], call, K, **kw)
    return g["ref"][key]


def _device(g, call, kw, K, **more):
    b, start = g["b"], dict(x0=g["x0"], y0=g["y0"], check_every=0)
    if call == "pdhg":
        return _host(b.pdhg(K, **start, **more), ("x", "y", "status", "kkt"))
    return _host(getattr(b, call)(K, **start, **kw, **more))


def _held(g, got, ref, K, what):
    """every entry within its own bound; returns the largest ratio"""
    n_inst = g["case"].K
    assert [list(s) for s in got["status"]] == [[6, K, 0, 0]] * n_inst, what
    words = got["kkt"].shape[1]
    rs = rw.ratios(got, ref, words)
    for field, v in rs.items():
        assert np.isfinite(np.asarray(got[field], np.float64)).all(), (what, field)
        worst = np.unravel_index(int(np.argmax(v)), v.shape) if v.size else ()
        assert v.max(initial=0.0) <= 1.0, f"{what}: {field}{list(worst)} is {v.max():.3g} bounds from the fp64 rule"
    return rw.worst(rs)


# ---------------------------------------------------------------------------------------------------
# the persistent calls, row by row
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("words", [None, SCRATCH_WORDS], ids=["lds", "scratch"])
@pytest.mark.parametrize("run", range(len(rw.RUNS)), ids=[f"{c}-{'-'.join(f'{k}={v}' for k, v in kw.items()) or 'defaults'}" for c, kw, _ in rw.RUNS])
@pytest.mark.parametrize("name", BATCHES)
def test_every_row_and_column_within_its_own_bound(batches, name, run, words):
    g = batches[name]
    call, kw, Ks = rw.RUNS[run]
    top = 0.0
    for K in Ks:
        got = _device(g, call, kw, K, max_lds_words=words)
        top = max(top, _held(g, got, _reference(g, call, kw, K), K, f"{name}, {call} {kw}, K = {K}, max_lds_words = {words}"))
    print(f"{name} {call} {kw} max_lds_words = {words}: largest ratio {top:.3f}")


def test_the_scratch_path_is_taken(batches):
    for name in ("tiers", "mixed"):
        case = batches[name]["case"]
        need = 3 * case.inst_n + 2 * case.inst_m
        assert (need > SCRATCH_WORDS).sum() >= (2 if name == "mixed" else 20) and (name == "mixed" or (need <= SCRATCH_WORDS).any())


# ---------------------------------------------------------------------------------------------------
# the wide calls: the persistent call's bits, and one run on the bound itself
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [0, 1, 2, 64])
@pytest.mark.parametrize("name", BATCHES)
def test_wide_rays_and_spectral_have_the_persistent_calls_bits(batches, name, K):
    g = batches[name]
    b = g["b"]
    kw = dict(x0=g["x0"], y0=g["y0"], check_every=0 if K < 64 else 16, eps=EPS_MANY)
    want = _bits(_host(b.pdhg_halpern(K, **kw)))
    for rows in (64, 128, 4096, None):
        for call, more in (("pdhg_wide", {}), ("pdhg_rays", dict(ray_eps=-1.0)), ("pdhg_spectral", dict(power_iters=0))):
            same_bits(_bits(_host(getattr(b, call)(K, rows_per_item=rows, **kw, **more))), want, f"{name}: {call}, K = {K}, rows_per_item = {rows}")


@pytest.mark.parametrize("name", BATCHES)
def test_the_wide_call_within_the_bound_on_its_own(batches, name):
    g = batches[name]
    for reflect in (True, False):
        got = _host(g["b"].pdhg_wide(2, x0=g["x0"], y0=g["y0"], check_every=0, reflect=reflect, rows_per_item=64))
        top = _held(g, got, _reference(g, "pdhg_halpern", dict(reflect=reflect), 2), 2, f"{name}, pdhg_wide, reflect = {reflect}, K = 2")
        print(f"{name} pdhg_wide reflect = {reflect}: largest ratio {top:.3f}")


@pytest.mark.parametrize("name", ["many", "mixed"])
def test_evaluating_rays_moves_no_bit_where_no_instance_stops_on_one(batches, name):
    """ray_eps = 0 evaluates both rays at every check (EvalPair, rays_eval on the tier edges) and stops only on an exact one"""
    g = batches[name]
    b = g["b"]
    kw = dict(x0=g["x0"], y0=g["y0"], check_every=16, eps=EPS_MANY)
    fields = ("x", "y", "status", "kkt")
    on = _host(b.pdhg_rays(64, ray_eps=0.0, **kw), fields + ("cert",))
    assert not np.isin(on["status"][:, 0], (4, 5)).any(), on["status"][np.isin(on["status"][:, 0], (4, 5))][:8]
    # d_cert starts as {+inf, 0, +inf, 0}: an objective that is not zero says that a check evaluated the instance's rays
    evaluated = (on["cert"][:, 1] != 0) | (on["cert"][:, 3] != 0)
    ran = on["status"][:, 1] > 16           # an instance that stops at its first check evaluates no ray
    print(f"{name}: {int(evaluated.sum())} instances evaluated their rays, {int(ran.sum())} ran past the first check, "
          f"{int(np.isfinite(on['cert'][:, [0, 2]]).any(1).sum())} with a finite quality")
    assert ran.any() and evaluated[ran].all(), np.flatnonzero(ran & ~evaluated)[:8]
    on.pop("cert")
    same_bits(_bits(on), _bits(_host(b.pdhg_rays(64, ray_eps=-1.0, **kw), fields)), f"{name}: ray_eps = 0 against ray_eps < 0")


@pytest.mark.parametrize("rounds", [1, 2])
@pytest.mark.parametrize("name", ["tiers", "mixed"])
def test_the_power_iteration_within_its_bound(batches, name, rounds):
    """d_norm[0] against the fp64 power iteration from the hash start, with its propagated bound: ScaledProd under the walks.
    What this sees is measured on the CPU (test_pdhg_rowwise_oracle.test_what_the_power_iteration_catches): after ONE round a
    dropped last term of any row or column of `tiers`, after two no longer that of a 1 x L row from L = 1023 on, and in
    `mixed`, whose estimate is one number for 193 x 2100 entries, only a term of a short row"""
    g = batches[name]
    ref = rw.power(rw.Ref(), g["case"], rounds)
    res = g["b"].pdhg_spectral(0, x0=g["x0"], y0=g["y0"], check_every=0, power_iters=rounds)
    torch.cuda.synchronize()
    got = res.norm.cpu().numpy()[:, 0]
    r = rw.ratio(got, ref)
    print(f"{name}: sigma_est after {rounds} round(s), largest ratio {r.max():.3f}; lane-order fp32 {rw.ratio(rw.power(rw.Lane(), g['case'], rounds), ref).max():.3f}")
    assert (got > 0).all() and r.max() <= 1.0, (name, int(r.argmax()), r.max())


# ---------------------------------------------------------------------------------------------------
# many: more than 1024 instances
# ---------------------------------------------------------------------------------------------------
def test_many_decisions_are_the_fp64_oracles(batches):
    """code, iterations and restarts of every instance whose fp64 run keeps every comparison at least 2^-7 (relative) from its
    threshold, as in the guarded tests of the single calls; the others -- 1.2 % -- are left out of this comparison only"""
    import pdhg_halpern_oracle as ph
    g = batches["many"]
    case, c = g["case"], g["case"].dict
    status, margin = [], []
    for k in range(case.K):
        r, s = slice(c["ptr_m"][k], c["ptr_m"][k + 1]), slice(c["ptr_n"][k], c["ptr_n"][k + 1])
        o = ph.solve(case.A[r, s], case.b[r], case.c[s], 64, check_every=16, eps=EPS_MANY, x0=case.x0[s], y0=case.y0[r])
        status.append(o["status"])
        margin.append(o["margin"])
    status, keep = np.array(status), np.array(margin) >= 2.0 ** -7
    print(f"many: {int((~keep).sum())} of {case.K} instances within 2^-7 of a decision; codes {np.bincount(status[:, 0])}")
    assert (~keep).mean() <= 0.05
    got = _host(g["b"].pdhg_halpern(64, x0=g["x0"], y0=g["y0"], check_every=16, eps=EPS_MANY), ("status",))["status"]
    bad = np.flatnonzero(keep & (got[:, :3] != status[:, :3]).any(1))
    assert bad.size == 0, (bad[:8], got[bad[:8]], status[bad[:8]])


def test_many_decisions_continuation_and_the_instance_behind_1024(batches, LPBatch):
    g = batches["many"]
    b, case = g["b"], g["case"]
    kw = dict(x0=g["x0"], y0=g["y0"], check_every=16, eps=EPS_MANY)
    want = _host(b.pdhg_halpern(64, **kw))
    codes = want["status"][:, 0]
    full = (case.inst_m > 0) & (case.inst_n > 0)
    assert (codes[full] == 0).sum() >= 50 and (codes[full] == 6).sum() >= 50, np.bincount(codes[full])     # some stop, others do not
    assert len(set(want["status"][codes == 0][:, 1])) >= 3 and codes[rw.MANY_BIG] == 6                       # ... at different checks
    for rows in (64, None):
        same_bits(_bits(_host(b.pdhg_wide(64, rows_per_item=rows, **kw))), _bits(want), f"many: K = 64, rows_per_item = {rows}")
    res = b.pdhg_wide(64, poll_every=32, **kw)
    assert res.calls == 2
    same_bits(_bits(_host(res)), _bits(want), "many: (0, 32) then (32, 64) against (0, 64)")
    # the instance behind 1024, alone
    k, c = rw.MANY_BIG, case.dict
    s, r = slice(c["ptr_n"][k], c["ptr_n"][k + 1]), slice(c["ptr_m"][k], c["ptr_m"][k + 1])
    one = tb.dense_case([rw.many_matrix(k)], 0)
    alone = tb._build(LPBatch, one, x1=tb._dev(case.c[s]), x2=tb._dev(case.b[r]))
    solo = _host(alone.pdhg_wide(64, x0=tb._dev(case.x0[s]), y0=tb._dev(case.y0[r]), check_every=16, eps=EPS_MANY))
    inside = dict(x=want["x"][s], y=want["y"][r], status=want["status"][k], kkt=want["kkt"][k], dr=want["dr"][r], dc=want["dc"][s])
    assert set(inside) == set(FIELDS)
    same_bits(_bits(solo), _bits(inside), "many: instance 1030 alone against its part of the batch")
