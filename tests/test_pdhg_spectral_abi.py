"""CPU: the C ABI of mllp_lp_pdhg_spectral without a GPU -- the three symbols are exported and bound, the limits answer, the
scratch has the header's closed form, every refusal of mllp_lp_pdhg_rays is refused here in that call's words under this call's
name, power_iters is held to 0 .. limits[4], the start may not lie on d_norm, and the header says what the call is.  Non-null
dummies stand for the graph and the device buffers: a refused call dereferences no pointer (the stand-in for a graph of sizes
alone is tests/test_pdhg_rays_oracle.py's).  The device is held to the oracle by tests/test_pdhg_spectral.py."""
import ctypes

from mllp_amd import _lib
from test_pdhg_rays_oracle import ORDER as RAYS
from test_pdhg_rays_oracle import _sizes

EPS = 2.0 ** -10
NEW = ("mllp_lp_pdhg_spectral_limits", "mllp_lp_pdhg_spectral_scratch_bytes", "mllp_lp_pdhg_spectral")
ORDER = ("g", "x1", "x2", "x0", "y0", "iter_begin", "iter_end", "check_every", "eps", "step", "beta", "ruiz", "pc", "pw", "span", "reflect",
         "ray_eps", "power", "rows", "x", "y", "dr", "dc", "ray_x", "ray_y", "status", "kkt", "cert", "norm", "scratch", "stream")


def _ok(p):
    return dict(g=p, x1=p, x2=p, x0=None, y0=None, iter_begin=0, iter_end=10, check_every=64, eps=EPS, step=0.9, beta=0.5, ruiz=10, pc=1, pw=1,
                span=16.0, reflect=1, ray_eps=-1.0, power=40, rows=0, x=p, y=p, dr=None, dc=None, ray_x=None, ray_y=None, status=p, kkt=None,
                cert=None, norm=None, scratch=None, stream=None)


def test_the_new_symbols_are_exported_and_bound():
    L = _lib.lib()
    header = open(_lib.HEADER_PATH).read()
    for name in NEW:
        assert name in _lib._PROTOTYPES and hasattr(L, name) and f"int {name}(" in header, name
    spec, rays = _lib._PROTOTYPES["mllp_lp_pdhg_spectral"][1], _lib._PROTOTYPES["mllp_lp_pdhg_rays"][1]
    assert len(spec) == len(ORDER) == len(rays) + 2
    assert [t for k, t in zip(ORDER, spec) if k in RAYS] == rays            # the rays call's arguments in that call's order
    at = dict(zip(ORDER, spec))
    assert at["power"] is ctypes.c_int64 and at["norm"] is ctypes.c_void_p
    assert ORDER.index("power") == ORDER.index("ray_eps") + 1 and ORDER.index("norm") == ORDER.index("scratch") - 1
    assert _lib._PROTOTYPES["mllp_lp_pdhg_spectral_scratch_bytes"] == _lib._PROTOTYPES["mllp_lp_pdhg_rays_scratch_bytes"]
    assert L.mllp_abi_version() == 6            # added without a bump


def test_the_limits_and_the_closed_form_answer_without_a_gpu():
    L = _lib.lib()
    lim = (ctypes.c_int64 * 5)()
    assert L.mllp_lp_pdhg_spectral_limits(lim) == 0 and list(lim) == [1024, 64, 64, 4096, 1024]
    from mllp_amd.graph import LPBatch, LPPdhgRays, LPPdhgSpectral, pdhg_rays_limits, pdhg_spectral_limits
    assert pdhg_spectral_limits() == pdhg_rays_limits() + (1024,)
    assert hasattr(LPBatch, "pdhg_spectral") and issubclass(LPPdhgSpectral, LPPdhgRays)
    assert L.mllp_lp_pdhg_spectral_limits(None) == -1 and b"mllp_lp_pdhg_spectral_limits" in L.mllp_last_error()
    g, n = _sizes(M=3, N=5, n_inst=2), ctypes.c_int64(-7)
    for rows in (0, 64, 4096):
        assert L.mllp_lp_pdhg_spectral_scratch_bytes(g, rows, ctypes.byref(n)) == 0 and n.value == 4 * (29 * 2 + 6 * 5 + 5 * 3)
        assert L.mllp_lp_pdhg_rays_scratch_bytes(g, rows, ctypes.byref(n)) == 0 and n.value == 4 * (27 * 2 + 6 * 5 + 5 * 3)       # ... unchanged
    for rows in (-64, 1, 96, 4160):
        n = ctypes.c_int64(-7)
        assert L.mllp_lp_pdhg_spectral_scratch_bytes(g, rows, ctypes.byref(n)) == -1 and n.value == -7
        assert b"mllp_lp_pdhg_spectral_scratch_bytes: rows_per_item" in L.mllp_last_error()
    assert L.mllp_lp_pdhg_spectral_scratch_bytes(None, 0, ctypes.byref(n)) == -1
    assert L.mllp_lp_pdhg_spectral_scratch_bytes(g, 0, None) == -1


def test_every_refusal_carries_the_rays_calls_words_under_this_calls_name():
    L = _lib.lib()
    p = ctypes.cast((ctypes.c_float * 64)(), ctypes.c_void_p)
    ok = _ok(p)
    nan, inf = float("nan"), float("inf")
    shared = [dict(g=None), dict(x1=None), dict(x2=None), dict(x=None), dict(y=None), dict(status=None), dict(iter_begin=-1), dict(iter_end=-1),
              dict(iter_begin=11), dict(iter_begin=5, iter_end=4), dict(check_every=-1), dict(eps=nan), dict(eps=inf), dict(eps=-1.0), dict(step=nan),
              dict(step=0.0), dict(step=1.5), dict(beta=nan), dict(beta=0.0), dict(beta=1.0), dict(ruiz=-1), dict(ruiz=65), dict(span=nan), dict(span=inf),
              dict(span=0.5), dict(ray_eps=nan), dict(ray_eps=inf), dict(ray_eps=-inf), dict(rows=-64), dict(rows=1), dict(rows=96), dict(rows=4160),
              dict(rows=1 << 40), dict(ruiz=65, span=0.5), dict(beta=nan, ruiz=-1), dict(eps=nan, ray_eps=nan), dict(span=0.5, power=-1),
              dict(ray_eps=nan, power=2000)]
    for kw in shared:
        args = dict(ok, **kw)
        assert L.mllp_lp_pdhg_spectral(*[args[k] for k in ORDER]) == -1, kw
        mine = L.mllp_last_error()
        assert L.mllp_lp_pdhg_rays(*[args[k] for k in RAYS]) == -1, kw
        theirs = L.mllp_last_error()
        assert mine.startswith(b"mllp_lp_pdhg_spectral: ") and theirs.startswith(b"mllp_lp_pdhg_rays: "), (kw, mine, theirs)
        assert mine.split(b": ", 1)[1].replace(b"mllp_lp_pdhg_spectral", b"@") == theirs.split(b": ", 1)[1].replace(b"mllp_lp_pdhg_rays", b"@"), (kw, mine, theirs)
    for kw in (dict(power=-1), dict(power=1025), dict(power=1 << 40), dict(power=-(1 << 40))):
        args = dict(ok, **kw)
        assert L.mllp_lp_pdhg_spectral(*[args[k] for k in ORDER]) == -1 and b"mllp_lp_pdhg_spectral: power_iters must be in 0 .. 1024" in L.mllp_last_error(), kw
    for kw in (dict(power=0), dict(power=1), dict(power=1024)):
        args = dict(ok, x=None, **kw)           # (accepted values: the refusal is the null d_x, not power_iters)
        assert L.mllp_lp_pdhg_spectral(*[args[k] for k in ORDER]) == -1 and b"null argument" in L.mllp_last_error(), kw
    # a non-zero scratch size and no scratch; the start may not lie on the new output
    g = _sizes(M=3, N=5, n_inst=2)
    assert L.mllp_lp_pdhg_spectral(*[dict(ok, g=g)[k] for k in ORDER]) == -1
    assert b"mllp_lp_pdhg_spectral: null d_scratch (mllp_lp_pdhg_spectral_scratch_bytes is not 0)" in L.mllp_last_error()
    q = ctypes.cast((ctypes.c_float * 64)(), ctypes.c_void_p)
    for kw in (dict(x0=q, norm=q), dict(y0=q, norm=q), dict(x0=ctypes.c_void_p(q.value + 12), norm=q), dict(y0=q, cert=q), dict(x0=q, ray_x=q)):
        args = dict(ok, g=g, scratch=p, **kw)
        assert L.mllp_lp_pdhg_spectral(*[args[k] for k in ORDER]) == -1, kw
        assert b"mllp_lp_pdhg_spectral: d_x0 or d_y0 overlaps an output" in L.mllp_last_error(), kw


def test_the_python_call_refuses_power_iters_before_the_library():
    import pytest
    from mllp_amd.graph import LPBatch
    for bad in (-1, 1025):
        with pytest.raises(ValueError, match="power_iters"):
            LPBatch.pdhg_spectral(None, 10, power_iters=bad)


def test_the_header_says_what_the_call_is():
    flat = " ".join(open(_lib.HEADER_PATH).read().replace("\n *", " ").split())
    assert "mllp_lp_pdhg_spectral is under the MEMORY CONTRACT below as mllp_lp_pdhg is" in flat         # a sentence of its own
    assert "mllp_lp_pdhg_rays is under the MEMORY CONTRACT below as mllp_lp_pdhg is" in flat             # ... beside its neighbour's
    assert "which is 4 (29 n_inst + 6 N + 5 M)" in flat and "which is 4 (27 n_inst + 6 N + 5 M)" in flat
    assert "h_j = 1 + ((j 2654435761 mod 2^32) >> 9) 2^-23" in flat
    assert "With power_iters = 0 every output that mllp_lp_pdhg_rays has is that call's, bit for bit" in flat
    assert "the set-up makes 3 P + 1 more" in flat and "EXACTLY the launches of mllp_lp_pdhg_rays" in flat
    assert "sigma_est is a LOWER bound of |S|_2" in flat
