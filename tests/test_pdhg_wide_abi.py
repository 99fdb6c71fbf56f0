"""CPU: the C ABI of mllp_lp_pdhg_wide without a GPU -- the three symbols are exported and bound, the limits answer, a null
argument and every bad scalar are refused before any HIP call (non-null dummies stand for the graph and the device buffers:
a refused call dereferences no pointer), in mllp_lp_pdhg_halpern's words where that call has the same refusal, and the header
says what the call is.  The device is held to mllp_lp_pdhg_halpern's bits by tests/test_pdhg_wide.py."""
import ctypes

from mllp_amd import _lib

EPS = 2.0 ** -10
NEW = ("mllp_lp_pdhg_wide_limits", "mllp_lp_pdhg_wide_scratch_bytes", "mllp_lp_pdhg_wide")
ORDER = ("g", "x1", "x2", "x0", "y0", "iter_begin", "iter_end", "check_every", "eps", "step", "beta", "ruiz", "pc", "pw", "span", "reflect",
         "rows", "x", "y", "dr", "dc", "status", "kkt", "scratch", "stream")
HALPERN = ("g", "x1", "x2", "x0", "y0", "iter_end", "check_every", "eps", "step", "beta", "ruiz", "pc", "pw", "span", "reflect", "lds", "x", "y",
           "dr", "dc", "status", "kkt", "scratch", "stream")


def test_the_new_symbols_are_exported_and_bound():
    L = _lib.lib()
    header = open(_lib.HEADER_PATH).read()
    for name in NEW:
        assert name in _lib._PROTOTYPES and hasattr(L, name) and f"int {name}(" in header, name
    wide, halpern = _lib._PROTOTYPES["mllp_lp_pdhg_wide"][1], _lib._PROTOTYPES["mllp_lp_pdhg_halpern"][1]
    assert len(wide) == len(ORDER) == len(halpern) + 1
    # iter_begin in front of the limit; rows_per_item where max_lds_words was
    assert wide[:5] == halpern[:5] and wide[5] is ctypes.c_int64 and wide[6:] == halpern[5:]
    assert _lib._PROTOTYPES["mllp_lp_pdhg_wide_scratch_bytes"] == _lib._PROTOTYPES["mllp_lp_pdhg_halpern_scratch_bytes"]
    assert L.mllp_abi_version() == 6            # added without a bump


def test_the_limits_answer_without_a_gpu():
    lim = (ctypes.c_int64 * 4)()
    assert _lib.lib().mllp_lp_pdhg_wide_limits(lim) == 0
    assert list(lim) == [1024, 64, 64, 4096]            # include/mllp_hip.h states all four
    assert lim[2] % 64 == 0 and lim[3] % 64 == 0 and 0 < lim[2] <= lim[3]
    from mllp_amd.graph import LPBatch, LPPdhgHalpern, LPPdhgWide, pdhg_halpern_limits, pdhg_wide_limits
    assert pdhg_wide_limits() == (1024, 64, 64, 4096) and pdhg_wide_limits()[:2] == pdhg_halpern_limits()[1:]
    assert hasattr(LPBatch, "pdhg_wide") and issubclass(LPPdhgWide, LPPdhgHalpern)
    assert _lib.lib().mllp_lp_pdhg_wide_limits(None) == -1 and b"mllp_lp_pdhg_wide_limits" in _lib.lib().mllp_last_error()


def test_null_arguments_are_refused_before_any_hip_call():
    L = _lib.lib()
    z = ctypes.c_void_p(0)
    assert L.mllp_lp_pdhg_wide(z, z, z, z, z, 0, 10, 64, EPS, 0.9, 0.5, 10, 1, 1, 16.0, 1, 0, z, z, z, z, z, z, z, z) == -1
    assert b"mllp_lp_pdhg_wide:" in L.mllp_last_error() and b"null" in L.mllp_last_error()
    n = ctypes.c_int64(-7)
    assert L.mllp_lp_pdhg_wide_scratch_bytes(z, 0, ctypes.byref(n)) == -1 and n.value == -7
    assert b"mllp_lp_pdhg_wide_scratch_bytes" in L.mllp_last_error()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for missing in ("g", "x1", "x2", "x", "y", "status"):
        args = dict(dict.fromkeys(ORDER, p), x0=None, y0=None, iter_begin=0, iter_end=10, check_every=64, eps=EPS, step=0.9, beta=0.5, ruiz=10, pc=1,
                    pw=1, span=16.0, reflect=1, rows=0, stream=None, **{missing: None})
        assert L.mllp_lp_pdhg_wide(*[args[k] for k in ORDER]) == -1 and b"null argument" in L.mllp_last_error(), missing


def test_every_scalar_refusal_comes_first_and_in_the_halpern_calls_words():
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = dict(g=p, x1=p, x2=p, x0=None, y0=None, iter_begin=0, iter_end=10, check_every=64, eps=EPS, step=0.9, beta=0.5, ruiz=10, pc=1, pw=1, span=16.0,
              reflect=1, rows=0, lds=0, x=p, y=p, dr=None, dc=None, status=p, kkt=None, scratch=None, stream=None)
    nan, inf = float("nan"), float("inf")
    shared = [dict(ruiz=-1), dict(ruiz=65), dict(span=nan), dict(span=inf), dict(span=0.5), dict(span=-2.0), dict(check_every=-1), dict(eps=nan),
              dict(eps=-1.0), dict(step=0.0), dict(step=1.5), dict(beta=1.0), dict(beta=nan), dict(ruiz=65, span=0.5), dict(beta=nan, ruiz=-1), dict(x=None)]
    for kw in shared:
        args = dict(ok, **kw)
        assert L.mllp_lp_pdhg_wide(*[args[k] for k in ORDER]) == -1, kw
        mine = L.mllp_last_error()
        assert L.mllp_lp_pdhg_halpern(*[args[k] for k in HALPERN]) == -1, kw
        theirs = L.mllp_last_error()
        assert mine.startswith(b"mllp_lp_pdhg_wide: ") and mine.split(b": ", 1)[1] == theirs.split(b": ", 1)[1], (kw, mine, theirs)
    own = {b"iter_begin": [dict(iter_begin=-1), dict(iter_begin=-1, iter_end=-5)], b"iter_end": [dict(iter_end=-1), dict(iter_begin=11), dict(iter_begin=5, iter_end=4)],
           b"rows_per_item": [dict(rows=-64), dict(rows=1), dict(rows=63), dict(rows=96), dict(rows=4096 + 64), dict(rows=1 << 40)]}
    for word, cases in own.items():
        for kw in cases:
            args = dict(ok, **kw)
            assert L.mllp_lp_pdhg_wide(*[args[k] for k in ORDER]) == -1 and word in L.mllp_last_error(), (kw, L.mllp_last_error())


def test_the_header_says_what_the_call_is():
    flat = " ".join(open(_lib.HEADER_PATH).read().replace("\n *", " ").split())
    assert "mllp_lp_pdhg_wide is under the MEMORY CONTRACT below as mllp_lp_pdhg is" in flat        # a sentence of its own
    assert "mllp_lp_pdhg_halpern is under the MEMORY CONTRACT below as mllp_lp_pdhg is" in flat      # ... beside its neighbour's
    # the rule's identity
    assert ("With iter_begin = 0 the outputs d_x, d_y, d_dr, d_dc, d_status and d_kkt are mllp_lp_pdhg_halpern's at max_iters = iter_end, "
            "bit for bit, for every instance, every rows_per_item and every batch composition") in flat
    assert "the calls (0, K1) then (K1, K2) give the bits of the call (0, K2), for any K1" in flat
    assert "gets code 9, STALE STATE" in flat and "which is 4 (21 n_inst + 6 N + 5 M)" in flat
    assert "No kernel waits on another workgroup" in flat and "No float atomics" in flat
