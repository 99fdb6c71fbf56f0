"""GPU: what the LP solver calls ask of their caller's scratch, and how the Python wrappers keep it.

One batch of four instances on both sides of the m = 192 threshold between "T in LDS" and "T in scratch" (m = 3, 192,
193, 200, a few columns each).  No solve is looked at: test 1 holds the five *_scratch_bytes entry points to the closed
forms of csrc/internal.h (basis_repair_words, simplex_words, pdhg_words, pdhg_scaled_side_words) at every row limit at
which the set of running instances changes; test 2 holds each wrapper to asking for its scratch once per key.
"""
import ctypes

import numpy as np
import pytest
import torch

from mllp_amd import _lib
from mllp_amd.data import LPInstance

pytestmark = pytest.mark.gpu

LDS_MAX = 192                                   # BASIS_LDS_MAX_M = SIMPLEX_LDS_MAX_M
MS, NS = (3, 192, 193, 200), (4, 5, 6, 7)
WORDS = [3 * n + 2 * m for m, n in zip(MS, NS)]     # pdhg_words: 18, 399, 404, 421
SIDE = sum(2 * n + 2 * m for m, n in zip(MS, NS))   # pdhg_scaled_side_words, of every instance


def _instance(k, m, n):
    """row i has one entry, 1.0 in column i mod n"""
    return LPInstance(f"diag{k}", np.arange(m + 1, dtype=np.int64), (np.arange(m) % n).astype(np.int32), np.ones(m), np.ones(n),
                      np.ones(m), np.zeros(n, dtype=np.int32))


@pytest.fixture(scope="module")
def batch():
    _lib.lib()
    assert torch.cuda.is_available()
    from mllp_amd.graph import LPBatch
    return LPBatch.from_instances([_instance(k, m, n) for k, (m, n) in enumerate(zip(MS, NS))])


def _bytes(b, entry, key):
    n = ctypes.c_int64(-1)
    _lib.check(getattr(_lib.lib(), entry)(b._h, key, ctypes.byref(n)))
    return n.value


def test_scratch_bytes_are_the_closed_forms(batch):
    for max_m in (0, LDS_MAX, LDS_MAX + 1, max(MS)):
        repair = 4 * sum(m * m for m in MS if LDS_MAX < m <= max_m)
        simplex = 4 * sum((m * m if m > LDS_MAX else 0) + n for m, n in zip(MS, NS) if m <= max_m)
        got = _bytes(batch, "mllp_basis_repair_scratch_bytes", max_m), _bytes(batch, "mllp_basis_simplex_scratch_bytes", max_m)
        print(f"max_m {max_m}: repair {got[0]} (closed form {repair}), simplex {got[1]} ({simplex})")
        assert got == (repair, simplex)
    for lim in (WORDS[2] - 1, WORDS[2]):        # instance 2 in scratch / in LDS
        plain = 4 * sum(w for w in WORDS if w > lim)
        got = _bytes(batch, "mllp_lp_pdhg_scratch_bytes", lim), _bytes(batch, "mllp_lp_pdhg_scaled_scratch_bytes", lim)
        print(f"max_lds_words {lim}: pdhg {got[0]} (closed form {plain}), pdhg_scaled {got[1]} ({plain + 4 * SIDE})")
        assert got == (plain, plain + 4 * SIDE)


def test_wrappers_keep_their_scratch_per_key(batch):
    b = batch
    order = torch.full((b.N,), -1, dtype=torch.int32, device="cuda")        # empty candidate lists: nothing is factorized
    start = torch.zeros(b.N, device="cuda")                                 # no basic column: code 3 at once
    calls = {"_repair_scratch": (lambda key: b.repair_basis(order=order, max_m=key, want=()), max(MS), LDS_MAX + 1,
                                 lambda key: sum(m * m for m in MS if LDS_MAX < m <= key)),
             "_simplex_scratch": (lambda key: b.simplex(start, 0, max_m=key, want=()), max(MS), LDS_MAX + 1,
                                  lambda key: sum((m * m if m > LDS_MAX else 0) + n for m, n in zip(MS, NS) if m <= key)),
             "_pdhg_scratch": (lambda key: b.pdhg(1, check_every=0, max_lds_words=key), WORDS[2] - 1, WORDS[2],
                               lambda key: sum(w for w in WORDS if w > key)),
             "_pdhg_scaled_scratch": (lambda key: b.pdhg_scaled(1, check_every=0, max_lds_words=key), WORDS[2] - 1, WORDS[2],
                                      lambda key: SIDE + sum(w for w in WORDS if w > key))}
    for attr, (call, key, other, words) in calls.items():
        call(key)
        first = getattr(b, attr)
        assert first[0] == key and first[1].numel() == words(key)
        call(key)
        again = getattr(b, attr)
        assert again[0] == key and again[1].data_ptr() == first[1].data_ptr() and again[1].numel() == words(key)
        call(other)
        asked = getattr(b, attr)
        assert asked[0] == other and asked[1].numel() == words(other) != words(key)
    torch.cuda.synchronize()
