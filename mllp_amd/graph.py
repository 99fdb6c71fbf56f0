"""HBM-resident batch of LP instances (block-diagonal constraint matrix, both orientations).

`LPBatch` replaces the reference's per-step graph build
(`build_graph_from_weights_sets`, reference linear_program_methods.py:89-103) and the
`BipartiteData.__inc__` batching rule (methods.py:60-72): the batch is built once, lives in HBM as
CSR(A) + CSR(A^T) behind an opaque `mllp_graph_t*`, and every model call takes it by handle.
"""
import contextlib
import ctypes
import itertools
import math
import time
from ctypes import c_int32, c_int64, c_double, c_void_p
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .data import LPInstance


# variant 4 (a lane per row): the 16 sets of 4 lanes that read the same bank quarter in one LDS cycle -- lanes of one
# ds_read_b128 lane group ({0-3,12-15,20-27}, {4-11,16-19,28-31} and the same + 32; MI355X_MICROARCH.md, LDS) with equal
# (lane & 3), which is the rotation the kernel reads the four 16-byte pieces of an H row in
_B128_GROUPS = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
                [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
LANE_GROUPS = [[l + h for l in grp if (l & 3) == r] for h in (0, 32) for grp in _B128_GROUPS for r in range(4)]


def set_fused_grid_limit(n):
    """mllp_set_fused_grid_limit: cap the workgroups of the fused sweeps of batches created from now on (0: no limit);
    returns the previous value.  Needs no GPU."""
    prev = c_int64()
    _lib.check(_lib.lib().mllp_set_fused_grid_limit(int(n), ctypes.byref(prev)))
    return int(prev.value)


@contextlib.contextmanager
def fused_grid_limit(n):
    """Batches created inside run their fused sweeps on at most `n` workgroups (rounded down to a multiple of 8, at least
    8); the previous limit is restored on exit.  A batch keeps the grid it was created with."""
    prev = set_fused_grid_limit(n)
    try:
        yield
    finally:
        set_fused_grid_limit(prev)


def build_tiled_arrays(ptr, idx, val, n_dst, R, CB, variant=0, entry_order="joint"):
    """Re-block one CSR orientation into the tiled layout of include/mllp_hip.h (mllp_graph_attach_tiled): row tiles
    of R rows x column blocks of CB columns, rows of a (tile, block) ordered by their entry count, entries of the
    four rows of a ds_read_b128 lane group ordered jointly over (column mod 4).  Variant 4 (destination-major
    backward, one LANE per row) keeps the rows of a tile in their own order and stores the entries of every 64-row
    chunk of a (tile, block) by step: entry j of the rows that have one, in row order -- at
    chunk_start + sum_l' min(len_l', j) + #{l' < l : len_l' > j} for the chunk's l-th row.  Pure torch, any device (the CPU
    tests check it against the CSR it came from).  `entry_order="perrow"` keeps the simpler per-row round-robin (used
    by the CPU test that compares the two orders).  Returns (arrays, info) or None when the matrix does not qualify."""
    dev, nnz = idx.device, int(idx.numel())
    if nnz == 0:
        return None
    n_tiles = (n_dst + R - 1) // R
    deg = (ptr[1:] - ptr[:-1]).long()
    rows = torch.repeat_interleave(torch.arange(n_dst, device=dev, dtype=torch.int32), deg)
    tile = torch.div(rows, R, rounding_mode="floor")
    blk = torch.div(idx, CB, rounding_mode="floor")
    tl = tile.long()
    lo = torch.full((n_tiles,), 2 ** 30, dtype=torch.int32, device=dev).scatter_reduce(0, tl, blk, "amin")
    hi = torch.full((n_tiles,), -1, dtype=torch.int32, device=dev).scatter_reduce(0, tl, blk, "amax")
    nbt = torch.where(hi >= 0, hi - lo + 1, torch.zeros_like(hi)).long()
    lo = torch.where(hi >= 0, lo, torch.zeros_like(lo))
    tile_blk = torch.zeros(n_tiles + 1, dtype=torch.int64, device=dev)
    tile_blk[1:] = torch.cumsum(nbt, 0)
    n_tb = int(tile_blk[-1])
    max_nbt = int(nbt.max())
    if n_tb * R >= 2 ** 31 - 1 or max_nbt > 255:
        return None
    key = (tile_blk[tl] + (blk - lo[tl]).long()) * R + (rows - tile * R).long()
    del rows, tile, tl
    counts = torch.bincount(key, minlength=n_tb * R)
    lane_fixed = int(variant) == 4                      # a lane owns a row of the tile: rows keep their order
    if lane_fixed and R % 64:
        return None
    # inside every (tile, block): rows ordered by their entry count, descending (stable)
    if lane_fixed:
        order = torch.arange(R, device=dev).expand(n_tb, R).contiguous()
    else:
        order = torch.argsort(counts.view(n_tb, R), dim=1, descending=True, stable=True)   # [n_tb, R] row of position k
    inv = torch.empty_like(order)
    inv.scatter_(1, order, torch.arange(R, device=dev).expand(n_tb, R))                    # position of row r
    sorted_counts = torch.gather(counts.view(n_tb, R), 1, order).reshape(-1)
    del counts
    ptr2 = torch.zeros(n_tb * R + 1, dtype=torch.int64, device=dev)
    ptr2[1:] = torch.cumsum(sorted_counts, 0)
    del sorted_counts
    max_run = int((ptr2[R::R] - ptr2[:-1:R]).max())     # longest (tile, block) segment (informational)
    ar = torch.arange(nnz, device=dev, dtype=torch.int64)
    is_start = torch.ones(nnz, dtype=torch.bool, device=dev)
    is_start[1:] = key[1:] != key[:-1]
    start_idx = torch.cummax(torch.where(is_start, ar, torch.zeros_like(ar)), 0)[0]
    pos_key = torch.div(key, R, rounding_mode="floor") * R + inv.reshape(-1)[key]          # (tb, sorted position)
    del key, inv, is_start
    # Order of the entries inside a (row, block) run.  A ds_read_b128 serves 16 lanes = 4 quads per LDS cycle and a
    # 64-byte H row covers a quarter of the 256-byte bank row, so four quads reading H rows with equal
    # (column mod 4) serialise (MI355X_MICROARCH.md, LDS).
    cls = ((idx - blk * CB) & 3).long()
    joint = int(variant) in (0, 1, 4) and R % 16 == 0 and entry_order != "perrow"
    if joint:
        # JOINT ordering of the four rows whose quads share a lane group ({0,3,5,6}, {1,2,4,7}, {8,11,13,14},
        # {9,10,12,15} of the 16 quads that walk positions 16 b .. 16 b + 15): at step p the four rows should
        # present four different column classes.  Greedy per step, the row that chooses first rotates with p;
        # a row takes its most numerous class that is still free (simulated: 2.05 random, 1.76 per-row
        # round-robin, 1.42 LDS cycles per step with this).
        n_run = n_tb * R
        cnt = torch.zeros(n_run * 4, dtype=torch.int32, device=dev)
        cnt.index_add_(0, pos_key * 4 + cls, torch.ones(nnz, dtype=torch.int32, device=dev))
        base = torch.cumsum(cnt, 0, dtype=torch.int64) - cnt              # start of (run, class) in canonical order
        order_c = torch.argsort(pos_key * 4 + cls, stable=True)            # canonical: (run, class, column)
        if lane_fixed:  # a lane per row: the lanes of one ds_read_b128 lane group that read with the same rotation
            QG, W = torch.tensor(LANE_GROUPS, device=dev), 64
        else:
            QG, W = torch.tensor([[0, 3, 5, 6], [1, 2, 4, 7], [8, 11, 13, 14], [9, 10, 12, 15]], device=dev), 16
        c = cnt.view(n_tb, R // W, W, 4)[:, :, QG].reshape(-1, 4, 4).contiguous()            # [G, slot, class]
        bs = base.view(n_tb, R // W, W, 4)[:, :, QG].reshape(-1, 4, 4).contiguous()
        p2 = ptr2[:-1].view(n_tb, R // W, W)[:, :, QG].reshape(-1, 4).contiguous()           # first slot of each run
        del cnt, base
        c0 = c.clone()
        rem = c.sum(-1)
        maxlen = int(rem.max())
        joint = maxlen <= 512                                             # pathological rows: per-row ordering below
    if joint:
        dest = torch.empty(nnz, dtype=torch.int64, device=dev)
        for p in range(maxlen):
            used = torch.zeros((c.shape[0], 4), dtype=torch.bool, device=dev)
            for j in range(4):
                i = (j + p) % 4
                ci = c[:, i, :]
                act = rem[:, i] > 0
                avail = (ci > 0) & ~used
                pick = torch.where(avail.any(1), torch.where(avail, ci, torch.full_like(ci, -1)).argmax(1), ci.argmax(1))
                pk = pick[:, None]
                occ = (c0[:, i, :].gather(1, pk) - ci.gather(1, pk)).squeeze(1).long()
                sel = act.nonzero().squeeze(1)
                src = order_c[(bs[:, i, :].gather(1, pk).squeeze(1) + occ)[sel]]
                dest[src] = p if lane_fixed else p2[sel, i] + p          # lane_fixed: the step, placed below
                ci.scatter_add_(1, pk, -act.to(ci.dtype)[:, None])
                rem[:, i] -= act.to(rem.dtype)
                used.scatter_(1, pk, used.gather(1, pk) | act[:, None])
        del c, c0, bs, p2, rem, order_c, used, cls, start_idx
        if lane_fixed:
            step = dest
        del ar
    else:
        # per-row ordering: round-robin over the classes, starting at the slot of the row's quad in its lane group
        g = ((pos_key & 7) >> 1)
        rank = torch.zeros(nnz, dtype=torch.int64, device=dev)
        for cc in range(4):
            ind = (cls == cc).long()
            ex = torch.cumsum(ind, 0) - ind                      # entries of class cc before this one
            rank = torch.where(cls == cc, ex - ex[start_idx], rank)
            del ind, ex
        k2 = rank * 4 + ((cls - g) & 3)
        del rank, cls, g
        K = int(k2.max()) + 1
        ordr = torch.argsort(start_idx * K + k2)                 # runs stay contiguous; inside a run by k2
        del k2
        new_off = torch.empty(nnz, dtype=torch.int64, device=dev)
        new_off[ordr] = ar
        del ordr
        dest = ptr2[pos_key] + (new_off - start_idx)
        if lane_fixed:
            step = new_off - start_idx
        del ar, start_idx, new_off
    if lane_fixed:
        # memory order = (tile-block, 64-row chunk, step inside the row, row): only existing entries, so the position of
        # an entry is its rank under that key
        K = int(step.max()) + 1
        ordr = torch.argsort((torch.div(pos_key, 64, rounding_mode="floor") * K + step) * 64 + (pos_key & 63))
        dest = torch.empty_like(ordr)
        dest[ordr] = torch.arange(nnz, device=dev, dtype=torch.int64)
        del step, ordr
    del pos_key
    # one padding entry behind the last: an empty (tile, block) at the very end still has a readable "first entry"
    ent = torch.zeros((nnz + 1, 2), dtype=torch.int32, device=dev)
    # byte offset of the column's staged item inside the block: 64-byte feature rows, 160-byte backward records
    # (variant 2) or 4-byte scalars (variant 3)
    ent[dest, 0] = (idx - blk * CB) * {0: 64, 1: 64, 2: 160, 3: 4, 4: 64}[int(variant)]
    ent[dest, 1] = val.view(torch.int32)
    del dest, blk
    perm = order.reshape(-1).to(torch.int32).contiguous()
    del order
    owner = torch.repeat_interleave(torch.arange(n_tiles, device=dev), nbt)
    blk_id = (lo[owner].long() + (torch.arange(n_tb, device=dev) - tile_blk[owner])).to(torch.int32)
    keep = dict(tile_blk=tile_blk.to(torch.int32).contiguous(), blk_id=blk_id.contiguous(),
                ptr2=ptr2.to(torch.int32).contiguous(), perm=perm, ent=ent.contiguous())
    info = dict(rows_per_tile=R, cols_per_block=CB, n_tiles=n_tiles, n_tb=n_tb, max_nbt=max_nbt, max_run=max_run,
                staged_bytes=n_tb * CB * 64, gathered_bytes=nnz * 64)
    return keep, info


# ---- what the wrappers below share: arguments in, buffers out ----------------------------------------------------------------
def _parse_want(who, want, names, saying, allow_empty=False, together=()):
    """The `want=` of a call as a tuple (a lone name stands for itself).  ValueError "<who>: <saying> (got ...)" unless it
    names only `names` -- at least one of them unless `allow_empty`, and all or none of `together`."""
    want = (want,) if isinstance(want, str) else tuple(want)
    if [w for w in want if w not in names] or not (want or allow_empty) or (together and len({w in want for w in together}) > 1):
        raise ValueError(f"{who}: {saying} (got {want!r})")
    return want


def _checked(who, what, t, n, dtype=torch.float32):
    """`t`, the argument `what` of `who`: a contiguous cuda tensor of n elements of `dtype`, or ValueError"""
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous() and t.numel() == n):
        raise ValueError(f"{who}: {what} must be a contiguous cuda {str(dtype).split('.')[1]} tensor of {n} elements")
    return t


def _out(n, dtype, dev, wanted=True):
    """An output buffer of n elements, None when not wanted.  At least one element: an empty torch tensor has a null
    pointer, which the library refuses or reads as "not wanted"."""
    return torch.empty(max(n, 1), dtype=dtype, device=dev) if wanted else None


def _pad(t):
    """`t` as an input of the library: one zero where it is empty (never a null pointer)"""
    return t if t.numel() else torch.zeros(1, dtype=t.dtype, device=t.device)


def _cut(t, *shape):
    """What the caller gets of the buffer `_out` made: its first elements, in `shape`; None for None"""
    if t is None:
        return None
    return t[:shape[0]] if len(shape) == 1 else t[:math.prod(shape)].view(shape)


class LPBatch:
    _tokens = itertools.count(1)
    # whole-model kernels: 0 = by size (fused latency-regime kernels below 32 M nonzeros, generic / LDS-tiled sweeps
    # above), 1 = always generic / tiled, 2 = always fused (mllp_graph_set_path).  Tests set the class default.
    default_path = 0

    def __init__(self, handle, M, N, nnz, n_inst, inst_m, inst_n, x1, x2, labels, names=None):
        self._h = handle
        self.token = next(LPBatch._tokens)     # never reused, unlike id(): keys per-batch caches (LPTrainer._plans)
        self.M, self.N, self.nnz, self.n_inst = int(M), int(N), int(nnz), int(n_inst)
        self.inst_m = [int(v) for v in inst_m]
        self.inst_n = [int(v) for v in inst_n]
        self.x1, self.x2, self.labels = x1, x2, labels      # cuda fp32: coefs (N,), rhs (M,), basis (N,)
        self.names = list(names) if names is not None else [f"inst{i}" for i in range(n_inst)]
        self._ws = None
        self._n_off = np.concatenate([[0], np.cumsum(self.inst_n)]).astype(np.int64)
        self._tiled = {}              # {(transpose, variant): arrays the library borrows, or None when it owns them}
        self._streams = None          # the streamed copies of the training step (LPTrainer._plan: enable_stream_step)
        self.tiled_build_s = 0.0      # seconds spent building LDS-tiled copies
        self.stream_build_s = 0.0     # ... streamed copies
        self.path = 0                 # the whole-model path last given to mllp_graph_set_path
        if LPBatch.default_path:
            self.set_path(LPBatch.default_path)

    def invalidate_inputs(self):
        """x1 / x2 / labels were changed in place: the fused path re-makes its renumbered copies on the next call."""
        _lib.check(_lib.lib().mllp_graph_invalidate_inputs(self._h))
        self._in_versions = None
        return self

    def _check_inputs(self):
        """torch counts in-place writes per tensor (`_version`): a change since the last whole-model call invalidates the
        library's renumbered copies (include/mllp_hip.h, input contract), so `batch.x1.mul_(2)` just works."""
        v = (self.x1._version, self.x2._version, self.labels._version, self.x1.data_ptr(), self.x2.data_ptr(),
             self.labels.data_ptr())
        if getattr(self, "_in_versions", None) != v:
            if getattr(self, "_in_versions", None) is not None:
                _lib.check(_lib.lib().mllp_graph_invalidate_inputs(self._h))
            self._in_versions = v

    def set_values(self, values):
        """New matrix values on the same sparsity pattern (mllp_graph_set_values): `values` is a cuda float32 tensor of
        nnz elements in the CSR order of A (`export(2)`, the order of `backward_inputs`' dvalues).  Every array of the batch
        that holds values -- both orientations, the fused path's copies, every streamed and device-built tiled copy -- is
        refreshed on the device; a backward needs a new forward afterwards.  The first call (and the first after a copy
        was built) allocates the position maps and synchronises; later calls only launch."""
        _checked("set_values", "values", values, self.nnz)
        _lib.check(_lib.lib().mllp_graph_set_values(self._h, _lib.ptr(values) if self.nnz else _lib.ptr(self.x1),
                                                    _lib.current_stream()))
        self._fwd_token = getattr(self, "_fwd_token", 0) + 1      # (model.py: a pending autograd backward must not run)
        return self

    def set_values_bytes(self):
        """Bytes of the position maps that `set_values` keeps for the copies attached now (mllp_graph_set_values_bytes)."""
        n = c_int64()
        _lib.check(_lib.lib().mllp_graph_set_values_bytes(self._h, ctypes.byref(n)))
        return n.value

    def rescale(self, row_scale=None, col_scale=None):
        """a_ij <- (r_i a_ij) s_j, x2 <- x2 r, x1 <- x1 s, in place (mllp_graph_scale_values): for positive scales the
        same LP in other units, with the same optimal basis -- the label-preserving augmentation of this model's data.
        `row_scale` [M] / `col_scale` [N] are cuda float32 tensors; None = ones.  `normalize` brings the rescaled batch
        back to the normalization the weights were trained on (it cancels a positive row scaling, a column scaling stays)."""
        for t, n, what in ((row_scale, self.M, "row_scale"), (col_scale, self.N, "col_scale")):
            if t is not None:
                _checked("rescale", what, t, n)
        _lib.check(_lib.lib().mllp_graph_scale_values(self._h, _lib.ptr(row_scale), _lib.ptr(col_scale),
                                                      _lib.current_stream()))
        self._fwd_token = getattr(self, "_fwd_token", 0) + 1
        if row_scale is not None:
            self.x2.mul_(row_scale.reshape(-1))
        if col_scale is not None:
            self.x1.mul_(col_scale.reshape(-1))
        return self.invalidate_inputs()

    def normalize(self, rhs_cap=5.0, compute_only=False):
        """The reference's normalization of the batch, in place on the device (mllp_graph_normalize): every constraint row
        to unit 2-norm, or to right-hand side +rhs_cap where unit norm would leave |b_i| above it (signed: a negative b_i
        flips the row), every instance's objective to unit 2-norm; `self.x1`, `self.x2` and every value-holding array of
        the batch are rewritten, and a backward needs a new forward afterwards.  rhs_cap <= 0, inf or nan: no cap.
        Returns (row_scale [M], obj_scale [n_inst]), the applied factors, as cuda tensors.  compute_only=True returns the
        factors and writes nothing else.  The first call allocates and synchronises; later calls only launch."""
        dev = self.x1.device
        row_scale = torch.empty(self.M, dtype=torch.float32, device=dev)
        obj_scale = torch.empty(self.n_inst, dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().mllp_graph_normalize(self._h, _lib.ptr(self.x1), _lib.ptr(self.x2), float(rhs_cap),
                                                   1 if compute_only else 0, _lib.ptr(row_scale), _lib.ptr(obj_scale),
                                                   _lib.current_stream()))
        if not compute_only:        # (the library has invalidated its copies of x1 / x2 itself: _in_versions stays)
            self._fwd_token = getattr(self, "_fwd_token", 0) + 1
        return row_scale, obj_scale

    def plant_basis(self, pivot, xstar, ystar, slack, dominance=1.25, floor=0.25):
        """Make the batch an LP whose unique optimal basis is the set of pivot columns, in place on the device
        (mllp_graph_plant_basis): `pivot` [M] int32 names one column of every row (global id; the entry must exist, no
        column twice), its entry becomes copysign(dominance * off_i + floor, old) with off_i the row's absolute sum over the
        other basic columns, and `self.x2` = b, `self.x1` = c, `self.labels` = the basis mask are rewritten so that
        (xstar on the basis, ystar) is primal and dual feasible with reduced costs `slack` off the basis.  xstar [N],
        ystar [M], slack [N]: cuda float32; positive xstar and slack give a unique optimum, nothing checks them
        (`certificate` reports).  Every value-holding array of the batch is refreshed as by `set_values`; a backward needs
        a new forward.  A setup call: validates the pivots on the device and synchronises; a bad pivot raises MllpError
        with nothing written."""
        _checked("plant_basis", "pivot", pivot, self.M, torch.int32)
        for t, n, what in ((xstar, self.N, "xstar"), (ystar, self.M, "ystar"), (slack, self.N, "slack")):
            _checked("plant_basis", what, t, n)
        args = [_pad(t) for t in (pivot, xstar, ystar, slack, self.x1, self.x2, self._labels)]
        _lib.check(_lib.lib().mllp_graph_plant_basis(self._h, *[_lib.ptr(a) for a in args[:4]], float(dominance), float(floor),
                                                     *[_lib.ptr(a) for a in args[4:]], _lib.current_stream()))
        self._fwd_token = getattr(self, "_fwd_token", 0) + 1      # (as set_values; the library invalidated its input copies)
        self._balanced_pw = None                                  # (the labels were written behind torch's version counter)
        return self

    def certificate(self, x, y, basis=None, out=None):
        """[n_inst, 6] cuda float32: what (x [N], y [M], basis [N], default `self.labels`) is worth as an optimal solution
        of every instance as the batch stores it now (mllp_lp_certificate): max |Ax - b|, min x over the basis, max |x| off
        it, min reduced cost c - A'y off the basis, max |reduced cost| on it, the basis' size.  An optimal basic solution
        has 0, >= 0, 0, >= 0, 0, m up to rounding; empty sets give +inf (min) and 0 (max).  No sync, no allocation in the
        library."""
        basis = self._labels if basis is None else basis
        for t, n, what in ((x, self.N, "x"), (y, self.M, "y"), (basis, self.N, "basis")):
            _checked("certificate", what, t, n)
        dev = self.x1.device
        if getattr(self, "_cert_scratch", None) is None:
            n = c_int64()
            _lib.check(_lib.lib().mllp_lp_certificate_scratch_bytes(self._h, ctypes.byref(n)))
            self._cert_scratch = torch.empty(n.value // 4, device=dev, dtype=torch.float32)
        if out is None:
            out = _cut(_out(self.n_inst * 6, torch.float32, dev), self.n_inst, 6)
        _lib.check(_lib.lib().mllp_lp_certificate(self._h, *[_lib.ptr(_pad(t)) for t in (self.x1, self.x2, x, y, basis)],
                                                  _lib.ptr(out), _lib.ptr(self._cert_scratch), _lib.current_stream()))
        return out

    @staticmethod
    def normalize_row_tier(row_nnz):
        """Which reduction of `normalize` a row of `row_nnz` nonzeros gets: 0 = 16-lane group, 1 = wavefront, 2 = workgroup."""
        t = ctypes.c_int()
        _lib.check(_lib.lib().mllp_normalize_row_tier(int(row_nnz), ctypes.byref(t)))
        return t.value

    def set_path(self, path):
        """0 = by size, 1 = generic / LDS-tiled sweeps, 2 = fused latency-regime kernels (whole-model calls only)."""
        _lib.check(_lib.lib().mllp_graph_set_path(self._h, int(path)))
        self.path = int(path)
        self._folded = None
        return self

    # ---- construction ------------------------------------------------------------------------
    @staticmethod
    def from_instances(instances: Sequence[LPInstance], device="cuda", tier_wave=0, tier_block=0) -> "LPBatch":
        L = _lib.lib()
        inst_m = np.array([i.m for i in instances], dtype=np.int64)
        inst_n = np.array([i.n for i in instances], dtype=np.int64)
        indptr = np.ascontiguousarray(np.concatenate([i.indptr.astype(np.int64) for i in instances]))
        indices = np.ascontiguousarray(np.concatenate([i.indices.astype(np.int32) for i in instances]))
        values = np.ascontiguousarray(np.concatenate([i.values.astype(np.float64) for i in instances]))
        if indices.size == 0:
            indices, values = np.zeros(1, np.int32), np.zeros(1, np.float64)
        torch.cuda.init()
        h = c_void_p()
        _lib.check(L.mllp_graph_create_host(len(instances), _lib.np_ptr(inst_m, c_int64), _lib.np_ptr(inst_n, c_int64),
                                            _lib.np_ptr(indptr, c_int64), _lib.np_ptr(indices, c_int32),
                                            _lib.np_ptr(values, c_double), tier_wave, tier_block, ctypes.byref(h)))
        # fp32 casts as reference methods.py:90-91,100
        x1 = torch.tensor(np.concatenate([i.coefs for i in instances]), dtype=torch.float32, device=device)
        x2 = torch.tensor(np.concatenate([i.rhs for i in instances]), dtype=torch.float32, device=device)
        y = torch.tensor(np.concatenate([i.basis for i in instances]), dtype=torch.float32, device=device)
        return LPBatch(h, inst_m.sum(), inst_n.sum(), sum(i.nnz for i in instances), len(instances), inst_m, inst_n,
                       x1, x2, y, [i.name for i in instances])

    @staticmethod
    def from_device_csr(inst_m, inst_n, csr_ptr, csr_idx, csr_val, x1, x2, labels, tier_wave=0, tier_block=0,
                        names=None, transpose="device") -> "LPBatch":
        """Batch from device CSR arrays in global ids (int32 ptr/idx, fp32 values).  The transposed orientation is
        built by the library (`mllp_csr_transpose_device`: counting, scatter, per-column ordering) -- or, with
        transpose="torch", by one stable device sort (the reference the tests compare with)."""
        L = _lib.lib()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        M, N, nnz = int(sum(inst_m)), int(sum(inst_n)), int(csr_idx.numel())
        if transpose == "torch":      # reference for the tests: one stable sort by column
            rows = torch.repeat_interleave(torch.arange(M, device=csr_idx.device, dtype=torch.int32),
                                           (csr_ptr[1:] - csr_ptr[:-1]).long())
            order = torch.sort(csr_idx.long(), stable=True)[1]        # stable: row ids ascend inside a column
            csc_idx = rows[order].contiguous()
            csc_val = csr_val[order].contiguous()
            counts = torch.bincount(csr_idx.long(), minlength=N)
            csc_ptr = torch.zeros(N + 1, dtype=torch.int32, device=csr_idx.device)
            csc_ptr[1:] = torch.cumsum(counts, 0).to(torch.int32)
            del rows, order, counts
        else:                         # the library's transposition kernels (transpose.hip)
            dev = csr_idx.device
            csc_ptr = torch.empty(N + 1, dtype=torch.int32, device=dev)
            csc_idx = torch.empty(nnz, dtype=torch.int32, device=dev)
            csc_val = torch.empty(nnz, dtype=torch.float32, device=dev)
            _lib.check(L.mllp_csr_transpose_device(M, N, nnz, _lib.ptr(csr_ptr), _lib.ptr(csr_idx), _lib.ptr(csr_val),
                                                   _lib.ptr(csc_ptr), _lib.ptr(csc_idx), _lib.ptr(csc_val),
                                                   _lib.current_stream()))
        pm = np.concatenate([[0], np.cumsum(inst_m)]).astype(np.int64)
        pn = np.concatenate([[0], np.cumsum(inst_n)]).astype(np.int64)
        h = c_void_p()
        torch.cuda.synchronize()
        _lib.check(L.mllp_graph_create_device(len(inst_m), _lib.np_ptr(pm, c_int64), _lib.np_ptr(pn, c_int64), nnz,
                                              _lib.ptr(csr_ptr), _lib.ptr(csr_idx), _lib.ptr(csr_val),
                                              _lib.ptr(csc_ptr), _lib.ptr(csc_idx), _lib.ptr(csc_val),
                                              tier_wave, tier_block, _lib.current_stream(), ctypes.byref(h)))
        torch.cuda.synchronize()
        b = LPBatch(h, M, N, nnz, len(inst_m), inst_m, inst_n, x1, x2, labels, names)
        b.graph_build_s = time.perf_counter() - t0     # transposition (one device sort) + row tiers (mllp_graph_create_device)
        return b

    # ---- LDS-tiled copies (throughput regime) -----------------------------------------------------
    def _device_orientation(self, transpose):
        """(ptr, idx, val) of one orientation as cuda tensors (downloaded from the graph once)."""
        base = 3 if transpose else 0
        dev = self.x1.device
        return (torch.from_numpy(self.export(base)).to(dev), torch.from_numpy(self.export(base + 1)).to(dev),
                torch.from_numpy(self.export(base + 2)).to(dev))

    def enable_tiled(self, transpose=False, arrays=None, variant=0, builder="device"):
        """Build and attach the LDS-tiled copy of A (transpose=False) or A^T.  Returns a dict with the
        geometry, or None when the matrix does not qualify (index range).
        builder="device": the library's HIP builder (mllp_graph_build_tiled, library-owned arrays);
        builder="torch" (or explicit `arrays`): the torch reference builder `build_tiled_arrays`, whose arrays the
        library borrows.  `self.tiled_build_s` accumulates the seconds spent building."""
        L = _lib.lib()
        R, CB = self._tiled_geometry(variant)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if arrays is None and builder == "device":
            if self.nnz == 0:
                return None                      # (nothing to re-block: the generic sweeps handle the empty matrix)
            rc = L.mllp_graph_build_tiled(self._h, int(transpose), int(variant), _lib.current_stream())
            torch.cuda.synchronize()
            self.tiled_build_s += time.perf_counter() - t0
            if rc == _lib.MLLP_ERANGE:
                return None
            _lib.check(rc)
            self._tiled[(bool(transpose), int(variant))] = None      # library-owned: nothing to keep alive here
            d = (c_int64 * 5)()
            _lib.check(L.mllp_graph_tiled_info(self._h, int(transpose), int(variant), d))
            return dict(rows_per_tile=R, cols_per_block=CB, n_tiles=int(d[0]), n_tb=int(d[1]), max_run=int(d[4]),
                        staged_bytes=int(d[1]) * CB * 64, gathered_bytes=self.nnz * 64, builder="device")
        assert builder in ("device", "torch")
        ptr, idx, val = arrays if arrays is not None else self._device_orientation(transpose)
        n_dst = self.N if transpose else self.M
        built = build_tiled_arrays(ptr, idx, val, n_dst, R, CB, variant)
        torch.cuda.synchronize()
        self.tiled_build_s += time.perf_counter() - t0
        if built is None:
            return None
        keep, info = built
        n_tiles, n_tb, max_nbt = info["n_tiles"], info["n_tb"], info.pop("max_nbt")
        torch.cuda.synchronize()
        _lib.check(L.mllp_graph_attach_tiled(self._h, int(transpose), int(variant), n_tiles, n_tb, max_nbt,
                                             _lib.ptr(keep["tile_blk"]),
                                             _lib.ptr(keep["blk_id"]), _lib.ptr(keep["ptr2"]), _lib.ptr(keep["perm"]),
                                             _lib.ptr(keep["ent"])))
        self._tiled[(bool(transpose), int(variant))] = keep          # the library borrows these arrays
        info["builder"] = "torch"
        return info

    @staticmethod
    def _tiled_geometry(variant):
        """(rows per tile, columns per block) of an LDS-tiled variant (mllp_tiled_geometry)."""
        R, CB, CAP = c_int32(), c_int32(), c_int32()
        _lib.check(_lib.lib().mllp_tiled_geometry(int(variant), ctypes.byref(R), ctypes.byref(CB), ctypes.byref(CAP)))
        return R.value, CB.value

    def export_tiled(self, transpose=False, variant=0):
        """The attached tiled copy as torch int32 device tensors (tile_blk, blk_id, ptr2, perm, ent [nnz + 1, 2]) (tests)."""
        L = _lib.lib()
        R = self._tiled_geometry(variant)[0]
        d = (c_int64 * 5)()
        _lib.check(L.mllp_graph_tiled_info(self._h, int(transpose), int(variant), d))
        n_tiles, n_tb = int(d[0]), int(d[1])
        sizes = [n_tiles + 1, n_tb, n_tb * R + 1, n_tb * R, (self.nnz + 1) * 2]
        out = []
        for which, n in enumerate(sizes):
            t = torch.empty(n, dtype=torch.int32, device=self.x1.device)
            _lib.check(L.mllp_graph_export_tiled(self._h, int(transpose), int(variant), which, _lib.ptr(t), n,
                                                 _lib.current_stream()))
            out.append(t)
        torch.cuda.synchronize()
        out[4] = out[4].view(-1, 2)
        return dict(zip(["tile_blk", "blk_id", "ptr2", "perm", "ent"], out))

    # ---- streamed SpMM copy (library-owned; stream_layout.h) -----------------------------------------
    # (geometry 0 of the streamed copies below)
    def build_spmm_copy(self, transpose=False, where="device"):
        """Build the streamed copy of A (or A^T) that `spmm` then runs on: `where` = "device" (HIP builder) or
        "host" (reference builder, same bytes).  Returns the info dict of `spmm_copy_info`."""
        self.build_stream_copy(transpose, self.GEOM_SPMM, where)
        return self.spmm_copy_info(transpose)

    def drop_spmm_copy(self, transpose=False):
        self.drop_stream_copy(transpose, self.GEOM_SPMM)

    def spmm_copy_info(self, transpose=False):
        i = self.stream_copy_info(transpose, self.GEOM_SPMM)
        keys = ["n_tiles", "n_tb", "n_groups", "entry_slots", "bytes", "build_us"]
        return dict({k: i[k] for k in keys}, rows_per_tile=i["row_slots"], cols_per_block=i["cols_per_block"],
                    wavefronts=i["wavefronts"])

    def export_spmm_copy(self, transpose=False):
        """(tile_blk, blk_id, rows [n_tb, 8, 16, 4], ent [groups + padding, 64, 3], tile_row, hdr [n_tb, 8, 4]) as
        numpy int32 arrays (tests)."""
        return self.export_stream_copy(transpose, self.GEOM_SPMM)

    # ---- streamed copies of the attention sweeps (round 4; stream_attn.hip) ----------------------------
    GEOM_SPMM, GEOM_ATTN, GEOM_BSRC, GEOM_BDST = 0, 1, 2, 3

    def build_stream_copy(self, transpose=False, geom=1, where="device"):
        """Build the streamed copy of geometry `geom` (0 plain SpMM, 1 attention forward, 2 source-major backward,
        3 destination-major backward, 4 lane-per-row copy of the layer-1 sweeps) of A (or A^T); the sweeps use it when
        present.  Returns `stream_copy_info`."""
        t0 = time.perf_counter()
        _lib.check(_lib.lib().mllp_graph_build_stream_copy(self._h, int(transpose), int(geom),
                                                           {"device": 0, "host": 1}[where], _lib.current_stream()))
        self.stream_build_s += time.perf_counter() - t0
        return self.stream_copy_info(transpose, geom)

    def drop_stream_copy(self, transpose=False, geom=1):
        _lib.check(_lib.lib().mllp_graph_drop_stream_copy(self._h, int(transpose), int(geom)))

    def stream_copy_info(self, transpose=False, geom=1):
        d = (c_int64 * 8)()
        _lib.check(_lib.lib().mllp_graph_stream_copy_info(self._h, int(transpose), int(geom), d))
        keys = ["n_tiles", "n_tb", "n_groups", "entry_slots", "bytes", "build_us"]
        out = dict(zip(keys, [int(v) for v in d[:6]]))
        out.update(row_slots=int(d[6]) & 0xffff, rows_per_quad=(int(d[6]) >> 16) & 0xff, item_bytes=int(d[6]) >> 24,
                   cols_per_block=int(d[7]) & 0xffff, wavefronts=(int(d[7]) >> 16) & 0xff, pad_groups=int(d[7]) >> 24)
        return out

    def export_stream_copy(self, transpose=False, geom=1):
        """The copy's arrays as numpy arrays (tests), geometries 0-3 (stream_layout.h, int32): (tile_blk, blk_id,
        rows [n_tb, nw, 16, 4], ent [groups + padding, 64, 3], tile_row, hdr [n_tb, nw, 4]); geometry 4 (lane_layout.h):
        (tile_blk, tile_col [n_tiles, 2], rows [n_tiles, R], offs [groups + padding, 64, 2] uint32, tile_row,
        whdr [n_tb * nw, 2], vals [groups + padding, 64, 4] float32)."""
        i = self.stream_copy_info(transpose, geom)
        nt, tb, nw, ng = i["n_tiles"], i["n_tb"], i["wavefronts"], i["n_groups"] + i["pad_groups"]
        if geom == 4:
            specs = [((nt + 1,), np.int32), ((nt, 2), np.int32), ((nt, i["row_slots"]), np.int32), ((ng, 64, 2), np.uint32),
                     ((nt + 1,), np.int32), ((tb * nw, 2), np.int32), ((ng, 64, 4), np.float32)]
        else:
            specs = [((nt + 1,), np.int32), ((tb,), np.int32), ((tb, nw, 16, 4), np.int32), ((ng, 64, 3), np.int32),
                     ((nt + 1,), np.int32), ((tb, nw, 4), np.int32)]
        out = []
        for which, (shp, dt) in enumerate(specs):
            a = np.empty(shp, dtype=dt)
            _lib.check(_lib.lib().mllp_graph_export_stream_copy(self._h, int(transpose), int(geom), which,
                                                                a.ctypes.data_as(c_void_p), a.nbytes))
            out.append(a)
        return tuple(out)

    def enable_stream_step(self, max_slots_per_nnz=2.0):
        """The streamed copies that the TRAINING STEP's attention sweeps use, both orientations: 16-channel forward (1),
        source-major backward (2), destination-major backward (3), and the lane-per-row copy of the layer-1 sweeps (4).
        Returns {(transpose, geom): info}.

        The copies pad the rows of a wavefront to its longest row (8-14 % of the slots on the synthetic batch, 4-6 % in
        geometry 4).  A batch whose row lengths are so skewed that a copy would take more than `max_slots_per_nnz` entry slots
        per nonzero does not keep that copy (info["dropped"] = True): the sweep then runs on the generic kernels, which
        split long rows over workgroups instead of padding."""
        out = {}
        for tr in (False, True):
            for g in self.STREAM_STEP_GEOMS:
                info = self.build_stream_copy(tr, g)
                if info["entry_slots"] > max_slots_per_nnz * max(self.nnz, 1):
                    self.drop_stream_copy(tr, g)
                    info = dict(info, dropped=True)
                out[(tr, g)] = info
        return out

    def disable_stream_step(self):
        for tr in (False, True):
            for g in self.STREAM_STEP_GEOMS:
                self.drop_stream_copy(tr, g)

    STREAM_STEP_GEOMS = (1, 2, 3, 4)

    def enable_tiled_all(self):
        """Attach every LDS-tiled copy (variants 0-4, both orientations): the throughput configuration for batches of
        hundreds of millions of nonzeros.  Costs ~8 bytes per nonzero and copy.  Returns {(transpose, variant): info}."""
        return {(tr, v): self.enable_tiled(tr, variant=v) for tr in (False, True) for v in (0, 1, 2, 3, 4)}

    def enable_tiled_step(self):
        """The LDS-tiled copies that the TRAINING STEP uses (variants 1-4, both orientations): the attention sweeps.
        Variant 0 belongs to the plain SpMM, which the step does not call (and which runs on the streamed copy,
        `build_spmm_copy`).  `self.tiled_build_s` accumulates the seconds spent in the torch builder."""
        return {(tr, v): self.enable_tiled(tr, variant=v) for tr in (False, True) for v in (1, 2, 3, 4)}

    def disable_tiled(self, transpose=False, variant=0):
        _lib.check(_lib.lib().mllp_graph_attach_tiled(self._h, int(transpose), int(variant), 0, 0, 0, c_void_p(0),
                                                      c_void_p(0), c_void_p(0), c_void_p(0), c_void_p(0)))
        self._tiled.pop((bool(transpose), int(variant)), None)

    def __del__(self):
        try:
            if self._h is not None and self._h.value:
                _lib.lib().mllp_graph_destroy(self._h)
                self._h = None
        except Exception:
            pass

    # ---- introspection -----------------------------------------------------------------------
    def dims(self):
        d = (c_int64 * 12)()
        _lib.check(_lib.lib().mllp_graph_dims(self._h, d))
        keys = ["M", "N", "nnz", "n_inst", "A_group", "A_wave", "A_block", "At_group", "At_wave", "At_block",
                "A_split", "At_split"]
        return dict(zip(keys, [int(v) for v in d]))

    def fused_grid_info(self):
        """(workgroups G of this batch's fused sweeps, partitions, the device's CUs, the grid limit it was created under)"""
        d = (c_int64 * 4)()
        _lib.check(_lib.lib().mllp_graph_fused_grid(self._h, d))
        return tuple(int(v) for v in d)

    def export(self, which):
        sizes = {0: (self.M + 1, np.int32), 1: (self.nnz, np.int32), 2: (self.nnz, np.float32),
                 3: (self.N + 1, np.int32), 4: (self.nnz, np.int32), 5: (self.nnz, np.float32),
                 6: (self.N, np.float32)}
        n, dt = sizes[which]
        out = np.empty(n, dtype=dt)
        _lib.check(_lib.lib().mllp_graph_export(self._h, which, out.ctypes.data_as(c_void_p), out.nbytes))
        return out

    def logits_per_instance(self, logits):
        return [logits[self._n_off[k]:self._n_off[k + 1]] for k in range(self.n_inst)]

    # ---- primitives --------------------------------------------------------------------------
    def spmm(self, H: torch.Tensor, transpose=False, out: Optional[torch.Tensor] = None):
        """Y = A @ H (transpose=False, H [N,16]) or A^T @ H (H [M,16])."""
        n_in, n_out = (self.M, self.N) if transpose else (self.N, self.M)
        assert H.is_cuda and H.dtype == torch.float32 and H.is_contiguous() and tuple(H.shape) == (n_in, 16)
        if out is None:
            out = torch.empty(n_out, 16, device=H.device, dtype=torch.float32)
        _lib.check(_lib.lib().mllp_spmm_csr_f32(self._h, int(transpose), _lib.ptr(H), _lib.ptr(out),
                                                _lib.current_stream()))
        return out

    def spmm_bf16(self, H: torch.Tensor, transpose=False, out: Optional[torch.Tensor] = None):
        """Opt-in bf16 feature image: the same product with H given as torch.bfloat16 [n, 16] (fp32 values, fp32
        accumulation, fp32 result).  Equals `spmm(H.float())` up to fp32 summation order, i.e. differs from the fp32
        product by the rounding of H to bf16 (2^-8 relative per element) -- not the parity path.  Needs the tiled copy
        (`enable_tiled(transpose)`)."""
        n_in, n_out = (self.M, self.N) if transpose else (self.N, self.M)
        assert H.is_cuda and H.dtype == torch.bfloat16 and H.is_contiguous() and tuple(H.shape) == (n_in, 16)
        if out is None:
            out = torch.empty(n_out, 16, device=H.device, dtype=torch.float32)
        _lib.check(_lib.lib().mllp_spmm_csr_bf16(self._h, int(transpose), _lib.ptr(H), _lib.ptr(out),
                                                 _lib.current_stream()))
        return out

    def tconv_workspace(self, dst_is_var, cin):
        n = c_int64()
        _lib.check(_lib.lib().mllp_tconv_workspace_floats(self._h, int(dst_is_var), cin, ctypes.byref(n)))
        return torch.empty(n.value, device=self.x1.device, dtype=torch.float32)

    def tconv_fwd(self, dst_is_var, cin, conv_params, x_src, x_dst, ws):
        n_dst = self.N if dst_is_var else self.M
        h = torch.empty(n_dst, 16, device=x_src.device, dtype=torch.float32)
        _lib.check(_lib.lib().mllp_tconv_fwd(self._h, int(dst_is_var), cin, _lib.ptr(conv_params), _lib.ptr(x_src),
                                             _lib.ptr(x_dst), _lib.ptr(h), _lib.ptr(ws), _lib.current_stream()))
        return h

    def tconv_bwd(self, dst_is_var, cin, conv_params, x_src, x_dst, h, ws, dh, want_input_grads=True):
        n_dst, n_src = (self.N, self.M) if dst_is_var else (self.M, self.N)
        dh = dh.clone()
        dxd = torch.empty(n_dst, cin, device=dh.device) if (want_input_grads and cin == 16) else None
        dxs = torch.empty(n_src, cin, device=dh.device) if (want_input_grads and cin == 16) else None
        pg = torch.empty(conv_params.numel(), device=dh.device, dtype=torch.float32)
        _lib.check(_lib.lib().mllp_tconv_bwd(self._h, int(dst_is_var), cin, _lib.ptr(conv_params), _lib.ptr(x_src),
                                             _lib.ptr(x_dst), _lib.ptr(h), _lib.ptr(ws), _lib.ptr(dh), _lib.ptr(dxd),
                                             _lib.ptr(dxs), 0, _lib.ptr(pg), _lib.current_stream()))
        return pg, dxd, dxs, dh

    # ---- whole model -------------------------------------------------------------------------
    def workspace(self):
        if self._ws is None:
            n = c_int64()
            _lib.check(_lib.lib().mllp_gnn_workspace_bytes(self._h, ctypes.byref(n)))
            self._ws = torch.empty(n.value // 4, device=self.x1.device, dtype=torch.float32)
        return self._ws

    def forward(self, params: torch.Tensor, logits: Optional[torch.Tensor] = None):
        assert params.is_cuda and params.dtype == torch.float32 and params.numel() == _lib.NUM_PARAMS
        if logits is None:
            logits = torch.empty(self.N, device=params.device, dtype=torch.float32)
        self._check_inputs()
        self._folded = None
        _lib.check(_lib.lib().mllp_gnn_forward(self._h, _lib.ptr(params), _lib.ptr(self.x1), _lib.ptr(self.x2),
                                               _lib.ptr(self.workspace()), _lib.ptr(logits), _lib.current_stream()))
        return logits

    def backward(self, params, dlogits, grads: Optional[torch.Tensor] = None):
        if grads is None:
            grads = torch.empty(_lib.NUM_PARAMS, device=params.device, dtype=torch.float32)
        dlogits = dlogits.contiguous().float()
        _lib.check(_lib.lib().mllp_gnn_backward(self._h, _lib.ptr(params), _lib.ptr(self.x1), _lib.ptr(self.x2),
                                                _lib.ptr(self.workspace()), _lib.ptr(dlogits), _lib.ptr(grads),
                                                _lib.current_stream()))
        return grads

    def backward_inputs(self, params, dlogits, x1=True, x2=True, values=True, grads=None):
        """mllp_gnn_backward plus the gradients with respect to the inputs, after `forward` on a generic path (path 1, or
        path 0 at 32 M nonzeros and above).  Returns (grads, dx1 [N], dx2 [M], dvalues [nnz]); dvalues is in the CSR order
        of A (`export(2)`), and an input whose flag is False gets None (and is not computed)."""
        dev = params.device
        if grads is None:
            grads = torch.empty(_lib.NUM_PARAMS, device=dev, dtype=torch.float32)
        dx1 = torch.empty(self.N, device=dev, dtype=torch.float32) if x1 else None
        dx2 = torch.empty(self.M, device=dev, dtype=torch.float32) if x2 else None
        dv = torch.empty(self.nnz, device=dev, dtype=torch.float32) if values else None
        dlogits = dlogits.contiguous().float()
        _lib.check(_lib.lib().mllp_gnn_backward_inputs(self._h, _lib.ptr(params), _lib.ptr(self.x1), _lib.ptr(self.x2),
                                                       _lib.ptr(self.workspace()), _lib.ptr(dlogits), _lib.ptr(grads),
                                                       _lib.ptr(dx1), _lib.ptr(dx2), _lib.ptr(dv), c_void_p(0),
                                                       _lib.current_stream()))
        return grads, dx1, dx2, dv

    def _input_grad_outputs(self, dev, x1, x2, values):
        return (torch.empty(self.N, device=dev, dtype=torch.float32) if x1 else None,
                torch.empty(self.M, device=dev, dtype=torch.float32) if x2 else None,
                torch.empty(self.nnz, device=dev, dtype=torch.float32) if values else None)

    def input_grads(self, params, dlogits, x1=True, x2=True, values=True, grads=None):
        """`backward_inputs` on whichever path `forward` used (mllp_gnn_input_grads): after a forward on the fused
        latency-regime path -- the default below 32 M nonzeros -- the fused backward and its own post-pass run, with no
        `set_path`.  Returns (grads, dx1 [N], dx2 [M], dvalues [nnz]) with the conventions of `backward_inputs`."""
        dev = params.device
        if grads is None:
            grads = torch.empty(_lib.NUM_PARAMS, device=dev, dtype=torch.float32)
        dx1, dx2, dv = self._input_grad_outputs(dev, x1, x2, values)
        dlogits = dlogits.contiguous().float()
        _lib.check(_lib.lib().mllp_gnn_input_grads(self._h, _lib.ptr(params), _lib.ptr(self.x1), _lib.ptr(self.x2),
                                                   _lib.ptr(self.workspace()), _lib.ptr(dlogits), _lib.ptr(grads),
                                                   _lib.ptr(dx1), _lib.ptr(dx2), _lib.ptr(dv), c_void_p(0),
                                                   _lib.current_stream()))
        return grads, dx1, dx2, dv

    def loss_step_inputs(self, params, inv_batch=None, logits=None, loss=None, grads=None, x1=True, x2=True, values=True):
        """`loss_step` plus the gradients of that loss with respect to the inputs, on the path in use
        (mllp_gnn_loss_step_inputs).  Returns (loss, logits, grads, dx1 [N], dx2 [M], dvalues [nnz]); dvalues is in the
        CSR order of A (`export(2)`, what `set_values` takes), and an input whose flag is False gets None (and is not
        computed).  The first call that asks for dvalues allocates: make it outside a graph capture."""
        dev = params.device
        logits = torch.empty(self.N, device=dev, dtype=torch.float32) if logits is None else logits
        loss = torch.empty(1, device=dev, dtype=torch.float32) if loss is None else loss
        grads = torch.empty(_lib.NUM_PARAMS, device=dev, dtype=torch.float32) if grads is None else grads
        dx1, dx2, dv = self._input_grad_outputs(dev, x1, x2, values)
        ib = (1.0 / self.n_inst) if inv_batch is None else float(inv_batch)
        self._check_inputs()
        self._folded = None          # (as loss_step)
        _lib.check(_lib.lib().mllp_gnn_loss_step_inputs(self._h, _lib.ptr(params), _lib.ptr(self.x1), _lib.ptr(self.x2),
                                                        _lib.ptr(self.labels), ib, _lib.ptr(self.workspace()),
                                                        _lib.ptr(logits), _lib.ptr(loss), _lib.ptr(grads), _lib.ptr(dx1),
                                                        _lib.ptr(dx2), _lib.ptr(dv), _lib.current_stream()))
        return loss, logits, grads, dx1, dx2, dv

    def loss_step(self, params, inv_batch=None, logits=None, loss=None, grads=None):
        """forward + BCEWithLogits + backward.  loss = inv_batch * sum_k mean_i BCE; default 1/n_inst."""
        dev = params.device
        logits = torch.empty(self.N, device=dev, dtype=torch.float32) if logits is None else logits
        loss = torch.empty(1, device=dev, dtype=torch.float32) if loss is None else loss
        grads = torch.empty(_lib.NUM_PARAMS, device=dev, dtype=torch.float32) if grads is None else grads
        ib = (1.0 / self.n_inst) if inv_batch is None else float(inv_batch)
        self._check_inputs()
        self._folded = None          # (this call folds the weights of ITS params into the workspace)
        _lib.check(_lib.lib().mllp_gnn_loss_step(self._h, _lib.ptr(params), _lib.ptr(self.x1), _lib.ptr(self.x2),
                                                 _lib.ptr(self.labels), ib, _lib.ptr(self.workspace()),
                                                 _lib.ptr(logits), _lib.ptr(loss), _lib.ptr(grads),
                                                 _lib.current_stream()))
        return loss, logits, grads

    def train_step(self, params, exp_avg, exp_avg_sq, state, eps=1e-8, inv_batch=None, logits=None, loss=None, grads=None,
                   param_gen=None):
        """loss_step + Adam in one library call (single rank; reference experiment.py:139-144).  On the latency-regime
        path the end of the step is one launch that also folds the weights for the next step into this batch's
        workspace; the next train_step on this batch skips its folding launch when `params` is provably unchanged since:
        same tensor, same torch version counter, and the caller's `param_gen` (a counter the caller bumps whenever the
        library writes `params` outside this method; None = never skip) is the one this call left behind."""
        dev = params.device
        logits = torch.empty(self.N, device=dev, dtype=torch.float32) if logits is None else logits
        loss = torch.empty(1, device=dev, dtype=torch.float32) if loss is None else loss
        grads = torch.empty(_lib.NUM_PARAMS, device=dev, dtype=torch.float32) if grads is None else grads
        ib = (1.0 / self.n_inst) if inv_batch is None else float(inv_batch)
        self._check_inputs()
        key = (params.data_ptr(), params._version, param_gen)
        weights_folded = param_gen is not None and getattr(self, "_folded", None) == key
        _lib.check(_lib.lib().mllp_gnn_train_step(self._h, _lib.ptr(params), _lib.ptr(self.x1), _lib.ptr(self.x2),
                                                  _lib.ptr(self.labels), ib, _lib.ptr(self.workspace()), _lib.ptr(logits),
                                                  _lib.ptr(loss), _lib.ptr(grads), _lib.ptr(exp_avg), _lib.ptr(exp_avg_sq),
                                                  _lib.ptr(state), float(eps), int(bool(weights_folded)),
                                                  _lib.current_stream()))
        self._folded = None if param_gen is None else (params.data_ptr(), params._version, param_gen + 1)
        return loss, logits, grads

    def small_step_fits(self):
        """Whether the batch is within the limits of the one-launch step (`small_step_limits`)."""
        fits = ctypes.c_int()
        _lib.check(_lib.lib().mllp_gnn_small_step_fits(self._h, ctypes.byref(fits)))
        return bool(fits.value)

    def train_step_small(self, params, exp_avg=None, exp_avg_sq=None, state=None, eps=1e-8, inv_batch=None, logits=None,
                         loss=None, grads=None):
        """The whole step as one launch of one workgroup (mllp_gnn_train_step_small), for a batch that `small_step_fits`.
        With the three optimizer buffers: loss_step + Adam, as `train_step`.  Without them: the loss step, `params` stay."""
        dev = params.device
        logits = torch.empty(self.N, device=dev, dtype=torch.float32) if logits is None else logits
        loss = torch.empty(1, device=dev, dtype=torch.float32) if loss is None else loss
        grads = torch.empty(_lib.NUM_PARAMS, device=dev, dtype=torch.float32) if grads is None else grads
        ib = (1.0 / self.n_inst) if inv_batch is None else float(inv_batch)
        self._check_inputs()
        self._folded = None          # (the library forgets the folded weights too)
        _lib.check(_lib.lib().mllp_gnn_train_step_small(self._h, _lib.ptr(params), _lib.ptr(self.x1), _lib.ptr(self.x2),
                                                        _lib.ptr(self.labels), ib, _lib.ptr(self.workspace()),
                                                        _lib.ptr(logits), _lib.ptr(loss), _lib.ptr(grads),
                                                        _lib.ptr(exp_avg), _lib.ptr(exp_avg_sq), _lib.ptr(state),
                                                        float(eps), _lib.current_stream()))
        return loss, logits, grads

    def topm_metrics(self, logits, out=None):
        """[n_inst, 2] = (correct_num, f1) per instance (reference experiment.py:146-151)."""
        if out is None:
            out = torch.empty(self.n_inst, 2, device=logits.device, dtype=torch.float32)
        _lib.check(_lib.lib().mllp_topm_metrics(self._h, _lib.ptr(logits), _lib.ptr(self.labels), c_void_p(0),
                                                _lib.ptr(out), _lib.current_stream()))
        return out

    # ---- weighted loss head (mllp_weighted_loss; csrc/weighted_loss.hip) ----------------------------------------
    @property
    def labels(self):
        return self._labels

    @labels.setter
    def labels(self, t):
        self._labels = t
        self._balanced_pw = None          # (balanced_pos_weight: the weights of the labels bound before)

    def balanced_pos_weight(self):
        """[n_inst] cuda float32: pw_k = (n_k - P_k) / P_k with P_k the positives among the instance's labels, the
        `pos_weight` that gives them the total weight of the negatives; 1 where an instance has no positive, no negative or
        no column (mllp_balanced_pos_weight).  Computed once and kept: rebinding `labels`, or writing them in place, makes
        the next call compute it again."""
        key = (self._labels.data_ptr(), self._labels._version)
        if self._balanced_pw is None or self._balanced_pw[0] != key:
            out = _out(self.n_inst, torch.float32, self._labels.device)
            _lib.check(_lib.lib().mllp_balanced_pos_weight(self._h, _lib.ptr(_pad(self._labels)), _lib.ptr(out), _lib.current_stream()))
            self._balanced_pw = (key, _cut(out, self.n_inst))
        return self._balanced_pw[1]

    def _per_instance(self, v, who, what, allow_balanced=False):
        """None, a float (broadcast), a tensor [n_inst] or (pos_weight only) 'balanced' -> None or a cuda float32 [n_inst]"""
        if v is None:
            return None
        if isinstance(v, str):
            if allow_balanced and v == "balanced":
                return self.balanced_pos_weight()
            raise ValueError(f"{who}: {what}: {v!r} is not understood" + (" (a float, a tensor [n_inst] or 'balanced')" if allow_balanced else ""))
        if isinstance(v, torch.Tensor):
            return _checked(who, what, v, self.n_inst)
        consts = self.__dict__.setdefault("_inst_consts", {})
        if float(v) not in consts:
            consts[float(v)] = torch.full((max(self.n_inst, 1),), float(v), device=self.x1.device, dtype=torch.float32)
        return consts[float(v)]

    def weighted_loss(self, logits, inst_weight=None, pos_weight=None, want=("loss", "inst_loss", "dlogits")):
        """torch's BCEWithLogitsLoss(pos_weight) per instance with a weight per instance, from `logits` and the batch's
        labels (mllp_weighted_loss): L_k = mean_i l_i (NOT multiplied by w_k: an instance of weight 0 still reports its
        loss), loss = sum_k w_k L_k, dlogits = d loss / d logits (what `backward` / `input_grads` take).  `inst_weight`:
        None (ones), a float or a tensor [n_inst]; `pos_weight`: None (ones), a float, a tensor [n_inst] or 'balanced'.
        Returns dict(loss [1], inst_loss [n_inst], dlogits [N]) of device tensors; those not named in `want` are None and
        cost nothing.  Bitwise reproducible, the same bits for an instance alone and inside any batch; no sync."""
        want = _parse_want("weighted_loss", want, ("loss", "inst_loss", "dlogits"), "want must name some of 'loss', 'inst_loss', 'dlogits'")
        _checked("weighted_loss", "logits", logits, self.N)
        dev = logits.device
        iw = self._per_instance(inst_weight, "weighted_loss", "inst_weight")
        pw = self._per_instance(pos_weight, "weighted_loss", "pos_weight", allow_balanced=True)
        loss = _out(1, torch.float32, dev, "loss" in want)
        # (loss without inst_loss: the L_k still get a buffer -- without one the library walks the instances in ONE workgroup)
        inst = _out(self.n_inst, torch.float32, dev, {"inst_loss", "loss"} & set(want))
        dz = _out(self.N, torch.float32, dev, "dlogits" in want)
        _lib.check(_lib.lib().mllp_weighted_loss(self._h, _lib.ptr(_pad(logits)), _lib.ptr(_pad(self._labels)), _lib.ptr(iw), _lib.ptr(pw),
                                                 _lib.ptr(dz), _lib.ptr(inst), _lib.ptr(loss), _lib.current_stream()))
        return dict(loss=loss, inst_loss=_cut(inst, self.n_inst) if "inst_loss" in want else None, dlogits=_cut(dz, self.N))

    def _loss_step_outputs(self, dev, logits, loss, inst_loss, grads):
        """What `loss_step_weighted` and `loss_step_topm` do first: the outputs the caller did not give, and `last_dlogits`,
        made once and kept on the batch"""
        logits = torch.empty(self.N, device=dev, dtype=torch.float32) if logits is None else logits
        loss = torch.empty(1, device=dev, dtype=torch.float32) if loss is None else loss
        inst_loss = _cut(_out(self.n_inst, torch.float32, dev), self.n_inst) if inst_loss is None else inst_loss
        grads = torch.empty(_lib.NUM_PARAMS, device=dev, dtype=torch.float32) if grads is None else grads
        if getattr(self, "last_dlogits", None) is None:
            self.last_dlogits = _cut(_out(self.N, torch.float32, dev), self.N)
        return logits, loss, inst_loss, grads

    def loss_step_weighted(self, params, inst_weight=None, pos_weight=None, logits=None, loss=None, inst_loss=None,
                           grads=None):
        """`forward`, `weighted_loss`, `backward` in one library call on the path in use (mllp_gnn_loss_step_weighted).
        Weights as in `weighted_loss`; inst_weight None is all ONES (loss = sum_k L_k) -- pass 1 / n_inst for the batch mean
        that `loss_step` computes.  Returns (loss [1], logits [N], grads, inst_loss [n_inst]); logits are bit for bit those
        of `forward`, and `input_grads` may follow with `self.last_dlogits`."""
        logits, loss, inst_loss, grads = self._loss_step_outputs(params.device, logits, loss, inst_loss, grads)
        iw = self._per_instance(inst_weight, "loss_step_weighted", "inst_weight")
        pw = self._per_instance(pos_weight, "loss_step_weighted", "pos_weight", allow_balanced=True)
        self._check_inputs()
        self._folded = None          # (as forward)
        _lib.check(_lib.lib().mllp_gnn_loss_step_weighted(self._h, _lib.ptr(params), _lib.ptr(self.x1), _lib.ptr(self.x2),
                                                          _lib.ptr(self._labels), _lib.ptr(iw), _lib.ptr(pw),
                                                          _lib.ptr(self.workspace()), _lib.ptr(logits), _lib.ptr(loss),
                                                          _lib.ptr(inst_loss), _lib.ptr(grads), _lib.ptr(self.last_dlogits),
                                                          _lib.current_stream()))
        return loss, logits, grads, inst_loss

    def evaluate(self, params, pos_weight=None):
        """Held-out evaluation: `forward`, the per-instance losses L_k of `weighted_loss` (no dlogits) and `topm_metrics`.
        Returns dict(logits [N], inst_loss [n_inst], metrics [n_inst, 2] = correct_num, f1) of device tensors.  No
        gradient is computed, nothing but this batch's workspace is written, and nothing synchronises."""
        logits = self.forward(params)
        inst = self.weighted_loss(logits, None, pos_weight, want="inst_loss")["inst_loss"]
        return dict(logits=logits, inst_loss=inst, metrics=self.topm_metrics(logits))

    # ---- soft top-m loss head (mllp_topm_loss; csrc/topm_loss.hip) ------------------------------------------------
    _TOPM_WANT = ("loss", "inst_loss", "dlogits", "prob", "info")

    def _inst_ids(self, inst_id, what):
        """None (instance k has id k) or an int32 cuda tensor [n_inst]: the id that seeds each instance's noise"""
        return None if inst_id is None else _checked(what, "inst_id", inst_id, self.n_inst, torch.int32)

    @staticmethod
    def _topm_args(what, tau, sigma, n_samples, seed):
        tau, sigma, n_samples, seed = float(tau), float(sigma), int(n_samples), int(seed)
        if not (0.0 < tau < float("inf")) or not (0.0 <= sigma < float("inf")) or n_samples < 0:
            raise ValueError(f"{what}: tau must be finite and > 0, sigma finite and >= 0, n_samples >= 0 "
                             f"(got tau={tau}, sigma={sigma}, n_samples={n_samples})")
        return tau, sigma, n_samples, seed & 0xFFFFFFFF

    def topm_loss(self, logits, tau=1.0, sigma=0.0, n_samples=0, seed=0, inst_weight=None, pos_weight=None,
                  want=("loss", "inst_loss", "dlogits"), inst_id=None):
        """The soft top-m loss head (mllp_topm_loss): per instance the probabilities p_i = sigmoid(z_i / tau + nu) with nu
        fixed by sum_i p_i = m_k (m_k = the instance's constraints), and `weighted_loss`'s BCE taken at z / tau + nu
        instead of z; dlogits carries the implicit-function term of nu.  n_samples = 0 is the noise-free head
        ('soft-topk'); n_samples = S >= 1 averages S evaluations with Gumbel noise of scale `sigma` on the logits
        ('gs-topk'), a pure function of (seed, instance id, column, sample).  tau = sinkhorn_tau / 2 of the reference's
        yaml.  Weights as in `weighted_loss`.  Returns a dict of device tensors over `want`, some of 'loss' [1],
        'inst_loss' [n_inst], 'dlogits' [N], 'prob' [N] (noise-free p, sums to m_k) and 'info' [n_inst, 4] = (nu, Q,
        sum p - m_k, largest iteration count); those not named are None and cost nothing.  Bitwise reproducible, the same
        bits for an instance alone (given its `inst_id`) and inside any batch; no sync."""
        want = _parse_want("topm_loss", want, self._TOPM_WANT, f"want must name some of {self._TOPM_WANT}")
        _checked("topm_loss", "logits", logits, self.N)
        tau, sigma, n_samples, seed = self._topm_args("topm_loss", tau, sigma, n_samples, seed)
        iw = self._per_instance(inst_weight, "topm_loss", "inst_weight")
        pw = self._per_instance(pos_weight, "topm_loss", "pos_weight", allow_balanced=True)
        ids = self._inst_ids(inst_id, "topm_loss")
        new = lambda n, wanted: _out(n, torch.float32, logits.device, wanted)  # noqa: E731
        loss = new(1, "loss" in want)
        inst = new(self.n_inst, {"inst_loss", "loss"} & set(want))       # (as weighted_loss: never the serial launch)
        dz, prob, info = new(self.N, "dlogits" in want), new(self.N, "prob" in want), new(4 * self.n_inst, "info" in want)
        _lib.check(_lib.lib().mllp_topm_loss(self._h, _lib.ptr(_pad(logits)), _lib.ptr(_pad(self._labels)), _lib.ptr(iw), _lib.ptr(pw),
                                             _lib.ptr(ids), tau, sigma, n_samples, seed, _lib.ptr(dz), _lib.ptr(inst), _lib.ptr(loss),
                                             _lib.ptr(prob), _lib.ptr(info), _lib.current_stream()))
        return dict(loss=loss, inst_loss=_cut(inst, self.n_inst) if "inst_loss" in want else None, dlogits=_cut(dz, self.N),
                    prob=_cut(prob, self.N), info=_cut(info, self.n_inst, 4))

    def topm_prob(self, logits, tau=1.0):
        """The soft basis: p_i = sigmoid(z_i / tau + nu_k) with sum_i p_i = m_k per instance ([N] cuda float32; 0 for an
        instance without constraints, 1 where m_k >= n_k).  The noise-free head's probabilities, labels not needed."""
        return self.topm_loss(logits, tau, want="prob")["prob"]

    def loss_step_topm(self, params, tau=1.0, sigma=0.0, n_samples=0, seed=0, inst_weight=None, pos_weight=None, logits=None,
                       loss=None, inst_loss=None, grads=None, inst_id=None):
        """`forward`, `topm_loss`, `backward` in one library call on the path in use (mllp_gnn_loss_step_topm).  Arguments
        as `topm_loss` and `loss_step_weighted`.  Returns (loss [1], logits [N], grads, inst_loss [n_inst]); logits are bit
        for bit those of `forward`, and `input_grads` may follow with `self.last_dlogits`."""
        tau, sigma, n_samples, seed = self._topm_args("loss_step_topm", tau, sigma, n_samples, seed)
        logits, loss, inst_loss, grads = self._loss_step_outputs(params.device, logits, loss, inst_loss, grads)
        iw = self._per_instance(inst_weight, "loss_step_topm", "inst_weight")
        pw = self._per_instance(pos_weight, "loss_step_topm", "pos_weight", allow_balanced=True)
        ids = self._inst_ids(inst_id, "loss_step_topm")
        self._check_inputs()
        self._folded = None          # (as forward)
        _lib.check(_lib.lib().mllp_gnn_loss_step_topm(self._h, _lib.ptr(params), _lib.ptr(self.x1), _lib.ptr(self.x2),
                                                      _lib.ptr(self._labels), _lib.ptr(iw), _lib.ptr(pw), _lib.ptr(ids), tau, sigma,
                                                      n_samples, seed, _lib.ptr(self.workspace()), _lib.ptr(logits), _lib.ptr(loss),
                                                      _lib.ptr(inst_loss), _lib.ptr(grads), _lib.ptr(self.last_dlogits),
                                                      _lib.current_stream()))
        return loss, logits, grads, inst_loss

    def predict_basis(self, logits, want=("mask", "index", "stats")):
        """The predicted basis of every instance, on the device and without labels (mllp_topm_select): the m_k largest
        logits of instance k (m_k = its constraints), ordered and tie-broken as `topm_metrics` does -- by the key of the
        bit pattern (-0.0 < +0.0), lowest index first among equal logits.  Returns a `BasisPrediction` whose `.mask`
        (uint8 [N]), `.index` (int32 [M], instance-local column ids, ascending, at the instance's constraint offset) and
        `.stats` (float32 [n_inst, 2] = threshold, runner-up) are device tensors; those not named in `want` are None and
        cost nothing."""
        want = _parse_want("predict_basis", want, _SELECT_WANT, "want must name some of 'mask', 'index', 'stats'")
        _checked("predict_basis", "logits", logits, self.N)
        bufs = _select_outputs(want, self.N, self.M, self.n_inst, logits.device)
        _lib.check(_lib.lib().mllp_topm_select(self._h, _lib.ptr(logits), *[_lib.ptr(b) for b in bufs], _lib.current_stream()))
        return BasisPrediction(_cut(bufs[0], self.N), _cut(bufs[1], self.M), bufs[2], self.inst_n, self.inst_m, self.names)

    # ---- repair and solve a predicted basis (mllp_basis_repair; csrc/basis.hip) ---------------------------------
    def _column_segments(self):
        """(instance of every column [N] int64, the instance's first column [N] int64), made once"""
        if getattr(self, "_col_seg", None) is None:
            dev = self.x1.device
            n = torch.tensor(self.inst_n, dtype=torch.int64, device=dev).reshape(-1)
            inst = torch.repeat_interleave(torch.arange(self.n_inst, device=dev), n)
            first = torch.repeat_interleave(torch.cumsum(n, 0) - n, n)
            self._col_seg = (inst, first)
        return self._col_seg

    def _kept_scratch(self, attr, key, scratch_bytes):
        """The scratch of a solver call (None when it needs none): asked of the library's entry point `scratch_bytes` once
        per `key`, the one argument its size depends on, and kept on the batch as `attr` = (key, scratch)"""
        kept = getattr(self, attr, None)
        if kept is None or kept[0] != key:
            n = c_int64()
            _lib.check(getattr(_lib.lib(), scratch_bytes)(self._h, key, ctypes.byref(n)))
            kept = (key, torch.empty(n.value // 4, device=self.x1.device, dtype=torch.float32) if n.value else None)
            setattr(self, attr, kept)
        return kept[1]

    def ranking(self, logits):
        """int32 [N]: the candidate list `repair_basis` walks -- per instance its LOCAL column ids by descending logit, in
        the total order of `predict_basis` (the key of the bit pattern, -0.0 < +0.0), lowest index first among equal
        logits.  Plain torch on the device: the key, then two stable sorts."""
        _checked("ranking", "logits", logits, self.N)
        inst, first = self._column_segments()
        v = logits.reshape(-1).view(torch.int32)
        key = torch.where(v >= 0, v, v ^ 0x7FFFFFFF)        # signed and monotone in the select kernels' unsigned key
        by_key = torch.sort(key, stable=True, descending=True)[1]
        by_inst = torch.sort(inst[by_key], stable=True)[1]
        cols = by_key[by_inst]
        return (cols - first).to(torch.int32)

    def repair_basis(self, logits=None, order=None, tol=2.0 ** -12, max_m=None,
                     want=("basis", "col_of_row", "x", "y", "quality")):
        """The best-ranked nonsingular basis of every instance and its basic solution, on the device
        (mllp_basis_repair; the rule is stated in include/mllp_hip.h).  `order`: int32 [N], per instance its local column
        ids, best first, ended by the first negative entry -- or `logits`, ranked by `ranking`.  `tol`: a column is
        accepted when its residual exceeds tol times its largest entry (2^-12: the customary sqrt(eps) of fp32).  `max_m`:
        instances with more rows are skipped (status code 2); None = the batch's largest m.  Returns a `BasisRepair` of
        device tensors; those not named in `want` are None and cost nothing (`x` and `y` come together, `status` always).
        The scratch is asked for once per max_m and kept on the batch.  No sync."""
        names = ("basis", "col_of_row", "x", "y", "quality")
        want = _parse_want("repair_basis", want, names, f"want names some of {names}, 'x' and 'y' together", allow_empty=True,
                           together=("x", "y"))
        if (logits is None) == (order is None):
            raise ValueError("repair_basis: give logits or order, one of them")
        if order is None:
            order = self.ranking(logits)
        _checked("repair_basis", "order", order, self.N, torch.int32)
        dev, f32, i32 = self.x1.device, torch.float32, torch.int32
        max_m = max(self.inst_m, default=0) if max_m is None else int(max_m)
        scratch = self._kept_scratch("_repair_scratch", max_m, "mllp_basis_repair_scratch_bytes")
        basis, col_of_row = _out(self.N, f32, dev, "basis" in want), _out(self.M, i32, dev, "col_of_row" in want)
        x, y = _out(self.N, f32, dev, "x" in want), _out(self.M, f32, dev, "y" in want)
        status, quality = _out(self.n_inst * 4, i32, dev), _out(self.n_inst * 2, f32, dev, "quality" in want)
        _lib.check(_lib.lib().mllp_basis_repair(self._h, _lib.ptr(_pad(self.x1)), _lib.ptr(_pad(self.x2)), _lib.ptr(_pad(order)), float(tol),
                                                max_m, *[_lib.ptr(t) for t in (basis, col_of_row, x, y, status, quality)],
                                                _lib.ptr(scratch), _lib.current_stream()))
        return BasisRepair(_cut(basis, self.N), _cut(col_of_row, self.M), _cut(x, self.N), _cut(y, self.M),
                           _cut(status, self.n_inst, 4), _cut(quality, self.n_inst, 2))

    def solve_basis(self, basis, tol=2.0 ** -12, max_m=None, want=("basis", "col_of_row", "x", "y", "quality")):
        """The basic solution of a GIVEN basis (labels, a solver's output; [N], nonzero = basic): `repair_basis` on the list
        "the mask's columns ascending, then -1".  Status code 1 when the basis is singular or has fewer than m columns."""
        if not (basis.is_cuda and basis.is_contiguous() and basis.numel() == self.N):
            raise ValueError(f"solve_basis: basis must be a contiguous cuda tensor of {self.N} elements")
        inst, first = self._column_segments()
        off = basis.reshape(-1) == 0
        cols = torch.sort(inst * 2 + off.to(torch.int64), stable=True)[1]
        order = torch.where(off[cols], torch.full_like(cols, -1), cols - first[cols]).to(torch.int32)
        return self.repair_basis(order=order, tol=tol, max_m=max_m, want=want)

    def solved(self, rep, feas_tol, opt_tol):
        """What a `BasisRepair` (with x, y and basis) is worth, per instance, as device booleans from its status and the six
        figures of `certificate`: `usable` (rank m: a basic solution exists), `primal_feasible` (usable, |Ax - b| <=
        feas_tol, x >= -feas_tol on the basis, |x| <= feas_tol off it, m basic columns), `optimal` (primal feasible, reduced
        costs >= -opt_tol off the basis and within opt_tol of 0 on it); `skipped`: m > max_m, never a failure of the
        basis.  Both tolerances are in the units of the stored LP and have no defaults.  No sync."""
        if rep.x is None or rep.y is None or rep.basis is None:
            raise ValueError("solved: the BasisRepair needs x, y and basis")
        feas_tol, opt_tol = float(feas_tol), float(opt_tol)
        cert = self.certificate(rep.x, rep.y, rep.basis)
        m = torch.tensor(self.inst_m, dtype=torch.float32, device=cert.device).reshape(-1)
        usable = rep.status[:, 3] == 0
        feasible = (usable & (cert[:, 0] <= feas_tol) & (cert[:, 1] >= -feas_tol) & (cert[:, 2] <= feas_tol) & (cert[:, 5] == m))
        optimal = feasible & (cert[:, 3] >= -opt_tol) & (cert[:, 4] <= opt_tol)
        return dict(usable=usable, primal_feasible=feasible, optimal=optimal, skipped=rep.status[:, 3] == 2, certificate=cert)

    # ---- pivot a basis to optimality (mllp_basis_simplex; csrc/simplex.hip) ----------------------------------------
    def simplex(self, start, max_pivots, tol=2.0 ** -12, ftol=2.0 ** -10, dtol=2.0 ** -10, ptol=2.0 ** -10, dshift=2.0 ** -4,
                max_m=None, want=("basis", "col_of_row", "trace"), refactor_every=0, stall_pivots=0):
        """Dual, then primal simplex pivots from a basis to the optimum, on the device (mllp_basis_simplex; the rule is
        stated in include/mllp_hip.h).  `start`: a mask tensor [N] (nonzero = basic) or a `BasisRepair`, whose `.basis` is
        used.  `max_pivots`: the limit per instance (code 6 beyond it).  `tol` is `repair_basis`'; `ftol`, `dtol`, `ptol`,
        `dshift` are the rule's feasibility, optimality and pivot tolerances and its cost shift, in the units of the stored
        LP.  `max_m`: instances with more rows are skipped (code 2); None = the batch's largest m.  Returns a `BasisSimplex`
        of device tensors; `col_of_row` and `trace` are None unless named in `want` (`basis` and `status` always come).  The
        scratch is asked for once per max_m and kept on the batch.  No sync.
        `refactor_every` = R > 0: the basis is factorized afresh after every R pivots; `stall_pivots` = S > 0: Bland's rule
        after S consecutive degenerate pivots of a stage.  With both 0 this is mllp_basis_simplex as ever; otherwise
        mllp_basis_simplex_guarded (code 7: a basis could not be refactorized), and the result has `.guard`."""
        names = ("basis", "col_of_row", "trace")
        want = _parse_want("simplex", want, names, f"want names some of {names}", allow_empty=True)
        if isinstance(start, BasisRepair):
            start = start.basis
        if start is None or not (start.is_cuda and start.numel() == self.N):
            raise ValueError(f"simplex: start must be a cuda tensor of {self.N} elements (or a BasisRepair with its basis)")
        start = start.reshape(-1).to(torch.float32).contiguous()
        max_pivots = int(max_pivots)
        if max_pivots < 0:
            raise ValueError("simplex: max_pivots must not be negative")
        refactor_every, stall_pivots = int(refactor_every), int(stall_pivots)
        if refactor_every < 0 or stall_pivots < 0:
            raise ValueError("simplex: refactor_every and stall_pivots must not be negative")
        dev, i32 = self.x1.device, torch.int32
        max_m = max(self.inst_m, default=0) if max_m is None else int(max_m)
        scratch = self._kept_scratch("_simplex_scratch", max_m, "mllp_basis_simplex_scratch_bytes")
        basis, status = _out(self.N, torch.float32, dev), _out(self.n_inst * 4, i32, dev)
        col_of_row = _out(self.M, i32, dev, "col_of_row" in want)
        trace = _out(self.n_inst * max_pivots * 2, i32, dev, "trace" in want)
        guarded = refactor_every != 0 or stall_pivots != 0
        guard = _out(self.n_inst * 2, i32, dev, guarded)
        head = (self._h, _lib.ptr(_pad(self.x1)), _lib.ptr(_pad(self.x2)), _lib.ptr(_pad(start)), float(tol), float(ftol), float(dtol),
                float(ptol), float(dshift), max_pivots, max_m)
        outs = (_lib.ptr(basis), _lib.ptr(col_of_row), _lib.ptr(trace), _lib.ptr(status))
        if guarded:
            _lib.check(_lib.lib().mllp_basis_simplex_guarded(*head, refactor_every, stall_pivots, *outs, _lib.ptr(guard),
                                                             _lib.ptr(scratch), _lib.current_stream()))
        else:
            _lib.check(_lib.lib().mllp_basis_simplex(*head, *outs, _lib.ptr(scratch), _lib.current_stream()))
        return BasisSimplex(_cut(basis, self.N), _cut(col_of_row, self.M), _cut(trace, self.n_inst, max_pivots, 2),
                            _cut(status, self.n_inst, 4), _cut(guard, self.n_inst, 2))

    def simplex_solved(self, res, feas_tol, opt_tol, tol=2.0 ** -12, max_m=None):
        """What a `BasisSimplex` is worth: `solve_basis(res.basis)` -- a FRESH factorization of the final basis, which the
        product-form pivots never got -- then `solved` (the certificate).  The dict of `solved`, and `pivots`: stage-D +
        stage-P pivots per instance (int32 [n_inst]).  No sync."""
        got = self.solved(self.solve_basis(res.basis, tol=tol, max_m=max_m, want=("basis", "x", "y")), feas_tol, opt_tol)
        got["pivots"] = res.status[:, 1] + res.status[:, 2]
        return got

    # ---- restarted PDHG on every instance: plain, preconditioned, and preconditioned with Halpern's iteration (mllp_lp_pdhg,
    # mllp_lp_pdhg_scaled, mllp_lp_pdhg_halpern; csrc/pdhg.hip) ----
    def _pdhg(self, who, max_iters, check_every, params, x0, y0, start, max_lds_words):
        """What `pdhg`, `pdhg_scaled` and `pdhg_halpern` share: the start, the validation, the scratch kept on the batch, the
        outputs and the call.  `who`: "pdhg", "pdhg_scaled" or "pdhg_halpern" -- the prefix of the messages, and what names
        the entry points (mllp_lp_<who> and its _scratch_bytes) and the attribute that keeps the scratch (`_<who>_scratch`).
        `params`: the entry point's own arguments between check_every and max_lds_words -- eps, step, beta, for pdhg_scaled
        also ruiz, pock_chambolle, primal_weight, weight_span, and for pdhg_halpern reflect behind those.  Returns x, y,
        status, kkt (and dr, dc)."""
        scaled = who != "pdhg"
        if start is not None:
            if x0 is not None or y0 is not None:
                raise ValueError(f"{who}: give start or x0 / y0, not both")
            if not isinstance(start, BasisRepair) or start.x is None or start.y is None:
                raise ValueError(f"{who}: start must be a BasisRepair with x and y")
            x0, y0 = start.x, start.y
        for t, n, what in ((x0, self.N, "x0"), (y0, self.M, "y0")):
            if t is not None:
                _checked(who, what, t, n)
        max_iters, check_every = int(max_iters), int(check_every)
        if scaled:
            params = params[:3] + (int(params[3]),) + params[4:]       # ruiz
        if max_iters < 0 or check_every < 0:
            raise ValueError(f"{who}: max_iters and check_every must not be negative")
        dev, f32 = self.x1.device, torch.float32
        max_lds_words = (pdhg_scaled_limits if scaled else pdhg_limits)()[0] if max_lds_words is None else int(max_lds_words)
        scratch = self._kept_scratch(f"_{who}_scratch", max_lds_words, f"mllp_lp_{who}_scratch_bytes")
        x, y = _out(self.N, f32, dev), _out(self.M, f32, dev)
        side = (_out(self.M, f32, dev), _out(self.N, f32, dev)) if scaled else ()         # dr, dc
        kkt_words = 6 if scaled else 4
        status, kkt = _out(self.n_inst * 4, torch.int32, dev), _out(self.n_inst * kkt_words, f32, dev)
        opt = lambda t: None if t is None or not t.numel() else t                             # noqa: E731
        flag = lambda v: int(bool(v))                                                         # noqa: E731
        _lib.check(getattr(_lib.lib(), f"mllp_lp_{who}")(
            self._h, _lib.ptr(_pad(self.x1)), _lib.ptr(_pad(self.x2)), _lib.ptr(opt(x0)), _lib.ptr(opt(y0)), max_iters, check_every,
            *[f(v) for f, v in zip((float, float, float, int, flag, flag, float, flag), params)], max_lds_words, _lib.ptr(x), _lib.ptr(y),
            *[_lib.ptr(t) for t in side], _lib.ptr(status), _lib.ptr(kkt), _lib.ptr(scratch), _lib.current_stream()))
        return (_cut(x, self.N), _cut(y, self.M), _cut(status, self.n_inst, 4), _cut(kkt, self.n_inst, kkt_words),
                *(_cut(t, n) for t, n in zip(side, (self.M, self.N))))

    def pdhg(self, max_iters, eps=2.0 ** -10, check_every=64, step=0.9, beta=0.5, x0=None, y0=None, start=None,
             max_lds_words=None):
        """A first-order solve of every instance on the device: PDHG with averaging and restarts (mllp_lp_pdhg; the rule
        is stated in include/mllp_hip.h).  No factorization and no row limit: memory O(n + m) per instance.  `max_iters`:
        the limit per instance (code 6 at it).  `eps`: the relative KKT error (primal, dual, gap) at which an instance stops
        with code 0.  `check_every`: iterations between two checks; 0: plain PDHG, no averaging, no restarts.  `step`: the
        fraction of 1 / sqrt(|A|_1 |A|_inf) both steps take, in (0, 1].  `beta`: a check restarts when the error fell below
        beta times the last restart's.  `x0` [N], `y0` [M]: the start (zeros when None), or `start`: a `BasisRepair` whose
        `x`, `y` are the warm start.  `max_lds_words`: test hook -- instances whose 3 n + 2 m words exceed it keep their
        vectors in scratch (None: the kernel's limit).  Returns an `LPPdhg` of device tensors.  The scratch is asked for
        once per max_lds_words and kept on the batch.  A BASELINE: no preconditioning, no adaptive step.  No sync."""
        return LPPdhg(*self._pdhg("pdhg", max_iters, check_every, (eps, step, beta), x0, y0, start, max_lds_words))

    def pdhg_scaled(self, max_iters, eps=2.0 ** -10, check_every=64, step=0.9, beta=0.5, ruiz=10, pock_chambolle=True,
                    primal_weight=True, weight_span=16.0, x0=None, y0=None, start=None, max_lds_words=None):
        """`pdhg` with diagonal preconditioning and a primal weight, both computed on the device by the call itself
        (mllp_lp_pdhg_scaled; the rule is stated in include/mllp_hip.h).  `ruiz`: passes of Ruiz equilibration (0 .. 64);
        `pock_chambolle`: one more pass on the row and column sums; `primal_weight`: start the weight at |dc c| / |dr b| and
        move it at every restart, inside [w0 / weight_span, w0 * weight_span].  The other arguments, the checks and the codes
        are `pdhg`'s (the errors are those of the original LP); with ruiz=0, pock_chambolle=False, primal_weight=False the
        result has `pdhg`'s bits.  Returns an `LPPdhgScaled`.  The scratch is asked for once per max_lds_words and kept on
        the batch.  No adaptive step, no infeasibility detection.  No sync."""
        return LPPdhgScaled(*self._pdhg("pdhg_scaled", max_iters, check_every,
                                        (eps, step, beta, ruiz, pock_chambolle, primal_weight, weight_span), x0, y0, start, max_lds_words))

    def pdhg_halpern(self, max_iters, eps=2.0 ** -10, check_every=64, step=0.9, beta=0.5, ruiz=10, pock_chambolle=True,
                     primal_weight=True, weight_span=16.0, reflect=True, x0=None, y0=None, start=None, max_lds_words=None):
        """`pdhg_scaled` with Halpern's iteration in place of the running average (mllp_lp_pdhg_halpern; the rule is stated
        in include/mllp_hip.h): after k iterations since the last restart the iterate moves to (k+1)/(k+2) of the reflected
        PDHG step 2 T(z) - z plus 1/(k+2) of the last restart point.  A check judges ONE point, the step's output T(z), which
        is also what the call returns; `status[:, 3]` is 0.  `reflect=False` is the unreflected iteration (slower than
        `pdhg_scaled`: it pins the reflection in tests).  The scaling, the step, the weight, the other arguments and the codes
        are `pdhg_scaled`'s, and so are `dr`, `dc`, `kkt[:, 3:5]`.  Returns an `LPPdhgHalpern`.  The scratch is asked for once
        per max_lds_words and kept on the batch.  No adaptive step, no infeasibility detection.  No sync."""
        return LPPdhgHalpern(*self._pdhg("pdhg_halpern", max_iters, check_every,
                                         (eps, step, beta, ruiz, pock_chambolle, primal_weight, weight_span, reflect), x0, y0, start,
                                         max_lds_words))

    def pdhg_wide(self, max_iters, eps=2.0 ** -10, check_every=64, step=0.9, beta=0.5, ruiz=10, pock_chambolle=True,
                  primal_weight=True, weight_span=16.0, reflect=True, x0=None, y0=None, start=None, rows_per_item=None,
                  poll_every=None):
        """`pdhg_halpern`, bit for bit, run across the whole device (mllp_lp_pdhg_wide; csrc/pdhg_wide.hip): every instance's
        rows and columns are cut into items of `rows_per_item` rows (a multiple of 64; None: the library's default), one
        workgroup each, and an iteration is two ordinary launches -- where `pdhg_halpern` lasts as long as its slowest instance
        on ONE compute unit.  The arguments, the codes and the tensors are `pdhg_halpern`'s; `rows_per_item` moves no bit.
        `poll_every=None`: one C call, no sync.  `poll_every=P`: calls of P iterations each, the codes read back after each
        (one sync per call), and no further call once no instance is at code 6 -- what makes an early stop cost nothing; the
        tensors have the single call's bits.  Returns an `LPPdhgWide`, whose `.calls` is the number of C calls made.  The
        scratch, which also carries the state from one call to the next, is asked for once per rows_per_item and kept on the
        batch."""
        return self._pdhg_wide("pdhg_wide", max_iters, check_every, (eps, step, beta, ruiz, pock_chambolle, primal_weight, weight_span, reflect),
                               x0, y0, start, rows_per_item, poll_every)

    def pdhg_rays(self, max_iters, eps=2.0 ** -10, check_every=64, step=0.9, beta=0.5, ruiz=10, pock_chambolle=True,
                  primal_weight=True, weight_span=16.0, reflect=True, ray_eps=2.0 ** -10, x0=None, y0=None, start=None,
                  rows_per_item=None, poll_every=None):
        """`pdhg_wide` that can say "this LP has no solution" (mllp_lp_pdhg_rays; the rule is stated in include/mllp_hip.h): at
        every check the direction from the anchor to the step's output is judged as a ray of the original LP, and an instance
        stops with code 4 (primal infeasible; `.ray_y` is the Farkas certificate) or code 5 (dual infeasible: unbounded if
        feasible; `.ray_x` is the recession ray) once its relative quality is at most `ray_eps`.  The test is RELATIVE: code 4
        proves that every feasible point has a 1-norm of at least 1 / ray_eps, which also holds for feasible LPs with large
        solutions -- choose `ray_eps` below 1 / |x|_1 of the solutions expected.  A negative `ray_eps` turns
        detection off, and the result has `pdhg_wide`'s bits.  The rays ride in the check's own sweeps: the call makes exactly
        `pdhg_wide`'s launches.  The other arguments are `pdhg_wide`'s; polling stops once no instance is at code 6.  Returns
        an `LPPdhgRays`.  The scratch is asked for once per rows_per_item and kept on the batch, under its own name."""
        return self._pdhg_wide("pdhg_rays", max_iters, check_every,
                               (eps, step, beta, ruiz, pock_chambolle, primal_weight, weight_span, reflect, ray_eps), x0, y0, start, rows_per_item,
                               poll_every)

    def pdhg_spectral(self, max_iters, eps=2.0 ** -10, check_every=64, step=0.9, beta=0.5, ruiz=10, pock_chambolle=True,
                      primal_weight=True, weight_span=16.0, reflect=True, power_iters=40, ray_eps=-1.0, x0=None, y0=None, start=None,
                      rows_per_item=None, poll_every=None):
        """`pdhg_rays` with a spectral step size (mllp_lp_pdhg_spectral; the rule is stated in include/mllp_hip.h): the step is
        `step` over an estimate of the scaled matrix's 2-norm from `power_iters` rounds of power iteration on the device, where
        every other call divides by sqrt(|S|_1 |S|_inf), an upper bound that is 1.3 to 6.7 times too large on this project's
        data.  The estimate is a LOWER bound; where it is void or above the bound, the bound is used.  `power_iters=0` gives
        `pdhg_rays`' bits.  Detection is OFF by default here (`ray_eps=-1`: 2^-10 stops 46 feasible Netlib LPs).  The other
        arguments are `pdhg_rays`'.  Returns an `LPPdhgSpectral`, whose `.norm` is [n_inst, 2] = the estimate (0: none), the
        bound; `.kkt[:, 3]` is the eta in use."""
        power_iters = int(power_iters)
        if power_iters < 0 or power_iters > pdhg_spectral_limits()[4]:
            raise ValueError(f"pdhg_spectral: power_iters must be in 0 .. {pdhg_spectral_limits()[4]}")
        return self._pdhg_wide("pdhg_spectral", max_iters, check_every,
                               (eps, step, beta, ruiz, pock_chambolle, primal_weight, weight_span, reflect, ray_eps, power_iters), x0, y0, start,
                               rows_per_item, poll_every)

    def _pdhg_wide(self, who, max_iters, check_every, params, x0, y0, start, rows_per_item, poll_every):
        """What `pdhg_wide`, `pdhg_rays` and `pdhg_spectral` share: the start, the validation, the scratch kept on the batch
        (`_<who>_scratch`), the outputs, the call mllp_lp_<who> and the continuation loop.  `params`: eps .. reflect, for pdhg_rays
        ray_eps behind them, and for pdhg_spectral power_iters behind that."""
        spectral = who == "pdhg_spectral"
        rays = spectral or who == "pdhg_rays"
        if start is not None:
            if x0 is not None or y0 is not None:
                raise ValueError(f"{who}: give start or x0 / y0, not both")
            if not isinstance(start, BasisRepair) or start.x is None or start.y is None:
                raise ValueError(f"{who}: start must be a BasisRepair with x and y")
            x0, y0 = start.x, start.y
        for t, n, what in ((x0, self.N, "x0"), (y0, self.M, "y0")):
            if t is not None:
                _checked(who, what, t, n)
        max_iters, check_every = int(max_iters), int(check_every)
        if max_iters < 0 or check_every < 0:
            raise ValueError(f"{who}: max_iters and check_every must not be negative")
        rows = 0 if rows_per_item is None else int(rows_per_item)
        if rows_per_item is not None and (rows <= 0 or rows % 64 or rows > pdhg_wide_limits()[3]):
            raise ValueError(f"{who}: rows_per_item must be a positive multiple of 64, at most {pdhg_wide_limits()[3]}")
        if poll_every is not None and int(poll_every) <= 0:
            raise ValueError(f"{who}: poll_every must be positive")
        dev, f32 = self.x1.device, torch.float32
        scratch = self._kept_scratch(f"_{who}_scratch", rows, f"mllp_lp_{who}_scratch_bytes")
        x, y, dr, dc = _out(self.N, f32, dev), _out(self.M, f32, dev), _out(self.M, f32, dev), _out(self.N, f32, dev)
        status, kkt = _out(self.n_inst * 4, torch.int32, dev), _out(self.n_inst * 6, f32, dev)
        ray_x, ray_y, cert = (_out(self.N, f32, dev), _out(self.M, f32, dev), _out(self.n_inst * 4, f32, dev)) if rays else (None, None, None)
        opt = lambda t: None if t is None or not t.numel() else t                             # noqa: E731
        flag = lambda v: int(bool(v))                                                         # noqa: E731
        x1, x2 = _pad(self.x1), _pad(self.x2)
        norm = _out(self.n_inst * 2, f32, dev) if spectral else None
        scalars = [f(v) for f, v in zip((float, float, float, int, flag, flag, float, flag, float, int), params)]
        outs = (x, y, dr, dc, ray_x, ray_y, status, kkt, cert) + ((norm,) if spectral else ()) if rays else (x, y, dr, dc, status, kkt)
        entry = getattr(_lib.lib(), f"mllp_lp_{who}")

        def call(begin, end):
            _lib.check(entry(self._h, _lib.ptr(x1), _lib.ptr(x2), _lib.ptr(opt(x0)), _lib.ptr(opt(y0)), begin, end, check_every, *scalars, rows,
                             *[_lib.ptr(t) for t in outs], _lib.ptr(scratch), _lib.current_stream()))
        calls = 0
        if poll_every is None:
            call(0, max_iters)
            calls = 1
        else:
            begin = 0
            while True:
                end = min(begin + int(poll_every), max_iters)
                call(begin, end)
                calls += 1
                begin = end
                if begin >= max_iters or not bool((_cut(status, self.n_inst, 4)[:, 0] == 6).any().item()):
                    break
        res = (_cut(x, self.N), _cut(y, self.M), _cut(status, self.n_inst, 4), _cut(kkt, self.n_inst, 6), _cut(dr, self.M), _cut(dc, self.N))
        if spectral:
            res = LPPdhgSpectral(*res, _cut(ray_x, self.N), _cut(ray_y, self.M), _cut(cert, self.n_inst, 4), _cut(norm, self.n_inst, 2))
        elif rays:
            res = LPPdhgRays(*res, _cut(ray_x, self.N), _cut(ray_y, self.M), _cut(cert, self.n_inst, 4))
        else:
            res = LPPdhgWide(*res)
        res.calls = calls
        return res

    def pdhg_basis(self, res, tol=2.0 ** -12, max_m=None):
        """The vertex a PDHG iterate points at: `repair_basis` on the ranking of `res.x` (its m largest entries first), so the
        `BasisRepair` of the best-ranked nonsingular basis and its basic solution, which `solved` certifies -- for the
        instances the dense call can hold (`max_m`; the others are skipped, code 2).  No sync."""
        if not isinstance(res, LPPdhg):
            raise ValueError("pdhg_basis: res must be the LPPdhg of LPBatch.pdhg")
        return self.repair_basis(order=self.ranking(res.x.contiguous()), tol=tol, max_m=max_m, want=("basis", "col_of_row", "x", "y", "quality"))


_SELECT_WANT = ("mask", "index", "stats")


def _select_outputs(want, n, m, n_seg, dev):
    """(mask, index, stats) buffers of the select entry points, None where not wanted"""
    return (_out(n, torch.uint8, dev, "mask" in want), _out(m, torch.int32, dev, "index" in want),
            torch.empty(max(n_seg, 1), 2, dtype=torch.float32, device=dev) if "stats" in want else None)


class BasisPrediction:
    """What `LPBatch.predict_basis`, `GNNModel.predict` and `AngleModel.predict` return: device tensors `.mask`
    (uint8, 1 = in the predicted basis), `.index` (int32, per segment the selected local column ids in ascending order,
    -1 in the slots past min(m, n)) and `.stats` (float32 [segments, 2] = threshold, runner-up); `seg_n` / `seg_m` are
    the segments' column counts and basis sizes.  Nothing here synchronises except `split`."""

    def __init__(self, mask, index, stats, seg_n, seg_m, names=None):
        self.mask, self.index, self.stats = mask, index, stats
        self.seg_n = [int(v) for v in seg_n]
        self.seg_m = [int(v) for v in seg_m]
        self.names = list(names) if names is not None else None

    def split(self):
        """Per instance, the selected column ids as a numpy int32 array (ONE copy back for the whole batch)."""
        if self.index is None:
            raise ValueError("BasisPrediction.split needs the index output (want=('index', ...))")
        idx = self.index.cpu().numpy()
        off = np.concatenate([[0], np.cumsum(self.seg_m)])
        return [idx[off[k]:off[k] + min(self.seg_m[k], self.seg_n[k])] for k in range(len(self.seg_m))]


class BasisRepair:
    """What `LPBatch.repair_basis` / `solve_basis` return, all device tensors, nothing copied back: `.basis` (float32 [N],
    1 = accepted: what `certificate` takes), `.col_of_row` (int32 [M]: the local column whose pivot row this is, or -1), `.x`
    [N] and `.y` [M] (the basic solution, zeros where rank < m), `.status` (int32 [n_inst, 4] = rank, candidates examined,
    rejected among the first m candidates, code: 0 rank == m, 1 list exhausted, 2 skipped, 3 bad id) and `.quality`
    (float32 [n_inst, 2] = smallest accepted, largest rejected residual ratio)."""

    def __init__(self, basis, col_of_row, x, y, status, quality):
        self.basis, self.col_of_row, self.x, self.y, self.status, self.quality = basis, col_of_row, x, y, status, quality


class BasisSimplex:
    """What `LPBatch.simplex` returns, all device tensors, nothing copied back: `.basis` (float32 [N], the basis at the
    stop; zeros for codes 1, 2, 3), `.col_of_row` (int32 [M]: the local basic column that owns this row of the inverse, or
    -1), `.trace` (int32 [n_inst, max_pivots, 2] = entering local column, leaving row of every pivot; -1 past the end) and
    `.status` (int32 [n_inst, 4] = code, stage-D pivots, stage-P pivots, rank of the start; code 0 optimal, 1 singular
    start, 2 skipped, 3 the mask does not have m columns, 4 primal infeasible, 5 unbounded, 6 max_pivots reached, 7 a basis
    could not be refactorized) and `.guard` (int32 [n_inst, 2] = refactorizations, pivots chosen by Bland's rule; None unless
    `refactor_every` or `stall_pivots` was given)."""

    def __init__(self, basis, col_of_row, trace, status, guard=None):
        self.basis, self.col_of_row, self.trace, self.status, self.guard = basis, col_of_row, trace, status, guard


class LPPdhg:
    """What `LPBatch.pdhg` returns, all device tensors, nothing copied back: `.x` [N], `.y` [M] (the output point: the
    candidate of the check that stopped, or the current iterate), `.status` (int32 [n_inst, 4] = code, iterations, restarts,
    1 if the average was returned; code 0 converged, 6 max_iters reached, 8 the error was not finite) and `.kkt` (float32
    [n_inst, 4] = relative primal residual, dual residual and gap of the output, and the step eta)."""

    def __init__(self, x, y, status, kkt):
        self.x, self.y, self.status, self.kkt = x, y, status, kkt


class LPPdhgScaled(LPPdhg):
    """What `LPBatch.pdhg_scaled` returns: an `LPPdhg` (so `pdhg_basis` and everything behind it take it) whose `.kkt` is
    float32 [n_inst, 6] = primal residual, dual residual, gap, the step eta, the starting weight w0 and the final weight,
    with `.dr` [M] and `.dc` [N], the row and column scaling factors the call computed."""

    def __init__(self, x, y, status, kkt, dr, dc):
        super().__init__(x, y, status, kkt)
        self.dr, self.dc = dr, dc


class LPPdhgHalpern(LPPdhgScaled):
    """What `LPBatch.pdhg_halpern` returns: an `LPPdhgScaled` whose `.x`, `.y` are the last step's output (the point that was
    checked, at codes 0 and 8) and whose `.status[:, 3]` is 0: there is no average to return."""


class LPPdhgWide(LPPdhgHalpern):
    """What `LPBatch.pdhg_wide` returns: `pdhg_halpern`'s tensors with `pdhg_halpern`'s bits, and `.calls`, the number of
    mllp_lp_pdhg_wide calls that made them (1 without `poll_every`).  `status[:, 0]` may also be 9, stale state, which
    `LPBatch.pdhg_wide` itself never produces: it continues only its own calls."""
    calls = 1


class LPPdhgRays(LPPdhgWide):
    """What `LPBatch.pdhg_rays` returns: an `LPPdhgWide` whose `status[:, 0]` may also be 4 (primal infeasible RELATIVE to
    ray_eps: no feasible point with a 1-norm below 1 / ray_eps, which a feasible LP with large solutions meets too) or 5 (dual
    infeasible in the same relative sense), with `.ray_y` [M] (the certificate of an instance at code 4, zeros elsewhere), `.ray_x` [N] (of one at code 5)
    and `.cert` (float32 [n_inst, 4] = qp, b'ry, qd, c'rx of the last check that evaluated the instance's rays; +inf, 0, +inf, 0
    if none did).  `.x`, `.y`, `.kkt` are the last step's output and its errors at every code."""

    def __init__(self, x, y, status, kkt, dr, dc, ray_x, ray_y, cert):
        super().__init__(x, y, status, kkt, dr, dc)
        self.ray_x, self.ray_y, self.cert = ray_x, ray_y, cert


class LPPdhgSpectral(LPPdhgRays):
    """What `LPBatch.pdhg_spectral` returns: an `LPPdhgRays` with `.norm` (float32 [n_inst, 2] = the power iteration's estimate
    of the scaled matrix's 2-norm, 0 where it is void or `power_iters` was 0, and the bound sqrt(|S|_1 |S|_inf)).  `.kkt[:, 3]`
    is the step eta in use: `step` over the estimate where that is positive and not above the bound, else over the bound."""

    def __init__(self, x, y, status, kkt, dr, dc, ray_x, ray_y, cert, norm):
        super().__init__(x, y, status, kkt, dr, dc, ray_x, ray_y, cert)
        self.norm = norm


def pdhg_spectral_limits():
    """`pdhg_wide_limits()` and the largest `power_iters` (mllp_lp_pdhg_spectral_limits; no GPU)"""
    lim = (c_int64 * 5)()
    _lib.check(_lib.lib().mllp_lp_pdhg_spectral_limits(lim))
    return int(lim[0]), int(lim[1]), int(lim[2]), int(lim[3]), int(lim[4])


def pdhg_rays_limits():
    """`pdhg_wide_limits()`, as the call with certificates reports them (mllp_lp_pdhg_rays_limits; no GPU)"""
    lim = (c_int64 * 4)()
    _lib.check(_lib.lib().mllp_lp_pdhg_rays_limits(lim))
    return int(lim[0]), int(lim[1]), int(lim[2]), int(lim[3])


def pdhg_wide_limits():
    """(threads per workgroup, the most Ruiz passes, the default and the largest rows_per_item) of `LPBatch.pdhg_wide`
    (mllp_lp_pdhg_wide_limits; no GPU)"""
    lim = (c_int64 * 4)()
    _lib.check(_lib.lib().mllp_lp_pdhg_wide_limits(lim))
    return int(lim[0]), int(lim[1]), int(lim[2]), int(lim[3])


def pdhg_halpern_limits():
    """`pdhg_scaled_limits()`, as the Halpern call reports them (mllp_lp_pdhg_halpern_limits; no GPU)"""
    lim = (c_int64 * 3)()
    _lib.check(_lib.lib().mllp_lp_pdhg_halpern_limits(lim))
    return int(lim[0]), int(lim[1]), int(lim[2])


def pdhg_scaled_limits():
    """(LDS words the preconditioned PDHG kernel can give to an instance's vectors, threads per workgroup, the most Ruiz
    passes) (mllp_lp_pdhg_scaled_limits; no GPU)"""
    lim = (c_int64 * 3)()
    _lib.check(_lib.lib().mllp_lp_pdhg_scaled_limits(lim))
    return int(lim[0]), int(lim[1]), int(lim[2])


def pdhg_limits():
    """(LDS words the PDHG kernel can give to an instance's vectors, threads per workgroup) (mllp_lp_pdhg_limits; no GPU)"""
    lim = (c_int64 * 2)()
    _lib.check(_lib.lib().mllp_lp_pdhg_limits(lim))
    return int(lim[0]), int(lim[1])


def topm_select_dense(logits, m, want=("mask", "index", "stats")):
    """`LPBatch.predict_basis` for ONE segment without a graph (mllp_topm_select_dense): the m largest of a contiguous
    cuda float32 vector, same order and tie rule.  `.index` has m entries (-1 past the vector's length)."""
    want = _parse_want("topm_select_dense", want, _SELECT_WANT, "want must name some of 'mask', 'index', 'stats'")
    if not (logits.is_cuda and logits.dtype == torch.float32 and logits.is_contiguous() and logits.dim() == 1):
        raise ValueError("topm_select_dense: logits must be a contiguous 1-d cuda float32 tensor")
    n, m, dev = int(logits.numel()), int(m), logits.device
    if m < 0:
        raise ValueError("topm_select_dense: m must not be negative")
    bufs = _select_outputs(want, n, m, 1, dev)
    _lib.check(_lib.lib().mllp_topm_select_dense(n, m, _lib.ptr(logits), *[_lib.ptr(b) for b in bufs], _lib.current_stream()))
    return BasisPrediction(_cut(bufs[0], n), _cut(bufs[1], m), bufs[2], [n], [m])


def small_step_limits():
    """dict(max_nodes, max_nnz, threads, lds_bytes) of the one-launch step (mllp_gnn_small_step_limits); needs no GPU."""
    out = (c_int64 * 4)()
    _lib.check(_lib.lib().mllp_gnn_small_step_limits(out))
    return dict(max_nodes=out[0], max_nnz=out[1], threads=out[2], lds_bytes=out[3])


def adam_step(params, grads, exp_avg, exp_avg_sq, state, eps=1e-8, grad_scale=1.0):
    """state: cuda float tensor [step, lr, beta1, beta2]; step is incremented on the device."""
    _lib.check(_lib.lib().mllp_adam_step(_lib.ptr(params), _lib.ptr(grads), _lib.ptr(exp_avg), _lib.ptr(exp_avg_sq),
                                         _lib.ptr(state), eps, grad_scale, params.numel(), _lib.current_stream()))


def optim_scratch_floats(n):
    """floats of scratch `optim_step` needs for n parameters (mllp_optim_scratch_floats; 0 for small n); needs no GPU."""
    out = c_int64()
    _lib.check(_lib.lib().mllp_optim_scratch_floats(int(n), ctypes.byref(out)))
    return int(out.value)


def optim_step(params, grads, exp_avg, exp_avg_sq, state, eps=1e-8, grad_scale=1.0, weight_decay=0.0, max_norm=0.0,
               scratch=None, info=None):
    """AdamW + global-norm clipping + warm-up / cosine schedule in one call, decided on the device (mllp_optim_step).
    state: cuda float tensor [step, lr_base, beta1, beta2, warmup W, total T, min_ratio r, 0]; step is incremented on the
    device unless the step is skipped (a non-finite gradient norm).  scratch: `optim_scratch_floats(n)` floats (None when
    that is 0); info: None or a float tensor [4] that receives {grad norm, clip coefficient, lr of the step, skipped}."""
    assert state.numel() >= 8, "optim_step: an 8-word state (pad mllp_adam_step's with four zeros)"
    _lib.check(_lib.lib().mllp_optim_step(_lib.ptr(params), _lib.ptr(grads), _lib.ptr(exp_avg), _lib.ptr(exp_avg_sq),
                                          _lib.ptr(state), eps, grad_scale, weight_decay, max_norm, _lib.ptr(scratch),
                                          _lib.ptr(info), params.numel(), _lib.current_stream()))


# ----------------------------------------------------------------------------------------------
# synthetic batches generated on the device (BASELINE.json configs[3]/[4])
# ----------------------------------------------------------------------------------------------
def synthetic_batch(n_inst=256, m=10000, n=20000, mean_row_nnz=200.0, seed=1234, device="cuda",
                    chunk=16, tier_wave=0, tier_block=0) -> LPBatch:
    """Random sparse LPs with Netlib-like statistics, generated on the GPU.

    Each row's columns come from a Bernoulli(p = mean_row_nnz / n) process realised as geometric gaps
    (row nnz ~ Binomial(n, p) ~ Poisson(mean), at least 1), values N(0,1) scaled to unit row 2-norm,
    coefs N(0,1) with 45% zeros then unit norm per instance, rhs 0 w.p. 0.73 else U(0,5), labels
    Bernoulli(0.37).  Instance i uses seed `seed + i` for its pattern chunk."""
    p = mean_row_nnz / n
    L = int(mean_row_nnz + 10 * np.sqrt(mean_row_nnz) + 16)     # gap slots per row (covers > 9 sigma)
    ptr_parts, idx_parts, val_parts = [], [], []
    nnz_off = 0
    log1mp = float(np.log1p(-p))
    for c0 in range(0, n_inst, chunk):
        k = min(chunk, n_inst - c0)
        g = torch.Generator(device=device).manual_seed(seed + c0)
        u = torch.rand(k * m, L, device=device, generator=g).clamp_(min=1e-12)
        gaps = torch.floor(torch.log(u) / log1mp).to(torch.int32) + 1          # geometric(p) >= 1
        cols = torch.cumsum(gaps, dim=1, dtype=torch.int32) - 1
        del u, gaps
        keep = cols < n
        keep[:, 0] = True                                                    # at least one nonzero per row
        cols[:, 0].clamp_(max=n - 1)
        cnt = keep.sum(dim=1)
        inst_of_row = torch.arange(k * m, device=device, dtype=torch.int64) // m
        gcols = (cols + ((c0 + inst_of_row) * n).to(torch.int32)[:, None])[keep]
        vals = torch.randn(gcols.numel(), device=device, generator=g)
        rows = torch.repeat_interleave(torch.arange(k * m, device=device), cnt)
        # row 2-norms by a per-row sequential reduction (rows are contiguous runs of `vals`): index_add_ uses floating-
        # point atomics and cumsum a decoupled look-back scan -- either makes the last bits of the matrix change from run
        # to run (tools/determinism_stream.py)
        nrm = torch.segment_reduce(vals * vals, "sum", lengths=cnt, unsafe=True).sqrt_().clamp_(min=1e-12)
        vals = vals / nrm[rows]
        ptr = torch.cumsum(cnt, 0) + nnz_off
        nnz_off = int(ptr[-1])
        ptr_parts.append(ptr.to(torch.int32))
        idx_parts.append(gcols.to(torch.int32))
        val_parts.append(vals)
        del cols, keep, rows, nrm, inst_of_row
    csr_ptr = torch.cat([torch.zeros(1, dtype=torch.int32, device=device)] + ptr_parts)
    csr_idx, csr_val = torch.cat(idx_parts), torch.cat(val_parts)
    del ptr_parts, idx_parts, val_parts
    g = torch.Generator(device=device).manual_seed(seed + 7919)
    N, M = n_inst * n, n_inst * m
    x1 = torch.randn(N, device=device, generator=g)
    x1[torch.rand(N, device=device, generator=g) < 0.45] = 0.0
    x1 = (x1.view(n_inst, n) / x1.view(n_inst, n).norm(dim=1, keepdim=True).clamp_(min=1e-12)).reshape(-1).contiguous()
    x2 = torch.where(torch.rand(M, device=device, generator=g) < 0.73, torch.zeros(M, device=device),
                     torch.rand(M, device=device, generator=g) * 5.0)
    y = (torch.rand(N, device=device, generator=g) < 0.37).float()
    return LPBatch.from_device_csr([m] * n_inst, [n] * n_inst, csr_ptr, csr_idx, csr_val, x1, x2, y,
                                   tier_wave, tier_block, names=[f"synth{seed + i}" for i in range(n_inst)])
