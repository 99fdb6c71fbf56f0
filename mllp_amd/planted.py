"""Planted-basis LPs: labelled training batches in any quantity, made where the batch lives.

An LP built around a chosen basis, a chosen primal point and a chosen dual point has that basis as its unique optimal
basis by construction (`LPBatch.plant_basis`, include/mllp_hip.h: mllp_graph_plant_basis) -- no solver is needed, and
`LPBatch.certificate` verifies it from the stored data with two sparse sweeps.

  planted_pattern          sparsity pattern + one pivot per row, pure torch on any device
  planted_batch            pattern -> LPBatch.from_device_csr -> N(0,1) values -> plant_basis -> optionally normalize
  pivots_by_matching       a row-perfect matching of a real pattern (host, scipy)
  planted_from_instances   planted data on the patterns (and values) of given instances, e.g. Netlib's
  planted_dataset          the driver's `train_data_type: 'planted'`: a planted batch exported to the reference's tuples
"""
import numpy as np
import torch

from .data import LPInstance

_STREAM = 0x5EED1E55        # offset of the per-instance seed of the numbers (values, xstar, ystar, slack) from the pattern's


def _instance_pattern(m, n, mean_row_nnz, seed, device):
    """(row counts [m] int64, local column ids ascending inside a row, local pivot of every row [m] int64) of ONE
    instance, from `seed` alone: the row process of `synthetic_batch` (geometric gaps of a Bernoulli(mean_row_nnz / n)
    process, at least one entry), one pivot per row drawn as an injection into the columns (the first m of a random
    permutation) and inserted, rows then sorted and deduplicated."""
    g = torch.Generator(device=device).manual_seed(int(seed))
    p = min(float(mean_row_nnz) / n, 1.0 - 1e-9)
    L = int(mean_row_nnz + 10 * np.sqrt(mean_row_nnz) + 16)     # gap slots per row (covers > 9 sigma)
    u = torch.rand(m, L, device=device, generator=g).clamp_(min=1e-12)
    gaps = torch.floor(torch.log(u) / float(np.log1p(-p))).to(torch.int64) + 1          # geometric(p) >= 1
    cols = torch.cumsum(gaps, dim=1) - 1
    keep = cols < n
    if m:
        keep[:, 0] = True                                       # at least one nonzero per row
        cols[:, 0].clamp_(max=n - 1)
    pivot = torch.randperm(n, device=device, generator=g)[:m].to(torch.int64)
    rows = torch.arange(m, device=device, dtype=torch.int64)
    key = torch.cat([(rows[:, None] * n + cols)[keep], rows * n + pivot])
    key = torch.unique(key)                                     # sorted: row-major, ascending inside a row, no duplicates
    cnt = torch.bincount(torch.div(key, n, rounding_mode="floor"), minlength=m)
    return cnt, key % n, pivot


def planted_pattern(n_inst, m, n, mean_row_nnz, seed, device="cuda"):
    """The pattern of `n_inst` LPs of m rows and n columns with one pivot per row, in global ids:
    (inst_m, inst_n, csr_ptr [M + 1] int32, csr_idx [nnz] int32, pivot [M] int32).  Pure torch, any device ('cpu'
    included).  Instance i is generated from `seed + i` alone, so it is the same alone and inside any batch (on one
    device type: torch's generators differ between cpu and cuda).  Rows are strictly ascending; the pivot of a row is an
    entry of it and no column is the pivot of two rows.  n < m has no injection: ValueError."""
    n_inst, m, n = int(n_inst), int(m), int(n)
    if n < m:
        raise ValueError(f"planted_pattern: n = {n} columns cannot hold one pivot for each of m = {m} rows (n >= m is needed)")
    if n_inst < 0 or m < 0 or n < 1 or not mean_row_nnz > 0:
        raise ValueError("planted_pattern: n_inst >= 0, m >= 0, n >= 1 and mean_row_nnz > 0 are needed")
    cnts, idxs, pivs = [], [], []
    for i in range(n_inst):
        cnt, idx, piv = _instance_pattern(m, n, mean_row_nnz, seed + i, device)
        cnts.append(cnt)
        idxs.append(idx + i * n)
        pivs.append(piv + i * n)
    cat = lambda parts: torch.cat(parts) if parts else torch.zeros(0, dtype=torch.int64, device=device)   # noqa: E731
    csr_ptr = torch.zeros(n_inst * m + 1, dtype=torch.int64, device=device)
    csr_ptr[1:] = torch.cumsum(cat(cnts), 0)
    if int(csr_ptr[-1]) >= 2 ** 31 or n_inst * n >= 2 ** 31:
        raise ValueError("planted_pattern: the batch exceeds int32 indexing")
    return ([m] * n_inst, [n] * n_inst, csr_ptr.to(torch.int32), cat(idxs).to(torch.int32).contiguous(),
            cat(pivs).to(torch.int32).contiguous())


def _numbers(seed, nnz, m, n, device):
    """(values N(0,1) [nnz], xstar U(0.5, 1.5) [n], ystar U(-1, 1) [m], slack U(0.5, 1.5) [n]) of one instance from `seed`"""
    g = torch.Generator(device=device).manual_seed(int(seed) + _STREAM)
    return (torch.randn(nnz, device=device, generator=g), torch.rand(n, device=device, generator=g) + 0.5,
            torch.rand(m, device=device, generator=g) * 2.0 - 1.0, torch.rand(n, device=device, generator=g) + 0.5)


def _transform_duals(batch, ystar, row_scale, obj_scale):
    """ystar of the un-normalized LP -> that of the normalized one: c' - A'^T y' = t_k (c - A^T y) for y'_i = t_k y_i / s_i"""
    inst = torch.repeat_interleave(torch.arange(batch.n_inst, device=ystar.device),
                                   torch.tensor(batch.inst_m, device=ystar.device, dtype=torch.int64))
    return (obj_scale[inst] * ystar / row_scale).contiguous()


def planted_batch(n_inst, m, n, mean_row_nnz, seed, device="cuda", dominance=1.25, floor=0.25, normalize=False, rhs_cap=5.0,
                  names=None):
    """A labelled batch built on the device: `planted_pattern` -> `LPBatch.from_device_csr` -> N(0,1) values ->
    `plant_basis` with xstar, slack in U(0.5, 1.5) and ystar in U(-1, 1) -> optionally `normalize`.  The numbers of instance
    i come from `seed + i` alone.  Returns (batch, xstar [N], ystar [M]): the primal and dual points that certify the
    labels, `batch.certificate(xstar * batch.labels, ystar)`.  With normalize=True ystar is transformed to
    t_k * ystar_i / s_i (the applied objective and row scales), so the certificate holds for what the batch now stores;
    xstar is unchanged."""
    from .graph import LPBatch
    inst_m, inst_n, csr_ptr, csr_idx, pivot = planted_pattern(n_inst, m, n, mean_row_nnz, seed, device)
    cnt = (csr_ptr[1:] - csr_ptr[:-1]).long().view(n_inst, m).sum(1).tolist() if n_inst else []
    parts = [_numbers(seed + i, int(cnt[i]), m, n, device) for i in range(n_inst)]
    empty = torch.zeros(0, device=device)
    val, xstar, ystar, slack = (torch.cat([p[k] for p in parts]).contiguous() if parts else empty for k in range(4))
    M, N = n_inst * m, n_inst * n
    x1, x2, labels = torch.empty(N, device=device), torch.empty(M, device=device), torch.empty(N, device=device)
    names = names if names is not None else [f"planted{seed + i}" for i in range(n_inst)]
    b = LPBatch.from_device_csr(inst_m, inst_n, csr_ptr, csr_idx, val, x1, x2, labels, names=names)
    b.plant_basis(pivot, xstar, ystar, slack, dominance, floor)
    if normalize:
        s, t = b.normalize(rhs_cap)
        ystar = _transform_duals(b, ystar, s, t)
    return b, xstar, ystar


def pivots_by_matching(instance):
    """One pivot column per row of `instance`'s pattern, no column twice: a maximum bipartite matching of rows to columns
    (host; scipy.sparse.csgraph.maximum_bipartite_matching).  Returns local column ids [m] int32.  A pattern without a
    row-perfect matching -- an empty row, more rows than columns, a structurally rank-deficient block -- raises
    ValueError naming the instance."""
    import scipy.sparse
    from scipy.sparse.csgraph import maximum_bipartite_matching
    m, n = instance.m, instance.n
    pat = scipy.sparse.csr_matrix((np.ones(instance.nnz, np.int8), np.asarray(instance.indices, np.int32),
                                   np.asarray(instance.indptr, np.int32)), shape=(m, n))
    match = np.asarray(maximum_bipartite_matching(pat, perm_type="column"), np.int64) if m else np.zeros(0, np.int64)
    missing = int((match < 0).sum())
    if missing:
        raise ValueError(f"pivots_by_matching: the pattern of {instance.name} has no row-perfect matching "
                         f"({missing} of its {m} rows stay without a pivot)")
    return match.astype(np.int32)


def planted_from_instances(instances, seed=0, on_deficient="raise", device="cuda", dominance=1.25, floor=0.25,
                           normalize=False, rhs_cap=5.0):
    """Planted data on real patterns: the batch of `instances` (their patterns AND values, e.g. Netlib's) with the pivots
    of `pivots_by_matching` planted, xstar / ystar / slack of instance i drawn from `seed + i`.  on_deficient: 'raise'
    (a pattern without a row-perfect matching is an error) or 'skip' (it is left out).  Returns (batch, xstar, ystar) as
    `planted_batch`; `batch.names` tells which instances were kept."""
    from .graph import LPBatch
    if on_deficient not in ("raise", "skip"):
        raise ValueError(f"planted_from_instances: on_deficient must be 'raise' or 'skip', got {on_deficient!r}")
    kept, pivots, off = [], [], 0
    for k, inst in enumerate(instances):
        try:
            piv = pivots_by_matching(inst)
        except ValueError:
            if on_deficient == "raise":
                raise
            continue
        kept.append((k, inst))
        pivots.append(piv.astype(np.int64) + off)
        off += inst.n
    if not kept:
        raise ValueError("planted_from_instances: no instance with a row-perfect matching is left")
    b = LPBatch.from_instances([i for _, i in kept], device=device)
    parts = [_numbers(seed + k, 0, i.m, i.n, device) for k, i in kept]
    xstar, ystar, slack = (torch.cat([p[j] for p in parts]).contiguous() for j in (1, 2, 3))
    pivot = torch.tensor(np.concatenate(pivots), dtype=torch.int32, device=device)
    b.plant_basis(pivot, xstar, ystar, slack, dominance, floor)
    if normalize:
        s, t = b.normalize(rhs_cap)
        ystar = _transform_duals(b, ystar, s, t)
    return b, xstar, ystar


def batch_to_instances(batch):
    """The resident batch as host `LPInstance`s (local ids, what the batch stores NOW: values, x1, x2, labels)."""
    ptr, idx, val = batch.export(0).astype(np.int64), batch.export(1), batch.export(2)
    x1, x2, y = (t.detach().cpu().numpy() for t in (batch.x1, batch.x2, batch.labels))
    out, r0, c0 = [], 0, 0
    for k in range(batch.n_inst):
        m, n = batch.inst_m[k], batch.inst_n[k]
        lo, hi = ptr[r0], ptr[r0 + m]
        out.append(LPInstance(batch.names[k], ptr[r0:r0 + m + 1] - lo, (idx[lo:hi] - c0).astype(np.int32),
                              val[lo:hi].astype(np.float64), x1[c0:c0 + n].astype(np.float64),
                              x2[r0:r0 + m].astype(np.float64), (y[c0:c0 + n] != 0).astype(np.int32)))
        r0, c0 = r0 + m, c0 + n
    return out


PLANTED_DEFAULTS = {"instances": 64, "m": 50, "n": 120, "row_nnz": 6.0, "seed": 0}


def planted_dataset(block=None, device="cuda"):
    """The driver's `train_data_type: 'planted'`: the yaml block `planted: {instances, m, n, row_nnz, seed}` -> a planted,
    normalized batch built on the device, exported to the reference's tuples.  Returns (dataset, train_dict) as
    `get_netlib_dataset` does, so batch_size, holdout, pos_weight, resume and the checkpoint names work unchanged."""
    block = dict(block or {})
    unknown = sorted(set(block) - set(PLANTED_DEFAULTS))
    if unknown:
        raise ValueError(f"planted: unknown key(s) {unknown} (understood: {sorted(PLANTED_DEFAULTS)})")
    p = dict(PLANTED_DEFAULTS, **block)
    if int(p["instances"]) < 1:
        raise ValueError("planted: instances must be at least 1")
    b, _, _ = planted_batch(int(p["instances"]), int(p["m"]), int(p["n"]), float(p["row_nnz"]), int(p["seed"]), device=device,
                            normalize=True)
    dataset, train_dict = [], {"obj": []}
    for inst in batch_to_instances(b):
        dataset.append(inst.as_reference_tuple())
        train_dict[inst.name] = []
    return dataset, train_dict
