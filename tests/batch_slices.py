"""Test infrastructure: cut one instance back out of a block-diagonal batch (the inverse of BipartiteData.__inc__ batching,
oracle/spmm_form.py::BatchCSR), so that a GPU batch too large for the fp64 oracle can be checked instance by instance.
Never imported by the product."""
import numpy as np

from mllp_amd.data import LPInstance


def cut_instance(ptr, idx, val, x1, x2, labels, inst_m, inst_n, k, name=None):
    """Instance `k` of a block-diagonal batch as an LPInstance with local ids.  ptr / idx / val: the batch's CSR (rows =
    constraints, columns = variables, global ids); x1 (N,) objective coefficients, x2 (M,) right-hand sides, labels (N,);
    inst_m / inst_n: rows and columns of every instance."""
    ptr = np.asarray(ptr, np.int64)
    m_off = np.concatenate([[0], np.cumsum(np.asarray(inst_m, np.int64))])
    n_off = np.concatenate([[0], np.cumsum(np.asarray(inst_n, np.int64))])
    r0, r1, c0, c1 = int(m_off[k]), int(m_off[k + 1]), int(n_off[k]), int(n_off[k + 1])
    e0, e1 = int(ptr[r0]), int(ptr[r1])
    cols = np.asarray(idx[e0:e1], np.int64)
    assert ((cols >= c0) & (cols < c1)).all(), f"instance {k}: a nonzero outside its own column block"
    return LPInstance(name or f"inst{k}", ptr[r0:r1 + 1] - e0, (cols - c0).astype(np.int32),
                      np.asarray(val[e0:e1], np.float64), np.asarray(x1[c0:c1], np.float64),
                      np.asarray(x2[r0:r1], np.float64), np.asarray(labels[c0:c1]).astype(np.int32))
