"""Parameter gradients compared tensor by tensor, each on its own scale (test infrastructure, no GPU needed).

`close` of tests/test_hip_parity.py divides one maximum error by one maximum reference value taken over all 4721
parameters.  The largest gradients are fc.weight and the value and skip tensors; the key, query and edge tensors are
orders of magnitude smaller, so a bound of RTOL_GRAD * max|g| is a large fraction of them, or more than all of them.
Here every tensor of the state dict is held to RTOL_GRAD of ITS OWN maximum, wherever the reference can afford it:

1. `tensor_slices()`: the 56 tensors of o1.state_dict_spec() as slices of the flat gradient, in three sets: the 42 live
   tensors, the five lin_key.bias (a per-destination constant cancels in the softmax: exactly 0 in exact arithmetic,
   rounding noise in fp32, masked everywhere) and the nine of gconv3_s2w (never called: the header promises zeros).
2. `own_scale_errors(got, want)`: per live tensor (max|want_t| / max|want|, max|got_t - want_t| / max|want_t|).
3. `yardstick(sd, batch, dlogits)`: the own-scale errors of fused_cases.model_dt in np.float32 against np.float64, the
   project's yardstick of what fp32 arithmetic can deliver on an input.
4. `close_per_tensor(got, want, yard, what, max_exempt)`: a live tensor whose yardstick is below RTOL_GRAD / 4 (the
   quarter-of-the-bar rule of tests/test_fused_oracle.py, per tensor) must be within RTOL_GRAD on its own scale.  A tensor
   whose yardstick is not below that is ill-conditioned ON THIS INPUT (cancellation: the fp32 reference misses it too); it is
   exempt, stays under the global bound only, and `max_exempt` caps how many there may be.  Exemption comes from the
   yardstick alone.

No tolerance is introduced: the bar is RTOL_GRAD of tests/test_hip_parity.py.  A tensor whose reference is exactly zero
(an input without nonzeros, a feature vector of zeros) has no scale of its own.  Where the fp32 restatement gives exact
zeros too, every term of the tensor is a product with an exact zero, in any order of summation: the kernels must write
zeros (+0 or -0), and the tensor counts among the checked ones.  Where the fp32 restatement does not (a cancellation to
zero, as on a 1 x 1 instance), the tensor is exempt like any other the yardstick cannot pin.
"""
import numpy as np

import fused_cases as fc
from oracle import pyg_restatement as o1
from test_hip_parity import RTOL_GRAD, close, grad_mask

UNUSED_CONV = "gconv3_s2w"
TINY = 1e-30                      # the scale floor of test_hip_parity.close


def tensor_slices():
    """(live, key_bias, unused): name -> slice of the flat gradient, in state-dict order"""
    live, key_bias, unused, off = {}, {}, {}, 0
    for name, shape in o1.state_dict_spec():
        n = int(np.prod(shape))
        s = slice(off, off + n)
        if name.startswith(UNUSED_CONV + "."):
            unused[name] = s
        elif name.endswith("lin_key.bias"):
            key_bias[name] = s
        else:
            live[name] = s
        off += n
    assert off == 4721 and (len(live), len(key_bias), len(unused)) == (42, 5, 9)
    return live, key_bias, unused


def own_scale_errors(got, want):
    """{live tensor: (max|want_t| / max|want|, max|got_t - want_t| / max|want_t|)}; max|want| over the unmasked entries.  A
    tensor whose reference is exactly zero: (0.0, 0.0 if got_t is zero too, else inf)."""
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    assert got.shape == want.shape == (4721,)
    top = max(float(np.abs(want[grad_mask()]).max()), TINY)
    out = {}
    for name, s in tensor_slices()[0].items():
        scale = float(np.abs(want[s]).max())
        diff = float(np.abs(got[s] - want[s]).max())
        out[name] = (scale / top, diff / scale) if scale > 0 else (0.0, 0.0 if diff == 0 else float("inf"))
    return out


def yardstick(sd, batch, dlogits=None):
    """own-scale errors of the oracle's decomposition run in fp32 against the same in fp64 (on the CPU)"""
    r32 = fc.model_dt(sd, batch, np.float32, dlogits=dlogits)
    r64 = fc.model_dt(sd, batch, np.float64, dlogits=dlogits)
    return own_scale_errors(r32["grads"], r64["grads"])


def exempt_tensors(yard):
    """live tensors that the fp32 reference itself does not deliver to a quarter of the bar on this input"""
    return sorted(name for name, (_, err) in yard.items() if not err < RTOL_GRAD / 4)


def zero_tensors(yard):
    """live tensors whose reference gradient is exactly zero on this input, in fp64 and in fp32: zeros are demanded"""
    return sorted(name for name, (size, err) in yard.items() if size == 0 and err == 0)


def checked_tensors(yard):
    return set(yard) - set(exempt_tensors(yard))


def table_lines(what, table):
    lines = [f"[per tensor] {what}: tensor, size relative to the largest gradient, yardstick, deviation"]
    for name, (size, yd, dev) in table.items():
        mark = "" if yd < RTOL_GRAD / 4 else "   exempt"
        mark = "   zero" if size == 0 and yd == 0 else mark
        lines.append(f"  {name:28s} {size:9.2e} {yd:9.2e} {dev:9.2e}{mark}")
    return lines


def close_per_tensor(got, want, yard, what="", max_exempt=0):
    """Returns ({tensor: (size, yardstick, deviation)}, set of tensors checked on their own scale); raises AssertionError
    with every offending tensor named."""
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    assert got.shape == want.shape == (4721,), what
    assert np.isfinite(got).all(), what
    live, _, unused = tensor_slices()
    assert set(yard) == set(live), what
    exempt = exempt_tensors(yard)
    assert len(exempt) <= max_exempt, f"{what}: {len(exempt)} exempt tensors, cap {max_exempt}: {exempt}"
    errs = own_scale_errors(got, want)
    table = {name: (errs[name][0], yard[name][1], errs[name][1]) for name in live}
    checked = checked_tensors(yard)
    assert all((errs[name][0] == 0) == (yard[name][0] == 0) for name in live), f"{what}: the yardstick is of another input"
    bad = [f"{name}: max|diff|/max|ref_t| = {table[name][2]:.3e} >= {RTOL_GRAD} (tensor at {table[name][0]:.1e} of the "
           f"largest gradient, yardstick {table[name][1]:.1e})" for name in live if name in checked and not table[name][2] < RTOL_GRAD]
    bad += [f"{name}: not exactly zero" for name, s in unused.items() if (got[s] != 0.0).any()]
    assert not bad, f"{what}: " + "; ".join(bad)
    keep = grad_mask()
    close(got[keep], want[keep], RTOL_GRAD, f"{what}: all tensors on the scale of the largest")      # the exempt ones too
    return table, checked
