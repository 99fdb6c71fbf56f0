"""ctypes binding of libmllp_hip.so (C ABI declared in include/mllp_hip.h).

There is NO CPU fallback: if the shared library is missing this module raises at import of the
symbol table (`lib()`), and every launch fails loudly without a HIP device.
"""
import ctypes
import os
import subprocess
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_uint32, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libmllp_hip.so")
HEADER_PATH = os.path.abspath(os.path.join(_HERE, "..", "include", "mllp_hip.h"))

ABI_VERSION = 6

# Layout of the flat parameter vector: GNNModel.state_dict() order, the same table as
# csrc/internal.h.  Six TransformerConvs (the last, gconv3_s2w, is never called), then fc (weight [16], bias).
FEAT = 16
CONV_NAMES = ("gconv1_w2s", "gconv1_s2w", "gconv2_w2s", "gconv2_s2w", "gconv3_w2s", "gconv3_s2w")
CONV_CIN = (1, 1, 16, 16, 16, 16)


def conv_param_count(cin):
    """Parameters of one conv: key, query, value and skip (weight [16, cin] + bias [16]) and the edge weight [16]."""
    return 4 * FEAT * cin + 5 * FEAT


_CONV_OFFSETS = [0]
for _cin in CONV_CIN:
    _CONV_OFFSETS.append(_CONV_OFFSETS[-1] + conv_param_count(_cin))
FC_OFFSET = _CONV_OFFSETS[-1]
NUM_PARAMS = FC_OFFSET + FEAT + 1


def conv_param_slice(conv):
    """Slice of the flat parameter (or gradient) vector that holds one conv, by name or by index in CONV_NAMES."""
    i = CONV_NAMES.index(conv) if isinstance(conv, str) else range(len(CONV_NAMES))[conv]
    return slice(_CONV_OFFSETS[i], _CONV_OFFSETS[i + 1])


class MllpError(RuntimeError):
    pass


_PROTOTYPES = {
    # name: (restype, [argtypes])
    "mllp_last_error": (c_char_p, []),
    "mllp_abi_version": (c_int, []),
    "mllp_graph_create_host": (c_int, [c_int64, POINTER(c_int64), POINTER(c_int64), POINTER(c_int64),
                                       POINTER(c_int32), POINTER(c_double), c_int32, c_int32,
                                       POINTER(c_void_p)]),
    "mllp_graph_create_device": (c_int, [c_int64, POINTER(c_int64), POINTER(c_int64), c_int64,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_int32, c_int32, c_void_p, POINTER(c_void_p)]),
    "mllp_graph_destroy": (c_int, [c_void_p]),
    "mllp_graph_dims": (c_int, [c_void_p, POINTER(c_int64)]),
    "mllp_graph_export": (c_int, [c_void_p, c_int, c_void_p, c_int64]),
    "mllp_graph_set_path": (c_int, [c_void_p, c_int]),
    "mllp_set_fused_grid_limit": (c_int, [c_int64, POINTER(c_int64)]),
    "mllp_graph_fused_grid": (c_int, [c_void_p, POINTER(c_int64)]),
    "mllp_graph_invalidate_inputs": (c_int, [c_void_p]),
    "mllp_graph_set_values": (c_int, [c_void_p, c_void_p, c_void_p]),
    "mllp_graph_set_values_bytes": (c_int, [c_void_p, POINTER(c_int64)]),
    "mllp_graph_scale_values": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "mllp_graph_normalize": (c_int, [c_void_p, c_void_p, c_void_p, c_float, c_int, c_void_p, c_void_p, c_void_p]),
    "mllp_normalize_row_tier": (c_int, [c_int64, POINTER(c_int)]),
    "mllp_graph_plant_basis": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float, c_void_p, c_void_p,
                                       c_void_p, c_void_p]),
    "mllp_lp_certificate_scratch_bytes": (c_int, [c_void_p, POINTER(c_int64)]),
    "mllp_lp_certificate": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mllp_basis_repair_scratch_bytes": (c_int, [c_void_p, c_int64, POINTER(c_int64)]),
    "mllp_basis_repair": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_void_p, c_void_p, c_void_p]),
    "mllp_basis_simplex_scratch_bytes": (c_int, [c_void_p, c_int64, POINTER(c_int64)]),
    "mllp_basis_simplex": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float, c_float, c_float, c_float, c_int64,
                                   c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mllp_basis_simplex_guarded": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float, c_float, c_float, c_float,
                                           c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_void_p, c_void_p]),
    "mllp_lp_pdhg_limits": (c_int, [POINTER(c_int64)]),
    "mllp_lp_pdhg_scratch_bytes": (c_int, [c_void_p, c_int64, POINTER(c_int64)]),
    "mllp_lp_pdhg": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_float, c_float, c_float, c_int64,
                             c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mllp_lp_pdhg_scaled_limits": (c_int, [POINTER(c_int64)]),
    "mllp_lp_pdhg_scaled_scratch_bytes": (c_int, [c_void_p, c_int64, POINTER(c_int64)]),
    "mllp_lp_pdhg_scaled": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_float, c_float, c_float,
                                    c_int64, c_int32, c_int32, c_float, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_void_p, c_void_p, c_void_p]),
    "mllp_lp_pdhg_halpern_limits": (c_int, [POINTER(c_int64)]),
    "mllp_lp_pdhg_halpern_scratch_bytes": (c_int, [c_void_p, c_int64, POINTER(c_int64)]),
    "mllp_lp_pdhg_halpern": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_float, c_float, c_float,
                                     c_int64, c_int32, c_int32, c_float, c_int32, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_void_p, c_void_p, c_void_p]),
    "mllp_lp_pdhg_wide_limits": (c_int, [POINTER(c_int64)]),
    "mllp_lp_pdhg_wide_scratch_bytes": (c_int, [c_void_p, c_int64, POINTER(c_int64)]),
    "mllp_lp_pdhg_wide": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_float, c_float,
                                  c_float, c_int64, c_int32, c_int32, c_float, c_int32, c_int64, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mllp_lp_pdhg_rays_limits": (c_int, [POINTER(c_int64)]),
    "mllp_lp_pdhg_rays_scratch_bytes": (c_int, [c_void_p, c_int64, POINTER(c_int64)]),
    "mllp_lp_pdhg_rays": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_float, c_float,
                                  c_float, c_int64, c_int32, c_int32, c_float, c_int32, c_float, c_int64, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mllp_lp_pdhg_spectral_limits": (c_int, [POINTER(c_int64)]),
    "mllp_lp_pdhg_spectral_scratch_bytes": (c_int, [c_void_p, c_int64, POINTER(c_int64)]),
    "mllp_lp_pdhg_spectral": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_float, c_float,
                                      c_float, c_int64, c_int32, c_int32, c_float, c_int32, c_float, c_int64, c_int64, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mllp_graph_build_spmm_copy": (c_int, [c_void_p, c_int, c_int, c_void_p]),
    "mllp_graph_drop_spmm_copy": (c_int, [c_void_p, c_int]),
    "mllp_graph_spmm_copy_info": (c_int, [c_void_p, c_int, POINTER(c_int64)]),
    "mllp_graph_export_spmm_copy": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int64]),
    "mllp_graph_build_stream_copy": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p]),
    "mllp_graph_drop_stream_copy": (c_int, [c_void_p, c_int, c_int]),
    "mllp_graph_stream_copy_info": (c_int, [c_void_p, c_int, c_int, POINTER(c_int64)]),
    "mllp_graph_export_stream_copy": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int64]),
    "mllp_csr_transpose_device": (c_int, [c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_void_p, c_void_p]),
    "mllp_graph_build_tiled": (c_int, [c_void_p, c_int, c_int, c_void_p]),
    "mllp_graph_tiled_info": (c_int, [c_void_p, c_int, c_int, POINTER(c_int64)]),
    "mllp_graph_export_tiled": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int64, c_void_p]),
    "mllp_spmm_csr_f32": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "mllp_spmm_csr_bf16": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "mllp_angle_num_params": (c_int, [c_int, POINTER(c_int64)]),
    "mllp_angle_workspace_floats": (c_int, [c_int64, c_int, POINTER(c_int64)]),
    "mllp_angle_forward": (c_int, [c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mllp_angle_backward": (c_int, [c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mllp_angle_backward_inputs": (c_int, [c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_void_p, c_void_p, c_void_p]),
    "mllp_tiled_geometry": (c_int, [c_int, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32)]),
    "mllp_graph_attach_tiled": (c_int, [c_void_p, c_int, c_int, c_int64, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_void_p]),
    "mllp_tconv_workspace_floats": (c_int, [c_void_p, c_int, c_int, POINTER(c_int64)]),
    "mllp_tconv_fwd": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mllp_tconv_bwd": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                               c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "mllp_gnn_workspace_bytes": (c_int, [c_void_p, POINTER(c_int64)]),
    "mllp_gnn_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mllp_gnn_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mllp_gnn_input_grads_scratch_bytes": (c_int, [c_void_p, POINTER(c_int64)]),
    "mllp_gnn_backward_inputs": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_void_p, c_void_p]),
    "mllp_gnn_input_grads": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_void_p, c_void_p, c_void_p]),
    "mllp_gnn_loss_step_inputs": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p,
                                          c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mllp_gnn_loss_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_void_p]),
    "mllp_gnn_train_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p,
                                    c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int, c_void_p]),
    "mllp_gnn_small_step_limits": (c_int, [POINTER(c_int64)]),
    "mllp_gnn_small_step_fits": (c_int, [c_void_p, POINTER(c_int)]),
    "mllp_gnn_train_step_small": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p,
                                          c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p]),
    "mllp_weighted_loss": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mllp_balanced_pos_weight": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "mllp_gnn_loss_step_weighted": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                            c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mllp_topm_loss": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float, c_int64, c_uint32,
                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mllp_topm_loss_limits": (c_int, [POINTER(c_int64)]),
    "mllp_topm_loss_math": (c_int, [c_int, c_int64, c_void_p, c_void_p, c_void_p]),
    "mllp_gnn_loss_step_topm": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float,
                                        c_float, c_int64, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_void_p]),
    "mllp_adam_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float, c_int64,
                               c_void_p]),
    "mllp_optim_scratch_floats": (c_int, [c_int64, POINTER(c_int64)]),
    "mllp_optim_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float, c_float, c_float,
                                c_void_p, c_void_p, c_int64, c_void_p]),
    "mllp_metrics_scratch_bytes": (c_int, [c_void_p, POINTER(c_int64)]),
    "mllp_topm_metrics": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mllp_topm_select": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mllp_topm_select_dense": (c_int, [c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mllp_mps_read": (c_int, [c_char_p, c_int, POINTER(c_void_p)]),
    "mllp_lp_dims": (c_int, [c_void_p, POINTER(c_int64)]),
    "mllp_lp_export": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mllp_lp_free": (c_int, [c_void_p]),
}

_lib = None


def build(verbose=False):
    """Compile libmllp_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    out = subprocess.run(["make", "-C", os.path.join(_HERE, "csrc"), "-j4"], capture_output=True, text=True)
    if verbose or out.returncode != 0:
        print(out.stdout[-4000:])
        print(out.stderr[-4000:])
    if out.returncode != 0:
        raise MllpError("building libmllp_hip.so failed")
    return LIB_PATH


def lib():
    """The loaded library with prototypes set; raises MllpError if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MllpError(f"{LIB_PATH} not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                            "(or `make -C mllp_amd/csrc`). The product path has no CPU fallback.")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _PROTOTYPES.items():
            fn = getattr(L, name)           # AttributeError if the .so misses a declared symbol
            fn.restype = res
            fn.argtypes = args
        if L.mllp_abi_version() != ABI_VERSION:
            raise MllpError("libmllp_hip.so ABI version mismatch")
        _lib = L
    return _lib


MLLP_ERANGE = -4          # include/mllp_hip.h


def check(rc):
    if rc != 0:
        msg = lib().mllp_last_error()
        raise MllpError(f"libmllp_hip error {rc}: {msg.decode() if msg else '?'}")


def ptr(t):
    """Device/host pointer of a torch tensor (or None) as c_void_p."""
    if t is None:
        return c_void_p(0)
    return c_void_p(t.data_ptr())


def np_ptr(a, ctype):
    return a.ctypes.data_as(POINTER(ctype))


def current_stream():
    import torch
    return c_void_p(torch.cuda.current_stream().cuda_stream)
