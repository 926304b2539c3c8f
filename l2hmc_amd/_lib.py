"""ctypes binding of libl2hmc_hip.so (include/l2hmc_hip.h).

There is no CPU fallback: if the library is missing, or a tensor is not a
contiguous fp32 CUDA tensor, the call raises.  PyTorch-ROCm is used only for
device memory and streams."""
import ctypes as C
import os
import re

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# L2HMC_LIB_PATH: load another build of the same ABI (diagnostic builds under tools/_diag); default = the in-tree library
LIB_PATH = os.environ.get("L2HMC_LIB_PATH") or os.path.join(_HERE, "libl2hmc_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "l2hmc_hip.h")

c_float_p = C.c_void_p   # device pointers travel as integers
MAX_MIX, MAX_SMALL_DIM, MAX_SMALL_NODES = 8, 8, 64
PLAN_LAYERED, PLAN_CONV3D, PLAN_SELECTED_ONLY, PLAN_RECOMPUTE, PLAN_TILES16_ONLY, PLAN_ALL_COLUMNS = 1, 2, 4, 8, 16, 32
PLAN_FULL_L1 = 64
PLAN_SINGLE_KICKS = 128
PLAN_PERIODIC = 256
PLAN_PERIODIC_STEP = 512     # with PLAN_PERIODIC only: the torus-exact mode's whole-step kernel where the plan has it
PLAN_PERIODIC_TRAIN = 1024   # with PLAN_PERIODIC only: the tiled training entries take the plan (widths multiples of 32)
PLAN_PERIODIC_TAPE = 2048    # with both of them only: the training forward as one taped whole-trajectory launch where the plan has it
GRAD_BUCKET_REST = 6
BUCKET_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int32)


class DenseNet(C.Structure):
    _fields_ = [("D", C.c_int32), ("H", C.c_int32), ("Ka", C.c_int32), ("Kb", C.c_int32),
                ("w1_t", c_float_p), ("wt", c_float_p), ("b1", c_float_p), ("wh_t", c_float_p),
                ("bh", c_float_p), ("whd_t", c_float_p), ("bhd", c_float_p),
                ("coeff_s", c_float_p), ("coeff_q", c_float_p),
                ("q_tanh", C.c_int32), ("reserved", C.c_int32), ("packed", c_float_p)]


class DenseGrads(C.Structure):
    _fields_ = [(n, c_float_p) for n in ("w1_t", "wt", "b1", "wh_t", "bh", "whd_t", "bhd", "coeff_s", "coeff_q")]


class Conv3DGrads(C.Structure):
    _fields_ = [(n, c_float_p) for n in ("w1_a", "b1_a", "w2_a", "b2_a", "w1_b", "b1_b", "w2_b", "b2_b")]


class Conv3DFront(C.Structure):
    _fields_ = [("F", C.c_int32), ("reserved", C.c_int32),
                ("w1_a", c_float_p), ("b1_a", c_float_p), ("w2_a", c_float_p), ("b2_a", c_float_p),
                ("w1_b", c_float_p), ("b1_b", c_float_p), ("w2_b", c_float_p), ("b2_b", c_float_p)]


class GaugePlan(C.Structure):
    _fields_ = [("T", C.c_int32), ("X", C.c_int32), ("num_steps", C.c_int32), ("hmc", C.c_int32),
                ("eps", C.c_float), ("flags", C.c_int32), ("masks", c_float_p),
                ("xnet", DenseNet), ("vnet", DenseNet), ("xfront", Conv3DFront), ("vfront", Conv3DFront),
                ("heads", C.c_void_p)]


TARGET_MIXTURE, TARGET_GAUSSIAN, TARGET_ROUGH_WELL, TARGET_FUNNEL = 0, 1, 2, 3     # l2hmc_mog_target::is_gaussian


class RoughWellParams(C.Structure):
    _fields_ = [("eps", C.c_float), ("easy", C.c_int32)]


class _MuSlot(C.Union):      # the rough well's scalars travel by value in the slot of `mu`
    _fields_ = [("mu", c_float_p), ("rough_well", RoughWellParams)]


class MogTarget(C.Structure):
    _anonymous_ = ("_slot",)
    _fields_ = [("dim", C.c_int32), ("K", C.c_int32), ("is_gaussian", C.c_int32),
                ("temperature", C.c_float), ("_slot", _MuSlot), ("prec", c_float_p),
                ("log_const", c_float_p)]


class SmallPlan(C.Structure):
    _fields_ = [("x_dim", C.c_int32), ("num_nodes", C.c_int32), ("trajectory_length", C.c_int32),
                ("hmc", C.c_int32), ("eps", C.c_float), ("first_layer_form", C.c_int32), ("masks", c_float_p),
                ("xnet", DenseNet), ("vnet", DenseNet), ("target", MogTarget)]


_P, _I32, _I64, _F, _SZ, _U64 = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_size_t, C.c_uint64
_PROTOS = {
    "l2hmc_abi_version": (C.c_int, []),
    "l2hmc_last_error": (C.c_char_p, []),
    "l2hmc_u1_action_force": (C.c_int, [_P, _I64, _I32, _I32, _F, _P, _P, _P, _P, _P]),
    "l2hmc_u1_plaq_sums": (C.c_int, [_P, _I64, _I32, _I32, _P, _P]),
    "l2hmc_wrap_angle": (C.c_int, [_P, _I64, _P, _P]),
    "l2hmc_kinetic_energy": (C.c_int, [_P, _I64, _I32, _P, _P]),
    "l2hmc_stq_ws_bytes": (_SZ, [_I64, _I32]),
    "l2hmc_stq_dense": (C.c_int, [C.POINTER(DenseNet), _P, _P, _P, _F, _F, _I64, _P, _P, _P, _P, _SZ, _P]),
    "l2hmc_stq_conv3d_ws_bytes": (_SZ, [_I64, _I32, _I32, _I32, _I32]),
    "l2hmc_stq_conv3d": (C.c_int, [C.POINTER(Conv3DFront), C.POINTER(DenseNet), _I32, _I32, _P, _P, _P, _F, _F,
                                   _I64, _P, _P, _P, _P, _SZ, _P]),
    "l2hmc_dense_pack_bytes": (_SZ, [C.POINTER(DenseNet)]),
    "l2hmc_dense_pack": (C.c_int, [C.POINTER(DenseNet), _P, _P]),
    "l2hmc_lf_update_v": (C.c_int, [_P, _P, _P, _P, _P, _F, _I32, _I64, _I32, _P, _P, _P]),
    "l2hmc_lf_update_x": (C.c_int, [_P, _P, _P, _P, _P, _P, _F, _I32, _I64, _I32, _P, _P, _P]),
    "l2hmc_accept_prob": (C.c_int, [_P, _P, _P, _I64, _P, _P]),
    "l2hmc_mix_accept": (C.c_int, [_P] * 9 + [_I32, _I64, _I32, _P, _P, _P, _P, _P]),
    "l2hmc_gauge_ws_bytes": (_SZ, [C.POINTER(GaugePlan), _I64]),
    "l2hmc_gauge_plan_fused": (C.c_int, [C.POINTER(GaugePlan)]),
    "l2hmc_gauge_plan_train_fused": (C.c_int, [C.POINTER(GaugePlan)]),
    "l2hmc_gauge_step_plan": (C.c_int, [_I64, _I32, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "l2hmc_gauge_pack_heads_bytes": (_SZ, [C.POINTER(GaugePlan)]),
    "l2hmc_gauge_pack_heads": (C.c_int, [C.POINTER(GaugePlan), _P, _P]),
    "l2hmc_gauge_leapfrog": (C.c_int, [C.POINTER(GaugePlan), _F, _I32, _P, _P, _P, _I64, _P, _P, _SZ, _P]),
    "l2hmc_gauge_leapfrog_steps": (C.c_int, [C.POINTER(GaugePlan), _F, _I32, _I32, _P, _P, _P, _I64, _P, _P, _SZ, _P]),
    "l2hmc_gauge_trajectory": (C.c_int, [C.POINTER(GaugePlan), _F, _P, _P, _P, _I64, _P, _P, _P, _P, _P,
                                         _SZ, _P]),
    "l2hmc_gauge_transition_ws_bytes": (_SZ, [C.POINTER(GaugePlan), _I64, _I32]),
    "l2hmc_gauge_transition": (C.c_int, [C.POINTER(GaugePlan), _F, _P, _P, _P, _P, _P, _I64, _I32, _P, _P,
                                         _P, _P, _P, _SZ, _P]),
    "l2hmc_gauge_transition_ladder": (C.c_int, [C.POINTER(GaugePlan), _P, _I64, _P, _P, _P, _P, _P, _I64, _I32, _P, _P,
                                                _P, _P, _P, _SZ, _P]),
    "l2hmc_gauge_transition_draw": (C.c_int, [C.POINTER(GaugePlan), _F, _P, _I64, _U64, _U64, _P, _P, _P, _P, _P, _SZ,
                                              _P]),
    "l2hmc_gauge_mcmc_step_ws_bytes": (_SZ, [C.POINTER(GaugePlan), _I64]),
    "l2hmc_gauge_mcmc_step": (C.c_int, [C.POINTER(GaugePlan), _F, _P, _I64, _U64, _U64, _P, _P, _P, _P, _P, _P,
                                        _SZ, _P]),
    "l2hmc_gauge_mcmc_step_ex": (C.c_int, [C.POINTER(GaugePlan), _F, _P, _P, _I64, _U64, _U64, _P, _P, _P, _P, _P, _P, _P,
                                           _SZ, _P]),
    "l2hmc_gauge_mcmc_step_ladder": (C.c_int, [C.POINTER(GaugePlan), _P, _I64, _P, _P, _I64, _U64, _U64, _P, _P, _P, _P, _P,
                                               _P, _P, _SZ, _P]),
    "l2hmc_gauge_hmc_run_ws_bytes": (_SZ, [C.POINTER(GaugePlan), _I64, _I32]),
    "l2hmc_gauge_hmc_run": (C.c_int, [C.POINTER(GaugePlan), _P, _P, _P, _I64, _U64, _U64, _I32, _P, _P, _P, _P, _P, _P,
                                      _P, _P, _SZ, _P]),
    "l2hmc_gauge_hmc_run_ladder_ws_bytes": (_SZ, [C.POINTER(GaugePlan), _I64, _I32]),
    "l2hmc_gauge_hmc_run_ladder": (C.c_int, [C.POINTER(GaugePlan), _P, _I64, _I64, _P, _P, _P, _I64, _U64, _U64, _I32,
                                             _P, _P, _P, _P, _P, _P, _P, _P, _SZ, _P]),
    "l2hmc_gauge_hmc_run_exchange_served": (C.c_int, [C.POINTER(GaugePlan), _I32]),
    "l2hmc_gauge_hmc_run_exchange_ws_bytes": (_SZ, [C.POINTER(GaugePlan), _I64, _I32]),
    "l2hmc_gauge_hmc_run_exchange": (C.c_int, [C.POINTER(GaugePlan), _P, _I64, _I64, _P, _P, _P, _I64, _U64, _U64, _I32,
                                               _I32, _I32, _I32, _I32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                               _SZ, _P]),
    "l2hmc_gauge_replica_swap": (C.c_int, [_I32, _I32, _P, _I64, _I32, _I32, _P, _I64, _U64, _U64, _P, _P, _P, _P, _P]),
    "l2hmc_gauge_loss_terms": (C.c_int, [_P, _P, _P, _P, _P, _I64, _I32, _I32, _I32, _F, _F, _F, _F, _P, _P]),
    "l2hmc_gauge_train_ws_bytes": (_SZ, [C.POINTER(GaugePlan), _I64]),
    "l2hmc_gauge_train_forward": (C.c_int, [C.POINTER(GaugePlan), _F, _P, _P, _P, _I64, _P, _P, _P, _P, _P, _SZ,
                                            _P]),
    "l2hmc_gauge_train_backward": (C.c_int, [C.POINTER(GaugePlan), _F, _P, _I64, _P, _P, _P,
                                             C.POINTER(DenseGrads), C.POINTER(DenseGrads),
                                             C.POINTER(Conv3DGrads), C.POINTER(Conv3DGrads), _P, _P, _SZ, _P]),
    "l2hmc_gauge_train_backward_buckets": (C.c_int, [C.POINTER(GaugePlan), _F, _P, _I64, _P, _P, _P,
                                                     C.POINTER(DenseGrads), C.POINTER(DenseGrads),
                                                     C.POINTER(Conv3DGrads), C.POINTER(Conv3DGrads), _P, _P, _SZ, _P,
                                                     BUCKET_FN, _P]),
    "l2hmc_gauge_loss_backward": (C.c_int, [_I32, _I32, _F, _P, _P, _P, _P, _I64, _I32, _F, _F, _F, _F, _F, _P, _P,
                                            _P, _P, _P]),
    "l2hmc_gauge_train_forward_ladder": (C.c_int, [C.POINTER(GaugePlan), _P, _I64, _I64, _P, _P, _P, _I64, _P, _P, _P,
                                                   _P, _P, _SZ, _P]),
    "l2hmc_gauge_train_backward_ladder": (C.c_int, [C.POINTER(GaugePlan), _P, _I64, _I64, _P, _I64, _P, _P, _P,
                                                    C.POINTER(DenseGrads), C.POINTER(DenseGrads),
                                                    C.POINTER(Conv3DGrads), C.POINTER(Conv3DGrads), _P, _P, _SZ, _P,
                                                    BUCKET_FN, _P]),
    "l2hmc_gauge_loss_backward_ladder": (C.c_int, [_I32, _I32, _P, _I64, _P, _P, _P, _P, _I64, _I32, _F, _F, _F, _F,
                                                   _F, _P, _P, _P, _P, _P]),
    "l2hmc_gauge_accept_backward": (C.c_int, [_I32, _I32, _F, _I64] + [_P] * 15 + [_P]),
    "l2hmc_gauge_accept_backward_ladder": (C.c_int, [_I32, _I32, _P, _I64, _I64, _I64] + [_P] * 15 + [_P]),
    "l2hmc_grad_sumsq": (C.c_int, [_P, _I64, _I64, _I64, _P, _I32, _P]),
    "l2hmc_adam_step": (C.c_int, [_P, _P, _P, _P, _I64, _F, _F, _F, _F, _P, _F, _I64, _I64, _P]),
    "l2hmc_mog_energy_grad": (C.c_int, [C.POINTER(MogTarget), _P, _I64, _P, _P, _P]),
    "l2hmc_small_trajectory": (C.c_int, [C.POINTER(SmallPlan), _P, _P, _P, _I64, _P, _P, _P, _P, _P]),
    "l2hmc_small_trajectory_tempered": (C.c_int, [C.POINTER(SmallPlan), _P, _I64, _I64, _P, _P, _P, _I64, _P, _P, _P, _P,
                                                  _P]),
    "l2hmc_small_propose": (C.c_int, [C.POINTER(SmallPlan), _P, _I64, C.c_uint64, C.c_uint64, _P, _P, _P, _P, _P]),
    "l2hmc_small_run": (C.c_int, [C.POINTER(SmallPlan), _P, _P, _I64, _U64, _U64, _I32, _P, _P, _P]),
    "l2hmc_small_run_tempered": (C.c_int, [C.POINTER(SmallPlan), _P, _P, _I64, _U64, _U64, _I32, _P, _I64, _I64, _P, _P,
                                           _P]),
    "l2hmc_small_hmc_run": (C.c_int, [C.POINTER(SmallPlan), _P, _P, _I64, _U64, _U64, _I32, _P, _I64, _I64, _P, _P, _P,
                                      _P]),
    "l2hmc_small_ais_run": (C.c_int, [C.POINTER(SmallPlan), C.POINTER(MogTarget), _P, _P, _P, _F, _I64, _U64, _U64,
                                      _I32, _P, _P, _P, _P]),
    "l2hmc_small_replica_swap": (C.c_int, [C.POINTER(SmallPlan), _P, _I64, _I32, _I32, _P, _I64, _U64, _U64, _P, _P, _P,
                                           _P, _P]),
    "l2hmc_small_hmc_run_exchange": (C.c_int, [C.POINTER(SmallPlan), _P, _P, _I64, _U64, _U64, _I32, _P, _I64, _I64, _P,
                                               _I32, _I32, _I32, _I32, _P, _P, _P, _P, _P, _P, _P]),
    "l2hmc_small_run_exchange": (C.c_int, [C.POINTER(SmallPlan), _P, _P, _I64, _U64, _U64, _I32, _P, _I64, _I64,
                                           _I32, _I32, _I32, _I32, _P, _P, _P, _P, _P, _P, _P]),
    "l2hmc_small_train_ws_bytes": (_SZ, [C.POINTER(SmallPlan), _I64]),
    "l2hmc_small_train_step": (C.c_int, [C.POINTER(SmallPlan), _P, _P, _P, _I64, _F, _F, _P, _P, _P, _P, _P, _P, _SZ,
                                         _P]),
    "l2hmc_small_train_step_tempered": (C.c_int, [C.POINTER(SmallPlan), _P, _I64, _I64, _P, _P, _P, _I64, _F, _F, _P, _P,
                                                  _P, _P, _P, _P, _SZ, _P]),
    "l2hmc_small_vjp": (C.c_int, [C.POINTER(SmallPlan), _P, _P, _P, _I64] + [_P] * 11 + [_P, _SZ, _P]),
    "l2hmc_small_vjp_tempered": (C.c_int, [C.POINTER(SmallPlan), _P, _I64, _I64, _P, _P, _P, _I64] + [_P] * 11
                                 + [_P, _SZ, _P]),
    "l2hmc_mog_energy_hvp": (C.c_int, [C.POINTER(MogTarget), _P, _P, _I64, _P, _P]),
    "l2hmc_u1_force_hvp": (C.c_int, [_P, _P, _I64, _I32, _I32, _F, _P, _P]),
    "l2hmc_stq_dense_taped": (C.c_int, [C.POINTER(DenseNet), _P, _P, _P, _F, _F, _I64, _P, _P, _P, _P, _P, _P]),
    "l2hmc_lf_update_v_vjp": (C.c_int, [_P, _P, _P, _P, _P, _F, _I32, _I64, _I32, _P, _P] + [_P] * 6 + [_P]),
    "l2hmc_lf_update_x_vjp": (C.c_int, [_P, _P, _P, _P, _P, _P, _F, _I32, _I64, _I32, _P, _P] + [_P] * 6 + [_P]),
    "l2hmc_lf_update_x_ncp": (C.c_int, [_P, _P, _P, _P, _P, _P, _F, _I32, _I64, _I32, _P, _P, _P]),
    "l2hmc_lf_update_x_ncp_vjp": (C.c_int, [_P, _P, _P, _P, _P, _P, _F, _I32, _I64, _I32, _P, _P] + [_P] * 6 + [_P]),
    "l2hmc_u1_angle_features": (C.c_int, [_P, _I64, _I32, _P, _P]),
    "l2hmc_u1_angle_features_vjp": (C.c_int, [_P, _P, _I64, _I64, _I32, _P, _P]),
    "l2hmc_dense_backward_data_ws_bytes": (_SZ, [C.POINTER(DenseNet)]),
    "l2hmc_dense_backward_data": (C.c_int, [C.POINTER(DenseNet)] + [_P] * 7 + [_I64] + [_P] * 6 + [_SZ, _P]),
    "l2hmc_dense_weight_grads_ws_bytes": (_SZ, [C.POINTER(DenseNet), _I64]),
    "l2hmc_dense_weight_grads": (C.c_int, [C.POINTER(DenseNet), _I64] + [_P] * 8 + [C.POINTER(DenseGrads), _P, _SZ,
                                                                                      _P]),
    "l2hmc_profile_begin": (C.c_int, [_I32]),
    "l2hmc_profile_end": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "l2hmc_fill_normal": (C.c_int, [_P, _I64, _U64, _U64, _P]),
    "l2hmc_fill_uniform": (C.c_int, [_P, _I64, _U64, _U64, _P]),
}

_lib = None


def declared_symbols():
    """Every function name include/l2hmc_hip.h declares."""
    with open(HEADER_PATH) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return sorted(set(re.findall(r"\b(l2hmc_[a-z0-9_]+)\s*\(", text)))


def lib():
    """The loaded library; raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -m l2hmc_amd.build` "
                "(or __graft_entry__.build()).  There is no CPU fallback.")
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in _PROTOS.items():
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = res, args
        if handle.l2hmc_abi_version() != 1:
            raise RuntimeError("libl2hmc_hip.so ABI version mismatch")
        _lib = handle
    return _lib


class L2HMCError(RuntimeError):
    pass


def check(rc):
    if rc != 0:
        msg = lib().l2hmc_last_error().decode()
        kind = {1: "bad argument", 2: "HIP error", 3: "workspace too small"}.get(rc, f"error {rc}")
        if rc == 1:
            raise ValueError(f"l2hmc_hip: {kind}: {msg}")
        raise L2HMCError(f"l2hmc_hip: {kind}: {msg}")


def dev_ptr(t, dtype=torch.float32, name="tensor"):
    """Device pointer of a contiguous CUDA tensor (None -> NULL)."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a CUDA (ROCm) tensor; the HIP path has no CPU fallback")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: tensor must be contiguous")
    return t.data_ptr()


def _shape_text(shape):
    return "(" + ", ".join("*" if s is None else str(s) for s in shape) + ("," if len(shape) == 1 else "") + ")"


def expect_shape(t, shape, name, who=None, fold=False):
    """Refuse a caller tensor `t` (tensor, array or nested list; None passes: an optional argument that was left out)
    whose shape is not `shape`, a tuple in which None matches any extent.  `fold`: `shape` is [rows, width] and any
    [rows, ...] whose trailing extents multiply to width matches too (a position given as [B, T, X, 2]).  The C ABI
    takes raw pointers and sizes its launches from one argument, so this is what keeps a kernel from reading past the
    end of another.  Host arithmetic on shape tuples only: no torch.cuda call, no synchronisation, no allocation.
    ValueError: `name: expected shape (..), got (..)` for the stateless operators, `who: name of shape (..): expected
    (..)` for a method `who`.  Returns t."""
    if t is None:
        return t
    got = tuple(t.shape) if hasattr(t, "shape") else np.shape(t)
    seen = got
    if fold and len(got) > 2:
        width = 1
        for n in got[1:]:
            width *= n
        seen = (got[0], width)
    if len(seen) != len(shape) or any(e is not None and e != g for e, g in zip(shape, seen)):
        if who is None:
            raise ValueError(f"{name}: expected shape {_shape_text(shape)}, got {_shape_text(got)}")
        raise ValueError(f"{who}: {name} of shape {_shape_text(got)}: expected {_shape_text(shape)}"
                         + (" (or any trailing extents with that product)" if fold else ""))
    return t


def stream_ptr(device=None):
    """Raw hipStream_t of torch's current stream on `device` (default: the current device).  Kernels are launched
    on the CURRENT device, so a tensor living elsewhere is an error, not a silent cross-device launch."""
    cur = torch.cuda.current_device()
    if device is not None:
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("the HIP path has no CPU fallback")
        if device.index is not None and device.index != cur:
            raise RuntimeError(f"object lives on cuda:{device.index} but the current device is cuda:{cur}; "
                               f"wrap the call in `with torch.cuda.device({device.index}):`")
    return torch._C._cuda_getCurrentRawStream(cur)      # current_stream(cur).cuda_stream without the Stream object


_CALL_DTYPES = frozenset((torch.float32, torch.int32, torch.uint8))


def call(name, *args, device=None, tail=()):
    """Run the C entry `name` on torch's current stream of `device` and check its status.  Every tensor argument travels
    as its device address after `dev_ptr`'s checks (on the GPU, contiguous; fp32, int32 or uint8), before the library
    or torch.cuda is touched; None stays NULL; plans (C.byref), numbers and workspace (ptr, nbytes) pairs pass as they
    are.  `tail`: what the entry takes after its stream."""
    ptrs = list(args)
    for i, a in enumerate(args):
        if hasattr(a, "data_ptr"):          # a tensor; isinstance(a, torch.Tensor) costs 0.2 us for every plain argument
            if not (a.is_cuda and a.dtype in _CALL_DTYPES and a.is_contiguous()):      # dev_ptr words the error
                dev_ptr(a, a.dtype if a.dtype in _CALL_DTYPES else torch.float32, f"{name}: argument {i}")
            ptrs[i] = a.data_ptr()
    check(getattr(lib(), name)(*ptrs, stream_ptr(device), *tail))


def step_draw_index(draws):
    """The native MCMC step (l2hmc_gauge_mcmc_step) consumes the Philox stream pair (2d, 2d+1) of its `draw`
    argument; `GaugeDynamics._normal/_uniform` consume stream `_draws` and advance it by one.  ONE counter serves
    both: the step takes the next even-aligned pair at or after `draws`.  Returns (d, new_draws)."""
    d = (int(draws) + 1) // 2
    return d, 2 * d + 2


def run_draw_index(draws, n_steps):
    """The draw indices of `n_steps` consecutive native steps (l2hmc_gauge_hmc_run) are draw0, draw0 + 1, ...:
    what `n_steps` calls of step_draw_index hand out.  Returns (draw0, new_draws)."""
    d, _ = step_draw_index(draws)
    return d, 2 * (d + int(n_steps) - 1) + 2


def exchange_rounds(n_steps, swap_every, swap_phase):
    """The rounds inside `n_steps` steps that start `swap_phase` steps into a period of `swap_every`: one after every
    step that completes a period."""
    return (int(swap_phase) + int(n_steps)) // int(swap_every)


def exchange_run_draw_index(draws, n_steps, swap_every, swap_phase):
    """The draws of `n_steps` native steps with the replica-exchange rounds between them in ONE launch
    (l2hmc_gauge_hmc_run_exchange): what the loop `step_draw_index` per step, `draws += 1` per round hands out, a round
    following step s (from 0) iff (swap_phase + s + 1) % swap_every == 0.  A step at draw index d leaves the counter at
    2 d + 2 and a round after it at 2 d + 3, so a step after a round has index d + 2.  Returns (draw0, rounds of the
    launch, new_draws)."""
    n, k, ph = int(n_steps), int(swap_every), int(swap_phase)
    d0, _ = step_draw_index(draws)
    d_last = d0 + n - 1 + (ph + n - 1) // k                 # the rounds ahead of the last step
    return d0, exchange_rounds(n, k, ph), 2 * d_last + (3 if (ph + n) % k == 0 else 2)


def as_dev(a, device=None, dtype=torch.float32):
    """numpy / tensor -> contiguous CUDA tensor of `dtype` (copy only if needed)."""
    device = device or torch.device("cuda", torch.cuda.current_device())
    if not isinstance(a, torch.Tensor):
        a = torch.as_tensor(a)
    return a.to(device=device, dtype=dtype).contiguous()


class Workspace:
    """Grow-only scratch buffer handed to the C ABI (which never allocates)."""

    def __init__(self):
        self.buf = None

    def get(self, nbytes, device):
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != device:
            self.buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        return self.buf.data_ptr(), self.buf.numel()
